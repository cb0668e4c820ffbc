// Track detection of the predict path on the device: the kernels behind
// identifytracks.get_end (reference identifytracks.py:21-48) and signal_noise
// (:51-143).  Stages, each one entry point of include/acfe.h:
//   acfe_stft_mag    |STFT| (n_fft 2048, hop 281) of the whole recording as
//                    [1025][T] fp32 + its maximum
//   acfe_median      exact np.median along either axis, by selection on the
//                    bit patterns of the raw magnitudes
//   acfe_signal_map  the two-median threshold -> 0 / 1 uint8 map
//   acfe_morph_box   OpenCV box erode / dilate, separable, sliding counts
//   acfe_map_runs    horizontal runs of the final map (the host unions them
//                    into 8-connected components)
//   acfe_chunk_flat  get_end's max == min test per chunk of the mel image
// Everything after the STFT reproduces the host arithmetic exactly: float32
// IEEE division (no fast-math in this build), comparisons, integer counts.
// Every image index is 64-bit (1025 x T passes 2^31 at about 3.3 hours), and
// no loop's trip count depends on the data beyond the image size.
#include "common.h"
#include "fft_stockham.h"

using namespace acfe;

namespace {

constexpr int TK_NFFT = 2048;      // identifytracks.py:55
constexpr int TK_NC = TK_NFFT / 2;  // complex FFT points (even / odd sample pairs)
constexpr int TK_F = TK_NC + 1;    // bins kept: all of them
constexpr int TK_FB = 16;          // frames per workgroup = 64-B runs in every bin row
constexpr int TK_TS = TK_F + 3;    // tile row stride = 4 mod 64: frame-major reads of 16 x 4 cells hit 64 banks

// workspace of acfe_stft_mag: twiddles + window (written by k_stft_tables on
// every call: no allocation, no state between calls), then the max partials
struct StftWs {
  float2* tw;   // W_1024^k, k < 1024
  float2* rtw;  // W_2048^k, k <= 1024
  float* win;   // periodic Hann [2048]
  float* part;  // [cdiv(T, TK_FB)]
};
constexpr int64_t TK_WS_TABLES = 8 * TK_NC + 8 * (TK_NC + 2) + 4 * TK_NFFT;
StftWs stft_ws(void* ws) {
  char* p = static_cast<char*>(ws);
  StftWs w;
  w.tw = reinterpret_cast<float2*>(p);
  w.rtw = reinterpret_cast<float2*>(p + 8 * TK_NC);
  w.win = reinterpret_cast<float*>(p + 8 * TK_NC + 8 * (TK_NC + 2));
  w.part = reinterpret_cast<float*>(p + TK_WS_TABLES);
  return w;
}

__global__ void __launch_bounds__(256) k_stft_tables(float2* __restrict__ tw, float2* __restrict__ rtw,
                                                     float* __restrict__ win) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < TK_NC) tw[i] = make_float2((float)cospi(i / 512.0), (float)-sinpi(i / 512.0));
  if (i <= TK_NC) rtw[i] = make_float2((float)cospi(i / 1024.0), (float)-sinpi(i / 1024.0));
  if (i < TK_NFFT) win[i] = (float)(0.5 - 0.5 * cospi(i / 1024.0));
}

// One 256-thread workgroup owns TK_FB consecutive frames.  Per frame: framing
// (centred, zero padding) + Hann fused into the radix-8 first pass, the
// remaining Stockham passes of k_mel<1024> (8, 8, 2) through one padded LDS
// buffer, then the real-FFT post-processing of ALL 1025 bins into one row of
// an LDS tile.  The tile is written out transposed: 16 consecutive lanes store
// the 16 frames of one bin, a 64-B run of that bin's row.  An all-zero frame
// stays +0 through every pass (sums and products of zeros, sqrt(+0)).
__global__ void __launch_bounds__(256) k_stft_mag(const float* __restrict__ x, int64_t n, int hop, int T,
                                                  const float2* __restrict__ tw, const float2* __restrict__ rtw,
                                                  const float* __restrict__ win, float* __restrict__ spec,
                                                  float* __restrict__ part) {
  constexpr int NC = TK_NC;
  constexpr int NB0 = NC / 8;  // first-pass butterflies: threads 0..127
  __shared__ float2 buf[NC + NC / 8];
  __shared__ float tile[TK_FB * TK_TS];
  __shared__ float wmax[4];
  const int f0 = blockIdx.x * TK_FB;
  const int nf = min(TK_FB, T - f0);
  float mx = 0.f;
  for (int i = 0; i < nf; ++i) {
    const int64_t start = (int64_t)(f0 + i) * hop - NC;  // centre: n_fft / 2 zeros in front
    {
      float2 v[8];
      const int j = threadIdx.x;
      if (j < NB0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int nn = j + r * NB0;
          const int64_t s = start + 2 * nn;
          const float a = (s >= 0 && s < n) ? x[s] : 0.f;
          const float c = (s + 1 >= 0 && s + 1 < n) ? x[s + 1] : 0.f;
          v[r] = make_float2(a * win[2 * nn], c * win[2 * nn + 1]);
        }
        dft<8>(v);
      }
      __syncthreads();  // previous frame's readers of buf are done
      if (j < NB0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[padx(j * 8 + r)] = v[r];
      }
      __syncthreads();
    }
    stockham_pass<NC, 8>(buf, 8, tw);
    stockham_pass<NC, 8>(buf, 64, tw);
    stockham_pass<NC, 2>(buf, 512, tw);
    for (int k = threadIdx.x; k < TK_F; k += 256) {
      const float2 zk = buf[padx(k & (NC - 1))];
      const float2 zm = buf[padx((NC - k) & (NC - 1))];
      // E = (zk + conj(zm)) / 2, O = (zk - conj(zm)) / (2i), X = E + W_2048^k O
      const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
      const float2 D = make_float2(zk.x - zm.x, zk.y + zm.y);
      const float2 O = make_float2(0.5f * D.y, -0.5f * D.x);
      const float2 X = cadd(E, cmul(rtw[k], O));
      const float m = sqrtf(X.x * X.x + X.y * X.y);
      tile[i * TK_TS + k] = m;
      mx = fmaxf(mx, m);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TK_F * TK_FB; e += 256) {
    const int k = e >> 4, fr = e & (TK_FB - 1);
    if (fr < nf) spec[(int64_t)k * T + f0 + fr] = tile[fr * TK_TS + k];
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

__global__ void __launch_bounds__(256) k_max_partials(const float* __restrict__ part, int np, float* __restrict__ out) {
  __shared__ float wmax[4];
  float mx = 0.f;  // magnitudes are >= 0
  for (int i = threadIdx.x; i < np; i += 256) mx = fmaxf(mx, part[i]);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// ------------------------------------------------------------ medians
// np.median(img / m) from the two middle order statistics a <= b of img (the
// same one when the count is odd): division by m > 0 is monotone, so the
// k-th smallest of img / m is (k-th smallest of img) / m.
__device__ __forceinline__ float median_of(uint32_t a, uint32_t b, bool odd, const float* __restrict__ scale) {
  const float m = scale ? scale[0] : 1.f;
  const float qa = __uint_as_float(a) / m;
  if (odd) return qa;
  const float qb = __uint_as_float(b) / m;
  return __fadd_rn(qa, qb) * 0.5f;  // np.mean of the two: one rounded add, an exact halving
}

// Row medians: one workgroup per row, radix select on the bit patterns (which
// order as the values do: finite, non-negative), 8 bits per pass.  Each pass
// histograms the digit of the elements that match the prefix found so far,
// once for each of the two order statistics (their prefixes can part ways).
__global__ void __launch_bounds__(256) k_median_rows(const float* __restrict__ img, int cols,
                                                     const float* __restrict__ scale, float* __restrict__ out) {
  __shared__ unsigned hist[2][256];
  __shared__ unsigned s_pre[2], s_k[2];
  const uint32_t* row = reinterpret_cast<const uint32_t*>(img) + (int64_t)blockIdx.x * cols;
  if (threadIdx.x < 2) {
    s_pre[threadIdx.x] = 0;
    s_k[threadIdx.x] = threadIdx.x ? cols / 2 : (cols - 1) / 2;
  }
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[0][threadIdx.x] = 0;
    hist[1][threadIdx.x] = 0;
    __syncthreads();
    const unsigned pre0 = s_pre[0], pre1 = s_pre[1];
    const unsigned high = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
    for (int c = threadIdx.x; c < cols; c += 256) {
      const unsigned u = row[c];
      const unsigned d = (u >> shift) & 255u;
      if ((u & high) == pre0) atomicAdd(&hist[0][d], 1u);
      if ((u & high) == pre1) atomicAdd(&hist[1][d], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2) {  // the digit whose cumulative count first exceeds k
      unsigned k = s_k[threadIdx.x], acc = 0, digit = 255, below = 0;
      bool found = false;
      for (unsigned d = 0; d < 256; ++d) {
        const unsigned h = hist[threadIdx.x][d];
        if (!found && k < acc + h) {
          found = true;
          digit = d;
          below = acc;
        }
        acc += h;
      }
      s_pre[threadIdx.x] |= digit << shift;
      s_k[threadIdx.x] = k - below;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = median_of(s_pre[0], s_pre[1], cols & 1, scale);
}

// Column medians: a workgroup owns CB adjacent columns (lanes run along a row,
// so loads coalesce) and 256 / CB interleaved row groups; each order statistic
// is built bit by bit from bit 30 down (the sign bit is clear): count the
// elements that agree with the prefix above the bit and have the bit clear.
// STAGED (rows <= 1025, the detector's case) keeps the CB = 16 columns in LDS
// and reads the image once; otherwise every bit re-reads its columns.
constexpr int TK_STAGE_ROWS = TK_F;
template <int CB, bool STAGED>
__global__ void __launch_bounds__(256) k_median_cols(const float* __restrict__ img, int rows, int cols,
                                                     const float* __restrict__ scale, float* __restrict__ out) {
  constexpr int RG = 256 / CB;
  __shared__ unsigned tile[STAGED ? TK_STAGE_ROWS * CB : 1];
  __shared__ unsigned cnt[2][RG][CB];
  const int cc = threadIdx.x % CB, rg = threadIdx.x / CB;
  const int c0 = blockIdx.x * CB;
  const bool valid = c0 + cc < cols;
  const uint32_t* base = reinterpret_cast<const uint32_t*>(img);
  if (STAGED) {
    for (int e = threadIdx.x; e < rows * CB; e += 256) {
      const int r = e / CB, c = c0 + e % CB;
      tile[e] = c < cols ? base[(int64_t)r * cols + c] : 0u;
    }
    __syncthreads();
  }
  unsigned pre0 = 0, pre1 = 0, k0 = (rows - 1) / 2, k1 = rows / 2;
  for (int b = 30; b >= 0; --b) {
    unsigned n0 = 0, n1 = 0;
    if (valid) {
      for (int r = rg; r < rows; r += RG) {
        const unsigned u = STAGED ? tile[r * CB + cc] : base[(int64_t)r * cols + c0 + cc];
        n0 += ((u ^ pre0) >> b) == 0;
        n1 += ((u ^ pre1) >> b) == 0;
      }
    }
    cnt[0][rg][cc] = n0;
    cnt[1][rg][cc] = n1;
    __syncthreads();
    unsigned t0 = 0, t1 = 0;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      t0 += cnt[0][g][cc];
      t1 += cnt[1][g][cc];
    }
    __syncthreads();
    if (k0 >= t0) {
      k0 -= t0;
      pre0 |= 1u << b;
    }
    if (k1 >= t1) {
      k1 -= t1;
      pre1 |= 1u << b;
    }
  }
  if (valid && rg == 0) out[c0 + cc] = median_of(pre0, pre1, rows & 1, scale);
}

// ------------------------------------------------------------ signal map
__global__ void __launch_bounds__(256) k_signal_map(const float* __restrict__ spec, int64_t cells, int cols,
                                                    const float* __restrict__ mx, const float* __restrict__ col_med,
                                                    const float* __restrict__ row_med, uint8_t* __restrict__ map) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cells) return;
  const int64_t r = e / cols;
  const int c = (int)(e - r * cols);
  const float s = spec[e] / mx[0];
  map[e] = (s > 2.f * col_med[c]) & (s > 3.f * row_med[r]);
}

// ------------------------------------------------------------ morphology
// One line pass of the separable box: `seg` outputs from x0 along a line of
// `len` cells spaced `es` apart, with a sliding count of the ones in the
// window [x - k/2, x - k/2 + k - 1] clipped to the line.  Dilate: any one.
// Erode: every in-line cell is one (cells outside the image are ignored).
__device__ __forceinline__ void morph_line(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t es,
                                           int len, int x0, int seg, int k, int op) {
  const int a = k / 2;
  const int x1 = min(x0 + seg, len);
  int cnt = 0;
  for (int i = max(x0 - a, 0); i <= min(x0 - a + k - 1, len - 1); ++i) cnt += src[i * es];
  for (int x = x0; x < x1; ++x) {
    const int lo = x - a, hi = lo + k - 1;
    const int nin = min(hi, len - 1) - max(lo, 0) + 1;
    dst[x * es] = op ? cnt > 0 : cnt == nin;
    if (lo >= 0) cnt -= src[lo * es];
    if (hi + 1 < len) cnt += src[(hi + 1) * es];
  }
}

constexpr int TK_SEG = 32;  // outputs per thread along the filtered axis

// along a row: thread = (row, segment)
__global__ void __launch_bounds__(256) k_morph_rows(const uint8_t* __restrict__ src, int rows, int cols, int k, int op,
                                                    uint8_t* __restrict__ dst) {
  const int nseg = (cols + TK_SEG - 1) / TK_SEG;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)rows * nseg) return;
  const int64_t r = e / nseg;
  const int sg = (int)(e - r * nseg);
  morph_line(src + r * cols, dst + r * cols, 1, cols, sg * TK_SEG, TK_SEG, k, op);
}

// along a column: thread = (row segment, column), lanes on adjacent columns
__global__ void __launch_bounds__(256) k_morph_cols(const uint8_t* __restrict__ src, int rows, int cols, int k, int op,
                                                    uint8_t* __restrict__ dst) {
  const int nseg = (rows + TK_SEG - 1) / TK_SEG;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)nseg * cols) return;
  const int64_t sg = e / cols;
  const int c = (int)(e - sg * cols);
  morph_line(src + c, dst + c, cols, rows, (int)sg * TK_SEG, TK_SEG, k, op);
}

// ------------------------------------------------------------ runs
// One wave per row walks it 64 cells at a time.  A lane whose cell ends a run
// finds the run's first column from the ballot of run starts at or below it,
// or from the start carried over from an earlier step; the wave reserves its
// slots with one atomic add, which keeps counting past `cap`.
__global__ void __launch_bounds__(256) k_map_runs(const uint8_t* __restrict__ map, int rows, int cols,
                                                  int* __restrict__ runs, int cap, int* __restrict__ count) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const uint8_t* row = map + (int64_t)r * cols;
  int open = 0;  // first column of a run that began in an earlier step
  for (int base = 0; base < cols; base += 64) {
    const int x = base + lane;
    const bool in = x < cols;
    const bool cur = in && row[x];
    const bool prv = in && x > 0 && row[x - 1];
    const bool nxt = x + 1 < cols && row[x + 1];
    const bool st = cur && !prv, en = cur && !nxt;
    const unsigned long long smask = __ballot(st), emask = __ballot(en);
    if (emask) {
      const int ne = __popcll(emask);
      int b = 0;
      if (lane == 0) b = atomicAdd(count, ne);
      b = __shfl(b, 0, 64);
      if (en) {
        const unsigned long long below = smask & ((2ull << lane) - 1ull);
        const int first = below ? base + 63 - __clzll(below) : open;
        const int64_t slot = (int64_t)b + __popcll(emask & ((1ull << lane) - 1ull));
        if (slot < cap) {
          runs[3 * slot] = r;
          runs[3 * slot + 1] = first;
          runs[3 * slot + 2] = x;
        }
      }
    }
    const int hs = smask ? 63 - __clzll(smask) : -1, he = emask ? 63 - __clzll(emask) : -1;
    if (hs > he) open = base + hs;
  }
}

// ------------------------------------------------------------ get_end
__global__ void __launch_bounds__(256) k_chunk_flat(const float* __restrict__ img, int rows, int cols, int chunk,
                                                    int* __restrict__ flags) {
  __shared__ float wmn[4], wmx[4];
  const float* p = img + (int64_t)blockIdx.x * chunk;
  float mn = p[0], mx = p[0];
  for (int e = threadIdx.x; e < rows * chunk; e += 256) {
    const int r = e / chunk, j = e - r * chunk;
    const float v = p[(int64_t)r * cols + j];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) {
    wmn[threadIdx.x >> 6] = mn;
    wmx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    flags[blockIdx.x] = fminf(fminf(wmn[0], wmn[1]), fminf(wmn[2], wmn[3])) ==
                        fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3]));
}

constexpr int64_t TK_MAX_BLOCKS = 0x7FFFFFFF;
int64_t stft_frames(int64_t n, int hop) { return 1 + n / hop; }

}  // namespace

ACFE_API int64_t acfe_stft_mag_workspace(int64_t n, int n_fft, int hop) {
  if (n <= 0 || n_fft != TK_NFFT || hop <= 0 || stft_frames(n, hop) > 0x7FFFFFFF) return ACFE_E_INVAL;
  return TK_WS_TABLES + 4 * (int64_t)cdiv(stft_frames(n, hop), TK_FB);
}

ACFE_API int acfe_stft_mag(const float* x, int64_t n, int n_fft, int hop, float* spec, float* max_out, void* ws,
                           void* stream) {
  if (!x || !spec || !max_out || !ws || acfe_stft_mag_workspace(n, n_fft, hop) < 0) return ACFE_E_INVAL;
  const int T = (int)stft_frames(n, hop);
  const int nb = cdiv(T, TK_FB);
  const StftWs w = stft_ws(ws);
  hipLaunchKernelGGL(k_stft_tables, dim3(TK_NFFT / 256 + 1), dim3(256), 0, strm(stream), w.tw, w.rtw, w.win);
  hipLaunchKernelGGL(k_stft_mag, dim3(nb), dim3(256), 0, strm(stream), x, n, hop, T, w.tw, w.rtw, w.win, spec,
                     w.part);
  hipLaunchKernelGGL(k_max_partials, dim3(1), dim3(256), 0, strm(stream), w.part, nb, max_out);
  return launch_rc("acfe_stft_mag");
}

ACFE_API int acfe_median(const float* img, int rows, int cols, int axis, const float* scale, float* out,
                         void* stream) {
  if (!img || !out || rows <= 0 || cols <= 0 || (axis != 0 && axis != 1)) return ACFE_E_INVAL;
  if (axis == 1)
    hipLaunchKernelGGL(k_median_rows, dim3(rows), dim3(256), 0, strm(stream), img, cols, scale, out);
  else if (rows <= TK_STAGE_ROWS)
    hipLaunchKernelGGL((k_median_cols<16, true>), dim3(cdiv(cols, 16)), dim3(256), 0, strm(stream), img, rows, cols,
                       scale, out);
  else
    hipLaunchKernelGGL((k_median_cols<64, false>), dim3(cdiv(cols, 64)), dim3(256), 0, strm(stream), img, rows, cols,
                       scale, out);
  return launch_rc("acfe_median");
}

ACFE_API int acfe_signal_map(const float* spec, int rows, int cols, const float* max, const float* col_med,
                             const float* row_med, uint8_t* map, void* stream) {
  if (!spec || !max || !col_med || !row_med || !map || rows <= 0 || cols <= 0) return ACFE_E_INVAL;
  const int64_t cells = (int64_t)rows * cols;
  if ((cells + 255) / 256 > TK_MAX_BLOCKS) return ACFE_E_INVAL;
  hipLaunchKernelGGL(k_signal_map, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, strm(stream), spec, cells,
                     cols, max, col_med, row_med, map);
  return launch_rc("acfe_signal_map");
}

ACFE_API int64_t acfe_morph_box_workspace(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return ACFE_E_INVAL;
  return (int64_t)rows * cols;  // the row pass's image
}

ACFE_API int acfe_morph_box(const uint8_t* src, int rows, int cols, int h, int w, int op, uint8_t* dst, void* ws,
                            void* stream) {
  if (!src || !dst || !ws || src == dst || rows <= 0 || cols <= 0 || rows > (1 << 30) || cols > (1 << 30) ||
      (op != 0 && op != 1))
    return ACFE_E_INVAL;
  if (h <= 0 || w <= 0) h = w = 3;  // OpenCV's default for an empty structuring element
  // a window of 2 * len cells already covers the whole line from every cell
  h = h < 2 * rows ? h : 2 * rows;
  w = w < 2 * cols ? w : 2 * cols;
  uint8_t* tmp = static_cast<uint8_t*>(ws);
  const int64_t nr = (int64_t)rows * cdiv(cols, TK_SEG), nc = (int64_t)cdiv(rows, TK_SEG) * cols;
  if ((nr + 255) / 256 > TK_MAX_BLOCKS || (nc + 255) / 256 > TK_MAX_BLOCKS) return ACFE_E_INVAL;
  hipLaunchKernelGGL(k_morph_rows, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, strm(stream), src, rows, cols, w,
                     op, tmp);
  hipLaunchKernelGGL(k_morph_cols, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, strm(stream), tmp, rows, cols, h,
                     op, dst);
  return launch_rc("acfe_morph_box");
}

ACFE_API int acfe_map_runs(const uint8_t* map, int rows, int cols, int* runs, int cap, int* count, void* stream) {
  if (!map || !count || rows <= 0 || cols <= 0 || cap < 0 || (cap > 0 && !runs)) return ACFE_E_INVAL;
  hipError_t e = hipMemsetAsync(count, 0, sizeof(int), strm(stream));
  if (e != hipSuccess) return hip_rc(e, "acfe_map_runs");
  hipLaunchKernelGGL(k_map_runs, dim3(cdiv(rows, 4)), dim3(256), 0, strm(stream), map, rows, cols, runs, cap, count);
  return launch_rc("acfe_map_runs");
}

ACFE_API int acfe_chunk_flat(const float* img, int rows, int cols, int chunk, int n_chunks, int* flags,
                             void* stream) {
  if (n_chunks == 0 && rows > 0 && cols > 0 && chunk > 0) return ACFE_OK;
  if (!img || !flags || rows <= 0 || cols <= 0 || chunk <= 0 || n_chunks < 0 || (int64_t)n_chunks * chunk > cols ||
      (int64_t)rows * chunk > 0x7FFFFFFF)
    return ACFE_E_INVAL;
  hipLaunchKernelGGL(k_chunk_flat, dim3(n_chunks), dim3(256), 0, strm(stream), img, rows, cols, chunk, flags);
  return launch_rc("acfe_chunk_flat");
}
