// The C = 1 stem convolution of resnet/wr_resnet.py and
// resnet/wr_resnet_bird.py (acfe_stem_*): direct and MFMA kernels of the
// forward, the input / weight gradients and the backward with the BN backward
// apply.  The 3 identical input channels of tfdataset.py:2053 are folded into
// one by summing the stem weights over Cin (exact up to fp reassociation).
#include "conv_common.h"

using namespace acfe;

// ------------------------------------------------------------------ stem (C = 1)
// y[n,h,w,k] = sum_{r,s} x[n, h - pt + r, w - pl + s] * weff[k][r][s] + b[k]
// (stride 1, P = H, Q = W).  Tile: 16 rows x 64 cols; thread = one column x
// 4 rows (lane = column, so LDS reads of consecutive lanes are consecutive
// words or 32 B pixels: conflict-free).  The 16 x R x S weights are read
// with wave-uniform indices (scalar loads), all R x S x 16 taps unrolled.
constexpr int STEM_TH = 16, STEM_TW = 64, STEM_K = 16, STEM_MAXR = 7, STEM_CAP = 2048;

// 16 channels of one pixel (32 B bf16 / 64 B fp32) from LDS -> fp32
__device__ __forceinline__ void unpack16(const uint16_t* p, float* f) {
  const u32x4 a = *reinterpret_cast<const u32x4*>(p), b = *reinterpret_cast<const u32x4*>(p + 8);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(a[i] << 16);
    f[2 * i + 1] = __uint_as_float(a[i] & 0xffff0000u);
    f[8 + 2 * i] = __uint_as_float(b[i] << 16);
    f[8 + 2 * i + 1] = __uint_as_float(b[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void unpack16(const float* p, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f4 v = *reinterpret_cast<const f4*>(p + 4 * i);
    f[4 * i] = v[0]; f[4 * i + 1] = v[1]; f[4 * i + 2] = v[2]; f[4 * i + 3] = v[3];
  }
}
__device__ __forceinline__ void store16(uint16_t* d, const float* f) {
  u32x4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = (unsigned)f2bf(f[2 * i]) | ((unsigned)f2bf(f[2 * i + 1]) << 16);
    b[i] = (unsigned)f2bf(f[8 + 2 * i]) | ((unsigned)f2bf(f[8 + 2 * i + 1]) << 16);
  }
  *reinterpret_cast<u32x4*>(d) = a;
  *reinterpret_cast<u32x4*>(d + 8) = b;
}
__device__ __forceinline__ void store16(float* d, const float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f4 v = {f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]};
    *reinterpret_cast<f4*>(d + 4 * i) = v;
  }
}

// x halo tile (single channel) -> fp32 LDS, zero outside the image.
template <typename TI, int XH, int XW>
__device__ __forceinline__ void stem_load_x(const TI* __restrict__ x, int n, int H, int W, int gh0, int gw0,
                                            float* xs) {
  for (int i = threadIdx.x; i < XH * XW; i += 256) {
    const int yy = i / XW, xx = i - (i / XW) * XW;
    const int h = gh0 + yy, w = gw0 + xx;
    float v = 0.f;
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) v = to_f(x[((long long)n * H + h) * W + w]);
    xs[i] = v;
  }
}

// Folded weights are laid out weff[r][s][k] (RSK): the 16 weights of one tap
// are one 64 B scalar load, used as SGPR operands of v_fmac.
template <typename TI, typename TO, int R, int S>
__global__ void __launch_bounds__(256)
k_stem_fwd(const TI* __restrict__ x, int N, int H, int W, int pt, int pl,
           const float* __restrict__ weff, const float* __restrict__ bias, TO* __restrict__ y,
           double* __restrict__ stats, int tiles_h, int tiles_w) {
  constexpr int XH = STEM_TH + R - 1, XW = STEM_TW + S - 1, RH = 4 + R - 1;
  __shared__ float xs[XH * XW];
  __shared__ double red[4][2][STEM_K];
  const int tid = threadIdx.x, ox = tid & 63, q = tid >> 6;
  const long long ntiles = (long long)N * tiles_h * tiles_w;
  double s1[STEM_K], s2[STEM_K];
#pragma unroll
  for (int k = 0; k < STEM_K; ++k) s1[k] = 0.0, s2[k] = 0.0;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int tw = (int)(t % tiles_w);
    const int th = (int)((t / tiles_w) % tiles_h);
    const int n = (int)(t / ((long long)tiles_w * tiles_h));
    const int h0 = th * STEM_TH, w0 = tw * STEM_TW;
    __syncthreads();
    stem_load_x<TI, XH, XW>(x, n, H, W, h0 - pt, w0 - pl, xs);
    __syncthreads();
    float acc[4][STEM_K];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < STEM_K; ++k) acc[j][k] = bias ? bias[k] : 0.f;
    // column s of the thread's halo: RH values; output row j uses halo row j + r
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      float xc[RH];
#pragma unroll
      for (int i = 0; i < RH; ++i) xc[i] = xs[(4 * q + i) * XW + ox + s];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float* wt = weff + (r * S + s) * STEM_K;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < STEM_K; ++k) acc[j][k] += xc[j + r] * wt[k];
      }
    }
    const int w = w0 + ox;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = h0 + 4 * q + j;
      if (h < H && w < W) {
        float o[STEM_K];
#pragma unroll
        for (int k = 0; k < STEM_K; ++k) o[k] = to_f(cvt_out(acc[j][k], TO()));  // stats of stored values
        store16(y + (((long long)n * H + h) * W + w) * STEM_K, o);
        if (stats) {
#pragma unroll
          for (int k = 0; k < STEM_K; ++k) s1[k] += o[k], s2[k] += (double)o[k] * o[k];
        }
      }
    }
  }
  if (stats) {
    const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
    for (int k = 0; k < STEM_K; ++k) {
      const double a = wave_sumd(s1[k]), b = wave_sumd(s2[k]);
      if (lane == 0) red[wid][0][k] = a, red[wid][1][k] = b;
    }
    __syncthreads();
    if (tid < 2 * STEM_K) {
      const int which = tid / STEM_K, k = tid % STEM_K;
      stats[((long long)blockIdx.x * 2 + which) * STEM_K + k] =
          red[0][which][k] + red[1][which][k] + red[2][which][k] + red[3][which][k];
    }
  }
}

// dx[n,h,w] = sum_{k,r,s} dy[n, h + pt - r, w + pl - s, k] * weff[r][s][k]
// dy halo tile kept pixel-major in LDS (16 channels = 32 B per pixel, copied
// with 16 B loads/stores); one tile per block.  Per halo column the thread
// holds its RH x 16 dy values in registers and applies all R taps of that
// column to its 4 output rows.
template <typename TG, typename TO, int R, int S>
__global__ void __launch_bounds__(256)
k_stem_dgrad(const TG* __restrict__ dy, int N, int H, int W, int pt, int pl,
             const float* __restrict__ weff, TO* __restrict__ dx, int tiles_h, int tiles_w) {
  constexpr int XH = STEM_TH + R - 1, XW = STEM_TW + S - 1, RH = 4 + R - 1;
  constexpr int CPP = STEM_K * (int)sizeof(TG) / 16;  // 16 B chunks per pixel
  __shared__ __attribute__((aligned(16))) TG gs[XH * XW * STEM_K];
  const int tid = threadIdx.x, ox = tid & 63, q = tid >> 6;
  const long long t = blockIdx.x;
  const int tw = (int)(t % tiles_w);
  const int th = (int)((t / tiles_w) % tiles_h);
  const int n = (int)(t / ((long long)tiles_w * tiles_h));
  const int h0 = th * STEM_TH, w0 = tw * STEM_TW;
  const int gh0 = h0 - (R - 1 - pt), gw0 = w0 - (S - 1 - pl);
  for (int i = tid; i < XH * XW * CPP; i += 256) {
    const int pos = i / CPP, c = i - (i / CPP) * CPP;
    const int yy = pos / XW, xx = pos - (pos / XW) * XW;
    const int h = gh0 + yy, w = gw0 + xx;
    u32x4 v = {0u, 0u, 0u, 0u};
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
      v = *reinterpret_cast<const u32x4*>(dy + (((long long)n * H + h) * W + w) * STEM_K + c * (16 / (int)sizeof(TG)));
    *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned char*>(gs) + (long long)i * 16) = v;
  }
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // halo row 4q + i, col ox + cc holds dy for output row j with r = j + R-1-i, s = S-1-cc
#pragma unroll 1
  for (int cc = 0; cc < S; ++cc) {
    float g[RH][STEM_K];
#pragma unroll
    for (int i = 0; i < RH; ++i) unpack16(gs + ((4 * q + i) * XW + ox + cc) * STEM_K, g[i]);
    const int s = S - 1 - cc;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float* wt = weff + (r * S + s) * STEM_K;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < STEM_K; ++k) acc[j] += g[j + R - 1 - r][k] * wt[k];
    }
  }
  const int w = w0 + ox;
  if (w < W) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = h0 + 4 * q + j;
      if (h < H) dx[((long long)n * H + h) * W + w] = cvt_out(acc[j], TO());
    }
  }
}

// dweff[k][r][s] partials per block: thread -> (column ox = lane, channels
// 4*kq .. 4*kq+3 with kq = wave), R*S*4 fp32 accumulators over the block's
// tiles, reduced across the wave in double at the end.  The x window of the
// thread (R rows x S cols) slides down the tile in registers.
template <typename TI, typename TG, int R, int S>
__global__ void __launch_bounds__(256)
k_stem_wgrad(const TI* __restrict__ x, const TG* __restrict__ dy, int N, int H, int W, int pt,
             int pl, double* __restrict__ part, int tiles_h, int tiles_w) {
  constexpr int XH = STEM_TH + R - 1, XW = STEM_TW + S - 1;
  __shared__ float xs[XH * XW];
  const int tid = threadIdx.x, ox = tid & 63, kq = tid >> 6;
  float acc[4][R * S];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int i = 0; i < R * S; ++i) acc[kk][i] = 0.f;
  const long long ntiles = (long long)N * tiles_h * tiles_w;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int tw = (int)(t % tiles_w);
    const int th = (int)((t / tiles_w) % tiles_h);
    const int n = (int)(t / ((long long)tiles_w * tiles_h));
    const int h0 = th * STEM_TH, w0 = tw * STEM_TW;
    __syncthreads();
    stem_load_x<TI, XH, XW>(x, n, H, W, h0 - pt, w0 - pl, xs);
    __syncthreads();
    const int w = w0 + ox;
    float win[R][S];
#pragma unroll
    for (int r = 0; r < R - 1; ++r)
#pragma unroll
      for (int s = 0; s < S; ++s) win[r + 1][s] = xs[r * XW + ox + s];
#pragma unroll 1
    for (int oy = 0; oy < STEM_TH; ++oy) {
#pragma unroll
      for (int r = 0; r < R - 1; ++r)
#pragma unroll
        for (int s = 0; s < S; ++s) win[r][s] = win[r + 1][s];
#pragma unroll
      for (int s = 0; s < S; ++s) win[R - 1][s] = xs[(oy + R - 1) * XW + ox + s];
      const int h = h0 + oy;
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if (h < H && w < W) {
        const TG* gp = dy + (((long long)n * H + h) * W + w) * STEM_K + 4 * kq;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) g[kk] = to_f(gp[kk]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) acc[kk][r * S + s] += g[kk] * win[r][s];
    }
  }
  const int lane = tid & 63;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int i = 0; i < R * S; ++i) {
      const double v = wave_sumd((double)acc[kk][i]);
      if (lane == 0) part[(long long)blockIdx.x * STEM_K * R * S + (4 * kq + kk) * R * S + i] = v;
    }
}

// dweff partials [blocks][k][r][s] -> dw[k][r][s][rep] (+beta*dw); one block per tap.
__global__ void k_stem_wgrad_reduce(const double* __restrict__ part, int np, int n, int rep, float beta,
                                    float* __restrict__ dw) {
  __shared__ double red[4];
  const int i = blockIdx.x;
  double s = 0.0;
  for (int j = threadIdx.x; j < np; j += 256) s += part[(long long)j * n + i];
  s = wave_sumd(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x < rep) {
    const double tot = red[0] + red[1] + red[2] + red[3];
    float* d = dw + (long long)i * rep + threadIdx.x;
    *d = beta != 0.f ? *d * beta + (float)tot : (float)tot;
  }
}

// weff[r][s][k] = sum_c w[k][r][s][c]  (folds the identical input channels)
__global__ void k_stem_fold(const float* __restrict__ w, int K, int RS, int rep, float* __restrict__ weff) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < K * RS; i += gridDim.x * 256) {
    const int k = i % K, rs = i / K;
    float s = 0.f;
    for (int c = 0; c < rep; ++c) s += w[((long long)k * RS + rs) * rep + c];
    weff[i] = s;
  }
}

// ---- MFMA stem (bf16 activations; R*S <= 32 taps) -------------------------
// Same tiles (16 rows x 64 columns, grid-stride) and slab contracts as the
// VALU kernels above; the 5x5 taps become the 32-deep reduction of
// v_mfma_f32_16x16x32_bf16 (zero-padded from 25), so the VALU work per pixel
// is an LDS gather instead of 400 FMAs:
//   fwd:   D[k][px] = sum_t weff[t][k] * x[px + off_t]      (A = weights, B = im2col gather)
//   dgrad: D[.][px] = sum_{t,k} dy[px - off_t][k] weff[t][k] (B = 16-B dy reads, 2 taps x 16
//          channels per k-step; the A rows are replicated, one row is the result)
//   wgrad: D[k][t]  = sum_px dy[px][k] * x[px + off_t]      (A = dy chunk read transposed,
//          B = im2col gather; k-dimension = 32 pixels of one row)
// Weights are bf16 (the VALU kernels keep fp32 weights: the fp32 path).
typedef __attribute__((address_space(3))) bf4* stem_lp;

__device__ __forceinline__ unsigned stem_pack2(float a, float b) {
  return (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16);
}

template <int R, int S>
__global__ void __launch_bounds__(256)
k_stem_fwd_mfma(const uint16_t* __restrict__ x, int N, int H, int W, int pt, int pl, const float* __restrict__ weff,
                const float* __restrict__ bias, uint16_t* __restrict__ y, double* __restrict__ stats, int tiles_h,
                int tiles_w) {
  constexpr int XH = STEM_TH + R - 1, XW = STEM_TW + S - 1, NT = R * S;
  static_assert(NT <= 32, "taps");
  __shared__ uint16_t xs[XH * XW];
  __shared__ double red[2][STEM_K];
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, q = lane >> 4, wid = tid >> 6;
  for (int i = tid; i < 2 * STEM_K; i += 256) (&red[0][0])[i] = 0.0;
  uint4 wa;
  int toff[8];
  {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = q * 8 + j;
      v[j] = t < NT ? weff[t * STEM_K + l16] : 0.f;
      toff[j] = t < NT ? (t / S) * XW + (t % S) : 0;
    }
    wa = uint4{stem_pack2(v[0], v[1]), stem_pack2(v[2], v[3]), stem_pack2(v[4], v[5]), stem_pack2(v[6], v[7])};
  }
  float bk[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bk[r] = bias ? bias[q * 4 + r] : 0.f;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  const long long ntiles = (long long)N * tiles_h * tiles_w;
  for (long long tt = blockIdx.x; tt < ntiles; tt += gridDim.x) {
    const int tw = (int)(tt % tiles_w), th = (int)((tt / tiles_w) % tiles_h);
    const int n = (int)(tt / ((long long)tiles_w * tiles_h));
    const int h0 = th * STEM_TH, w0 = tw * STEM_TW;
    __syncthreads();
    for (int i = tid; i < XH * XW; i += 256) {
      const int yy = i / XW, xx = i - yy * XW;
      const int h = h0 - pt + yy, w = w0 - pl + xx;
      xs[i] = ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) ? x[((long long)n * H + h) * W + w] : 0;
    }
    __syncthreads();
#pragma unroll 2
    for (int blk = 0; blk < 16; ++blk) {
      const int ry = wid * 4 + (blk >> 2), cx = (blk & 3) * 16 + l16;
      const uint16_t* src = xs + ry * XW + cx;
      unsigned tv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) tv[j] = (q * 8 + j < NT) ? src[toff[j]] : 0u;
      const uint4 b = uint4{tv[0] | (tv[1] << 16), tv[2] | (tv[3] << 16), tv[4] | (tv[5] << 16), tv[6] | (tv[7] << 16)};
      const f4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, wa), __builtin_bit_cast(bf8, b),
                                                             f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      const int h = h0 + ry, w = w0 + cx;
      if (h < H && w < W) {
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = bf2f(f2bf(acc[r] + bk[r]));
        *reinterpret_cast<uint2*>(y + (((long long)n * H + h) * W + w) * STEM_K + q * 4) =
            uint2{stem_pack2(o[0], o[1]), stem_pack2(o[2], o[3])};
        if (stats) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s1[r] += o[r], s2[r] += (double)o[r] * o[r];
        }
      }
    }
  }
  if (stats) {
    // lanes with the same q hold the same 4 channels: reduce over l16
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        s1[r] += __shfl_xor(s1[r], o, 64);
        s2[r] += __shfl_xor(s2[r], o, 64);
      }
    }
    __syncthreads();
    if (l16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        atomicAdd(&red[0][q * 4 + r], s1[r]);
        atomicAdd(&red[1][q * 4 + r], s2[r]);
      }
    }
    __syncthreads();
    if (tid < 2 * STEM_K) stats[(long long)blockIdx.x * 2 * STEM_K + tid] = (&red[0][0])[tid];
  }
}

template <int R, int S>
__global__ void __launch_bounds__(256)
k_stem_dgrad_mfma(const uint16_t* __restrict__ dy, int N, int H, int W, int pt, int pl,
                  const float* __restrict__ weff, uint16_t* __restrict__ dx, int tiles_h, int tiles_w) {
  constexpr int XH = STEM_TH + R - 1, XW = STEM_TW + S - 1, NT = R * S, NKT = (NT + 1) / 2;
  __shared__ __attribute__((aligned(16))) uint16_t gs[XH * XW * STEM_K];
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, q = lane >> 4, wid = tid >> 6;
  // k-step kt: k-slot q*8 + j <-> (tap 2kt + (q >> 1), channel (q & 1)*8 + j); A rows replicated
  uint4 wa[NKT];
  int goff[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const int t = 2 * kt + (q >> 1), r = t / S, s = t % S;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t < NT ? weff[t * STEM_K + (q & 1) * 8 + j] : 0.f;
    wa[kt] = uint4{stem_pack2(v[0], v[1]), stem_pack2(v[2], v[3]), stem_pack2(v[4], v[5]), stem_pack2(v[6], v[7])};
    goff[kt] = t < NT ? ((R - 1 - r) * XW + (S - 1 - s)) * STEM_K + (q & 1) * 8 : -1;
  }
  const uint4 z4 = {0u, 0u, 0u, 0u};
  const long long ntiles = (long long)N * tiles_h * tiles_w;
  for (long long tt = blockIdx.x; tt < ntiles; tt += gridDim.x) {
    const int tw = (int)(tt % tiles_w), th = (int)((tt / tiles_w) % tiles_h);
    const int n = (int)(tt / ((long long)tiles_w * tiles_h));
    const int h0 = th * STEM_TH, w0 = tw * STEM_TW;
    const int gh0 = h0 - (R - 1 - pt), gw0 = w0 - (S - 1 - pl);
    __syncthreads();
    for (int i = tid; i < XH * XW * 2; i += 256) {
      const int pos = i >> 1, c = i & 1;
      const int yy = pos / XW, xx = pos - yy * XW;
      const int h = gh0 + yy, w = gw0 + xx;
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
        v = *reinterpret_cast<const u32x4*>(dy + (((long long)n * H + h) * W + w) * STEM_K + c * 8);
      *reinterpret_cast<u32x4*>(gs + (long long)i * 8) = v;
    }
    __syncthreads();
#pragma unroll 2
    for (int blk = 0; blk < 16; ++blk) {
      const int ry = wid * 4 + (blk >> 2), cx = (blk & 3) * 16 + l16;
      const uint16_t* base = gs + (ry * XW + cx) * STEM_K;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const uint4 b = goff[kt] >= 0 ? *reinterpret_cast<const uint4*>(base + goff[kt]) : z4;
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, wa[kt]), __builtin_bit_cast(bf8, b), acc,
                                                      0, 0, 0);
      }
      const int h = h0 + ry, w = w0 + cx;
      if (q == 0 && h < H && w < W) dx[((long long)n * H + h) * W + w] = f2bf(acc[0]);
    }
  }
}

template <int R, int S>
__global__ void __launch_bounds__(256)
k_stem_wgrad_mfma(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, int N, int H, int W, int pt,
                  int pl, double* __restrict__ part, int tiles_h, int tiles_w) {
  constexpr int XH = STEM_TH + R - 1, XW = STEM_TW + S - 1, NT = R * S, LDG = 24;
  __shared__ uint16_t xs[XH * XW];
  __shared__ __attribute__((aligned(16))) uint16_t gch[4][32 * LDG];  // per wave: 32 px x 16 ch of dy
  __shared__ float red[4][STEM_K][32];
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, q = lane >> 4, wid = tid >> 6;
  const int grp = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  // B k-slot (q, j) <-> chunk pixel j<4: 4q+j, else 16+4q+(j-4) (the transposed-read order)
  int tof0, tof1;
  {
    const int t0 = l16, t1 = 16 + l16;
    tof0 = t0 < NT ? (t0 / S) * XW + (t0 % S) : -1;
    tof1 = t1 < NT ? (t1 / S) * XW + (t1 % S) : -1;
  }
  f4 d0 = f4{0.f, 0.f, 0.f, 0.f}, d1 = d0;
  uint16_t* gw = gch[wid];
  const long long ntiles = (long long)N * tiles_h * tiles_w;
  for (long long tt = blockIdx.x; tt < ntiles; tt += gridDim.x) {
    const int tw = (int)(tt % tiles_w), th = (int)((tt / tiles_w) % tiles_h);
    const int n = (int)(tt / ((long long)tiles_w * tiles_h));
    const int h0 = th * STEM_TH, w0 = tw * STEM_TW;
    __syncthreads();
    for (int i = tid; i < XH * XW; i += 256) {
      const int yy = i / XW, xx = i - yy * XW;
      const int h = h0 - pt + yy, w = w0 - pl + xx;
      xs[i] = ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) ? x[((long long)n * H + h) * W + w] : 0;
    }
    __syncthreads();
    for (int c = 0; c < 8; ++c) {  // the wave's 4 rows x 64 columns in 32-pixel chunks
      const int ry = wid * 4 + (c >> 1), cx0 = (c & 1) * 32;
      const int h = h0 + ry;
      {
        const int px = lane >> 1, half = lane & 1, w = w0 + cx0 + px;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (h < H && w < W)
          v = *reinterpret_cast<const u32x4*>(dy + (((long long)n * H + h) * W + w) * STEM_K + half * 8);
        *reinterpret_cast<u32x4*>(gw + px * LDG + half * 8) = v;
      }
      const bf4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (stem_lp)(reinterpret_cast<const __bf16*>(gw + (4 * grp + qq) * LDG + 4 * pp)));
      const bf4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (stem_lp)(reinterpret_cast<const __bf16*>(gw + (16 + 4 * grp + qq) * LDG + 4 * pp)));
      const bf8 a = bf8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      const uint16_t* src = xs + ry * XW + cx0;
      unsigned b0[8], b1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int px = j < 4 ? 4 * q + j : 16 + 4 * q + (j - 4);
        b0[j] = tof0 >= 0 ? src[px + tof0] : 0u;
        b1[j] = tof1 >= 0 ? src[px + tof1] : 0u;
      }
      const uint4 B0 = uint4{b0[0] | (b0[1] << 16), b0[2] | (b0[3] << 16), b0[4] | (b0[5] << 16), b0[6] | (b0[7] << 16)};
      const uint4 B1 = uint4{b1[0] | (b1[1] << 16), b1[2] | (b1[3] << 16), b1[4] | (b1[5] << 16), b1[6] | (b1[7] << 16)};
      d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf8, B0), d0, 0, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf8, B1), d1, 0, 0, 0);
    }
  }
  // D lane: row k = q*4 + r, column t = l16 (+16)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[wid][q * 4 + r][l16] = d0[r];
    red[wid][q * 4 + r][16 + l16] = d1[r];
  }
  __syncthreads();
  for (int i = tid; i < STEM_K * NT; i += 256) {
    const int k = i / NT, t = i - k * NT;
    part[(long long)blockIdx.x * STEM_K * NT + i] =
        ((double)red[0][k][t] + (double)red[1][k][t]) + ((double)red[2][k][t] + (double)red[3][k][t]);
  }
}


// ------------------------------------------------------------------ stem backward with the BN backward apply
// wr_resnet_bird's stem conv1_1 (5 x 5, 16 filters, bias) -> BatchNormalization
// -> MaxPool2D((1, 2)) (resnet/wr_resnet_bird.py:22-30).  The BN backward's
// elementwise pass dX_bn = a*g*[x*scale+shift > 0] + b*x + c (k_bn_bwd_apply8:
// reads g and x, writes dX_bn, 3 x 1.07 GB per T1 step) is formed while the
// stem dgrad stages its dY halo; the weight gradient and the conv-bias sums
// read the same LDS image, so dX_bn is never stored and the separate wgrad's
// re-read of it is gone.  dX bit-identical to the apply8 -> k_stem_dgrad_mfma
// chain (the same bf16 dX_bn and MFMA operands); dW the k_stem_wgrad_mfma
// arithmetic over stem_bwd_grid's workgroups (its fp32 partials summed in
// another grouping than acfe_stem_wgrad's); bias sums [block][2][16] of the
// bf16 dX_bn values over each tile's own pixels.
template <int R, int S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3)))
k_stem_bwd_bn(const uint16_t* __restrict__ g, const uint16_t* __restrict__ xb, const uint16_t* __restrict__ xin,
              int N, int H, int W, int pt, int pl, const float* __restrict__ weff, const float* __restrict__ scale,
              const float* __restrict__ shift, const float* __restrict__ coef, int relu, uint16_t* __restrict__ dxin,
              double* __restrict__ wpart, double* __restrict__ bpart, int tiles_h, int tiles_w) {
  constexpr int XH = STEM_TH + R - 1, XW = STEM_TW + S - 1, NT = R * S, NKT = (NT + 1) / 2;
  constexpr int GSZ = XH * XW * STEM_K;
  static_assert(GSZ * 2 >= 4 * STEM_K * 32 * 4, "the wgrad reduction aliases the dY image");
  __shared__ __attribute__((aligned(16))) uint16_t gs[GSZ];
  __shared__ uint16_t xs[XH * XW];
  __shared__ double bred[4][STEM_K];
  __shared__ __attribute__((aligned(16))) float bnc[5][STEM_K];  // scale, shift, coef a, b, c
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, q = lane >> 4, wid = tid >> 6;
  if (tid < 5 * STEM_K) {
    const int a = tid / STEM_K, k = tid - a * STEM_K;
    bnc[a][k] = a == 0 ? scale[k] : (a == 1 ? shift[k] : coef[(a - 2) * STEM_K + k]);
  }
  // dgrad A operand (k_stem_dgrad_mfma): flipped folded weights, k-slot q*8 + j <-> (tap 2kt + (q >> 1), ch (q & 1)*8 + j)
  uint4 wa[NKT];
  int goff[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const int t = 2 * kt + (q >> 1), r = t / S, s = t % S;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t < NT ? weff[t * STEM_K + (q & 1) * 8 + j] : 0.f;
    wa[kt] = uint4{stem_pack2(v[0], v[1]), stem_pack2(v[2], v[3]), stem_pack2(v[4], v[5]), stem_pack2(v[6], v[7])};
    goff[kt] = t < NT ? ((R - 1 - r) * XW + (S - 1 - s)) * STEM_K + (q & 1) * 8 : -1;
  }
  // wgrad B operand (k_stem_wgrad_mfma): tap of column l16 / 16 + l16
  const int grp = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  int tof0, tof1;
  {
    const int t0 = l16, t1 = 16 + l16;
    tof0 = t0 < NT ? (t0 / S) * XW + (t0 % S) : -1;
    tof1 = t1 < NT ? (t1 / S) * XW + (t1 % S) : -1;
  }
  // this thread's 8 staging channels: its index parity
  const int c8 = (tid & 1) * 8;
  double s1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = 0.0;
  f4 d0 = f4{0.f, 0.f, 0.f, 0.f}, d1 = d0;
  const uint4 z4 = {0u, 0u, 0u, 0u};
  const long long ntiles = (long long)N * tiles_h * tiles_w;
  for (long long tt = blockIdx.x; tt < ntiles; tt += gridDim.x) {
    const int tw = (int)(tt % tiles_w), th = (int)((tt / tiles_w) % tiles_h);
    const int n = (int)(tt / ((long long)tiles_w * tiles_h));
    const int h0 = th * STEM_TH, w0 = tw * STEM_TW;
    const int gh0 = h0 - (R - 1 - pt), gw0 = w0 - (S - 1 - pl);
    __syncthreads();
    for (int i = tid; i < XH * XW * 2; i += 256) {
      const int pos = i >> 1;
      const int yy = pos / XW, xx = pos - yy * XW;
      const int h = gh0 + yy, w = gw0 + xx;
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
        const long long e = (((long long)n * H + h) * W + w) * STEM_K + c8;
        const u32x4 gv = *reinterpret_cast<const u32x4*>(g + e);
        const u32x4 xv = *reinterpret_cast<const u32x4*>(xb + e);
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned gw = gv[j >> 1], xw = xv[j >> 1];
          const float gf = __uint_as_float((j & 1) ? (gw & 0xffff0000u) : (gw << 16));
          const float xf = __uint_as_float((j & 1) ? (xw & 0xffff0000u) : (xw << 16));
          const float gj = (relu && !(xf * bnc[0][c8 + j] + bnc[1][c8 + j] > 0.f)) ? 0.f : gf;
          o[j] = __builtin_fmaf(bnc[2][c8 + j], gj, __builtin_fmaf(bnc[3][c8 + j], xf, bnc[4][c8 + j]));  // as k_bn_bwd_apply8
        }
        v = u32x4{stem_pack2(o[0], o[1]), stem_pack2(o[2], o[3]), stem_pack2(o[4], o[5]), stem_pack2(o[6], o[7])};
        if ((unsigned)(yy - (R - 1 - pt)) < (unsigned)STEM_TH && (unsigned)(xx - (S - 1 - pl)) < (unsigned)STEM_TW) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const unsigned vw = v[j >> 1];
            s1[j] += (double)__uint_as_float((j & 1) ? (vw & 0xffff0000u) : (vw << 16));
          }
        }
      }
      *reinterpret_cast<u32x4*>(gs + (long long)i * 8) = v;
    }
    for (int i = tid; i < XH * XW; i += 256) {
      const int yy = i / XW, xx = i - yy * XW;
      const int h = h0 - pt + yy, w = w0 - pl + xx;
      xs[i] = ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) ? xin[((long long)n * H + h) * W + w] : 0;
    }
    __syncthreads();
    // dX of the stem input (k_stem_dgrad_mfma)
#pragma unroll 2
    for (int blk = 0; blk < 16; ++blk) {
      const int ry = wid * 4 + (blk >> 2), cx = (blk & 3) * 16 + l16;
      const uint16_t* base = gs + (ry * XW + cx) * STEM_K;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const uint4 b = goff[kt] >= 0 ? *reinterpret_cast<const uint4*>(base + goff[kt]) : z4;
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, wa[kt]), __builtin_bit_cast(bf8, b), acc,
                                                      0, 0, 0);
      }
      const int h = h0 + ry, w = w0 + cx;
      if (q == 0 && h < H && w < W) dxin[((long long)n * H + h) * W + w] = f2bf(acc[0]);
    }
    // dW (k_stem_wgrad_mfma): dY^T chunks read from the tile's own pixels of the image
    for (int c = 0; c < 8; ++c) {
      const int ry = wid * 4 + (c >> 1), cx0 = (c & 1) * 32;
      const uint16_t* gw = gs + ((ry + R - 1 - pt) * XW + cx0 + S - 1 - pl) * STEM_K;
      const bf4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (stem_lp)(reinterpret_cast<const __bf16*>(gw + (4 * grp + qq) * STEM_K + 4 * pp)));
      const bf4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (stem_lp)(reinterpret_cast<const __bf16*>(gw + (16 + 4 * grp + qq) * STEM_K + 4 * pp)));
      const bf8 a = bf8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      const uint16_t* src = xs + ry * XW + cx0;
      unsigned b0[8], b1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int px = j < 4 ? 4 * q + j : 16 + 4 * q + (j - 4);
        b0[j] = tof0 >= 0 ? src[px + tof0] : 0u;
        b1[j] = tof1 >= 0 ? src[px + tof1] : 0u;
      }
      const uint4 B0 = uint4{b0[0] | (b0[1] << 16), b0[2] | (b0[3] << 16), b0[4] | (b0[5] << 16), b0[6] | (b0[7] << 16)};
      const uint4 B1 = uint4{b1[0] | (b1[1] << 16), b1[2] | (b1[3] << 16), b1[4] | (b1[5] << 16), b1[6] | (b1[7] << 16)};
      d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf8, B0), d0, 0, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf8, B1), d1, 0, 0, 0);
    }
  }
  // bias sums: lanes of one parity hold the same 8 channels
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int o = 2; o < 64; o <<= 1) s1[j] += __shfl_xor(s1[j], o, 64);
  }
  __syncthreads();  // last tile's image reads done: the wgrad reduction reuses it
  float(*red)[STEM_K][32] = reinterpret_cast<float(*)[STEM_K][32]>(gs);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[wid][q * 4 + r][l16] = d0[r];
    red[wid][q * 4 + r][16 + l16] = d1[r];
  }
  if (lane < 2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) bred[wid][lane * 8 + j] = s1[j];
  }
  __syncthreads();
  for (int i = tid; i < STEM_K * NT; i += 256) {
    const int k = i / NT, t = i - k * NT;
    wpart[(long long)blockIdx.x * STEM_K * NT + i] =
        ((double)red[0][k][t] + (double)red[1][k][t]) + ((double)red[2][k][t] + (double)red[3][k][t]);
  }
  // row 1 of the [2][16] slab (sums of squares in the statistics layout) is not used by the channel sums
  if (tid < 2 * STEM_K)
    bpart[(long long)blockIdx.x * 2 * STEM_K + tid] =
        tid < STEM_K ? (bred[0][tid] + bred[1][tid]) + (bred[2][tid] + bred[3][tid]) : 0.0;
}

ACFE_API int acfe_stem_blocks(int N, int H, int W) {
  const long long t = (long long)N * ((H + STEM_TH - 1) / STEM_TH) * ((W + STEM_TW - 1) / STEM_TW);
  return (int)(t < STEM_CAP ? t : STEM_CAP);
}

// weff[r][s][k] = sum_c w[k][r][s][c]  (folds the identical input channels)
ACFE_API int acfe_stem_fold_weights(const float* w, int K, int R, int S, int C, float* weff, void* stream) {
  if (!w || !weff || K != STEM_K || R > STEM_MAXR || S > STEM_MAXR || C <= 0) return ACFE_E_INVAL;
  hipLaunchKernelGGL(k_stem_fold, dim3(cdiv(K * R * S, 256)), dim3(256), 0, strm(stream), w, K, R * S, C, weff);
  return launch_rc("acfe_stem_fold_weights");
}

ACFE_API int acfe_stem_fwd(const void* x, int x_dtype, int N, int H, int W, int R, int S, int pad_top,
                           int pad_left, const float* weff, const float* bias, void* y, int y_dtype,
                           double* stats_partial, void* stream) {
  if (!x || !weff || !y || N < 0 || H <= 0 || W <= 0 || R != S || (R != 5 && R != 3)) return ACFE_E_INVAL;
  if (N == 0) return ACFE_OK;
  const int th = (H + STEM_TH - 1) / STEM_TH, tw = (W + STEM_TW - 1) / STEM_TW;
  const int grid = acfe_stem_blocks(N, H, W);
#define SF1(TI, TO, RR)                                                                                      \
  hipLaunchKernelGGL((k_stem_fwd<TI, TO, RR, RR>), dim3(grid), dim3(256), 0, strm(stream), (const TI*)x, N, H, W, \
                     pad_top, pad_left, weff, bias, (TO*)y, stats_partial, th, tw)
#define SF(TI, TO) if (R == 5) SF1(TI, TO, 5); else SF1(TI, TO, 3)
  if (x_dtype == ACFE_DTYPE_BF16 && y_dtype == ACFE_DTYPE_BF16) {
    // one resident round (7 workgroups per CU at 62 VGPRs) instead of 2048 in
    // 1.14 rounds; the statistics slab rows past the grid are zeroed
    const int g1 = grid < 7 * 256 ? grid : 7 * 256;
    if (stats_partial && g1 < grid) {
      const hipError_t e = hipMemsetAsync(stats_partial + (size_t)g1 * 2 * STEM_K, 0,
                                          sizeof(double) * 2 * STEM_K * (grid - g1), strm(stream));
      if (e != hipSuccess) return hip_rc(e, "acfe_stem_fwd");
    }
    if (R == 5)
      hipLaunchKernelGGL((k_stem_fwd_mfma<5, 5>), dim3(g1), dim3(256), 0, strm(stream), (const uint16_t*)x, N, H, W,
                         pad_top, pad_left, weff, bias, (uint16_t*)y, stats_partial, th, tw);
    else
      hipLaunchKernelGGL((k_stem_fwd_mfma<3, 3>), dim3(g1), dim3(256), 0, strm(stream), (const uint16_t*)x, N, H, W,
                         pad_top, pad_left, weff, bias, (uint16_t*)y, stats_partial, th, tw);
  } else if (x_dtype == ACFE_DTYPE_BF16 && y_dtype == ACFE_DTYPE_BF16) SF(uint16_t, uint16_t);
  else if (x_dtype == ACFE_DTYPE_BF16) SF(uint16_t, float);
  else if (y_dtype == ACFE_DTYPE_BF16) SF(float, uint16_t);
  else SF(float, float);
#undef SF
  return launch_rc("acfe_stem_fwd");
}

ACFE_API int acfe_stem_dgrad(const void* dy, int dy_dtype, int N, int H, int W, int R, int S, int pad_top,
                             int pad_left, const float* weff, void* dx, int dx_dtype, void* stream) {
  if (!dy || !weff || !dx || N < 0 || R != S || (R != 5 && R != 3)) return ACFE_E_INVAL;
  if (N == 0) return ACFE_OK;
  const int th = (H + STEM_TH - 1) / STEM_TH, tw = (W + STEM_TW - 1) / STEM_TW;
  const long long grid = (long long)N * th * tw;  // one tile per block
#define SD1(TG, TO, RR)                                                                                      \
  hipLaunchKernelGGL((k_stem_dgrad<TG, TO, RR, RR>), dim3(grid), dim3(256), 0, strm(stream), (const TG*)dy, N, H, \
                     W, pad_top, pad_left, weff, (TO*)dx, th, tw)
#define SD(TG, TO) if (R == 5) SD1(TG, TO, 5); else SD1(TG, TO, 3)
  if (dy_dtype == ACFE_DTYPE_BF16 && dx_dtype == ACFE_DTYPE_BF16) {
    const int g2 = acfe_stem_blocks(N, H, W);
    if (R == 5)
      hipLaunchKernelGGL((k_stem_dgrad_mfma<5, 5>), dim3(g2), dim3(256), 0, strm(stream), (const uint16_t*)dy, N, H,
                         W, pad_top, pad_left, weff, (uint16_t*)dx, th, tw);
    else
      hipLaunchKernelGGL((k_stem_dgrad_mfma<3, 3>), dim3(g2), dim3(256), 0, strm(stream), (const uint16_t*)dy, N, H,
                         W, pad_top, pad_left, weff, (uint16_t*)dx, th, tw);
  } else if (dy_dtype == ACFE_DTYPE_BF16 && dx_dtype == ACFE_DTYPE_BF16) SD(uint16_t, uint16_t);
  else if (dy_dtype == ACFE_DTYPE_BF16) SD(uint16_t, float);
  else if (dx_dtype == ACFE_DTYPE_BF16) SD(float, uint16_t);
  else SD(float, float);
#undef SD
  return launch_rc("acfe_stem_dgrad");
}

// Workgroups of k_stem_bwd_bn: one resident round (3 per CU: 168 VGPRs, 46 KB
// of LDS) each walking its share of the tiles, instead of acfe_stem_blocks'
// 2048 in 2.7 rounds.  <= acfe_stem_blocks, which sizes the workspaces.
static int stem_bwd_grid(int N, int H, int W) {
  static const int cap = getenv("ACFE_STEM_BWD_GRID") ? atoi(getenv("ACFE_STEM_BWD_GRID")) : 768;
  const int nb = acfe_stem_blocks(N, H, W);
  return cap > 0 && cap < nb ? cap : nb;
}

// workspace: double[acfe_stem_blocks(N,H,W) * 16 * R * S]
ACFE_API int acfe_stem_wgrad(const void* x, int x_dtype, const void* dy, int dy_dtype, int N, int H, int W,
                             int R, int S, int pad_top, int pad_left, int rep, float* dw, float beta,
                             double* workspace, void* stream) {
  if (!x || !dy || !dw || !workspace || N <= 0 || R != S || (R != 5 && R != 3) || rep <= 0) return ACFE_E_INVAL;
  const int th = (H + STEM_TH - 1) / STEM_TH, tw = (W + STEM_TW - 1) / STEM_TW;
  const int grid = acfe_stem_blocks(N, H, W);
#define SW1(TI, TG, RR)                                                                                      \
  hipLaunchKernelGGL((k_stem_wgrad<TI, TG, RR, RR>), dim3(grid), dim3(256), 0, strm(stream), (const TI*)x,        \
                     (const TG*)dy, N, H, W, pad_top, pad_left, workspace, th, tw)
#define SW(TI, TG) if (R == 5) SW1(TI, TG, 5); else SW1(TI, TG, 3)
  if (x_dtype == ACFE_DTYPE_BF16 && dy_dtype == ACFE_DTYPE_BF16) {
    if (R == 5)
      hipLaunchKernelGGL((k_stem_wgrad_mfma<5, 5>), dim3(grid), dim3(256), 0, strm(stream), (const uint16_t*)x,
                         (const uint16_t*)dy, N, H, W, pad_top, pad_left, workspace, th, tw);
    else
      hipLaunchKernelGGL((k_stem_wgrad_mfma<3, 3>), dim3(grid), dim3(256), 0, strm(stream), (const uint16_t*)x,
                         (const uint16_t*)dy, N, H, W, pad_top, pad_left, workspace, th, tw);
  } else if (x_dtype == ACFE_DTYPE_BF16 && dy_dtype == ACFE_DTYPE_BF16) SW(uint16_t, uint16_t);
  else if (x_dtype == ACFE_DTYPE_BF16) SW(uint16_t, float);
  else if (dy_dtype == ACFE_DTYPE_BF16) SW(float, uint16_t);
  else SW(float, float);
#undef SW
  int rc = launch_rc("acfe_stem_wgrad");
  if (rc) return rc;
  const int n = STEM_K * R * S;
  if (rep > 256) return ACFE_E_INVAL;
  hipLaunchKernelGGL(k_stem_wgrad_reduce, dim3(n), dim3(256), 0, strm(stream), workspace, grid, n, rep, beta, dw);
  return launch_rc("acfe_stem_wgrad(reduce)");
}

// The stem backward with the BN backward apply folded in (k_stem_bwd_bn): g =
// the BN output gradient (bf16 [N][H][W][16], e.g. acfe_maxpool2d_bwd_argmax_bn's
// dX), xb = the BN input (= the stem output), coef = acfe_bn_bwd_finalize_ex's
// [3][16] coefficients.  dxin: the stem input gradient (bf16 [N][H][W]); dw: [16][R][S][rep] fp32 (beta as acfe_stem_wgrad); bias_part:
// double[acfe_stem_blocks(N,H,W)][2][16] channel sums of dX_bn (for
// acfe_channel_sum_finalize); workspace: double[acfe_stem_blocks(N,H,W) * 16 * R * S].
ACFE_API int acfe_stem_bwd_bn(const void* g, const void* xb, const void* xin, int N, int H, int W, int R, int S,
                              int pad_top, int pad_left, const float* weff, const float* scale, const float* shift,
                              const float* coef, int relu, void* dxin, int rep, float* dw, float beta,
                              double* bias_part, double* workspace, void* stream) {
  if (!g || !xb || !xin || !weff || !scale || !shift || !coef || !dw || !bias_part || !workspace || N <= 0 ||
      H <= 0 || W <= 0 || R != S || (R != 5 && R != 3) || rep <= 0 || rep > 256 || ((uintptr_t)g & 15) ||
      ((uintptr_t)xb & 15))
    return ACFE_E_INVAL;
  const int th = (H + STEM_TH - 1) / STEM_TH, tw = (W + STEM_TW - 1) / STEM_TW;
  const int nb = acfe_stem_blocks(N, H, W), grid = stem_bwd_grid(N, H, W);
  if (grid < nb) {  // bias slab rows past the grid: zero
    const hipError_t e =
        hipMemsetAsync(bias_part + (size_t)grid * 2 * STEM_K, 0, sizeof(double) * 2 * STEM_K * (nb - grid), strm(stream));
    if (e != hipSuccess) return hip_rc(e, "acfe_stem_bwd_bn");
  }
  uint16_t* dxo = (uint16_t*)dxin;
  if (!dxo) return ACFE_E_INVAL;
#define SB(RR)                                                                                                \
  hipLaunchKernelGGL((k_stem_bwd_bn<RR, RR>), dim3(grid), dim3(256), 0, strm(stream), (const uint16_t*)g,        \
                     (const uint16_t*)xb, (const uint16_t*)xin, N, H, W, pad_top, pad_left, weff, scale, shift, coef, \
                     relu, dxo, workspace, bias_part, th, tw)
  if (R == 5) SB(5); else SB(3);
#undef SB
  int rc = launch_rc("acfe_stem_bwd_bn");
  if (rc) return rc;
  const int n = STEM_K * R * S;
  hipLaunchKernelGGL(k_stem_wgrad_reduce, dim3(n), dim3(256), 0, strm(stream), workspace, grid, n, rep, beta, dw);
  return launch_rc("acfe_stem_bwd_bn(reduce)");
}
