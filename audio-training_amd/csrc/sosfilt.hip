// Butterworth band-pass of the tracks of the predict path, on the device:
// acfe_sosfilt_segments is scipy.signal.sosfilt (reference predict_utils.py
// :103-113, :245-262) over many segments of one device-resident recording, each
// with its own two-section filter, written float32 into one packed buffer that
// acfe_windows_normalize then cuts the windows from.
//
// An IIR filter is a linear recurrence.  The two cascaded biquads (transposed
// direct form II, the arithmetic of scipy's _sosfilt) are one linear system
//   z' = M z + B x,   y = C z + D x          z = (p0, p1, q0, q1)
// so a segment is cut into chunks of SF_L samples, one per lane, SF_CH chunks
// (one workgroup, SF_TILE samples) per tile:
//   k_sos_prep    per segment: clamp the descriptor, P_k = (M^L)^(2^k), and the
//                 tile -> segment map
//   k_sos_local   per tile: (a) every lane runs its chunk from a zero state;
//                 the chunk end states are scanned inside each wave
//                 (v[c] = P_k v[c - 2^k] + v[c]) and the four wave totals
//                 combined into the tile's end state from a zero entry
//   k_sos_carry   per segment: tile entry states, in = P_8 in + end, serially
//                 (a tile is 8192 samples: 59 steps for 10 s of audio)
//   k_sos_apply   per tile: (b) the lane's true entry state from the tile
//                 entry, the wave totals and the scanned states; (c) the chunk
//                 again from that state, stored float32
// Everything is float64 until the store.  (c) recomputes instead of keeping a
// float64 copy of the audio; the recording is read twice (the second time from
// L2) and 32 B of state per chunk go through the workspace.
//
// A lane owns SF_L consecutive samples, a stride-SF_L access across the wave,
// so tiles are staged through LDS: coalesced 16-B global loads and stores on
// one side, lanes walking rows of pitch SF_L + 1 dwords on the other (an odd
// pitch: the 32 lanes of a ds_read_b32 group hit 32 banks).
#include "common.h"

using namespace acfe;

namespace {

constexpr int SF_L = 32;                 // samples per lane (chunk); 2^SF_LOG_L
constexpr int SF_LOG_L = 5;
constexpr int SF_CH = 256;               // chunks per tile = threads per workgroup
constexpr int SF_TILE = SF_L * SF_CH;    // samples per tile
constexpr int SF_PITCH = SF_L + 1;       // LDS row pitch in dwords
constexpr int SF_NPOW = 9;               // P_0 .. P_8: in-wave steps 1 .. 32, wave (64), tile (256)
constexpr int64_t SF_SRC_LIM = (int64_t)1 << 62;

// device workspace, carved by sos_ws (every part 64-B aligned)
struct SosWs {
  int64_t* seg;    // [n_seg][4]  clamped {src, len, dst, identity}
  int64_t* tile0;  // [n_seg + 1] first tile of each segment
  double* pw;      // [n_seg][SF_NPOW][16] row-major 4 x 4
  double* tend;    // [max_tiles][4] tile end state from a zero entry
  double* tin;     // [max_tiles][4] tile entry state
  double* chunk;   // [max_tiles][SF_CH][4] chunk end states, scanned within each wave
  int64_t bytes;
};
int64_t up64(int64_t v) { return (v + 63) & ~(int64_t)63; }
int64_t sos_max_tiles(int64_t total_len, int n_seg) { return total_len / SF_TILE + n_seg; }
SosWs sos_ws(void* ws, int64_t total_len, int n_seg) {
  const int64_t mt = sos_max_tiles(total_len, n_seg);
  char* p = static_cast<char*>(ws);
  int64_t o = 0;
  SosWs w;
  w.seg = reinterpret_cast<int64_t*>(p + o), o += up64(32 * (int64_t)n_seg);
  w.tile0 = reinterpret_cast<int64_t*>(p + o), o += up64(8 * ((int64_t)n_seg + 1));
  w.pw = reinterpret_cast<double*>(p + o), o += up64(8 * 16 * SF_NPOW * (int64_t)n_seg);
  w.tend = reinterpret_cast<double*>(p + o), o += up64(32 * mt);
  w.tin = reinterpret_cast<double*>(p + o), o += up64(32 * mt);
  w.chunk = reinterpret_cast<double*>(p + o), o += up64(32 * SF_CH * mt);
  w.bytes = o;
  return w;
}

// the two sections without a0 (== 1)
struct Sos2 {
  double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2;
};
__device__ __forceinline__ Sos2 load_sos(const double* __restrict__ s) {
  return Sos2{s[0], s[1], s[2], s[4], s[5], s[6], s[7], s[8], s[10], s[11]};
}
// one sample through both sections (scipy _sosfilt's loop body)
__device__ __forceinline__ double sos_step(const Sos2& f, double x, double (&z)[4]) {
  const double y1 = f.b0 * x + z[0];
  z[0] = f.b1 * x - f.a1 * y1 + z[1];
  z[1] = f.b2 * x - f.a2 * y1;
  const double y2 = f.c0 * y1 + z[2];
  z[2] = f.c1 * y1 - f.d1 * y2 + z[3];
  z[3] = f.c2 * y1 - f.d2 * y2;
  return y2;
}
// r = A v + r   (A row-major 4 x 4 at a wave-uniform address)
__device__ __forceinline__ void mat_acc(const double* __restrict__ A, const double (&v)[4], double (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] += A[4 * i] * v[0] + A[4 * i + 1] * v[1] + A[4 * i + 2] * v[2] + A[4 * i + 3] * v[3];
}
__device__ __forceinline__ void mat_apply(const double* __restrict__ A, double (&v)[4]) {
  double r[4] = {0, 0, 0, 0};
  mat_acc(A, v, r);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = r[i];
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return min(max(v, lo), hi); }

// One workgroup.  Pass 1: thread k (strided) clamps segment k -- len to
// [0, out_len - dst], or to 0 for a dst outside [0, out_len]; src to +-2^62 so
// that src + i cannot wrap; a source index outside rec[0, rec_len) is read as
// zero later, never dereferenced --, tests for the identity filter and builds the powers of the
// state transition.  Pass 2: the exclusive prefix sum of the tile counts,
// capped at max_tiles (disjoint dst ranges inside out never reach the cap; an
// overlapping table loses its last tiles instead of overrunning the workspace).
__global__ void __launch_bounds__(SF_CH) k_sos_prep(const int64_t* __restrict__ seg, const double* __restrict__ sos,
                                                    int n_seg, int64_t out_len, int64_t max_tiles, SosWs w) {
  __shared__ int64_t cnt[SF_CH];
  __shared__ int64_t carry;
  for (int k = threadIdx.x; k < n_seg; k += SF_CH) {
    const int64_t src = clamp64(seg[3 * k], -SF_SRC_LIM, SF_SRC_LIM);
    const int64_t dst = seg[3 * k + 2];
    const int64_t len = (dst < 0 || dst > out_len) ? 0 : clamp64(seg[3 * k + 1], 0, out_len - dst);
    const double* s = sos + 12 * (int64_t)k;
    bool ident = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) ident = ident && s[j] == ((j == 0 || j == 3 || j == 6 || j == 9) ? 1.0 : 0.0);
    w.seg[4 * k] = src, w.seg[4 * k + 1] = len, w.seg[4 * k + 2] = dst, w.seg[4 * k + 3] = ident;
    // M column j = one step of unit state j with x = 0; then M^L by squaring, then (M^L)^(2^k)
    const Sos2 f = load_sos(s);
    double A[16], B[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double z[4] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, j == 3 ? 1.0 : 0.0};
      sos_step(f, 0.0, z);
#pragma unroll
      for (int i = 0; i < 4; ++i) A[4 * i + j] = z[i];
    }
    double* pw = w.pw + (int64_t)k * SF_NPOW * 16;
    for (int q = 0; q < SF_LOG_L + SF_NPOW; ++q) {
      if (q >= SF_LOG_L)
        for (int i = 0; i < 16; ++i) pw[(q - SF_LOG_L) * 16 + i] = A[i];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
          B[4 * i + j] = A[4 * i] * A[j] + A[4 * i + 1] * A[4 + j] + A[4 * i + 2] * A[8 + j] + A[4 * i + 3] * A[12 + j];
      for (int i = 0; i < 16; ++i) A[i] = B[i];
    }
  }
  if (threadIdx.x == 0) carry = 0, w.tile0[0] = 0;
  __syncthreads();  // also orders pass 1's w.seg stores before the reads below (same workgroup)
  for (int base = 0; base < n_seg; base += SF_CH) {
    const int k = base + threadIdx.x;
    cnt[threadIdx.x] = k < n_seg ? (w.seg[4 * k + 1] + SF_TILE - 1) / SF_TILE : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t c = carry;
      for (int i = 0; i < SF_CH; ++i) c = min(c + cnt[i], max_tiles), cnt[i] = c;
      carry = c;
    }
    __syncthreads();
    if (k < n_seg) w.tile0[k + 1] = cnt[threadIdx.x];
    __syncthreads();
  }
}

// the segment that owns tile b: the last k with tile0[k] <= b (tile0 is
// non-decreasing, empty segments repeat a value), or -1 past the last tile
__device__ __forceinline__ int find_seg(const int64_t* __restrict__ tile0, int n_seg, int64_t b) {
  if (b >= tile0[n_seg]) return -1;
  int lo = 0, hi = n_seg;  // tile0[lo] <= b < tile0[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile0[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int sm_at(int e) { return (e >> SF_LOG_L) * SF_PITCH + (e & (SF_L - 1)); }

// sm <- samples g0 .. g0 + count of rec (zero where the index is outside
// rec[0, rec_len)), zeros up to SF_TILE: 16-B loads from the 16-B lines of the
// actual address, the lines that straddle an end of the recording by element
__device__ __forceinline__ void stage_in(float* __restrict__ sm, const float* __restrict__ rec, int64_t rec_len,
                                         int64_t g0, int count) {
  const int mis = (int)(((int64_t)(reinterpret_cast<uintptr_t>(rec) >> 2) + g0) & 3);
  const int nvec = (mis + count + 3) >> 2;
  for (int q = threadIdx.x; q < nvec; q += SF_CH) {
    const int64_t gi = g0 - mis + 4 * (int64_t)q;
    float v[4];
    if (gi >= 0 && gi + 4 <= rec_len) {
      const float4 t = *reinterpret_cast<const float4*>(rec + gi);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (gi + u >= 0 && gi + u < rec_len) ? rec[gi + u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = 4 * q + u - mis;
      if (e >= 0 && e < count) sm[sm_at(e)] = v[u];
    }
  }
  for (int e = count + threadIdx.x; e < SF_TILE; e += SF_CH) sm[sm_at(e)] = 0.f;
}

// out[o0 .. o0 + count) <- sm, 16-B stores on the 16-B lines of the actual
// address, the two end lines by element; nothing else is written
__device__ __forceinline__ void store_out(const float* __restrict__ sm, float* __restrict__ out, int64_t o0,
                                          int count) {
  const int mis = (int)(((int64_t)(reinterpret_cast<uintptr_t>(out) >> 2) + o0) & 3);
  const int nvec = (mis + count + 3) >> 2;
  for (int q = threadIdx.x; q < nvec; q += SF_CH) {
    const int e0 = 4 * q - mis;
    if (e0 >= 0 && e0 + 4 <= count) {
      *reinterpret_cast<float4*>(out + o0 + e0) =
          make_float4(sm[sm_at(e0)], sm[sm_at(e0 + 1)], sm[sm_at(e0 + 2)], sm[sm_at(e0 + 3)]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u >= 0 && e0 + u < count) out[o0 + e0 + u] = sm[sm_at(e0 + u)];
    }
  }
}

__global__ void __launch_bounds__(SF_CH) k_sos_local(const float* __restrict__ rec, int64_t rec_len,
                                                     const double* __restrict__ sos, int n_seg, SosWs w) {
  __shared__ float sm[SF_CH * SF_PITCH];
  __shared__ double tot[SF_CH / 64][4];
  const int64_t b = blockIdx.x;
  const int k = find_seg(w.tile0, n_seg, b);
  if (k < 0 || w.seg[4 * k + 3]) return;  // identity: k_sos_apply copies
  const int64_t i0 = (b - w.tile0[k]) * SF_TILE;
  const int count = (int)min((int64_t)SF_TILE, w.seg[4 * k + 1] - i0);
  stage_in(sm, rec, rec_len, w.seg[4 * k] + i0, count);
  __syncthreads();

  const Sos2 f = load_sos(sos + 12 * (int64_t)k);
  double z[4] = {0, 0, 0, 0};
  const float* row = sm + threadIdx.x * SF_PITCH;
#pragma unroll 8
  for (int j = 0; j < SF_L; ++j) sos_step(f, (double)row[j], z);

  // inclusive scan inside the wave: z <- end state of this chunk had the wave's first chunk started from zero
  const double* pw = w.pw + (int64_t)k * SF_NPOW * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    double t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = __shfl_up(z[i], 1 << s, 64);
    if (lane >= (1 << s)) mat_acc(pw + 16 * s, t, z);
  }
  double* c = w.chunk + (b * SF_CH + threadIdx.x) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = z[i];
  if (lane == 63)
#pragma unroll
    for (int i = 0; i < 4; ++i) tot[wave][i] = z[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double a[4] = {tot[0][0], tot[0][1], tot[0][2], tot[0][3]};
    for (int v = 1; v < SF_CH / 64; ++v) {
      mat_apply(pw + 16 * 6, a);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] += tot[v][i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) w.tend[4 * b + i] = a[i];
  }
}

__global__ void __launch_bounds__(64) k_sos_carry(int n_seg, SosWs w) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_seg || w.seg[4 * k + 3]) return;
  const double* P = w.pw + ((int64_t)k * SF_NPOW + 8) * 16;
  double a[4] = {0, 0, 0, 0};
  for (int64_t t = w.tile0[k]; t < w.tile0[k + 1]; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w.tin[4 * t + i] = a[i];
    mat_apply(P, a);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] += w.tend[4 * t + i];
  }
}

__global__ void __launch_bounds__(SF_CH) k_sos_apply(const float* __restrict__ rec, int64_t rec_len,
                                                     const double* __restrict__ sos, int n_seg,
                                                     float* __restrict__ out, SosWs w) {
  __shared__ float sm[SF_CH * SF_PITCH];
  const int64_t b = blockIdx.x;
  const int k = find_seg(w.tile0, n_seg, b);
  if (k < 0) return;
  const int64_t i0 = (b - w.tile0[k]) * SF_TILE;
  const int count = (int)min((int64_t)SF_TILE, w.seg[4 * k + 1] - i0);
  stage_in(sm, rec, rec_len, w.seg[4 * k] + i0, count);
  __syncthreads();

  if (!w.seg[4 * k + 3]) {
    const double* pw = w.pw + (int64_t)k * SF_NPOW * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // entry state of the wave's first chunk: the tile's, carried over the waves in front
    double z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = w.tin[4 * b + i];
    for (int v = 0; v < wave; ++v) {
      const double* t = w.chunk + (b * SF_CH + 64 * v + 63) * 4;
      mat_apply(pw + 16 * 6, z);
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] += t[i];
    }
    // ... carried over the `lane` chunks in front inside the wave: (M^L)^lane z + their scanned end state
#pragma unroll
    for (int s = 0; s < 6; ++s)
      if ((lane >> s) & 1) mat_apply(pw + 16 * s, z);
    if (lane) {
      const double* t = w.chunk + (b * SF_CH + threadIdx.x - 1) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] += t[i];
    }
    const Sos2 f = load_sos(sos + 12 * (int64_t)k);
    float* row = sm + threadIdx.x * SF_PITCH;
#pragma unroll 8
    for (int j = 0; j < SF_L; ++j) row[j] = (float)sos_step(f, (double)row[j], z);
    __syncthreads();
  }
  store_out(sm, out, w.seg[4 * k + 2] + i0, count);
}

}  // namespace

ACFE_API int64_t acfe_sosfilt_workspace(int64_t total_len, int n_seg) {
  if (total_len < 0 || n_seg < 0 || total_len >= SF_SRC_LIM || sos_max_tiles(total_len, n_seg) > 0x7FFFFFFF)
    return ACFE_E_INVAL;
  return sos_ws(nullptr, total_len, n_seg).bytes;
}

ACFE_API int acfe_sosfilt_segments(const float* rec, int64_t rec_len, const int64_t* seg, const double* sos,
                                   int n_seg, float* out, int64_t out_len, void* ws, void* stream) {
  if (n_seg == 0 && rec_len >= 0 && out_len >= 0) return ACFE_OK;
  if (!rec || !seg || !sos || !out || !ws || rec_len < 0 || n_seg < 0 || acfe_sosfilt_workspace(out_len, n_seg) < 0)
    return ACFE_E_INVAL;
  const int64_t mt = sos_max_tiles(out_len, n_seg);
  const SosWs w = sos_ws(ws, out_len, n_seg);
  hipLaunchKernelGGL(k_sos_prep, dim3(1), dim3(SF_CH), 0, strm(stream), seg, sos, n_seg, out_len, mt, w);
  hipLaunchKernelGGL(k_sos_local, dim3((unsigned)mt), dim3(SF_CH), 0, strm(stream), rec, rec_len, sos, n_seg, w);
  hipLaunchKernelGGL(k_sos_carry, dim3(cdiv(n_seg, 64)), dim3(64), 0, strm(stream), n_seg, w);
  hipLaunchKernelGGL(k_sos_apply, dim3((unsigned)mt), dim3(SF_CH), 0, strm(stream), rec, rec_len, sos, n_seg, out,
                     w);
  return launch_rc("acfe_sosfilt_segments");
}
