// PCEN's normalize_minmax per segment of a launch (tfpcen.py:105-110 as the
// reference's predict path meets it: predict.py:887 hands one track's windows
// to Keras predict, which normalises every batch of 32 by its own extrema).
// The clips of a launch are split into contiguous segments by a table of
// offsets; each segment is normalised by the min / max of its own elements, so
// that its output is bit-identical to acfe_pcen_normalize run on that
// segment's clips alone, while the launch keeps its full batch.
//
// Three streaming passes over y [batch][clip_elems]:
//   (a) k_seg_slice_minmax  grid (clip, slice of SEG_SLICE elements): min / max
//       of the slice into ws, and the clip's pair reset to {+inf, -inf};
//   (b) k_seg_fold          one wave per segment: folds the slice partials of
//       its clips, writes seg_minmax[s] and the pair of each of its clips;
//   (c) k_seg_norm          grid (clip, slice): 2 * ((y - mn) / (mx - mn)) - 1
//       with the clip's pair, written as fp32 or bf16.
// fminf / fmaxf are exact and order independent, so (a) + (b) give the extrema
// that k_pcen_fwd's row-block partials give; (c) is k_pcen_norm's expression,
// compiled under the same contraction rule.
#include "common.h"

using namespace acfe;

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_SLICE = 16384;  // elements per workgroup: 16 x 16-B loads per thread

// floats in front of p's next 16-byte boundary (p is 4-byte aligned)
__device__ __forceinline__ int to_align16(const float* p) {
  return (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
}

// ws layout (floats): part[batch * nsl][2], then clip[batch][2]
__global__ void __launch_bounds__(SEG_THREADS) k_seg_slice_minmax(const float* __restrict__ y, int64_t ce, int nsl,
                                                                  float* __restrict__ part,
                                                                  float* __restrict__ clip) {
  __shared__ float smn[SEG_THREADS / 64], smx[SEG_THREADS / 64];
  const int64_t b = blockIdx.x / nsl;
  const int k = blockIdx.x % nsl;
  const int64_t e0 = (int64_t)k * SEG_SLICE;
  const int len = (int)min((int64_t)SEG_SLICE, ce - e0);
  const float* p = y + b * ce + e0;  // p[0 .. len) is inside clip b
  float mn[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const int head = min(len, to_align16(p));
  const int nv = (len - head) >> 2;
  const float4* xv = reinterpret_cast<const float4*>(p + head);
  int i = threadIdx.x;
  for (; i + 3 * SEG_THREADS < nv; i += 4 * SEG_THREADS) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = xv[i + u * SEG_THREADS];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      mn[u] = fminf(fminf(mn[u], v[u].x), fminf(v[u].y, fminf(v[u].z, v[u].w)));
      mx[u] = fmaxf(fmaxf(mx[u], v[u].x), fmaxf(v[u].y, fmaxf(v[u].z, v[u].w)));
    }
  }
  for (; i < nv; i += SEG_THREADS) {
    const float4 v = xv[i];
    mn[0] = fminf(fminf(mn[0], v.x), fminf(v.y, fminf(v.z, v.w)));
    mx[0] = fmaxf(fmaxf(mx[0], v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
  }
  // the scalar ends: at most 3 floats in front of the 16-B body and 3 behind
  const int tail = head + (nv << 2);
  const int e = (int)threadIdx.x < head ? (int)threadIdx.x : tail + (int)threadIdx.x - head;
  if (e < len) {
    const float v = p[e];
    mn[1] = fminf(mn[1], v);
    mx[1] = fmaxf(mx[1], v);
  }
  const float a = wave_min(fminf(fminf(mn[0], mn[1]), fminf(mn[2], mn[3])));
  const float c = wave_max(fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3])));
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = a;
    smx[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    part[2 * (int64_t)blockIdx.x + 1] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    if (k == 0) {  // a clip that no segment covers keeps this pair
      clip[2 * b] = INFINITY;
      clip[2 * b + 1] = -INFINITY;
    }
  }
}

// One wave per segment.  The table entries are clamped to [0, batch] and a
// range that runs backwards is empty, so whatever the table holds only
// part[0, batch * nsl) is read and only clip[0, batch) written (overlapping
// segments of a malformed table race for a clip's pair; either value is in ws).
__global__ void __launch_bounds__(SEG_THREADS) k_seg_fold(const int32_t* __restrict__ seg_start, int n_seg, int batch,
                                                          int nsl, const float* __restrict__ part,
                                                          float* __restrict__ clip, float* __restrict__ seg_minmax) {
  const int s = blockIdx.x * (SEG_THREADS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= n_seg) return;
  const int b0 = min(max(seg_start[s], 0), batch);
  const int b1 = max(min(max(seg_start[s + 1], 0), batch), b0);
  float a = INFINITY, c = -INFINITY;
  for (int64_t i = (int64_t)b0 * nsl + lane; i < (int64_t)b1 * nsl; i += 64) {
    a = fminf(a, part[2 * i]);
    c = fmaxf(c, part[2 * i + 1]);
  }
  a = wave_min(a);
  c = wave_max(c);
  if (lane == 0) {
    seg_minmax[2 * s] = a;
    seg_minmax[2 * s + 1] = c;
  }
  for (int b = b0 + lane; b < b1; b += 64) {
    clip[2 * (int64_t)b] = a;
    clip[2 * (int64_t)b + 1] = c;
  }
}

// k_pcen_norm's expression (tfpcen.py:110), under the same default contraction
__device__ __forceinline__ float seg_norm1(float v, float mn, float d) { return 2.0f * ((v - mn) / d) - 1.0f; }

template <typename T>
__device__ __forceinline__ void seg_store(T* o, float v);
template <>
__device__ __forceinline__ void seg_store<float>(float* o, float v) { *o = v; }
template <>
__device__ __forceinline__ void seg_store<uint16_t>(uint16_t* o, float v) { *o = f2bf(v); }

__device__ __forceinline__ void seg_store4(float* o, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(o) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void seg_store4(uint16_t* o, float a, float b, float c, float d) {
  uint2 w;
  w.x = (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
  w.y = (uint32_t)f2bf(c) | ((uint32_t)f2bf(d) << 16);
  *reinterpret_cast<uint2*>(o) = w;
}

template <typename T>
__global__ void __launch_bounds__(SEG_THREADS) k_seg_norm(const float* __restrict__ y, int64_t ce, int nsl,
                                                          const float* __restrict__ clip, T* __restrict__ out) {
  const int64_t b = blockIdx.x / nsl;
  const int k = blockIdx.x % nsl;
  const int64_t e0 = (int64_t)k * SEG_SLICE;
  const int len = (int)min((int64_t)SEG_SLICE, ce - e0);
  const float* p = y + b * ce + e0;
  T* o = out + b * ce + e0;
  const float mn = clip[2 * b], mx = clip[2 * b + 1];
  const float d = mx - mn;
  const int head = min(len, to_align16(p));
  // 4 elements per store only where the output is aligned for it at the body's first element
  const bool wide = (reinterpret_cast<uintptr_t>(o + head) & (4 * sizeof(T) - 1)) == 0;
  const int nv = wide ? (len - head) >> 2 : 0;
  const float4* xv = reinterpret_cast<const float4*>(p + head);
  int i = threadIdx.x;
  for (; i + 3 * SEG_THREADS < nv; i += 4 * SEG_THREADS) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = xv[i + u * SEG_THREADS];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      seg_store4(o + head + 4 * (i + u * SEG_THREADS), seg_norm1(v[u].x, mn, d), seg_norm1(v[u].y, mn, d),
                 seg_norm1(v[u].z, mn, d), seg_norm1(v[u].w, mn, d));
  }
  for (; i < nv; i += SEG_THREADS) {
    const float4 v = xv[i];
    seg_store4(o + head + 4 * i, seg_norm1(v.x, mn, d), seg_norm1(v.y, mn, d), seg_norm1(v.z, mn, d),
               seg_norm1(v.w, mn, d));
  }
  // the scalar ends (everything behind the head when the output is not aligned)
  const int tail = head + (nv << 2);
  for (int e = threadIdx.x; e < head; e += SEG_THREADS) seg_store<T>(o + e, seg_norm1(p[e], mn, d));
  for (int e = tail + threadIdx.x; e < len; e += SEG_THREADS) seg_store<T>(o + e, seg_norm1(p[e], mn, d));
}

inline int seg_slices(int64_t clip_elems) { return (int)((clip_elems + SEG_SLICE - 1) / SEG_SLICE); }

// batch * slices as a grid size, or 0 when it does not fit one
inline int64_t seg_grid(int batch, int64_t clip_elems) {
  if (batch <= 0 || clip_elems <= 0 || clip_elems > ((int64_t)1 << 40)) return 0;
  const int64_t g = (int64_t)batch * ((clip_elems + SEG_SLICE - 1) / SEG_SLICE);
  return g <= 0x7fffffff ? g : 0;
}

}  // namespace

ACFE_API int64_t acfe_pcen_segments_workspace(int batch, int64_t clip_elems) {
  const int64_t g = seg_grid(batch, clip_elems);
  if (g == 0) return ACFE_E_INVAL;
  return (int64_t)sizeof(float) * 2 * (g + batch);
}

ACFE_API int acfe_pcen_normalize_segments(const float* y, int batch, int64_t clip_elems, const int32_t* seg_start,
                                          int n_seg, void* out, int out_dtype, float* seg_minmax, void* ws,
                                          void* stream) {
  const int64_t g = seg_grid(batch, clip_elems);
  if (!y || !seg_start || !out || !seg_minmax || !ws || g == 0 || n_seg <= 0 || n_seg > batch ||
      (out_dtype != ACFE_DTYPE_F32 && out_dtype != ACFE_DTYPE_BF16))
    return ACFE_E_INVAL;
  const int nsl = seg_slices(clip_elems);
  float* part = reinterpret_cast<float*>(ws);
  float* clip = part + 2 * g;
  hipLaunchKernelGGL(k_seg_slice_minmax, dim3((unsigned)g), dim3(SEG_THREADS), 0, strm(stream), y, clip_elems, nsl,
                     part, clip);
  int rc = launch_rc("acfe_pcen_normalize_segments");
  if (rc) return rc;
  hipLaunchKernelGGL(k_seg_fold, dim3(cdiv(n_seg, SEG_THREADS / 64)), dim3(SEG_THREADS), 0, strm(stream), seg_start,
                     n_seg, batch, nsl, part, clip, seg_minmax);
  rc = launch_rc("acfe_pcen_normalize_segments");
  if (rc) return rc;
  if (out_dtype == ACFE_DTYPE_BF16)
    hipLaunchKernelGGL(k_seg_norm<uint16_t>, dim3((unsigned)g), dim3(SEG_THREADS), 0, strm(stream), y, clip_elems,
                       nsl, clip, reinterpret_cast<uint16_t*>(out));
  else
    hipLaunchKernelGGL(k_seg_norm<float>, dim3((unsigned)g), dim3(SEG_THREADS), 0, strm(stream), y, clip_elems, nsl,
                       clip, reinterpret_cast<float*>(out));
  return launch_rc("acfe_pcen_normalize_segments");
}
