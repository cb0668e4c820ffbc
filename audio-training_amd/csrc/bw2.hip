// Eval-mode layer kernels between the convolutions of badwinner2
// (badwinner2.py:212-324):
//   acfe_mag_rownorm  MagTransform (:33-49) + the input BatchNormalization over
//                     the mel axis (axis=1, scale=False, center=False, :233)
//   acfe_leaky_bn     LeakyReLU(alpha) -> BatchNormalization (:236-237 ... :296-297)
//                     and the bare LeakyReLU of :307
//   acfe_softmax      the softmax of :321
// All three are streaming passes: 16-B accesses where the buffers allow them,
// a scalar path otherwise; arithmetic in fp32, one rounding on store.
#include "common.h"

using namespace acfe;

namespace {

template <typename T> __device__ __forceinline__ float ld1(const T* p, long long i);
template <> __device__ __forceinline__ float ld1<uint16_t>(const uint16_t* p, long long i) { return bf2f(p[i]); }
template <> __device__ __forceinline__ float ld1<float>(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ void st1(uint16_t* p, long long i, float v) { p[i] = f2bf(v); }
__device__ __forceinline__ void st1(float* p, long long i, float v) { p[i] = v; }

// 16 bytes of T as floats: 4 fp32 or 8 bf16
template <typename T> struct Vec;
template <> struct Vec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void ld(const float* p, float* f) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* f) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
};
template <> struct Vec<uint16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void ld(const uint16_t* p, float* f) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[2 * j] = __uint_as_float(w[j] << 16);
      f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void st(uint16_t* p, const float* f) {
    uint4 v;
    v.x = (uint32_t)f2bf(f[0]) | ((uint32_t)f2bf(f[1]) << 16);
    v.y = (uint32_t)f2bf(f[2]) | ((uint32_t)f2bf(f[3]) << 16);
    v.z = (uint32_t)f2bf(f[4]) | ((uint32_t)f2bf(f[5]) << 16);
    v.w = (uint32_t)f2bf(f[6]) | ((uint32_t)f2bf(f[7]) << 16);
    *reinterpret_cast<uint4*>(p) = v;
  }
};

// four outputs of one dtype as one store (16 B of fp32, 8 B of bf16)
__device__ __forceinline__ void st4(float* p, const float* f) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
}
__device__ __forceinline__ void st4(uint16_t* p, const float* f) {
  uint2 v;
  v.x = (uint32_t)f2bf(f[0]) | ((uint32_t)f2bf(f[1]) << 16);
  v.y = (uint32_t)f2bf(f[2]) | ((uint32_t)f2bf(f[3]) << 16);
  *reinterpret_cast<uint2*>(p) = v;
}

int grid_of(long long work, int cap) {
  long long g = (work + 255) / 256;
  return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ---------------------------------------------------------------- MagTransform + row BN
constexpr int MAG_MAX_M = 4096;  // 2 M floats of LDS per workgroup

// x^p for x >= 0 from the hardware base-2 log / exp (as PCEN's powers, frontend.hip):
// x = 0 -> log2 = -inf -> exp2(-inf) = 0 for p > 0; x < 0 -> NaN
__device__ __forceinline__ float pow_hw(float x, float p) {
  return __builtin_amdgcn_exp2f(__fmul_rn(p, __builtin_amdgcn_logf(x)));
}

// y[i] = (x[i]^p - mean[m]) * inv[m], m = (i / T) % M, p = sigmoid(a[0]),
// inv = 1 / sqrt(var + eps) formed in double and rounded once to float (the
// fp32 hardware sqrt is a 1-ulp instruction; this way a host can restate inv
// bit for bit, and it costs M values per workgroup).  The flat array is cut
// into `head` leading scalars (up to x's first 16-B boundary), nvec groups of
// four and a scalar tail; a thread's group may straddle a row (T is odd in the
// model).
template <typename TO>
__global__ void __launch_bounds__(256) k_mag_rownorm(const float* __restrict__ x, long long n, int M, int T,
                                                      const float* __restrict__ a, const float* __restrict__ mean,
                                                      const float* __restrict__ var, float eps, int head,
                                                      long long nvec, TO* __restrict__ y) {
  extern __shared__ float sm[];  // mean[M], inv[M]
  for (int m = threadIdx.x; m < M; m += 256) {
    sm[m] = mean[m];
    sm[M + m] = (float)(1.0 / sqrt((double)var[m] + (double)eps));
  }
  const float p = __fdiv_rn(1.0f, 1.0f + expf(-a[0]));
  __syncthreads();
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (long long v = t0; v < nvec; v += stride) {
    const long long i = head + v * 4;
    const float4 q = *reinterpret_cast<const float4*>(x + i);
    const float in[4] = {q.x, q.y, q.z, q.w};
    const long long row = i / T;
    int col = (int)(i - row * T), m = (int)(row % M);
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = __fmul_rn(__fsub_rn(pow_hw(in[j], p), sm[m]), sm[M + m]);
      if (++col == T) {
        col = 0;
        if (++m == M) m = 0;
      }
    }
    st4(y + i, o);
  }
  // head and tail scalars: at most 3 + 3 elements
  const long long tail0 = head + nvec * 4;
  const long long nscalar = head + (n - tail0);
  for (long long s = t0; s < nscalar; s += stride) {
    const long long i = s < head ? s : tail0 + (s - head);
    const int m = (int)((i / T) % M);
    st1(y, i, __fmul_rn(__fsub_rn(pow_hw(x[i], p), sm[m]), sm[M + m]));
  }
}

// ---------------------------------------------------------------- LeakyReLU + BN affine
template <typename T>
__global__ void k_leaky_bn(const T* x, long long n, int C, float alpha, const float* __restrict__ scale,
                           const float* __restrict__ shift, T* y) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = ld1(x, i);
    float l = v > 0.f ? v : __fmul_rn(alpha, v);
    if (scale) {
      const int c = (int)(i % C);
      l = fmaf(scale[c], l, shift[c]);
    }
    st1(y, i, l);
  }
}
// one thread per 16 B: the group's channels are contiguous and inside one row
// (C is a multiple of the group size); x may alias y (each thread reads its
// group before it writes it)
template <typename T>
__global__ void __launch_bounds__(256) k_leaky_bn_v(const T* x, unsigned nvec, int C, float alpha,
                                                    const float* __restrict__ scale,
                                                    const float* __restrict__ shift, T* y) {
  constexpr int V = Vec<T>::N;
  const unsigned CV = (unsigned)C / V;
  for (unsigned v = blockIdx.x * 256 + threadIdx.x; v < nvec; v += gridDim.x * 256) {
    float f[V];
    Vec<T>::ld(x + (size_t)v * V, f);
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] = f[j] > 0.f ? f[j] : __fmul_rn(alpha, f[j]);
    if (scale) {
      const int c0 = (int)(v % CV) * V;
      float s[V], h[V];
#pragma unroll
      for (int j = 0; j < V; j += 4) {
        const float4 a = *reinterpret_cast<const float4*>(scale + c0 + j);
        const float4 b = *reinterpret_cast<const float4*>(shift + c0 + j);
        s[j] = a.x; s[j + 1] = a.y; s[j + 2] = a.z; s[j + 3] = a.w;
        h[j] = b.x; h[j + 1] = b.y; h[j + 2] = b.z; h[j + 3] = b.w;
      }
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] = fmaf(s[j], f[j], h[j]);
    }
    Vec<T>::st(y + (size_t)v * V, f);
  }
}

// ---------------------------------------------------------------- softmax
// one wave per row: running maximum, sum of exp2((z - max) log2 e), then the
// quotient; the row is re-read from the cache (L <= a few thousand)
__global__ void __launch_bounds__(256) k_softmax(const float* __restrict__ z, int B, int L, float* __restrict__ p) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  const float* zr = z + (size_t)row * L;
  float* pr = p + (size_t)row * L;
  float mx = -INFINITY;
  for (int j = lane; j < L; j += 64) mx = fmaxf(mx, zr[j]);
  mx = wave_max(mx);
  constexpr float LOG2E = 1.44269504088896340736f;
  float sum = 0.f;
  for (int j = lane; j < L; j += 64) sum += __builtin_amdgcn_exp2f((zr[j] - mx) * LOG2E);
  sum = wave_sum(sum);
  const float inv = __fdiv_rn(1.0f, sum);
  for (int j = lane; j < L; j += 64) pr[j] = __builtin_amdgcn_exp2f((zr[j] - mx) * LOG2E) * inv;
}

}  // namespace

ACFE_API int acfe_mag_rownorm(const float* x, int B, int M, int T, const float* a, const float* mean,
                              const float* var, float eps, void* y, int y_dtype, void* stream) {
  if (!x || !a || !mean || !var || !y || B < 0 || M < 1 || M > MAG_MAX_M || T < 1 || !(eps >= 0.f) ||
      (y_dtype != ACFE_DTYPE_F32 && y_dtype != ACFE_DTYPE_BF16) || !aligned(x, 4))
    return ACFE_E_INVAL;
  const size_t osz = y_dtype == ACFE_DTYPE_BF16 ? 2 : 4;
  if (!aligned(y, osz)) return ACFE_E_INVAL;
  const long long n = (long long)B * M * T;
  if (n == 0) return ACFE_OK;
  // the leading scalars up to x's 16-B boundary; the groups of four need y
  // aligned to four outputs there, else everything is scalar
  long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 4;
  if (head > n) head = n;
  long long nvec = (n - head) / 4;
  if (!aligned(static_cast<const char*>(y) + head * osz, 4 * osz)) head = n, nvec = 0;
  const int grid = grid_of(nvec > 0 ? nvec : n, 2048);
  const size_t lds = 2 * (size_t)M * sizeof(float);
  if (y_dtype == ACFE_DTYPE_BF16)
    hipLaunchKernelGGL(k_mag_rownorm<uint16_t>, dim3(grid), dim3(256), lds, strm(stream), x, n, M, T, a, mean, var,
                       eps, (int)(nvec ? head : 0), nvec, (uint16_t*)y);
  else
    hipLaunchKernelGGL(k_mag_rownorm<float>, dim3(grid), dim3(256), lds, strm(stream), x, n, M, T, a, mean, var,
                       eps, (int)(nvec ? head : 0), nvec, (float*)y);
  return launch_rc("acfe_mag_rownorm");
}

ACFE_API int acfe_leaky_bn(const void* x, long long rows, int C, float alpha, const float* scale, const float* shift,
                           void* y, int dtype, void* stream) {
  if (!x || !y || rows < 0 || C < 1 || (scale == nullptr) != (shift == nullptr) ||
      (dtype != ACFE_DTYPE_F32 && dtype != ACFE_DTYPE_BF16))
    return ACFE_E_INVAL;
  const size_t sz = dtype == ACFE_DTYPE_BF16 ? 2 : 4;
  if (!aligned(x, sz) || !aligned(y, sz)) return ACFE_E_INVAL;
  const long long n = rows * C;
  if (n == 0) return ACFE_OK;
  const int V = (int)(16 / sz);
  const bool vec = C % V == 0 && aligned(x, 16) && aligned(y, 16) && (!scale || (aligned(scale, 16) && aligned(shift, 16))) &&
                   n / V < (1ll << 31);  // (the grid-stride index stays below 2^32)
  if (vec) {
    const int grid = grid_of(n / V, 4096);
    if (dtype == ACFE_DTYPE_BF16)
      hipLaunchKernelGGL(k_leaky_bn_v<uint16_t>, dim3(grid), dim3(256), 0, strm(stream), (const uint16_t*)x,
                         (unsigned)(n / V), C, alpha, scale, shift, (uint16_t*)y);
    else
      hipLaunchKernelGGL(k_leaky_bn_v<float>, dim3(grid), dim3(256), 0, strm(stream), (const float*)x,
                         (unsigned)(n / V), C, alpha, scale, shift, (float*)y);
  } else {
    const int grid = grid_of(n, 4096);
    if (dtype == ACFE_DTYPE_BF16)
      hipLaunchKernelGGL(k_leaky_bn<uint16_t>, dim3(grid), dim3(256), 0, strm(stream), (const uint16_t*)x, n, C,
                         alpha, scale, shift, (uint16_t*)y);
    else
      hipLaunchKernelGGL(k_leaky_bn<float>, dim3(grid), dim3(256), 0, strm(stream), (const float*)x, n, C, alpha,
                         scale, shift, (float*)y);
  }
  return launch_rc("acfe_leaky_bn");
}

ACFE_API int acfe_softmax(const float* z, int B, int L, float* p, void* stream) {
  if (!z || !p || B < 0 || L < 1) return ACFE_E_INVAL;
  if (B == 0) return ACFE_OK;
  hipLaunchKernelGGL(k_softmax, dim3((B + 3) / 4), dim3(256), 0, strm(stream), z, B, L, p);
  return launch_rc("acfe_softmax");
}
