// Generic LDS Stockham FFT passes shared by the mel front end (frontend.hip,
// k_mel<NC>) and the track detector's magnitude STFT (tracks.hip): complex
// helpers, radix-2/4/8 butterflies held in VGPRs, one padded LDS buffer.
#pragma once
#include <hip/hip_runtime.h>

// ------------------------------------------------------------ FFT helpers
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // a * (-i)

template <int R>
__device__ __forceinline__ void dft(float2* v);

template <>
__device__ __forceinline__ void dft<2>(float2* v) {
  float2 a = v[0], b = v[1];
  v[0] = cadd(a, b);
  v[1] = csub(a, b);
}
template <>
__device__ __forceinline__ void dft<4>(float2* v) {
  float2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
  float2 t2 = cadd(v[1], v[3]), t3 = mul_mi(csub(v[1], v[3]));
  v[0] = cadd(t0, t2);
  v[2] = csub(t0, t2);
  v[1] = cadd(t1, t3);
  v[3] = csub(t1, t3);
}
template <>
__device__ __forceinline__ void dft<8>(float2* v) {
  float2 e[4] = {v[0], v[2], v[4], v[6]};
  float2 o[4] = {v[1], v[3], v[5], v[7]};
  dft<4>(e);
  dft<4>(o);
  const float c = 0.70710678118654752440f;
  // W8^1 = c(1 - i), W8^2 = -i, W8^3 = -c(1 + i)
  float2 o1 = make_float2(c * (o[1].x + o[1].y), c * (o[1].y - o[1].x));
  float2 o2 = mul_mi(o[2]);
  float2 o3 = make_float2(c * (o[3].y - o[3].x), -c * (o[3].x + o[3].y));
  v[0] = cadd(e[0], o[0]); v[4] = csub(e[0], o[0]);
  v[1] = cadd(e[1], o1);   v[5] = csub(e[1], o1);
  v[2] = cadd(e[2], o2);   v[6] = csub(e[2], o2);
  v[3] = cadd(e[3], o3);   v[7] = csub(e[3], o3);
}

// LDS index with one float2 of padding per 8 (breaks the power-of-two strides
// of the Stockham writes: pass-1 stores go from 8-way conflicted to conflict-free).
__device__ __forceinline__ int padx(int i) { return i + (i >> 3); }

// One in-place Stockham pass (Govindaraju et al. formulation) over NC points
// held in LDS `buf`, radix R, span Ns.  256 threads.
template <int NC, int R>
__device__ __forceinline__ void stockham_pass(float2* buf, int Ns, const float2* __restrict__ tw) {
  constexpr int NB = NC / R;
  constexpr int PER = (NB + 255) / 256;
  float2 v[PER][R];
#pragma unroll
  for (int p = 0; p < PER; ++p) {
    const int j = threadIdx.x + 256 * p;
    if (NB % 256 == 0 || j < NB) {
      const int jm = j & (Ns - 1);
      const int tstep = jm * (NC / (Ns * R));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float2 a = buf[padx(j + r * NB)];
        if (r) a = cmul(a, tw[r * tstep]);
        v[p][r] = a;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < PER; ++p) {
    const int j = threadIdx.x + 256 * p;
    if (NB % 256 == 0 || j < NB) {
      dft<R>(v[p]);
      const int idxD = (j / Ns) * Ns * R + (j & (Ns - 1));
#pragma unroll
      for (int r = 0; r < R; ++r) buf[padx(idxD + r * Ns)] = v[p][r];
    }
  }
  __syncthreads();
}
