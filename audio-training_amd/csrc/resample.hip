// Resampling of a recording to the model's rate, on the device:
// acfe_resample_poly is scipy.signal.resample_poly(x, up, down) (the host
// resampler of predict.load_recording, which stands in for the librosa.resample
// of reference predict.py:59-66) for taps and an offset the host supplies
// (predict.resample_plan):
//   t = n * down + t0,  p = t % up,  j0 = t / up
//   out[n] = sum over k >= 0 with p + k * up < n_taps of h[p + k * up] * x[j0 - k]
// with x = 0 outside [0, n_in): the polyphase form of "insert up - 1 zeros,
// filter with h, keep every down-th sample".
//
// One lane per output, consecutive lanes on consecutive outputs: their j0 lie
// (down / up) apart, so a wave's loads of x[j0 - k] fall into a few
// neighbouring lines and hit L1 from the second k on, and the store is one
// full line per wave.  The taps (at most 16384, 64 KiB) are staged once per
// workgroup in LDS; lanes read h[p + k * up] there at a lane stride of
// down % up dwords -- odd whenever up is even (gcd(up, down) = 1), and at most
// `up` distinct addresses when up is small (broadcast).  A workgroup walks the
// outputs in a grid-stride loop of RS_TILE outputs per step, so the taps are
// staged 2048 times at most, not once per tile; p and j0 advance by the
// constant (step * down) % up and / up, one 64-bit division per lane in all.
//
// Every product of two float32 values is exact in float64 and the at most 41
// (any n_taps / up) of them are summed in float64, then rounded to float32
// once: the result does not depend on the order of the terms to far below a
// float32 ulp.  All sample indices are 64-bit (t passes 2^32 after 609 s of
// 44.1 kHz audio).  The range of k is cut to the terms whose sample lies in
// x[0, n_in) and whose tap lies in h[0, n_taps) BEFORE the loop, so nothing
// else is ever addressed, whatever the arguments.
#include "common.h"

using namespace acfe;

namespace {

constexpr int RS_TILE = 256;         // outputs per workgroup and step = threads per workgroup
constexpr int RS_MAX_BLOCKS = 2048;  // 8 workgroups of 4 waves on each of 256 CUs
constexpr int RS_MAX_TAPS = 16384;   // 64 KiB of LDS

__device__ __forceinline__ float sample(const float* __restrict__ x, int64_t j) { return x[j]; }
// load_recording's conversion: float32(v) / 32767, the correctly rounded quotient
__device__ __forceinline__ float sample(const int16_t* __restrict__ x, int64_t j) {
  return __fdiv_rn((float)x[j], 32767.0f);
}

template <typename T>
__global__ void __launch_bounds__(RS_TILE) k_resample_poly(const T* __restrict__ x, int64_t n_in,
                                                           const float* __restrict__ h, int n_taps, int up, int down,
                                                           int64_t t0, float* __restrict__ out, int64_t n_out) {
  extern __shared__ float sh[];  // [n_taps]
  for (int i = threadIdx.x; i < n_taps; i += RS_TILE) sh[i] = h[i];
  __syncthreads();

  const int64_t step = (int64_t)gridDim.x * RS_TILE;  // outputs per grid step
  const int64_t dj = step * down / up, dp = step * down % up;
  int64_t n = (int64_t)blockIdx.x * RS_TILE + threadIdx.x;
  if (n >= n_out) return;
  const int64_t t = n * down + t0;  // < 2^63: checked by the host
  int64_t j0 = t / up, p = t % up;
  for (; n < n_out; n += step) {
    double acc = 0.0;
    if (p < n_taps) {
      // k in [k_lo, k_hi]: tap p + k * up <= n_taps - 1, sample 0 <= j0 - k <= n_in - 1
      const int64_t k_hi = min((int64_t)(n_taps - 1 - (int)p) / up, j0);
      const int64_t k_lo = max((int64_t)0, j0 - (n_in - 1));
      if (k_lo <= k_hi) {
        // 64-bit bases once, 32-bit offsets in the loop: (k_hi - k_lo) * up < n_taps
        const float* hp = sh + p + k_lo * up;
        const T* xp = x + (j0 - k_lo);
        const int cnt = (int)(k_hi - k_lo);
#pragma unroll 4
        for (int k = 0; k <= cnt; ++k) acc = fma((double)hp[k * up], (double)sample(xp, -k), acc);
      }
    }
    out[n] = (float)acc;
    j0 += dj, p += dp;
    if (p >= up) p -= up, ++j0;
  }
}

}  // namespace

ACFE_API int acfe_resample_poly(const void* x, int x_dtype, int64_t n_in, const float* h, int n_taps, int up,
                                int down, int64_t t0, float* out, int64_t n_out, void* stream) {
  if (up < 1 || down < 1 || n_taps < 1 || n_taps > RS_MAX_TAPS || t0 < 0 || n_in < 0 || n_out < 0 ||
      (x_dtype != ACFE_DTYPE_F32 && x_dtype != ACFE_DTYPE_I16))
    return ACFE_E_INVAL;
  if (n_out == 0) return ACFE_OK;
  // t = n * down + t0 for n < n_out, and one grid step more, must fit int64
  if (n_out > (INT64_MAX - t0) / down - (int64_t)RS_MAX_BLOCKS * RS_TILE) return ACFE_E_INVAL;
  if (!out || !h || (!x && n_in > 0)) return ACFE_E_INVAL;
  if (n_in == 0)  // every sample is zero: no kernel
    return hip_rc(hipMemsetAsync(out, 0, (size_t)n_out * sizeof(float), strm(stream)), "acfe_resample_poly");
  const int64_t tiles = (n_out + RS_TILE - 1) / RS_TILE;
  const dim3 grid((unsigned)(tiles < RS_MAX_BLOCKS ? tiles : RS_MAX_BLOCKS)), block(RS_TILE);
  const size_t lds = (size_t)n_taps * sizeof(float);
  if (x_dtype == ACFE_DTYPE_F32)
    hipLaunchKernelGGL(k_resample_poly<float>, grid, block, lds, strm(stream), static_cast<const float*>(x), n_in, h,
                       n_taps, up, down, t0, out, n_out);
  else
    hipLaunchKernelGGL(k_resample_poly<int16_t>, grid, block, lds, strm(stream), static_cast<const int16_t*>(x),
                       n_in, h, n_taps, up, down, t0, out, n_out);
  return launch_rc("acfe_resample_poly");
}
