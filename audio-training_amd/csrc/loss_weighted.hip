// acfe_loss with Keras class weights and label smoothing in the same launch
// (model.fit(class_weight=...) of audiomodel.py:523-562 on one-hot targets, and
// label_smoothing of audiomodel.loss, :1206-1223).
//
// Per row b of z, y [B][L]:
//   w_b   = class_weight[argmax_j y[b][j]] on the unsmoothed targets, ties and an
//           all-zero row to the lowest index (tf.argmax); 1 without class_weight
//   y'    = y * (1 - s) + (mode 0: 0.5 * s, mode 1: s / L)
//   l_b   = k_loss's row loss (nn.hip) on y', the same float32 operations in the
//           same order
//   row_loss[b] = w_b * l_b,  dz[b][:] = w_b * (k_loss's dz on y')
// and loss[0] = (1 / B) * sum_b row_loss[b] in double (Keras sum_over_batch_size:
// the divisor is B, not sum w).
//
// With class_weight NULL or all 1 and s = 0 the results are bit-identical to
// acfe_loss: y' = fmaf(y, 1, 0) = y and the products by w = 1 are exact, and
// every other operation is k_loss's, compiled under the same contraction rule.
#include <limits.h>
#include "common.h"

using namespace acfe;

namespace {

// (value, index) order of the argmax: the larger value, then the lower index
__device__ __forceinline__ bool arg_before(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

// One 256-thread block per row, strided over L, as k_loss.  ya = 1 - s and
// yc = 0.5 * s (mode 0) or s / L (mode 1) come from the host.
__global__ void __launch_bounds__(256) k_loss_weighted(const float* __restrict__ z, const float* __restrict__ y, int B,
                                                       int L, int mode, float inv_scale,
                                                       const float* __restrict__ class_weight, float ya, float yc,
                                                       float* __restrict__ row_loss, float* __restrict__ dz,
                                                       float* __restrict__ row_weight) {
  const int b = blockIdx.x;
  __shared__ float red[4];
  __shared__ float sh[2];
  __shared__ float best_v[4];
  __shared__ int best_i[4];
  __shared__ float sh_w;
  const float* zr = z + (long long)b * L;
  const float* yr = y + (long long)b * L;
  float* dr = dz + (long long)b * L;
  float w = 1.f;
  if (class_weight) {  // uniform over the launch
    // per lane over its stride (ascending indices), per wave, then across the
    // four waves through LDS; at every level the lower index wins a tie
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = threadIdx.x; i < L; i += 256) {
      const float v = yr[i];
      if (arg_before(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (arg_before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if ((threadIdx.x & 63) == 0) {
      best_v[threadIdx.x >> 6] = bv;
      best_i[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < 4; ++k)
        if (arg_before(best_v[k], best_i[k], bv, bi)) {
          bv = best_v[k];
          bi = best_i[k];
        }
      // a row of NaNs orders nothing: keep the lookup inside class_weight[0, L)
      sh_w = class_weight[bi >= 0 && bi < L ? bi : 0];
    }
    __syncthreads();
    w = sh_w;
  }
  if (row_weight && threadIdx.x == 0) row_weight[b] = w;
  if (mode == 0) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < L; i += 256) {
      const float zz = zr[i], yy = fmaf(yr[i], ya, yc);
      acc += fmaxf(zz, 0.f) - zz * yy + log1pf(expf(-fabsf(zz)));
      const float p = 1.f / (1.f + expf(-zz));
      dr[i] = w * ((p - yy) / (float)L * inv_scale);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) row_loss[b] = w * ((red[0] + red[1] + red[2] + red[3]) / (float)L);
  } else {
    float sp = 0.f;
    for (int i = threadIdx.x; i < L; i += 256) sp += 1.f / (1.f + expf(-zr[i]));
    sp = wave_sum(sp);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sp;
    __syncthreads();
    const float S = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    const float lo = 1e-7f, hi = 1.f - 1e-7f;
    float acc = 0.f, gq = 0.f;
    for (int i = threadIdx.x; i < L; i += 256) {
      const float yy = fmaf(yr[i], ya, yc);
      const float p = 1.f / (1.f + expf(-zr[i]));
      const float q = p / S;
      const float qc = fminf(fmaxf(q, lo), hi);
      acc += -yy * logf(qc);
      const float g = (q >= lo && q <= hi) ? -yy / qc : 0.f;  // dL/dq
      gq += g * q;
    }
    acc = wave_sum(acc);
    gq = wave_sum(gq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) sh[0] = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = gq;
    __syncthreads();
    if (threadIdx.x == 0) sh[1] = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    const float sgq = sh[1];
    for (int i = threadIdx.x; i < L; i += 256) {
      const float yy = fmaf(yr[i], ya, yc);
      const float p = 1.f / (1.f + expf(-zr[i]));
      const float q = p / S;
      const float qc = fminf(fmaxf(q, lo), hi);
      const float g = (q >= lo && q <= hi) ? -yy / qc : 0.f;
      const float dp = (g - sgq) / S;  // dL/dp_j = (g_j - sum_i g_i q_i) / S
      dr[i] = w * (dp * p * (1.f - p) * inv_scale);
    }
    if (threadIdx.x == 0) row_loss[b] = w * sh[0];
  }
}

// k_mean of nn.hip: the mean over the batch in double, fixed order
__global__ void __launch_bounds__(256) k_row_mean(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
  acc = wave_sumd(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)((red[0] + red[1] + red[2] + red[3]) / n);
}

}  // namespace

ACFE_API int acfe_loss_weighted(const float* z, const float* y, int B, int L, int mode, float grad_scale,
                                const float* class_weight, float label_smoothing, float* loss, float* dz,
                                float* row_loss, float* row_weight, void* stream) {
  const float s = label_smoothing;
  if (!z || !y || !loss || !dz || !row_loss || (mode != 0 && mode != 1) || B <= 0 || L <= 0 ||
      !(s >= 0.f && s < 1.f))  // a NaN fails both comparisons
    return ACFE_E_INVAL;
  const float ya = 1.f - s, yc = mode == 0 ? 0.5f * s : s / (float)L;
  hipLaunchKernelGGL(k_loss_weighted, dim3(B), dim3(256), 0, strm(stream), z, y, B, L, mode, grad_scale, class_weight,
                     ya, yc, row_loss, dz, row_weight);
  int rc = launch_rc("acfe_loss_weighted");
  if (rc) return rc;
  hipLaunchKernelGGL(k_row_mean, dim3(1), dim3(256), 0, strm(stream), row_loss, B, loss);
  return launch_rc("acfe_loss_weighted(mean)");
}
