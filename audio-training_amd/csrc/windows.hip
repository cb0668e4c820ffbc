// Classification windows of the predict path, cut and normalised on the
// device: acfe_windows_normalize turns the device-resident recording plus a
// table of window descriptors (predict.track_window_plan, the index arithmetic
// of reference predict_utils.load_samples :59-150) into the normalised [batch][n]
// input of the STFT, without the windows ever existing on the host.
//
// Window b is the virtual zero-padded vector
//   v[i] = rec[src + i - pad]   for pad <= i < pad + count,   0 elsewhere,
// and the output is tfdataset.normalize of it: the min / max reductions of
// k_norm_stats and the pointwise norm1 of k_norm_apply (IEEE division), so the
// result is bit-identical to normalising the materialised window.
#include "common.h"

using namespace acfe;

namespace {

constexpr int WN_THREADS = 1024;
constexpr int WN_WAVES = WN_THREADS / 64;

// floats in front of p's next 16-byte boundary (p is 4-byte aligned)
__device__ __forceinline__ int to_align16(const float* p) {
  return (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
}

// One workgroup per window.  Pass 1 streams the window's source run with 16-B
// loads from the source's own alignment (src is arbitrary, so the run starts
// anywhere in a 16-B line) and reduces min / max; pass 2 walks the OUTPUT row
// in 16-B stores (rows are 16-B aligned when n % 4 == 0; any other row gets a
// scalar head and tail) and re-reads the source, now in L2, with four dword
// loads per store.
//
// The descriptor is clamped before use, whatever the host checked: pad to
// [0, n], count to [0, n - pad], and the source run to rec[0, rec_len) -- a
// source index outside the recording reads as zero, it is never dereferenced.
__global__ void __launch_bounds__(WN_THREADS) k_windows_norm(const float* __restrict__ rec, int64_t rec_len,
                                                             const int64_t* __restrict__ plan, int n,
                                                             float* __restrict__ out, float* __restrict__ stats) {
  __shared__ float smn[WN_WAVES], smx[WN_WAVES];
  const int64_t b = blockIdx.x;
  const int64_t src = plan[3 * b];
  const int pad = (int)min(max(plan[3 * b + 2], (int64_t)0), (int64_t)n);
  const int count = (int)min(max(plan[3 * b + 1], (int64_t)0), (int64_t)(n - pad));
  // j in [lo, hi) of the run has its source sample src + j inside the recording
  int lo = 0, hi = 0;
  if (src >= -(int64_t)count && src < rec_len) {
    lo = src < 0 ? (int)-src : 0;
    hi = (int)min((int64_t)count, rec_len - src);
  }
  const int len = hi - lo;
  const float* run = rec + (len > 0 ? src + lo : 0);  // run[0 .. len) is inside rec

  // ---- pass 1: min / max of the run, zeros included when anything is padded
  float mn[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (len < n) mn[0] = mx[0] = 0.f;
  {
    const int head = min(len, to_align16(run));
    const int nv = (len - head) >> 2;
    const float4* xv = reinterpret_cast<const float4*>(run + head);
    int i = threadIdx.x;
    for (; i + 3 * WN_THREADS < nv; i += 4 * WN_THREADS) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = xv[i + u * WN_THREADS];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        mn[u] = fminf(fminf(mn[u], v[u].x), fminf(v[u].y, fminf(v[u].z, v[u].w)));
        mx[u] = fmaxf(fmaxf(mx[u], v[u].x), fmaxf(v[u].y, fmaxf(v[u].z, v[u].w)));
      }
    }
    for (; i < nv; i += WN_THREADS) {
      const float4 v = xv[i];
      mn[0] = fminf(fminf(mn[0], v.x), fminf(v.y, fminf(v.z, v.w)));
      mx[0] = fmaxf(fmaxf(mx[0], v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    // the scalar ends: at most 3 floats in front of the 16-B body and 3 behind
    const int tail = head + (nv << 2);
    const int e = threadIdx.x < head ? (int)threadIdx.x : tail + (int)threadIdx.x - head;
    if (e < len) {
      const float v = run[e];
      mn[1] = fminf(mn[1], v);
      mx[1] = fmaxf(mx[1], v);
    }
  }
  float a = wave_min(fminf(fminf(mn[0], mn[1]), fminf(mn[2], mn[3])));
  float c = wave_max(fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3])));
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = a;
    smx[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  a = smn[0];
  c = smx[0];
#pragma unroll
  for (int k = 1; k < WN_WAVES; ++k) a = fminf(a, smn[k]), c = fmaxf(c, smx[k]);
  const float lowest = a, rng = c - a;  // == max(v - min) (fl is monotone)
  if (stats && threadIdx.x == 0) {
    stats[2 * b] = lowest;
    stats[2 * b + 1] = rng;
  }

  // ---- pass 2: out[b][i] = norm1(v[i]); v[i] = run[i - first] for first <= i < last
  float* row = out + b * n;
  const int first = pad + lo, last = first + len;
  auto vi = [&](int i) { return (i >= first && i < last) ? run[i - first] : 0.f; };
  const int head = min(n, to_align16(row));
  const int nv = (n - head) >> 2;
  float4* yv = reinterpret_cast<float4*>(row + head);
  int q = threadIdx.x;
  for (; q + WN_THREADS < nv; q += 2 * WN_THREADS) {
    float v[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[u][k] = vi(head + 4 * (q + u * WN_THREADS) + k);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      yv[q + u * WN_THREADS] = make_float4(norm1(v[u][0], lowest, rng), norm1(v[u][1], lowest, rng),
                                           norm1(v[u][2], lowest, rng), norm1(v[u][3], lowest, rng));
  }
  for (; q < nv; q += WN_THREADS) {
    const int i = head + 4 * q;
    yv[q] = make_float4(norm1(vi(i), lowest, rng), norm1(vi(i + 1), lowest, rng), norm1(vi(i + 2), lowest, rng),
                        norm1(vi(i + 3), lowest, rng));
  }
  const int tail = head + (nv << 2);
  const int e = threadIdx.x < head ? (int)threadIdx.x : tail + (int)threadIdx.x - head;
  if (e < n) row[e] = norm1(vi(e), lowest, rng);
}

}  // namespace

ACFE_API int acfe_windows_normalize(const float* rec, int64_t rec_len, const int64_t* plan, int batch, int n,
                                    float* out, float* stats, void* stream) {
  if (batch == 0 && n > 0 && rec_len >= 0) return ACFE_OK;
  if (!rec || !plan || !out || rec_len < 0 || batch < 0 || n <= 0) return ACFE_E_INVAL;
  hipLaunchKernelGGL(k_windows_norm, dim3(batch), dim3(WN_THREADS), 0, strm(stream), rec, rec_len, plan, n, out,
                     stats);
  return launch_rc("acfe_windows_normalize");
}
