// Temporal causality weights (Wang, Sankaran, Perdikaris, arXiv 2203.07404) of the collocation points,
// recomputed on the device after every loss pass (ops/causal.py, Adaptive_type 4).
//
//   L_b = (1 / n_b) sum_{i in bin b} r2[i] * inv_c          (0 for an empty bin)
//   W_b = expf((float)(-eps * sum_{b' < b} L_b'))           (W_0 = 1)
//   lam[i] = W_bin(i)
//
// The points keep the user's order: `order` is the permutation that sorts them by bin and `bin_start`
// the M + 1 offsets into it, both built once on the host.  Two launches, no atomics, every sum in a
// fixed order and in double, so two calls on the same inputs give the same bits:
//   pass 1  one workgroup per bin: strided lanes over the bin's points, then a fixed LDS tree;
//   pass 2  every workgroup scans the M bin means in LDS (exclusive, fixed order), takes the M
//           weights and writes lam of its 256 sorted positions; workgroup 0 also writes w_bins and
//           stats = {min_b W_b, sum_b L_b}.
// Loads are unconditional from clamped indices and masked after; a point index outside [0, n) in
// `order` is clamped, so no access leaves r2[0, n) / lam[0, n).
#include "common.h"

namespace {

constexpr int CAUSAL_BLOCK = 256;
constexpr int CAUSAL_MAX_BINS = 1024;
constexpr int CAUSAL_PER_LANE = CAUSAL_MAX_BINS / CAUSAL_BLOCK;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// mean[b] = inv_c * sum_{j in [bin_start[b], bin_start[b+1])} r2[order[j]] / n_b
__global__ __launch_bounds__(CAUSAL_BLOCK) void causal_bin_means(const float* __restrict__ r2, double inv_c,
                                                                 const int* __restrict__ order,
                                                                 const int* __restrict__ bin_start, int n,
                                                                 double* __restrict__ mean) {
  __shared__ double red[CAUSAL_BLOCK];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lo = clampi(bin_start[b], 0, n);
  const int hi = clampi(bin_start[b + 1], lo, n);
  double acc = 0.0;
  for (int base = lo; base < hi; base += CAUSAL_BLOCK) {   // (uniform over the workgroup)
    const int j = base + tid;
    const int i = clampi(order[j < hi ? j : hi - 1], 0, n - 1);
    const double v = (double)r2[i];
    acc += j < hi ? v : 0.0;
  }
  red[tid] = acc;
  __syncthreads();
#pragma unroll
  for (int s = CAUSAL_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) mean[b] = hi > lo ? red[0] * inv_c / (double)(hi - lo) : 0.0;
}

__global__ __launch_bounds__(CAUSAL_BLOCK) void causal_weights(const double* __restrict__ mean,
                                                               const int* __restrict__ order,
                                                               const int* __restrict__ bin_start, int M, int n,
                                                               const float* __restrict__ eps_ptr,
                                                               float* __restrict__ lam, float* __restrict__ w_bins,
                                                               float* __restrict__ stats) {
  __shared__ double part[CAUSAL_BLOCK];
  __shared__ float W[CAUSAL_MAX_BINS];
  __shared__ int start[CAUSAL_MAX_BINS + 1];
  __shared__ float wmin[CAUSAL_BLOCK];
  const int tid = threadIdx.x;
  const double eps = (double)eps_ptr[0];
  // exclusive scan of the M means: lane t owns the bins [4 t, 4 t + 4), summed left to right; the
  // lanes' totals are scanned by a fixed doubling ladder
  double m[CAUSAL_PER_LANE];
  double own = 0.0;
#pragma unroll
  for (int k = 0; k < CAUSAL_PER_LANE; ++k) {
    const int b = tid * CAUSAL_PER_LANE + k;
    const double v = mean[b < M ? b : M - 1];
    m[k] = b < M ? v : 0.0;
    own += m[k];
  }
  part[tid] = own;
  for (int b = tid; b <= M; b += CAUSAL_BLOCK) start[b] = bin_start[b];
  __syncthreads();
#pragma unroll
  for (int s = 1; s < CAUSAL_BLOCK; s <<= 1) {
    const double add = tid >= s ? part[tid - s] : 0.0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  double cum = part[tid] - own;   // sum of the bins before this lane's first one
  float lo_w = __builtin_inff();
#pragma unroll
  for (int k = 0; k < CAUSAL_PER_LANE; ++k) {
    const int b = tid * CAUSAL_PER_LANE + k;
    const float w = expf((float)(-eps * cum));
    if (b < M) {
      W[b] = w;
      lo_w = fminf(lo_w, w);
    }
    cum += m[k];
  }
  __syncthreads();
  // the bin of sorted position j: the last b with start[b] <= j
  const int j = blockIdx.x * CAUSAL_BLOCK + tid;
  if (n > 0) {
    int lo = 0, hi = M;   // invariant: start[lo] <= j, and j < start[hi] or hi == M
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (start[mid] <= j) lo = mid; else hi = mid;
    }
    const int i = clampi(order[j < n ? j : n - 1], 0, n - 1);
    if (j < n) lam[i] = W[lo];
  }
  if (blockIdx.x == 0) {
    for (int b = tid; b < M; b += CAUSAL_BLOCK) w_bins[b] = W[b];
    wmin[tid] = lo_w;
    __syncthreads();
#pragma unroll
    for (int s = CAUSAL_BLOCK / 2; s > 0; s >>= 1) {
      if (tid < s) wmin[tid] = fminf(wmin[tid], wmin[tid + s]);
      __syncthreads();
    }
    if (tid == 0) {
      stats[0] = wmin[0];
      stats[1] = (float)part[CAUSAL_BLOCK - 1];
    }
  }
}

}  // namespace

extern "C" {

// Doubles of `work` that tdq_causal_update needs for M bins.
int tdq_causal_work_doubles(int M) { return M < 1 ? 1 : M; }

// lam[i] = W_bin(i) from r2[i] = c f_i^2 (the loss executors' adjoint of the weight array), inv_c = 1 / c.
//   order (n) int32: the points sorted by bin; bin_start / bin_start_host (M + 1) int32: the bins'
//   offsets into `order`, on the device and the same values on the host (checked here, before any
//   launch: 0 = bin_start[0] <= ... <= bin_start[M] = n);
//   eps_ptr: the device scalar eps; work: tdq_causal_work_doubles(M) doubles (the bin means);
//   lam (n), w_bins (M), stats (2) = {min_b W_b, sum_b L_b}: every element is written.
// hipErrorInvalidValue, and nothing launched, for M outside 1..1024, n < 0 or a bad bin_start.
int tdq_causal_update(const float* r2, double inv_c, const int* order, const int* bin_start,
                      const int* bin_start_host, int M, int n, const float* eps_ptr, double* work, float* lam,
                      float* w_bins, float* stats, void* stream) {
  if (M < 1 || M > CAUSAL_MAX_BINS || n < 0 || bin_start_host == nullptr) return (int)hipErrorInvalidValue;
  if (bin_start_host[0] != 0 || bin_start_host[M] != n) return (int)hipErrorInvalidValue;
  for (int b = 0; b < M; ++b)
    if (bin_start_host[b + 1] < bin_start_host[b]) return (int)hipErrorInvalidValue;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(causal_bin_means, dim3(M), dim3(CAUSAL_BLOCK), 0, st, r2, inv_c, order, bin_start, n, work);
  TDQ_CHECK_LAUNCH();
  const int blocks = n > 0 ? (n + CAUSAL_BLOCK - 1) / CAUSAL_BLOCK : 1;
  hipLaunchKernelGGL(causal_weights, dim3(blocks), dim3(CAUSAL_BLOCK), 0, st, work, order, bin_start, M, n, eps_ptr,
                     lam, w_bins, stats);
  TDQ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
