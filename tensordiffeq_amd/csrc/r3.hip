// R3 (retain-resample-release) resampling of the collocation points (Daw, Bu, Wang, Perdikaris, Karpatne,
// ICML 2023), run on the device after every loss pass (ops/r3.py, compile(resample="r3")).
//
//   a_i = sqrt((double) r2[i] * inv_c)                      (|f_i|: r2 is c f^2, inv_c = 1 / c)
//   tau = (sum_i a_i) / n                                   (double, fixed order)
//   row i is retained iff a_i > tau; every other row (a tie, a NaN anywhere, a lone point) is released:
//   x_ij = (float)(lo_j + u * (hi_j - lo_j)),  u = (w >> 8) * 2^-24,
//   w = word j % 4 of Philox4x32-10(counter (i, j / 4, step_lo, step_hi), key (seed_lo, seed_hi))
//
// in double with the multiply and the add rounded separately (this file is built with -ffp-contract=off
// and the function says so again).  Rows keep their place and retained rows are not written, so there is
// no compaction, no sort and no atomic; every sum has a fixed order and two calls on the same inputs
// give the same bits.  Two launches:
//   pass 1  up to 1024 workgroups, workgroup b sums the 256-point blocks b, b + G, ... (strided lanes,
//           then a fixed LDS tree) into work[b]; workgroup 0 also copies the step counter into
//           work[G], so that no workgroup of pass 2 reads `state` itself;
//   pass 2  one workgroup per 256 points: every workgroup sums the G partials in the same order,
//           takes tau and the step from `work`, draws and writes its released rows (both destinations
//           get the same value) and its released count; workgroup 0 writes stats and state = step + 1.
// Loads are unconditional from clamped indices and masked after.
#include "common.h"

namespace {

constexpr int R3_BLOCK = 256;
constexpr int R3_MAX_PART = 1024;
constexpr int R3_PER_LANE = R3_MAX_PART / R3_BLOCK;
constexpr int R3_MAX_DIN = 8;

__host__ __device__ inline int r3_blocks(int n) { return (int)(((long long)n + R3_BLOCK - 1) / R3_BLOCK); }
__host__ __device__ inline int r3_parts(int n) { const int b = r3_blocks(n); return b < R3_MAX_PART ? b : R3_MAX_PART; }

struct Philox4 { unsigned v[4]; };

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC 2011; the Random123 constants)
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                 unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const unsigned hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ double r3_abs_f(const float* __restrict__ r2, long long i, int n, double inv_c) {
  return sqrt((double)r2[i < n ? i : n - 1] * inv_c);
}

// red[0] <- sum of the 256 lanes' values, a fixed tree
__device__ __forceinline__ void r3_tree(double* red, int tid) {
  __syncthreads();
#pragma unroll
  for (int s = R3_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
}

__global__ __launch_bounds__(R3_BLOCK) void r3_partial_sums(const float* __restrict__ r2, double inv_c, int n,
                                                            const long long* __restrict__ state,
                                                            double* __restrict__ work) {
  __shared__ double red[R3_BLOCK];
  const int tid = threadIdx.x, G = gridDim.x;
  const int nblk = r3_blocks(n);
  double acc = 0.0;
  for (int blk = blockIdx.x; blk < nblk; blk += G) {   // (uniform over the workgroup)
    const long long i = (long long)blk * R3_BLOCK + tid;
    const double a = r3_abs_f(r2, i, n, inv_c);
    acc += i < n ? a : 0.0;
  }
  red[tid] = acc;
  r3_tree(red, tid);
  if (tid == 0) {
    work[blockIdx.x] = red[0];
    if (blockIdx.x == 0) work[G] = __longlong_as_double(state[0]);
  }
}

__global__ __launch_bounds__(R3_BLOCK) void r3_release(const float* __restrict__ r2, double inv_c,
                                                       const double* __restrict__ box, unsigned long long seed,
                                                       int n, int d_in, int parts, const double* __restrict__ work,
                                                       float* __restrict__ X, long long ldx, float* __restrict__ X2,
                                                       long long ldx2, long long start2,
                                                       long long* __restrict__ state, double* __restrict__ stats,
                                                       int* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ double red[R3_BLOCK];
  __shared__ int cnt[R3_BLOCK];
  const int tid = threadIdx.x;
  // the mean: lane t owns the partials [4 t, 4 t + 4), summed left to right, then the tree - the same
  // order in every workgroup
  double own = 0.0;
#pragma unroll
  for (int k = 0; k < R3_PER_LANE; ++k) {
    const int b = tid * R3_PER_LANE + k;
    const double v = work[b < parts ? b : parts - 1];
    own += b < parts ? v : 0.0;
  }
  red[tid] = own;
  r3_tree(red, tid);
  const double tau = red[0] / (double)n;
  const long long step = __double_as_longlong(work[parts]);
  const long long i = (long long)blockIdx.x * R3_BLOCK + tid;
  const double a = r3_abs_f(r2, i, n, inv_c);
  const bool released = i < n && !(a > tau);
  if (released) {
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const unsigned s0 = (unsigned)(unsigned long long)step, s1 = (unsigned)((unsigned long long)step >> 32);
    float* __restrict__ row = X + i * ldx;
    float* __restrict__ row2 = X2 != nullptr ? X2 + (start2 + i) * ldx2 : nullptr;
    for (int blk = 0; blk * 4 < d_in; ++blk) {
      const Philox4 w = philox4x32_10((unsigned)i, (unsigned)blk, s0, s1, k0, k1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = blk * 4 + q;
        if (j < d_in) {
          const double lo = box[2 * j], hi = box[2 * j + 1];
          const double u = (double)(w.v[q] >> 8) * 0x1p-24;
          const double span = hi - lo;
          const double prod = u * span;
          const float x = (float)(lo + prod);
          row[j] = x;
          if (row2 != nullptr) row2[j] = x;
        }
      }
    }
  }
  cnt[tid] = released ? 1 : 0;
  __syncthreads();
#pragma unroll
  for (int s = R3_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) cnt[tid] += cnt[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    counts[blockIdx.x] = cnt[0];
    if (blockIdx.x == 0) {
      stats[0] = tau;
      stats[1] = (double)step;
      state[0] = step + 1;
    }
  }
}

}  // namespace

extern "C" {

// Doubles of `work` that tdq_r3_resample needs for n points (the partial sums and the step snapshot).
int tdq_r3_work_doubles(int n) { return n < 1 ? 2 : r3_parts(n) + 1; }

// Ints of `counts` for n points: one released count per workgroup of pass 2.
int tdq_r3_count_ints(int n) { return n < 1 ? 1 : r3_blocks(n); }

// One R3 update of the n residual rows of X (row stride ldx floats) from r2[i] = c f_i^2, inv_c = 1 / c.
//   box (2 d_in doubles): lo_j, hi_j of every input variable; state: the device step counter (read, then
//   advanced by one); seed: the Philox key; X2 (or null): a second destination whose rows start2 + i
//   (row stride ldx2) receive the same values; work: tdq_r3_work_doubles(n) doubles;
//   stats (2 doubles) = {tau, the step whose draw was used}; counts: tdq_r3_count_ints(n) ints, the
//   released rows per workgroup (their sum is the released count).
// hipErrorInvalidValue, and nothing launched, for n < 1, d_in outside 1..8, a row stride below d_in, a
// negative start2 or a null pointer (X2 alone may be null).
int tdq_r3_resample(const float* r2, double inv_c, const double* box, long long* state, unsigned long long seed,
                    float* X, int ldx, float* X2, int ldx2, long long start2, int n, int d_in, double* work,
                    double* stats, int* counts, void* stream) {
  if (n < 1 || d_in < 1 || d_in > R3_MAX_DIN || ldx < d_in) return (int)hipErrorInvalidValue;
  if (r2 == nullptr || box == nullptr || state == nullptr || X == nullptr || work == nullptr || stats == nullptr ||
      counts == nullptr)
    return (int)hipErrorInvalidValue;
  if (X2 != nullptr && (ldx2 < d_in || start2 < 0)) return (int)hipErrorInvalidValue;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int parts = r3_parts(n);
  hipLaunchKernelGGL(r3_partial_sums, dim3(parts), dim3(R3_BLOCK), 0, st, r2, inv_c, n, state, work);
  TDQ_CHECK_LAUNCH();
  hipLaunchKernelGGL(r3_release, dim3(r3_blocks(n)), dim3(R3_BLOCK), 0, st, r2, inv_c, box, seed, n, d_in, parts,
                     work, X, (long long)ldx, X2, (long long)ldx2, start2, state, stats, counts);
  TDQ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
