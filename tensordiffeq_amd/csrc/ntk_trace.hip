// Per-instance squared parameter-gradient norms for NTK loss weighting (Wang, Yu, Perdikaris,
// arXiv 2007.14527, Algorithm 1), gfx950.
//
// For one loss output f and every instance i (a point, or an (upper, lower) point pair of a periodic
// group) the kernel returns n2[i] = || d f_i / d theta ||^2 from the jet seeds dJ = d f / d J and the
// pre-activation streams saved by tdq_jet_fwd.  No gradient is materialised: with the rows
// r = (point, stream) of the instance, Z_l[r] the adjoint of layer l's pre-activation stream and
// H_{l-1}[r] the activation stream below it, the weight gradient of layer l is sum_r H[r] Z[r]^T, so
//   || d f / d K_l ||_F^2 = sum_{r, r'} (Z[r] . Z[r']) (H[r] . H[r']),   || d f / d b_l ||^2 = || sum_{value rows} Z[r] ||^2
// - two Gram matrices over the rows, each fully reduced over the features before they are multiplied.
//
// The kernel is jet_bwd_kernel (jet_mlp.hip) with the dK transposes and MFMAs replaced by that Gram
// epilogue: the same feature-major layout (lane l: column l & 15, features 16 t + 4 (l >> 4) + c),
// the same exact-fp32 MFMA propagation hb = K zb from the padded [in][out] images, the adjoints
// hb parked in a wave-private LDS image.  A wave owns 16 columns and never talks to another wave.
// Per layer every lane accumulates Gz[s][s'] and Gh[s][s'] (s <= s') over its own features, the four
// lanes of a column are summed with the row-swap instructions (col4_sum), then the products join the
// column's running norm.
//
// A column finds its point by a 16-byte gather: point n of the forward sits in workgroup n >> 6,
// wave (n >> 4) & 3, lane column n & 15 of the saved register images (zs_index), so a launch covers
// any contiguous instance range [0, n_inst) of a segment at offset offA of the forward's point set.
// Pair mode: the two points of instance i (offA + i, offB + i) sit in adjacent columns (p, p ^ 1); the
// cross blocks Za[s] . Zb[s'] and Ha[s] . Hb[s'] come from a quad_perm lane swap, and
//   n2 = (aa block + bias_a) + (bb block + bias_b) + 2 (cross + Za[0] . Zb[0]).
#include "jet_common.h"
#include "jet_tanh.h"

namespace {

// Gram matrix of the S rows of a column over the features seen so far: d = the upper triangle of the
// column's own block; x (pair mode) = the full S x S block against the partner column p ^ 1.
template <int S, bool PAIR>
struct Gram {
  static constexpr int ND = S * (S + 1) / 2;
  static constexpr int NX = PAIR ? S * S : 1;
  float d[ND];
  float x[NX];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < ND; ++k) d[k] = 0.f;
#pragma unroll
    for (int k = 0; k < NX; ++k) x[k] = 0.f;
  }

  // one feature of every row
  __device__ __forceinline__ void add(const float (&v)[S]) {
    int k = 0;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int s2 = s; s2 < S; ++s2, ++k) d[k] = fmaf(v[s], v[s2], d[k]);
    if constexpr (PAIR) {
      float pv[S];
#pragma unroll
      for (int s = 0; s < S; ++s) pv[s] = dpp<0xB1>(v[s]);  // quad_perm [1,0,3,2]: column p ^ 1
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) x[s * S + s2] = fmaf(v[s], pv[s2], x[s * S + s2]);
    }
  }

  // the four features of a tile
  __device__ __forceinline__ void add4(const f32x4 (&v)[S]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float f[S];
#pragma unroll
      for (int s = 0; s < S; ++s) f[s] = v[s][c];
      add(f);
    }
  }

  // sum over the four lanes of the column (their features are disjoint)
  __device__ __forceinline__ void reduce() {
#pragma unroll
    for (int k = 0; k < ND; ++k) d[k] = col4_sum(d[k]);
    if constexpr (PAIR) {
#pragma unroll
      for (int k = 0; k < NX; ++k) x[k] = col4_sum(x[k]);
    }
  }
};

// the column's share of one dense layer: own weight block + bias (+ cross block + cross bias)
template <int S, bool PAIR>
__device__ __forceinline__ float layer_term(const Gram<S, PAIR>& gz, const Gram<S, PAIR>& gh) {
  float r = gz.d[0];
  int k = 0;
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int s2 = s; s2 < S; ++s2, ++k) r = fmaf((s == s2 ? 1.f : 2.f) * gz.d[k], gh.d[k], r);
  if constexpr (PAIR) {
    r += gz.x[0];
#pragma unroll
    for (int q = 0; q < S * S; ++q) r = fmaf(gz.x[q], gh.x[q], r);
  }
  return r;
}

template <int WT, int S, bool PAIR>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
ntk_norm_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ Kp,
                const float* __restrict__ dJ, const float* __restrict__ Zs, float* __restrict__ n2, int N,
                int offA, int offB, int n_inst, NetDims d, JetSpec sp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int W = 16 * WT;
  constexpr int IPW = PAIR ? 8 : 16;  // instances per wave
  const int tid = threadIdx.x, l = tid & 63, p = l & 15, g = l >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int inst = ((int)blockIdx.x * 4 + w) * IPW + (PAIR ? (p >> 1) : p);
  const bool valid = inst < n_inst;
  // a column past the range reads instance 0's point with zero seeds: every adjoint is 0
  const int n = ((PAIR && (p & 1)) ? offB : offA) + (valid ? inst : 0);
  const int nwg = (N + 63) / 64;                                  // the forward's grid
  // the point's home in the saved images: workgroup n >> 6, wave (n >> 4) & 3, lane (g, n & 15).  Its float
  // offset inside a (layer, stream, tile) block is per lane, everything else of zs_index is wave-uniform:
  // passed as zs_index's `lane` with workgroup 0 and wave 0, the loads keep a scalar base address
  const int hl = (((n >> 6) * S * 4 + ((n >> 4) & 3)) * WT) * 64 + ((g << 4) | (n & 15));
  constexpr int hg = 0, hw = 0;
  const int Lh = d.n_hidden;
  float* hstage = lds + (size_t)w * (S * WT * 256);
  float acc = 0.f;

  // ---- output layer: Z = the seeds (d_out features), H = h of the last hidden layer ; hb = Ko ub --
  {
    const float* Ko = P + off_layer(d, Lh);
    float ub[S][TDQ_MAXO];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int q = 0; q < TDQ_MAXO; ++q)
        ub[s][q] = (valid && q < d.d_out) ? dJ[((size_t)s * N + n) * d.d_out + q] : 0.f;
    Gram<S, PAIR> gz, gh;
    gz.clear();
    gh.clear();
#pragma unroll
    for (int q = 0; q < TDQ_MAXO; ++q) {
      float f[S];
#pragma unroll
      for (int s = 0; s < S; ++s) f[s] = ub[s][q];
      gz.add(f);
    }
    f32x4 zc[S], zn[S];
    z_load<S, WT>(zc, Zs, Lh - 1, nwg, hg, hw, 0, hl);
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      if (t + 1 < WT) z_load<S, WT>(zn, Zs, Lh - 1, nwg, hg, hw, t + 1, hl);
      f32x4 zl[S][1], hh[S][1], ht[S], hbt[S];
#pragma unroll
      for (int s = 0; s < S; ++s) zl[s][0] = zc[s];
      tanh_jet_fwd<S, 1>(sp, zl, 0, hh, 0);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        ht[s] = hh[s][0];
        hbt[s] = zero4();
      }
      gh.add4(ht);
#pragma unroll
      for (int q = 0; q < TDQ_MAXO; ++q) {
        if (q >= d.d_out) break;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int f = 16 * t + 4 * g + c;
          const float kq = f < d.width ? Ko[f * d.d_out + q] : 0.f;
#pragma unroll
          for (int s = 0; s < S; ++s) hbt[s][c] = fmaf(kq, ub[s][q], hbt[s][c]);
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) *reinterpret_cast<f32x4*>(&hstage[((s * WT + t) * 64 + l) * 4]) = hbt[s];
      if (t + 1 < WT) {
#pragma unroll
        for (int s = 0; s < S; ++s) zc[s] = zn[s];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    gh.reduce();  // (gz: every lane of the column holds all d_out seed features)
    acc += layer_term<S, PAIR>(gz, gh);
  }

  // ---- hidden layers i = Lh-1 .. 1: Z = zb_i, H = h_{i-1} ; hb_{i-1} = K_i zb ------------------------
  for (int i = Lh - 1; i >= 1; --i) {
    // the Gram of h_{i-1} first: nothing but the accumulators is live across it (zb comes after)
    Gram<S, PAIR> gh;
    gh.clear();
    {
      f32x4 zc[S], zn[S];
      z_load<S, WT>(zc, Zs, i - 1, nwg, hg, hw, 0, hl);
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        if (t + 1 < WT) z_load<S, WT>(zn, Zs, i - 1, nwg, hg, hw, t + 1, hl);
        f32x4 zl[S][1], hh[S][1], ht[S];
#pragma unroll
        for (int s = 0; s < S; ++s) zl[s][0] = zc[s];
        tanh_jet_fwd<S, 1>(sp, zl, 0, hh, 0);
#pragma unroll
        for (int s = 0; s < S; ++s) ht[s] = hh[s][0];
        gh.add4(ht);
        if (t + 1 < WT) {
#pragma unroll
          for (int s = 0; s < S; ++s) zc[s] = zn[s];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    gh.reduce();
    Gram<S, PAIR> gz;
    gz.clear();
    f32x4 zb[S][WT];
    {
      f32x4 zc[S], zn[S];
      z_load<S, WT>(zc, Zs, i, nwg, hg, hw, 0, hl);
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        if (t + 1 < WT) z_load<S, WT>(zn, Zs, i, nwg, hg, hw, t + 1, hl);
        f32x4 hh[S], oo[S];
#pragma unroll
        for (int s = 0; s < S; ++s) hh[s] = *reinterpret_cast<const f32x4*>(&hstage[((s * WT + t) * 64 + l) * 4]);
        tanh_jet_bwd<S>(sp, zc, hh, oo);
        gz.add4(oo);
#pragma unroll
        for (int s = 0; s < S; ++s) zb[s][t] = oo[s];
        if (t + 1 < WT) {
#pragma unroll
          for (int s = 0; s < S; ++s) zc[s] = zn[s];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    gz.reduce();
    acc += layer_term<S, PAIR>(gz, gh);
    // hb_{i-1} = K_i zb  (MFMA; A = padded [in][out] image from global, B = zb registers)
    {
      const float* Ki = Kp + (size_t)(i - 1) * W * W + (unsigned)(p * W + 4 * g);
      f32x4 a_cur = *reinterpret_cast<const f32x4*>(Ki);
#pragma unroll
      for (int o = 0; o < WT; ++o) {
        f32x4 hb[S];
#pragma unroll
        for (int s = 0; s < S; ++s) hb[s] = zero4();
#pragma unroll
        for (int t = 0; t < WT; ++t) {
          const int nt = (t + 1 < WT) ? t + 1 : 0, no = (t + 1 < WT) ? o : o + 1;
          f32x4 a_nxt = a_cur;
          if (no < WT) a_nxt = *reinterpret_cast<const f32x4*>(Ki + (size_t)16 * no * W + 16 * nt);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < S; ++s) hb[s] = mfma16x16x4(a_cur[r], zb[s][t][r], hb[s]);
          a_cur = a_nxt;
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int s = 0; s < S; ++s) *reinterpret_cast<f32x4*>(&hstage[((s * WT + o) * 64 + l) * 4]) = hb[s];
      }
    }
  }

  // ---- first layer: Z = zb_0, H = the input jets (x on the value stream, e_a on a first-order stream
  //      in variable a, 0 on second-order streams): d_in features that every lane holds in full
  {
    Gram<S, PAIR> gz, gh;
    gz.clear();
    gh.clear();
    f32x4 zc[S], zn[S];
    z_load<S, WT>(zc, Zs, 0, nwg, hg, hw, 0, hl);
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      if (t + 1 < WT) z_load<S, WT>(zn, Zs, 0, nwg, hg, hw, t + 1, hl);
      f32x4 hh[S], oo[S];
#pragma unroll
      for (int s = 0; s < S; ++s) hh[s] = *reinterpret_cast<const f32x4*>(&hstage[((s * WT + t) * 64 + l) * 4]);
      tanh_jet_bwd<S>(sp, zc, hh, oo);
      gz.add4(oo);
      if (t + 1 < WT) {
#pragma unroll
        for (int s = 0; s < S; ++s) zc[s] = zn[s];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < TDQ_MAXD; ++j) {
      const float xj = j < d.d_in ? X[(size_t)n * d.d_in + j] : 0.f;
      float f[S];
      f[0] = xj;
#pragma unroll
      for (int s = 1; s < S; ++s) f[s] = (sp.stype[s] == 1 && sp.var[s] == j && j < d.d_in) ? 1.f : 0.f;
      gh.add(f);
    }
    gz.reduce();
    acc += layer_term<S, PAIR>(gz, gh);
  }

  if constexpr (PAIR) acc += dpp<0xB1>(acc);  // the instance's two columns
  if (valid && g == 0 && (!PAIR || !(p & 1))) n2[inst] = acc;
}

// out[0] = sum of v[0 .. n) in a fixed order (thread-strided partials, then a tree): bitwise repeatable
__global__ void __launch_bounds__(256) ntk_sum_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ float sh[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

size_t norm_lds_bytes(int WT, int S) { return (size_t)4 * S * WT * 256 * sizeof(float); }

template <int WT, int S, bool PAIR>
int launch_norm_p(const float* X, const float* P, const float* Kp, const float* dJ, const float* Zs, float* n2, int N,
                  int offA, int offB, int n_inst, NetDims d, JetSpec sp, hipStream_t st) {
  constexpr int IPG = PAIR ? 32 : 64;  // instances per workgroup
  const int nwg = (n_inst + IPG - 1) / IPG;
  const size_t lds = norm_lds_bytes(WT, S);
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&ntk_norm_kernel<WT, S, PAIR>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = true;
  }
  hipLaunchKernelGGL((ntk_norm_kernel<WT, S, PAIR>), dim3(nwg), dim3(256), lds, st, X, P, Kp, dJ, Zs, n2, N, offA,
                     offB, n_inst, d, sp);
  TDQ_CHECK_LAUNCH();
  return 0;
}

template <int WT, int S>
int launch_norm(const float* X, const float* P, const float* Kp, const float* dJ, const float* Zs, float* n2, int N,
                int offA, int offB, int n_inst, NetDims d, JetSpec sp, hipStream_t st) {
  if (offB >= 0) return launch_norm_p<WT, S, true>(X, P, Kp, dJ, Zs, n2, N, offA, offB, n_inst, d, sp, st);
  return launch_norm_p<WT, S, false>(X, P, Kp, dJ, Zs, n2, N, offA, offB, n_inst, d, sp, st);
}

#define NTK_DISPATCH_S(WT_, ...)                                             \
  switch (S) {                                                               \
    case 1: return launch_norm<WT_, 1>(__VA_ARGS__);                         \
    case 2: return launch_norm<WT_, 2>(__VA_ARGS__);                         \
    case 3: return launch_norm<WT_, 3>(__VA_ARGS__);                         \
    case 4: return launch_norm<WT_, 4>(__VA_ARGS__);                         \
    default: break;                                                          \
  }                                                                          \
  if (WT_ * 8 <= 32) switch (S) {                                            \
      case 5: return launch_norm<(WT_ <= 4 ? WT_ : 4), 5>(__VA_ARGS__);      \
      case 6: return launch_norm<(WT_ <= 4 ? WT_ : 4), 6>(__VA_ARGS__);      \
      case 7: return launch_norm<(WT_ <= 4 ? WT_ : 4), 7>(__VA_ARGS__);      \
      case 8: return launch_norm<(WT_ <= 4 ? WT_ : 4), 8>(__VA_ARGS__);      \
      default: break;                                                        \
    }                                                                        \
  return (int)hipErrorInvalidValue;

}  // namespace

extern "C" {

// n2[i] = || d f_i / d theta ||^2 for the instances i < n_inst of one loss output.
//   X (N, d_in), dJ (S, N, d_out): the points and the seeds d f / d J of the forward's whole point set;
//   Zs: that forward's saved pre-activation streams (the scratch of tdq_jet_fwd over the same N points);
//   Kp: the [in][out] weight images of tdq_jet_pad_kp;
//   instance i is point offA + i, or the pair (offA + i, offB + i) when offB >= 0.
// Shapes outside the exact-fp32 envelope (order <= 2, equal widths <= 128, S x width tiles <= 32,
// d_in <= 8, d_out <= 4, <= 16 hidden layers) and ranges outside the point set are hipErrorInvalidValue.
int tdq_ntk_norm(const float* X, const float* P, const float* Kp, const float* dJ, const float* Zs, float* n2, int N,
                 int offA, int offB, int n_inst, int d_in, int width, int d_out, int n_hidden, int S, const int* spec,
                 void* stream) {
  if (n_inst == 0) return 0;
  const int WT = width_tiles(width);
  JetSpec sp;
  if (WT < 0 || WT > 8 || S * WT > 32 || d_in < 1 || d_in > TDQ_MAXD || d_out < 1 || d_out > TDQ_MAXO ||
      n_hidden < 1 || n_hidden > TDQ_MAXL || !make_spec(S, spec, sp))
    return (int)hipErrorInvalidValue;
  if ((int64_t)N * S * WT >= ((int64_t)1 << 27)) return (int)hipErrorInvalidValue;  // 32-bit lane offsets
  if (n_inst < 0 || N < 1 || offA < 0 || (int64_t)offA + n_inst > N || (offB >= 0 && (int64_t)offB + n_inst > N))
    return (int)hipErrorInvalidValue;
  for (int s = 0; s < S; ++s)  // a first-order stream names an input variable (the first layer reads x[var])
    if (sp.stype[s] == 1 && sp.var[s] >= d_in) return (int)hipErrorInvalidValue;
  NetDims d = uniform_dims(d_in, width, d_out, n_hidden);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (WT) {
    case 1: { NTK_DISPATCH_S(1, X, P, Kp, dJ, Zs, n2, N, offA, offB, n_inst, d, sp, st) }
    case 2: { NTK_DISPATCH_S(2, X, P, Kp, dJ, Zs, n2, N, offA, offB, n_inst, d, sp, st) }
    case 4: { NTK_DISPATCH_S(4, X, P, Kp, dJ, Zs, n2, N, offA, offB, n_inst, d, sp, st) }
    case 8: { NTK_DISPATCH_S(8, X, P, Kp, dJ, Zs, n2, N, offA, offB, n_inst, d, sp, st) }
    default: return (int)hipErrorInvalidValue;
  }
}

// out[0] = sum_i n2[i], i < n, in a fixed order (two calls give the same bits)
int tdq_ntk_sum(const float* n2, int n, float* out, void* stream) {
  if (n < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ntk_sum_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), n2, n, out);
  TDQ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
