// One dense layer's share of the per-instance squared parameter-gradient norm (NTK loss weighting,
// ops/ntk.py), from plain fp32 row-major planes, gfx950.
//
// H [S N][ldh] holds the layer's input rows and Z [S N][ldz] its pre-activation adjoints: row s N + n is
// stream s of point n.  With the rows r of instance i - the S streams of point offA + i, in pair mode
// (offB >= 0) the 2 S rows of the points offA + i and offB + i -
//   n2[i] (+)= sum_{r, r'} (Z[r] . Z[r']) (H[r] . H[r']) + || sum_{value rows} Z[r] ||^2
// (the weight block and the bias of the layer; value rows = stream 0 of each point of the instance).
//
// An instance has R = S or 2 S <= 16 rows, so its Gram matrix V V^T is ONE 16 x 16 accumulator of the
// 16x16x4 fp32 MFMA with A and B from the same register: lane l supplies A[l & 15][l >> 4] and
// B[l >> 4][l & 15], so a lane that holds V[row l & 15][feature k] passes it as both operands (the order
// of k is free - both operands see the same one).  A lane loads four consecutive features
// 16 j + 4 (l >> 4) of its row (the four lanes of a row read 64 contiguous bytes) and issues one MFMA per
// component.  Rows >= R and features >= W are zeros.  One wave per instance: Gh, then Gz (4 VGPRs each);
//   n2 = sum Gz o (Gh + M),   M = 1 on the (value row, value row) entries
// gives the bias term from the same accumulators (D layout: lane l, reg c holds D[4 (l >> 4) + c][l & 15]),
// then one wave reduction in a fixed order.  No LDS, no atomics: two calls give the same bits.
#include "common.h"

namespace {

// Gram accumulator of one plane: this lane's row (nullptr: a zero row) over W features.  VEC: 16-byte
// loads (W, the leading dimension and the base are multiples of 4 floats), else element-wise.
template <bool VEC>
__device__ __forceinline__ f32x4 gram_plane(const float* __restrict__ row, int W, int g) {
  f32x4 acc = zero4();
  const int nj = (W + 15) >> 4;  // (wave-uniform: every lane issues every MFMA)
#pragma unroll 2
  for (int j = 0; j < nj; ++j) {
    const int f = 16 * j + 4 * g;
    f32x4 v = zero4();
    if constexpr (VEC) {
      if (row != nullptr && f < W) v = *reinterpret_cast<const f32x4*>(row + f);  // (W % 4 == 0: all in or out)
    } else {
      if (row != nullptr) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (f + c < W) v[c] = row[f + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc = mfma16x16x4(v[c], v[c], acc);
  }
  return acc;
}

__global__ void __launch_bounds__(256)
ntk_gram_kernel(const float* __restrict__ H, int ldh, int Win, int vech, const float* __restrict__ Z, int ldz,
                int Wout, int vecz, int S, int N, int offA, int offB, int n_inst, int accumulate,
                float* __restrict__ n2) {
  const int l = threadIdx.x & 63, r = l & 15, g = l >> 4;
  const int inst = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (inst >= n_inst) return;  // (wave-uniform)
  const bool pair = offB >= 0;
  const int R = pair ? 2 * S : S;
  // row r: stream r of point offA + inst, in pair mode rows S .. 2 S - 1 the streams of point offB + inst
  const bool live = r < R;
  const int s = r < S ? r : r - S;
  const int n = (r < S ? offA : offB) + inst;
  const int grow = live ? s * N + n : 0;  // (< 2^31 / ld: checked by the host)
  const float* hrow = live ? H + (size_t)grow * ldh : nullptr;
  const float* zrow = live ? Z + (size_t)grow * ldz : nullptr;
  const f32x4 gh = vech ? gram_plane<true>(hrow, Win, g) : gram_plane<false>(hrow, Win, g);
  const f32x4 gz = vecz ? gram_plane<true>(zrow, Wout, g) : gram_plane<false>(zrow, Wout, g);
  // this lane holds D[4 g + c][r]; the value rows are 0 and (pair mode) S
  const bool vcol = r == 0 || (pair && r == S);
  float t = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int dr = 4 * g + c;
    const float m = (vcol && (dr == 0 || (pair && dr == S))) ? 1.f : 0.f;
    t = fmaf(gz[c], gh[c] + m, t);
  }
  // fixed-order butterfly over the 64 lanes
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) t += __shfl_xor(t, k, 64);
  if (l == 0) n2[inst] = accumulate ? n2[inst] + t : t;
}

bool vec_ok(const float* p, long long ld, int W) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0 && (W & 3) == 0;
}

}  // namespace

extern "C" {

// n2[i] (+)= the layer's share of || d f_i / d theta ||^2 for the instances i < n_inst (accumulate: +=).
//   H [S N][ldh] fp32, Win features; Z [S N][ldz] fp32, Wout features; instance i is point offA + i, or the
//   pair (offA + i, offB + i) when offB >= 0.  Nothing outside n2[0 .. n_inst) is written.
// S outside 1..8, widths < 1, a leading dimension below its width, ranges outside the N points and planes
// whose element offsets pass 32 bits are hipErrorInvalidValue.
int tdq_ntk_gram(const float* H, long long ldh, int Win, const float* Z, long long ldz, int Wout, int S, int N,
                 int offA, int offB, int n_inst, int accumulate, float* n2, void* stream) {
  if (S < 1 || S > 8 || Win < 1 || Wout < 1 || ldh < Win || ldz < Wout || N < 1 || n_inst < 0 || offA < 0 ||
      (long long)offA + n_inst > N || (offB >= 0 && (long long)offB + n_inst > N))
    return (int)hipErrorInvalidValue;
  if ((long long)S * N * ldh > 0x7fffffffLL || (long long)S * N * ldz > 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  if (n_inst == 0) return 0;
  if (H == nullptr || Z == nullptr || n2 == nullptr) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((n_inst + 3) / 4));
  hipLaunchKernelGGL(ntk_gram_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), H, (int)ldh, Win,
                     (int)vec_ok(H, ldh, Win), Z, (int)ldz, Wout, (int)vec_ok(Z, ldz, Wout), S, N, offA,
                     offB < 0 ? -1 : offB, n_inst, accumulate != 0, n2);
  TDQ_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
