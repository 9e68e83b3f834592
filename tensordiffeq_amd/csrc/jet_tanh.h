// Per-tile building blocks of the exact-fp32 jet kernels: the tanh jet of one 16-feature tile
// (forward and adjoint) and the loads of the saved pre-activation streams.  Shared by the
// forward / backward kernels (jet_mlp.hip) and the per-instance gradient-norm kernel (ntk_trace.hip).
#pragma once
#include "jet_common.h"

template <int S, int WT>
__device__ __forceinline__ f32x4 pick(const f32x4 (&v)[S][WT], const float (&sel)[TDQ_MAXS], int t) {
  f32x4 r = zero4();
#pragma unroll
  for (int q = 1; q < S; ++q) r += sel[q] * v[q][t];
  return r;
}

// forward tanh jet on feature tile t: z -> h  (in place allowed: writes h after reading z)
template <int S, int WT>
__device__ __forceinline__ void tanh_jet_fwd(const JetSpec sp, const f32x4 (&z)[S][WT], int t,
                                             f32x4 (&h)[S][WT], int to) {
  f32x4 za2[S], zb2[S];
#pragma unroll
  for (int s = 1; s < S; ++s) {
    if (sp.stype[s] == 2) {
      za2[s] = pick<S, WT>(z, sp.selA[s], t);
      zb2[s] = pick<S, WT>(z, sp.selB[s], t);
    } else {
      za2[s] = zero4();
      zb2[s] = zero4();
    }
  }
  f32x4 zz[S];
#pragma unroll
  for (int s = 0; s < S; ++s) zz[s] = z[s][t];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float hv = tanhf(zz[0][c]);
    const float s1 = 1.f - hv * hv;
    const float s2 = -2.f * hv * s1;
    h[0][to][c] = hv;
#pragma unroll
    for (int s = 1; s < S; ++s) {
      float v = s1 * zz[s][c];
      if (sp.stype[s] == 2) v = fmaf(s2 * za2[s][c], zb2[s][c], v);
      h[s][to][c] = v;
    }
  }
}

template <int S>
__device__ __forceinline__ void tanh_jet_bwd(const JetSpec sp, const f32x4 (&z)[S], const f32x4 (&hb)[S],
                                             f32x4 (&zb)[S]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float hv = tanhf(z[0][c]);
    const float s1 = 1.f - hv * hv;
    const float s2 = -2.f * hv * s1;
    const float s3 = -2.f * s1 * s1 - 2.f * hv * s2;
    float sb1 = 0.f, sb2 = 0.f;
    float zbv[S];
    zbv[0] = s1 * hb[0][c];
#pragma unroll
    for (int s = 1; s < S; ++s) {
      zbv[s] = s1 * hb[s][c];
      sb1 = fmaf(z[s][c], hb[s][c], sb1);
    }
#pragma unroll
    for (int s = 1; s < S; ++s) {
      if (sp.stype[s] == 2) {
        float za = 0.f, zbb = 0.f;
#pragma unroll
        for (int q = 1; q < S; ++q) {
          za = fmaf(sp.selA[s][q], z[q][c], za);
          zbb = fmaf(sp.selB[s][q], z[q][c], zbb);
        }
        const float hbs = hb[s][c];
        sb2 = fmaf(za * zbb, hbs, sb2);
        const float ga = s2 * zbb * hbs, gb = s2 * za * hbs;
#pragma unroll
        for (int q = 1; q < S; ++q) zbv[q] = fmaf(sp.selA[s][q], ga, fmaf(sp.selB[s][q], gb, zbv[q]));
      }
    }
    zbv[0] = fmaf(s2, sb1, fmaf(s3, sb2, zbv[0]));
#pragma unroll
    for (int s = 0; s < S; ++s) zb[s][c] = zbv[s];
  }
}

// saved pre-activation streams needed to rebuild h stream `s` of a layer on one feature tile
struct HLoad {
  f32x4 z0, zs, za, zb;
};

template <int S>
__device__ __forceinline__ void h_load(HLoad& L, const JetSpec sp, const float* __restrict__ Zs, int layer,
                                       int nwg, int wg, int s, int w, int WT, int t, int lane) {
  L.z0 = *reinterpret_cast<const f32x4*>(Zs + zs_index(layer, nwg, wg, S, 0, w, WT, t, lane));
  L.zs = L.za = L.zb = zero4();
  if (s > 0) L.zs = *reinterpret_cast<const f32x4*>(Zs + zs_index(layer, nwg, wg, S, s, w, WT, t, lane));
  if (sp.stype[s] == 2) {
    L.za = *reinterpret_cast<const f32x4*>(Zs + zs_index(layer, nwg, wg, S, sp.ia[s], w, WT, t, lane));
    L.zb = *reinterpret_cast<const f32x4*>(Zs + zs_index(layer, nwg, wg, S, sp.ib[s], w, WT, t, lane));
  }
}

__device__ __forceinline__ f32x4 h_compute(const HLoad& L, const JetSpec sp, int s) {
  f32x4 out;
  const bool second = sp.stype[s] == 2;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float hv = tanhf(L.z0[c]);
    const float s1 = 1.f - hv * hv;
    const float s2 = -2.f * hv * s1;
    const float v = second ? fmaf(s2 * L.za[c], L.zb[c], s1 * L.zs[c]) : s1 * L.zs[c];
    out[c] = s == 0 ? hv : v;
  }
  return out;
}

template <int S, int WT>
__device__ __forceinline__ void z_load(f32x4 (&z)[S], const float* __restrict__ Zs, int layer, int nwg, int wg,
                                       int w, int t, int lane) {
#pragma unroll
  for (int s = 0; s < S; ++s) z[s] = *reinterpret_cast<const f32x4*>(Zs + zs_index(layer, nwg, wg, S, s, w, WT, t, lane));
}

// zero-padded [in][out] images of the hidden kernels (the A operand of hb = K zb) at `img`:
// (n_hidden - 1) x W x W floats, W = 16 width_tiles(width)
extern "C" int tdq_jet_pad_kp(const float* P, float* img, int d_in, int width, int d_out, int n_hidden, void* stream);
