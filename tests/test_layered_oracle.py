"""The layer-wise jet engine (ops/jet_layered.py, csrc/lay_gemm.hip, csrc/jet_layered.hip,
csrc/lay_reduce.hip) per stream, per layer and per parameter block against float64, at every stream
count S = 1..8 (point tiles of PT = 128 // S), at the point-tile edges (N = 1, PT - 1, PT, PT + 1,
2 PT + 3), the feature-tile edges and every output-layer branch.

Reference (float64, CPU): ``jet_forward`` + autograd of ``<G, J>`` for J and the flat gradient; the
float64 CPU run of the same engine (validated against ``jet_forward`` by
tests/test_layered_jet.py::test_layered_engine_cpu_float64) for the saved per-layer activations.

Comparator: the same inputs through ``TDQ_LAY_GEMM=0`` - the library GEMMs and the standalone epilogue
pass, which share none of the hand-written GEMMs or in-GEMM epilogues.  Its error against float64 on
the same quantity is the yardstick: a quantity's bound is ``max(LTOL[prec][k], 3 x comparator error)``
(k = 0 forward, 1 gradient; LTOL from tests/test_layered_jet.py; 3 the usual margin over a measured
error, tests/test_systems_fused_step.py).  No bound comes from the path under test.

Checked per case and precision, nothing skipped or filtered:
  1. every saved activation ``Hs[i]`` and J, per stream: max abs error / max(|fp64| of that stream
     over the layer, 1e-3);
  2. every parameter block - each input-layer row ``K0[j]`` (rows fed by first-order streams take
     their own route through ``tdq_lay_l0grad``), ``b0``, each hidden ``K_i`` / ``b_i``, each
     output column ``Ko[:, q]`` and each ``bo[q]``: max abs error / the block's max |fp64| (which
     must be non-zero);
  3. the whole-theta relative norm against ``LTOL[prec][1]``.
All failures of a case are collected before the assertion.

Measured on an MI355X (each figure: error of the default path / error of the comparator on the same
quantity; per network and stream count the worst over the listed point counts, with the layer and
stream or the block and the N where it occurred; the line of every single N is in
profiles/r17_layered_oracle_errors.txt).  Every quantity is within its bound, no block needed the
per-block margin of tests/test_hip_kernels.py.  S = 1..8 all ran the GEMM-epilogue path
(``saved[-1]`` asserted); [2, 30, 22, 1] and [10, 36, 20, 1] ran the standalone-epilogue default path.

[2, 36, 20, 1] S=1 N=1,127,128,129,259
  fp32   fwd 4.28e-07 / 4.28e-07 (J s0, N=127)  block 2.28e-06 / 2.09e-06 (K0[1], N=129)  theta 4.29e-07 / 4.22e-07
  bf16x3 fwd 1.21e-05 / 1.74e-05 (J s0, N=127)  block 5.91e-05 / 5.32e-05 (K0[1], N=129)  theta 1.31e-05 / 1.46e-05
  bf16   fwd 5.87e-03 / 6.23e-03 (J s0, N=128)  block 2.90e-02 / 2.87e-02 (K0[1], N=129)  theta 5.77e-03 / 6.23e-03
[2, 36, 20, 1] S=2 N=1,63,64,65,131
  fp32   fwd 4.78e-07 / 4.63e-07 (J s1, N=64)  block 1.80e-06 / 1.35e-06 (K0[0], N=64)  theta 4.27e-07 / 3.48e-07
  bf16x3 fwd 2.32e-05 / 2.58e-05 (J s1, N=64)  block 2.73e-05 / 2.56e-05 (b0, N=131)  theta 1.10e-05 / 1.09e-05
  bf16   fwd 1.43e-02 / 1.83e-02 (J s1, N=64)  block 1.76e-02 / 1.76e-02 (K0[0], N=64)  theta 5.00e-03 / 6.03e-03
[2, 36, 20, 1] S=3 N=1,41,42,43,87
  fp32   fwd 9.05e-07 / 1.02e-06 (J s2, N=43)  block 1.78e-06 / 1.11e-08 (bo[0], N=41)  theta 2.33e-07 / 2.23e-07
  bf16x3 fwd 2.74e-05 / 4.83e-05 (J s2, N=43)  block 1.98e-05 / 4.52e-06 (b1, N=41)  theta 7.17e-06 / 5.96e-06
  bf16   fwd 1.34e-02 / 1.43e-02 (J s2, N=43)  block 6.15e-03 / 6.15e-03 (K0[0], N=42)  theta 3.72e-03 / 3.92e-03
[2, 36, 20, 1] S=4 N=1,31,32,33,67
  fp32   fwd 1.54e-06 / 1.25e-06 (J s2, N=67)  block 1.06e-06 / 4.96e-07 (bo[0], N=32)  theta 2.49e-07 / 2.64e-07
  bf16x3 fwd 8.59e-05 / 6.87e-05 (J s2, N=67)  block 2.00e-05 / 1.61e-05 (b0, N=67)  theta 5.41e-06 / 5.26e-06
  bf16   fwd 2.77e-02 / 2.97e-02 (J s2, N=67)  block 6.99e-03 / 6.99e-03 (K1, N=33)  theta 2.83e-03 / 2.96e-03
[2, 36, 20, 1] S=5 N=1,24,25,26,53
  fp32   fwd 3.31e-06 / 3.28e-06 (J s1, N=25)  block 1.73e-06 / 2.07e-06 (b0, N=25)  theta 2.66e-07 / 3.36e-07
  bf16x3 fwd 8.37e-05 / 1.02e-04 (J s1, N=25)  block 4.83e-05 / 4.38e-05 (b0, N=25)  theta 8.94e-06 / 8.58e-06
  bf16   fwd 4.27e-02 / 5.41e-02 (J s1, N=25)  block 6.53e-03 / 6.52e-03 (b1, N=25)  theta 3.60e-03 / 3.84e-03
[2, 36, 20, 1] S=6 N=1,20,21,22,45
  fp32   fwd 9.75e-07 / 6.88e-07 (J s2, N=20)  block 8.36e-07 / 9.05e-07 (K1, N=22)  theta 4.13e-07 / 4.14e-07
  bf16x3 fwd 2.70e-05 / 3.45e-05 (J s2, N=20)  block 1.39e-05 / 9.10e-06 (b0, N=22)  theta 1.25e-05 / 1.21e-05
  bf16   fwd 1.09e-02 / 1.85e-02 (J s2, N=20)  block 6.03e-03 / 6.03e-03 (K0[0], N=22)  theta 4.98e-03 / 5.19e-03
[3, 36, 20, 1] S=7 N=1,17,18,19,39
  fp32   fwd 1.52e-06 / 6.73e-07 (J s3, N=19)  block 1.01e-06 / 1.34e-06 (b0, N=17)  theta 2.08e-07 / 2.54e-07
  bf16x3 fwd 3.67e-05 / 3.76e-05 (J s1, N=39)  block 2.11e-05 / 2.05e-05 (b0, N=17)  theta 5.69e-06 / 5.10e-06
  bf16   fwd 1.89e-02 / 1.93e-02 (J s3, N=19)  block 6.64e-03 / 6.64e-03 (K0[2], N=19)  theta 2.81e-03 / 2.80e-03
[3, 36, 20, 1] S=8 N=1,15,16,17,35
  fp32   fwd 2.01e-06 / 7.47e-07 (J s3, N=1)  block 7.68e-07 / 7.18e-07 (K0[0], N=15)  theta 2.41e-07 / 2.37e-07
  bf16x3 fwd 1.34e-04 / 1.23e-04 (J s3, N=16)  block 2.02e-05 / 1.60e-05 (K0[2], N=35)  theta 5.93e-06 / 6.10e-06
  bf16   fwd 3.74e-02 / 3.27e-02 (J s3, N=1)  block 5.46e-03 / 5.46e-03 (K0[0], N=15)  theta 3.47e-03 / 3.71e-03
[2, 132, 68, 2] S=4 N=33
  fp32   fwd 1.05e-06 / 1.13e-06 (J s1, N=33)  block 3.46e-07 / 4.42e-07 (K1, N=33)  theta 2.09e-07 / 2.21e-07
  bf16x3 fwd 2.23e-05 / 2.68e-05 (J s1, N=33)  block 8.30e-06 / 9.17e-06 (Ko[:,1], N=33)  theta 4.66e-06 / 6.77e-06
  bf16   fwd 9.10e-03 / 1.30e-02 (J s1, N=33)  block 3.69e-03 / 3.42e-03 (Ko[:,0], N=33)  theta 2.21e-03 / 3.14e-03
[2, 132, 68, 2] S=5 N=26
  fp32   fwd 8.93e-07 / 1.03e-06 (J s2, N=26)  block 1.33e-06 / 1.43e-06 (Ko[:,1], N=26)  theta 2.88e-07 / 2.84e-07
  bf16x3 fwd 2.13e-05 / 3.05e-05 (J s2, N=26)  block 1.64e-05 / 1.58e-05 (Ko[:,1], N=26)  theta 6.89e-06 / 9.70e-06
  bf16   fwd 9.30e-03 / 2.01e-02 (J s2, N=26)  block 3.41e-03 / 4.03e-03 (Ko[:,0], N=26)  theta 3.51e-03 / 5.65e-03
[2, 64, 136, 1] S=4 N=33
  fp32   fwd 4.16e-07 / 3.71e-07 (H1 s1, N=33)  block 1.35e-06 / 1.74e-06 (K0[0], N=33)  theta 2.01e-07 / 2.03e-07
  bf16x3 fwd 8.89e-06 / 9.10e-06 (H1 s1, N=33)  block 1.78e-05 / 1.80e-05 (K0[0], N=33)  theta 4.34e-06 / 4.50e-06
  bf16   fwd 4.34e-03 / 4.34e-03 (H1 s3, N=33)  block 7.86e-03 / 7.86e-03 (K0[0], N=33)  theta 2.37e-03 / 2.50e-03
[2, 64, 136, 1] S=5 N=26
  fp32   fwd 6.49e-07 / 5.68e-07 (J s2, N=26)  block 7.99e-07 / 5.25e-07 (K0[1], N=26)  theta 2.07e-07 / 2.19e-07
  bf16x3 fwd 1.04e-05 / 8.56e-06 (H1 s3, N=26)  block 6.99e-06 / 5.80e-06 (K0[1], N=26)  theta 3.43e-06 / 3.89e-06
  bf16   fwd 4.55e-03 / 3.59e-03 (J s4, N=26)  block 2.55e-03 / 2.55e-03 (K0[1], N=26)  theta 1.69e-03 / 2.00e-03
[2, 36, 6] S=4 N=1,33
  fp32   fwd 3.22e-07 / 2.20e-07 (J s1, N=33)  block 2.73e-07 / 2.20e-07 (Ko[:,2], N=33)  theta 1.21e-07 / 1.06e-07
  bf16x3 fwd 1.36e-05 / 1.36e-05 (J s2, N=33)  block 9.62e-06 / 7.88e-06 (Ko[:,4], N=1)  theta 3.36e-06 / 3.78e-06
  bf16   fwd 5.82e-03 / 5.82e-03 (J s2, N=33)  block 3.96e-03 / 3.96e-03 (K0[0], N=33)  theta 1.73e-03 / 2.22e-03
[2, 36, 3] S=4 N=1,33
  fp32   fwd 2.39e-07 / 1.90e-07 (J s2, N=33)  block 2.69e-07 / 3.25e-07 (Ko[:,1], N=33)  theta 1.23e-07 / 1.04e-07
  bf16x3 fwd 1.30e-05 / 1.29e-05 (J s1, N=33)  block 4.37e-06 / 9.66e-06 (Ko[:,0], N=33)  theta 1.72e-06 / 3.30e-06
  bf16   fwd 7.32e-03 / 7.32e-03 (J s2, N=1)  block 4.37e-06 / 5.62e-03 (Ko[:,0], N=33)  theta 1.72e-06 / 1.73e-03
[2, 36, 20, 6] S=4 N=1,33
  fp32   fwd 4.14e-07 / 3.27e-07 (H1 s3, N=33)  block 4.29e-07 / 7.56e-07 (Ko[:,0], N=33)  theta 1.96e-07 / 2.18e-07
  bf16x3 fwd 9.62e-06 / 9.62e-06 (H1 s3, N=1)  block 8.94e-06 / 8.82e-06 (b0, N=1)  theta 7.27e-06 / 7.27e-06
  bf16   fwd 5.81e-03 / 5.81e-03 (J s1, N=33)  block 7.50e-03 / 7.50e-03 (K1, N=1)  theta 3.92e-03 / 4.06e-03
[2, 36, 20, 70] S=4 N=1,33
  fp32   fwd 4.06e-07 / 3.68e-07 (H1 s3, N=33)  block 1.61e-06 / 1.42e-06 (Ko[:,17], N=33)  theta 2.33e-07 / 2.18e-07
  bf16x3 fwd 1.06e-05 / 1.06e-05 (J s1, N=1)  block 3.48e-05 / 2.64e-05 (Ko[:,35], N=33)  theta 5.96e-06 / 5.99e-06
  bf16   fwd 5.41e-03 / 5.41e-03 (J s1, N=1)  block 1.09e-02 / 1.09e-02 (Ko[:,13], N=33)  theta 3.40e-03 / 3.40e-03
[2, 30, 22, 1] S=4 N=1,43
  fp32   fwd 6.15e-06 / 1.26e-05 (J s3, N=1)  block 7.36e-07 / 5.93e-07 (K0[0], N=43)  theta 3.06e-07 / 3.01e-07
  bf16x3 fwd 1.49e-04 / 2.38e-04 (J s3, N=1)  block 8.92e-06 / 8.92e-06 (b0, N=1)  theta 9.26e-06 / 9.22e-06
  bf16   fwd 4.77e-01 / 4.77e-01 (J s3, N=1)  block 6.17e-03 / 6.17e-03 (K1, N=43)  theta 5.01e-03 / 5.01e-03
[10, 36, 20, 1] S=5 N=1,43
  fp32   fwd 3.46e-07 / 3.72e-07 (J s1, N=43)  block 7.53e-07 / 5.93e-07 (K0[3], N=43)  theta 2.84e-07 / 2.46e-07
  bf16x3 fwd 2.12e-05 / 2.12e-05 (J s1, N=43)  block 1.39e-05 / 1.27e-05 (K0[3], N=43)  theta 4.43e-06 / 4.50e-06
  bf16   fwd 1.84e-02 / 1.84e-02 (J s1, N=43)  block 6.41e-03 / 6.41e-03 (K0[3], N=43)  theta 2.79e-03 / 2.79e-03

The 4.77e-01 of bf16 [2, 30, 22, 1] at N = 1 (J, stream 3) is bf16 rounding, not an O(1) error: the
float64 second derivative at that single point is 5.4e-04, below the 1e-3 clamp of the scale, the sum
of bf16-rounded terms of size 0.1 - 0.4; the absolute error is 4.8e-04 on both paths, which round the
same operands.  In bf16 [2, 36, 3] (one hidden layer, d_out <= 4) the default path's gradient has no
bf16 GEMM at all (exact-fp32 input layer, FMA output-layer adjoint), hence 4e-06 against 6e-03.
"""
import functools

import pytest
import torch

from tensordiffeq_amd.jet import JetPlan, jet_forward
from tensordiffeq_amd.models.networks import TanhMLP
from tests.test_layered_jet import LTOL

pytestmark = pytest.mark.gpu

PRECS = ("fp32", "bf16x3", "bf16")
MARGIN = 3            # over the comparator's measured error (tests/test_systems_fused_step.py)

# one plan per stream count
PLANS = {
    1: (2, []),
    2: (2, [(0,)]),
    3: (2, [(0, 0)]),
    4: (2, [(0,), (1,), (0, 0)]),
    5: (2, [(0, 0), (1, 1)]),
    6: (2, [(0, 0), (0, 1), (1, 1)]),
    7: (3, [(0,), (1,), (2,), (0, 0), (1, 1), (0, 1)]),
    8: (3, [(0, 0), (1, 1), (2, 2), (0, 1)]),
}


def _edge_counts(S):
    PT = 128 // S
    return [n for n in (1, PT - 1, PT, PT + 1, 2 * PT + 3) if n > 0]


@functools.lru_cache(maxsize=None)
def _case(sizes, reqs, N):
    """Inputs and the float64 reference of one case (CPU tensors; shared by the precisions, never
    modified): the net, X, G, plan, J, the per-layer activations, the flat gradient."""
    from tensordiffeq_amd.ops import jet_layered
    sizes, reqs = list(sizes), [tuple(r) for r in reqs]
    torch.manual_seed(1000 * len(sizes) + 100 * len(reqs) + N)
    net = TanhMLP(sizes)
    with torch.no_grad():
        net.flat.add_(0.05 * torch.randn_like(net.flat))
    X = torch.rand(N, sizes[0]) * 2 - 1
    plan = JetPlan(reqs, sizes[0])
    G = torch.randn(plan.S, N, sizes[-1])
    p64 = net.flat.detach().double().clone().requires_grad_(True)
    Jr = jet_forward(X.double(), net.weights(p64), plan)
    (Jr * G.double()).sum().backward()
    _, saved = jet_layered.forward_raw(X.double(), net.flat.detach().double(), net, plan)
    Hr = [h.reshape(plan.S, N, -1) for h in saved[5]]
    return net, X, G, plan, Jr.detach(), Hr, p64.grad


def _blocks(net, sizes):
    """(name, index into the flat vector) of every checked parameter block."""
    out = []
    idx = torch.arange(net.flat.numel())
    ws = net.weights(idx)
    last = len(ws) - 1
    for i, (K, b) in enumerate(ws):
        if i == 0:
            out += [(f"K0[{j}]", K[j]) for j in range(K.shape[0])] + [("b0", b)]
        elif i == last:
            out += [(f"Ko[:,{q}]", K[:, q]) for q in range(K.shape[1])] + [(f"bo[{q}]", b[q:q + 1]) for q in range(K.shape[1])]
        else:
            out += [(f"K{i}", K.reshape(-1)), (f"b{i}", b)]
    assert sorted(torch.cat([ix.reshape(-1) for _, ix in out]).tolist()) == idx.tolist()   # every parameter, once
    return out


def _planes(H, S, N):
    x = H[0].float() + H[1].float() if isinstance(H, tuple) else H
    return x.double().reshape(S, N, -1).cpu()


def _run(net, X, G, plan, prec):
    """``(J, [Hs_i], grad, epilogue path?)`` of the engine on the GPU, as float64 CPU tensors."""
    from tensordiffeq_amd.ops import jet_layered
    P = net.flat.detach().cuda()
    J, saved = jet_layered.forward_raw(X.cuda(), P, net, plan, prec)
    Hs = [_planes(H, plan.S, X.shape[0]) for H in saved[5]]
    g = jet_layered.backward_raw(saved, G.cuda())
    return J.double().cpu(), Hs, g.double().cpu(), bool(saved[-1])


def _errors(net, sizes, ref, out):
    """({(layer, stream): err}, {block: err}, whole-theta relative norm) of one run against float64."""
    _, _, _, plan, Jr, Hr, gr = ref
    J, Hs, g, _ = out
    fwd = {}
    assert len(Hs) == len(Hr) == len(sizes) - 2
    for name, a, r in [(f"H{i}", Hs[i], Hr[i]) for i in range(len(Hr))] + [("J", J, Jr)]:
        assert a.shape == r.shape, (name, a.shape, r.shape)
        scale = r.abs().amax(dim=(1, 2)).clamp_min(1e-3)
        e = (a - r).abs().amax(dim=(1, 2)) / scale
        for s in range(plan.S):
            fwd[(name, s)] = e[s].item()
    blk = {}
    for name, ix in _blocks(net, sizes):
        rmax = gr[ix].abs().max().item()
        assert rmax > 0, f"reference block {name} is all zero"
        blk[name] = (g[ix] - gr[ix]).abs().max().item() / rmax
    return fwd, blk, ((g - gr).norm() / gr.norm()).item()


def _check(monkeypatch, prec, sizes, reqs, N, want_S, want_fused):
    """One case: the default path and the library comparator against float64; returns the list of
    failures (strings).  Prints the case's LAYERED_ORACLE line."""
    ref = _case(tuple(sizes), tuple(reqs), N)
    net, X, G, plan = ref[:4]
    assert plan.S == want_S
    monkeypatch.delenv("TDQ_LAY_GEMM", raising=False)
    monkeypatch.delenv("TDQ_LAY_FUSED", raising=False)
    out = _run(net, X, G, plan, prec)
    assert out[3] is want_fused, "GEMM-epilogue path" if want_fused else "standalone-epilogue path"
    monkeypatch.setenv("TDQ_LAY_GEMM", "0")
    cmp_ = _run(net, X, G, plan, prec)
    monkeypatch.delenv("TDQ_LAY_GEMM")
    assert cmp_[3] is False
    fwd, blk, rel = _errors(net, sizes, ref, out)
    cfwd, cblk, crel = _errors(net, sizes, ref, cmp_)
    tag = f"{prec} {sizes} S={plan.S} N={N}"
    fails, worst = [], []
    for what, err, cerr, tol in (("fwd", fwd, cfwd, LTOL[prec][0]), ("block", blk, cblk, LTOL[prec][1])):
        w = None
        for k, e in err.items():
            bound = max(tol, MARGIN * cerr[k])
            if not e <= bound:
                fails.append(f"{tag} {what} {k}: {e:.3e} > bound {bound:.3e} (comparator {cerr[k]:.3e})")
            if w is None or not e / bound <= w[0]:
                w = (e / bound, k, e, cerr[k])
        worst.append(w)
    if not rel < LTOL[prec][1]:
        fails.append(f"{tag} whole-theta rel {rel:.3e} >= {LTOL[prec][1]:.1e} (comparator {crel:.3e})")
    (_, fk, fe, fc), (_, bk, be, bc) = worst
    print(f"LAYERED_ORACLE {tag} worst fwd {fk[0]} s{fk[1]} {fe:.2e} / {fc:.2e} worst block {bk} {be:.2e} / {bc:.2e} "
          f"theta {rel:.2e} / {crel:.2e}")
    return fails


# ---- A: every stream count at every point-tile edge (GEMM-epilogue path, J formed with the last hidden layer)

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S", sorted(PLANS))
def test_every_stream_count_at_tile_edges(S, prec, monkeypatch):
    d_in, reqs = PLANS[S]
    fails = []
    for N in _edge_counts(S):
        fails += _check(monkeypatch, prec, [d_in, 36, 20, 1], reqs, N, S, True)
    assert not fails, "\n".join(fails)


# ---- B: feature-dimension edges: Nout over the 128-column tile and the 64-column J group; K = 132 (not
# a multiple of 8: element-wise loads) and K = 64 / 136 (vector loads)

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S", [4, 5])
@pytest.mark.parametrize("sizes", [[2, 132, 68, 2], [2, 64, 136, 1]])
def test_feature_tile_edges(sizes, S, prec, monkeypatch):
    fails = _check(monkeypatch, prec, sizes, PLANS[S][1], 128 // S + 1, S, True)
    assert not fails, "\n".join(fails)


# ---- C: output-layer branches: one hidden layer with 5 <= d_out <= 64 (ZB0 from the standalone pass on the
# hi / lo pair) and d_out <= 4 (EPI_BWD0 inside tdq_lay_out_bwd); two hidden layers with 5 <= d_out <= 64 and
# d_out > 64 (dKo from the TN GEMM)

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("sizes", [[2, 36, 6], [2, 36, 3], [2, 36, 20, 6], [2, 36, 20, 70]])
def test_output_layer_branches(sizes, prec, monkeypatch):
    fails = []
    for N in (1, 33):
        fails += _check(monkeypatch, prec, sizes, PLANS[4][1], N, 4, True)
    assert not fails, "\n".join(fails)


# ---- D: the default path that is not the GEMM-epilogue path (hand-written GEMMs + standalone epilogue pass):
# hidden widths not a multiple of 4, input width > 8

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("sizes,reqs,S", [([2, 30, 22, 1], [(0,), (1,), (0, 0)], 4),
                                          ([10, 36, 20, 1], [(0,), (9,), (3, 3)], 5)])   # (3,3) brings stream (3,)
def test_standalone_epilogue_default_path(sizes, reqs, S, prec, monkeypatch):
    fails = []
    for N in (1, 43):
        fails += _check(monkeypatch, prec, sizes, reqs, N, S, False)
    assert not fails, "\n".join(fails)


# ---- E, F: determinism and never-written blocks (S = 5, N = PT + 1)

def _s5_inputs():
    net, X, G, plan = _case((2, 36, 20, 1), tuple(PLANS[5][1]), 128 // 5 + 1)[:4]
    return net, X.cuda(), net.flat.detach().cuda(), G.cuda(), plan


@pytest.mark.parametrize("prec", PRECS)
def test_two_runs_are_bitwise_equal(prec, monkeypatch):
    from tensordiffeq_amd.ops import jet_layered
    monkeypatch.delenv("TDQ_LAY_GEMM", raising=False)
    monkeypatch.delenv("TDQ_LAY_FUSED", raising=False)
    net, X, P, G, plan = _s5_inputs()
    runs = []
    for _ in range(2):
        J, saved = jet_layered.forward_raw(X, P, net, plan, prec)
        assert saved[-1] is True
        runs.append((J.clone(), jet_layered.backward_raw(saved, G).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("prec", PRECS)
def test_backward_writes_every_gradient_element(prec, monkeypatch):
    from tensordiffeq_amd.ops import jet_layered
    monkeypatch.delenv("TDQ_LAY_GEMM", raising=False)
    monkeypatch.delenv("TDQ_LAY_FUSED", raising=False)
    net, X, P, G, plan = _s5_inputs()
    J, saved = jet_layered.forward_raw(X, P, net, plan, prec)
    assert saved[-1] is True
    grad = torch.full_like(P, float("nan"))
    g = jet_layered.backward_raw(saved, G, grad=grad)
    assert g.data_ptr() == grad.data_ptr() and torch.isfinite(g).all().item()
