"""The layer-wise NTK path on the GPU: the Gram-product kernel (``csrc/ntk_gram.hip``) against the float64
formula, the whole per-instance norm (layered fp32 forward, adjoints-only pass, one Gram launch per layer)
against float64 per-instance autograd on shapes beyond ``tdq_ntk_norm``'s envelope, and the solver's routing
(``LayeredNTKOp``, kind ``"hip-layered"``) on a wave program with five streams at width 128.

Bounds.  Gram kernel: derived, per instance, ``(Win + Wout + R^2 + 8) 2^-23 A_i`` (tests/test_ntk_layered.py).
Whole norm and solver: the larger of ``NORM_BOUND`` of tests/test_ntk_gpu.py and 3 x the error of
``TorchNTK``'s float32 formula (the path that served these shapes before) on the same case against the same
oracle, never above 1e-4; error = max error over max norm.

Measured on an MI355X (profiles/r18_ntk_layered_errors.txt):
  Gram kernel    worst |err| / bound 0.0003 .. 0.0152 over the seven cases, 0.0018 .. 0.0111 with H = 0
  whole norm     1.0e-7 .. 9.2e-7 of the largest norm (worst: n20_w128_l3_s8); the torch path's float32 formula
                 7.8e-8 .. 3.0e-7, so the bound was NORM_BOUND = 1.23e-6 in every case
  solver (wave)  traces <= 8.7e-8 (torch path <= 6.7e-8), per-instance norms <= 2.8e-7 (torch path <= 3.7e-7)
"""
import math
import warnings

import pytest
import torch

from tensordiffeq_amd.jet import JetPlan, jet_forward
from tensordiffeq_amd.models.networks import TanhMLP
from tests import test_ntk as cpu
from tests import test_ntk_layered as lay
from tests.test_ntk_gpu import NORM_BOUND

pytestmark = pytest.mark.gpu

GRAM_CASES = lay.GRAM_CASES


def _gram_case(name, zero_h=False):
    """``(got (n,), ref, bound)`` of one case; ``n2`` sits between two guard entries."""
    from tensordiffeq_amd.ops import ntk
    n, S, _, _, _, _, offA, offB, N, _ = GRAM_CASES[name]
    Hs, Zs = lay.gram_planes(name, zero_h)
    H, Z = lay.gram_views(name, Hs, Zs)
    ref, bound = lay.gram_ref(H, Z, S, N, n, offA, offB), lay.gram_bound(name, H, Z)
    Hd, Zd = lay.gram_views(name, Hs.cuda(), Zs.cuda())
    out = torch.full((n + 2,), -7.0, device="cuda")
    ntk.gram_norms(Hd, Zd, S, N, n, offA, offB, out=out[1:n + 1])
    torch.cuda.synchronize()
    assert out[0] == -7.0 and out[-1] == -7.0              # nothing outside the instance range is written
    again = torch.full((n,), -7.0, device="cuda")
    ntk.gram_norms(Hd, Zd, S, N, n, offA, offB, out=again)
    assert torch.equal(again, out[1:n + 1])                # two launches give equal bits
    return out[1:n + 1].double().cpu(), ref, bound, (Hd, Zd)


# ------------------------------------------------------------------------------------------
# a. the Gram kernel alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAM_CASES))
def test_gram_kernel_matches_fp64(name):
    from tensordiffeq_amd.ops import ntk
    n, S, _, _, _, _, offA, offB, N, _ = GRAM_CASES[name]
    got, ref, bound, (Hd, Zd) = _gram_case(name)
    ratio = float(((got - ref).abs() / bound).max())
    print(f"ntk gram kernel {name}: worst |err| / bound = {ratio:.4f}   "
          f"(max err / max norm {float((got - ref).abs().max() / ref.max()):.3e})")
    assert torch.isfinite(got).all() and float(ref.max()) > 0
    assert ratio <= 1.0
    # accumulate=1 on a prefilled n2: the same value added in fp32
    pre = torch.linspace(1.0, 2.0, n, device="cuda")
    acc = pre.clone()
    ntk.gram_norms(Hd, Zd, S, N, n, offA, offB, out=acc, accumulate=True)
    assert torch.equal(acc.cpu(), pre.cpu() + got.float())


@pytest.mark.parametrize("name", ["n70_s5_128x128_off3", "n9_s8_3x20", "pair9_s8_128x128", "pair7_s3_20x2"])
def test_gram_kernel_with_zero_inputs_leaves_the_bias_term(name):
    n, S, _, _, _, _, offA, offB, N, _ = GRAM_CASES[name]
    got, ref, bound, (_, Zd) = _gram_case(name, zero_h=True)
    Zv = Zd.double().cpu().reshape(S, N, -1)[0]
    bias = (Zv[offA:offA + n] + (Zv[offB:offB + n] if offB is not None else 0.0)).square().sum(1)
    assert float((ref - bias).abs().max()) <= 1e-12 * float(bias.max())   # the formula's own mask
    ratio = float(((got - bias).abs() / bound).max())
    print(f"ntk gram kernel, H = 0, {name}: worst |err| / bound = {ratio:.4f}")
    assert float(bias.min()) > 0 and ratio <= 1.0


def test_gram_kernel_refuses_bad_geometry():
    from tensordiffeq_amd.ops import _lib, ntk
    S, N = 3, 8
    H, Z = torch.zeros(S * N, 8, device="cuda"), torch.zeros(S * N, 4, device="cuda")
    for offA, offB, n in ((4, None, 5), (-1, None, 2), (0, 5, 4)):                 # ranges past the point set
        with pytest.raises(RuntimeError, match="tdq_ntk_gram"):
            ntk.gram_norms(H, Z, S, N, n, offA, offB)
    for S_bad in (0, 9):                                                          # S outside 1..8
        with pytest.raises(RuntimeError, match="tdq_ntk_gram"):
            ntk.gram_norms(torch.zeros(S_bad * N, 8, device="cuda"), torch.zeros(S_bad * N, 4, device="cuda"),
                           S_bad, N, 1)
    with pytest.raises(ValueError, match="tdq_ntk_gram"):                         # planes of another extent
        ntk.gram_norms(H[:5], Z, S, N, 1)
    # the entry point itself (every call is refused before a launch): widths < 1, a leading dimension below
    # its width, element offsets past 32 bits
    lib = _lib.load(required=True)
    n2 = torch.full((4,), -7.0, device="cuda")
    st = _lib.stream_ptr(H.device)

    def call(ldh, Win, ldz, Wout, S_, N_, n):
        return lib.tdq_ntk_gram(_lib.ptr(H), ldh, Win, _lib.ptr(Z), ldz, Wout, S_, N_, 0, -1, n, 0, _lib.ptr(n2), st)

    assert call(8, 8, 4, 4, S, N, 4) == 0
    for args in ((8, 0, 4, 4, S, N, 4), (8, 8, 4, 0, S, N, 4), (7, 8, 4, 4, S, N, 4), (8, 8, 3, 4, S, N, 4),
                 (8, 8, 4, 4, S, 0, 0), (8, 8, 4, 4, S, N, -1), (128, 128, 4, 4, 8, 1 << 22, 4),
                 (8, 8, 128, 128, 8, 1 << 22, 4)):
        n2.fill_(-7.0)
        assert call(*args) != 0, args
        torch.cuda.synchronize()
        assert (n2 == -7.0).all()
    with pytest.raises(RuntimeError, match="tdq_ntk_gram"):
        _lib.check(call(7, 8, 4, 4, S, N, 4), "tdq_ntk_gram")


# ------------------------------------------------------------------------------------------
# b. the whole norm against float64 per-instance autograd
# ------------------------------------------------------------------------------------------
REQ = {4: {(0, 1)}, 5: {(0, 0), (1, 1)}, 6: {(0, 0), (0, 1), (1, 1)}, 8: {(0, 0), (0, 1), (1, 1), (2, 2)}}

# id: (instances, hidden widths, streams, d_in, d_out, offA, offB or None, points)
NORM_CASES = {
    "n70_w128_l2_s5": (70, [128, 128], 5, 2, 1, 0, None, 70),
    "n20_w128_l3_s8": (20, [128, 128, 128], 8, 3, 1, 2, None, 23),
    "pair9_w128_l2_s5": (9, [128, 128], 5, 2, 1, 1, 11, 20),
    "n15_w64_128_32_s4_o2": (15, [64, 128, 32], 4, 2, 2, 3, None, 18),
    "n6_w64_l1_s6": (6, [64], 6, 2, 1, 0, None, 6),
}


def _torch_formula(X, W, plan, dJ, n, offA, offB):
    """``TorchNTK``'s formula (tapped torch jet, ``_gram_norms``) in the dtype of its arguments, for the
    instances of a norm case."""
    from tensordiffeq_amd.ops import ntk
    idx = torch.arange(offA, offA + n, device=X.device)
    if offB is not None:
        idx = torch.cat([idx, torch.arange(offB, offB + n, device=X.device)])
    with torch.enable_grad():
        z, taps = ntk._tapped_jet(X[idx], W, plan)
        f = sum((dJ[plan.index[mi]][idx] * zm).sum() for mi, zm in z.items() if zm is not None)
        flat = [zt for _, Z in taps for zt in Z.values()]
        gs = iter(torch.autograd.grad(f, flat, allow_unused=True))
        grads = [{mi: next(gs) for mi in Z} for _, Z in taps]
    return ntk._gram_norms(taps, grads, n, 1 if offB is None else 2).detach()


def _norm_case(name):
    """``(layered norms, TorchNTK float32 formula, float64 oracle)``: random Gaussian seeds and biases."""
    from tensordiffeq_amd.ops import jet_layered, ntk
    n, hidden, streams, d_in, d_out, offA, offB, N = NORM_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    net = TanhMLP([d_in] + hidden + [d_out], generator=g)
    with torch.no_grad():
        net.flat.add_(0.2 * torch.randn(net.flat.shape, generator=g))
    plan = JetPlan(REQ[streams], d_in)
    assert plan.S == streams
    X = torch.rand(N, d_in, generator=g) * 2 - 1
    dJ = torch.randn(plan.S, N, d_out, generator=g)
    # oracle
    p = net.flat.detach().double().requires_grad_(True)
    J = jet_forward(X.double(), net.weights(p), plan)
    w = (dJ.double() * J).sum((0, 2))
    inst = [w[offA + i] + (w[offB + i] if offB is not None else 0.0) for i in range(n)]
    ref = torch.stack([torch.autograd.grad(f, p, retain_graph=True)[0].square().sum() for f in inst])
    # the layered chain
    net = net.to("cuda")
    Xd, dJd = X.cuda(), dJ.cuda().contiguous()
    P = net.flat.detach()
    _, saved = jet_layered.forward_raw(Xd, P, net, plan, precision="fp32")
    out = torch.full((n + 2,), -7.0, device="cuda")
    layers = 0
    for li, (H, Z) in enumerate(jet_layered.adjoint_planes(saved, dJd)):
        ntk.gram_norms(H, Z, plan.S, N, n, offA, offB, out=out[1:n + 1], accumulate=li > 0)
        layers += 1
    torch.cuda.synchronize()
    assert layers == len(hidden) + 1 and out[0] == -7.0 and out[-1] == -7.0
    # the float32 formula of the torch path on the same device
    t32 = _torch_formula(Xd, [(k.detach(), b.detach()) for k, b in net.weights(P)], plan, dJd, n, offA, offB)
    return out[1:n + 1].double().cpu(), t32.double().cpu(), ref


def _rule(torch_err):
    """The bound of (b): the larger of NORM_BOUND and 3 x the torch path's own error, never above 1e-4."""
    bound = max(NORM_BOUND, 3 * torch_err)
    assert bound <= 1e-4, f"3 x the torch path's error {torch_err:.3e} passes 1e-4"
    return bound


@pytest.mark.parametrize("name", list(NORM_CASES))
def test_layered_norm_matches_fp64(name):
    got, t32, ref = _norm_case(name)
    assert float(ref.max()) > 0 and torch.isfinite(got).all()
    err = float((got - ref).abs().max() / ref.abs().max())
    terr = float((t32 - ref).abs().max() / ref.abs().max())
    bound = _rule(terr)
    print(f"ntk layered norm {name}: max err / max norm = {err:.3e}   torch fp32 formula {terr:.3e}   "
          f"bound {bound:.3e}   (max norm {float(ref.max()):.3e})")
    assert err < bound


# ------------------------------------------------------------------------------------------
# c. the solver
# ------------------------------------------------------------------------------------------
def test_wave_at_width_128_runs_on_the_layered_hip_path():
    from tensordiffeq_amd.ops import ntk
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = cpu.model("wave", device="cuda", backend="hip", layers=[2, 128, 128, 1], precision="bf16")
        assert m.active_backend == "hip"
        op = m._ntk_op()
    prog = m.program()
    assert prog.plan.S == 5
    assert op.kind == "hip-layered"
    assert not any("NTK traces on the torch jet" in r for r in prog.reasons)
    assert not [w for w in rec if "NTK traces on the torch jet" in str(w.message)]
    T1 = op.traces().clone()
    n1 = {key: op.instance_norms(*key).clone() for key in op.norms}
    T2 = op.traces().clone()
    torch.cuda.synchronize()
    assert torch.equal(T1, T2) and all(torch.equal(v, op.instance_norms(*key)) for key, v in n1.items())
    T_ref, norms_ref = cpu.oracle(m)
    assert (T_ref > 0).all()
    # the torch path on the same program: its error sets the bound
    top = ntk.TorchNTK(prog, op.fl, m.lambdas)
    T_t = top.traces().double().cpu()
    err = (T1.double().cpu() - T_ref).abs() / T_ref
    terr = (T_t - T_ref).abs() / T_ref
    bound = _rule(float(terr.max()))
    print(f"ntk layered traces wave: rel err per term {[f'{e:.2e}' for e in err.tolist()]}   torch path "
          f"{[f'{e:.2e}' for e in terr.tolist()]}   bound {bound:.3e}")
    assert torch.isfinite(T1).all() and float(err.max()) < bound
    for key, ref in norms_ref.items():
        assert float(ref.max()) > 0
        e, te = cpu.maxrel(op.instance_norms(*key), ref), cpu.maxrel(top.instance_norms(*key), ref)
        b = _rule(te)
        print(f"   instance norms {key}: max err / max norm = {e:.3e}   torch path {te:.3e}   bound {b:.3e}")
        assert e < b


def test_wave_trains_with_updates_on_the_layered_path():
    m = cpu.model("wave", device="cuda", backend="hip", layers=[2, 128, 128, 1], precision="bf16", ntk_every=4)
    m.fit(tf_iter=10, newton_iter=4)
    assert m._ntk_op().kind == "hip-layered" and [h[0] for h in m.ntk_history] == [0, 4, 8]
    assert len(m.losses) == 10 and all(math.isfinite(v) for h in m.losses for v in h.values())
    assert math.isfinite(m.min_loss["l-bfgs"])


def test_inside_the_fused_envelope_the_norm_kernel_still_serves():
    m = cpu.model("burgers", device="cuda", backend="hip", layers=[2, 32, 32, 1], precision="bf16")
    assert m._ntk_op().kind == "hip"
