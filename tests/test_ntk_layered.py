"""The layer-wise NTK path (``LayeredNTKOp``, ``ops/ntk.py``) on the CPU: the adjoints-only pass of the
layer-wise engine against float64 autograd, the torch mirror of the Gram kernel against the plain float64
formula, and the whole op (torch seeds, torch Gram) against the per-instance oracle of ``tests/test_ntk.py``.
Also the wave program, the Gram case table, its float64 formula and its bound, shared with
``tests/test_ntk_gram_gpu.py``.

Gram bound (derived, per instance): ``|got - ref| <= (Win + Wout + R^2 + 8) 2^-23 A_i`` with ``A_i`` the
formula on absolute values - the first-order fp32 bound of two dot products (Win / Wout terms), one product
and an R^2-term sum, doubled for the higher-order terms.
"""
import math

import numpy as np
import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd import fusion
from tensordiffeq_amd.boundaries import IC, FunctionNeumannBC, dirichletBC
from tensordiffeq_amd.jet import JetPlan
from tensordiffeq_amd.models.networks import TanhMLP
from tensordiffeq_amd.ops import jet_layered, ntk
from tests import test_ntk as cpu


def wave(n_f=40):
    """u_tt = 4 u_xx: the five streams (), x, t, xx, tt; an IC, a Neumann condition in t, two walls."""
    D = cpu._domain(n_f, xlim=(0.0, 1.0))

    def u_t(u_model, x, t):
        return tdq.grad(cpu._u(u_model, x, t), t)

    def f_model(u_model, x, t):
        u = cpu._u(u_model, x, t)
        return tdq.grad(tdq.grad(u, t), t) - 4.0 * tdq.grad(tdq.grad(u, x), x)

    bcs = [IC(D, [lambda x: np.sin(math.pi * x) + 0.5 * np.sin(4 * math.pi * x)], var=[["x"]]),
           FunctionNeumannBC(D, fun=[lambda x: 0.0 * x], var="t", target="lower", deriv_model=[u_t],
                             func_inputs=["x"]),
           dirichletBC(D, val=0.0, var="x", target="lower"), dirichletBC(D, val=0.0, var="x", target="upper")]
    return [2, 12, 12, 1], f_model, D, bcs


cpu.PROGRAMS["wave"] = wave

# id: (instances, S, Win, Wout, ldh, ldz, offA, offB or None, points, column offset of the planes' base)
GRAM_CASES = {
    "n1_s1_1x1": (1, 1, 1, 1, 1, 1, 0, None, 1, 0),
    "n70_s5_128x128_off3": (70, 5, 128, 128, 128, 128, 3, None, 75, 0),
    "n9_s8_3x20": (9, 8, 3, 20, 3, 20, 0, None, 9, 0),
    "n5_s4_100x36_ld104_ld40": (5, 4, 100, 36, 104, 40, 0, None, 5, 0),
    "pair9_s8_128x128": (9, 8, 128, 128, 128, 128, 0, 9, 18, 0),
    "pair7_s3_20x2": (7, 3, 20, 2, 20, 2, 2, 11, 18, 0),
    "n6_s2_16x8_base_off1": (6, 2, 16, 8, 20, 12, 1, None, 7, 1),   # widths % 4 == 0, base 4 bytes off a quad
}


def gram_planes(name, zero_h=False):
    """``(H, Z)`` float32 Gaussian planes of a case: views of width W into ``[S N, ld]`` storage."""
    n, S, Win, Wout, ldh, ldz, offA, offB, N, c0 = GRAM_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Hs = torch.randn(S * N, ldh, generator=g)
    Zs = torch.randn(S * N, ldz, generator=g)
    if zero_h:
        Hs.zero_()
    return Hs, Zs


def gram_views(name, Hs, Zs):
    _, _, Win, Wout, _, _, _, _, _, c0 = GRAM_CASES[name]
    return Hs[:, c0:c0 + Win], Zs[:, c0:c0 + Wout]


def gram_ref(H, Z, S, N, n, offA, offB, absolute=False):
    """The formula of ``ops/ntk.py``'s header in float64, one instance at a time (``absolute``: on absolute
    values, with the Gram products formed from absolute rows - the bound's ``A_i``)."""
    H, Z = H.double().cpu(), Z.double().cpu()
    if absolute:
        H, Z = H.abs(), Z.abs()
    out = torch.zeros(n, dtype=torch.float64)
    for i in range(n):
        pts = [offA + i] + ([offB + i] if offB is not None else [])
        rows = [s * N + p for p in pts for s in range(S)]
        value = [k * S for k in range(len(pts))]
        Gz, Gh = Z[rows] @ Z[rows].T, H[rows] @ H[rows].T
        M = torch.zeros_like(Gz)
        for a in value:
            for b in value:
                M[a, b] = 1.0
        out[i] = (Gz * (Gh + M)).sum()
    return out


def gram_bound(name, H, Z):
    """Per-instance bound ``(Win + Wout + R^2 + 8) 2^-23 A_i``."""
    n, S, Win, Wout, _, _, offA, offB, N, _ = GRAM_CASES[name]
    R = S if offB is None else 2 * S
    return (Win + Wout + R * R + 8) * 2.0 ** -23 * gram_ref(H, Z, S, N, n, offA, offB, absolute=True)


# ------------------------------------------------------------------------------------------
# 1. the adjoints-only pass
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [[12], [12, 20, 12]], ids=["one_hidden", "three_hidden"])
def test_adjoint_planes_match_fp64_autograd(hidden):
    d_in, d_out, N = 2, 2, 11
    g = torch.Generator().manual_seed(5 + len(hidden))
    net = TanhMLP([d_in] + hidden + [d_out], generator=g)
    with torch.no_grad():
        net.flat.add_(0.2 * torch.randn(net.flat.shape, generator=g))
    plan = JetPlan({(0, 0), (1, 1)}, d_in)
    S = plan.S
    assert S == 5
    X = torch.rand(N, d_in, generator=g) * 2 - 1
    dJ = torch.randn(S, N, d_out, generator=g)
    # float64 autograd of <dJ, J> with respect to every layer's pre-activation streams
    P64 = net.flat.detach().double()
    z, taps = ntk._tapped_jet(X.double(), [(k, b) for k, b in net.weights(P64)], plan)
    loss = sum((dJ[plan.index[mi]].double() * zm).sum() for mi, zm in z.items() if zm is not None)
    flat = [zt for _, Zd in taps for zt in Zd.values()]
    gs = iter(torch.autograd.grad(loss, flat))
    ref = [({mi: h.detach() for mi, h in Hd.items()}, {mi: next(gs) for mi in Zd}) for Hd, Zd in taps]
    assert len(ref) == len(hidden) + 1
    # float64 engine: the chain itself; float32: fp32 round-off of <= 4 layers of <= 20-term dot products and
    # ~10-term jet adjoints, (4 * 30) 2^-24 = 7e-6 of the plane's largest entry
    for dt, tol in ((torch.float64, 1e-11), (torch.float32, 1e-5)):
        P = net.flat.detach().to(dt)
        J, saved = jet_layered.forward_raw(X.to(dt), P, net, plan, precision="fp32")
        planes = list(jet_layered.adjoint_planes(saved, dJ.to(dt)))
        assert len(planes) == len(ref)
        for (H, Z), (Href, Zref) in zip(planes, reversed(ref)):
            assert H.shape[0] == Z.shape[0] == S * N and H.stride(1) == 1 and Z.stride(1) == 1
            Hv, Zv = H.view(S, N, -1).double(), Z.view(S, N, -1).double()
            zmax = max(float(v.abs().max()) for v in Zref.values())
            hmax = max(float(v.abs().max()) for v in Href.values())
            for mi, s in plan.index.items():
                if mi in Zref:
                    assert float((Zv[s] - Zref[mi]).abs().max()) <= tol * zmax, (dt, mi)
                    assert float((Hv[s] - Href[mi]).abs().max()) <= tol * hmax, (dt, mi)
                else:      # a second-order stream of the input jets: H is identically 0
                    assert not Hv[s].any()


def test_adjoint_planes_refuse_a_bf16_forward():
    net = TanhMLP([2, 12, 1])
    plan = JetPlan({(0,)}, 2)
    X = torch.rand(4, 2)
    _, saved = jet_layered.forward_raw(X, net.flat.detach(), net, plan, precision="bf16")
    with pytest.raises(ValueError, match="fp32"):
        next(jet_layered.adjoint_planes(saved, torch.zeros(plan.S, 4, 1)))


# ------------------------------------------------------------------------------------------
# 2. the torch mirror of the Gram kernel
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAM_CASES))
def test_torch_gram_matches_the_fp64_formula(name):
    n, S, _, _, _, _, offA, offB, N, _ = GRAM_CASES[name]
    H, Z = gram_views(name, *gram_planes(name))
    ref = gram_ref(H, Z, S, N, n, offA, offB)
    got = ntk.gram_norms_torch(H, Z, S, N, n, offA, offB)
    assert got.dtype == torch.float32 and got.shape == (n,)
    ratio = float(((got.double() - ref).abs() / gram_bound(name, H, Z)).max())
    print(f"torch gram {name}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # float64 planes: the mirror is the formula
    assert float((ntk.gram_norms_torch(H.double(), Z.double(), S, N, n, offA, offB) - ref).abs().max()) \
        <= 1e-12 * float(ref.max())
    # accumulate on a prefilled n2, and plain assignment
    out = torch.full((n,), 3.0)
    ntk.gram_norms_torch(H, Z, S, N, n, offA, offB, out=out, accumulate=True)
    assert torch.equal(out, 3.0 + got)
    ntk.gram_norms_torch(H, Z, S, N, n, offA, offB, out=out)
    assert torch.equal(out, got)


@pytest.mark.parametrize("name", ["n70_s5_128x128_off3", "pair7_s3_20x2"])
def test_torch_gram_with_zero_inputs_leaves_the_bias_term(name):
    n, S, _, _, _, _, offA, offB, N, _ = GRAM_CASES[name]
    H, Z = gram_views(name, *gram_planes(name, zero_h=True))
    Zv = Z.double().reshape(S, N, -1)[0]
    bias = (Zv[offA:offA + n] + (Zv[offB:offB + n] if offB is not None else 0.0)).square().sum(1)
    got = ntk.gram_norms_torch(H, Z, S, N, n, offA, offB)
    assert float((got.double() - bias).abs().max()) <= 1e-5 * float(bias.max())
    assert float((gram_ref(H, Z, S, N, n, offA, offB) - bias).abs().max()) <= 1e-12 * float(bias.max())


def test_torch_gram_refuses_bad_geometry():
    H, Z = torch.zeros(3 * 8, 4), torch.zeros(3 * 8, 4)
    for S, N, n, offA, offB in ((3, 8, 9, 0, None), (3, 8, 4, 5, None), (3, 8, 4, 0, 5), (3, 8, 2, -1, None),
                                (9, 8, 1, 0, None), (2, 8, 1, 0, None)):
        with pytest.raises(ValueError, match="tdq_ntk_gram"):
            ntk.gram_norms_torch(H, Z, S, N, n, offA, offB)


# ------------------------------------------------------------------------------------------
# 3. the op on the CPU: torch seeds, layered forward and adjoints, torch Gram
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wave", "periodic"])
def test_layered_op_on_the_cpu_matches_the_oracle(name):
    m = cpu.model(name)
    prog = m.program()
    fl = prog.fused_op.fl if prog.fused_op is not None else fusion.build(prog, m.lambdas)
    op = ntk.LayeredNTKOp(prog, fl, m.lambdas)
    assert op.kind == "hip-layered" and not op.hip
    if name == "wave":
        assert prog.plan.S == 5
    else:
        assert any(len(gr.segs) == 2 for gr in fl.groups)      # pair mode
    T_ref, norms_ref = cpu.shared_oracle(name)
    assert (T_ref > 0).all()
    T = op.traces().clone()
    assert T.dtype == torch.float32 and torch.equal(T, op.traces())
    err = float(((T.double() - T_ref).abs() / T_ref).max())
    print(f"layered op on the CPU {name}: worst rel trace err {err:.2e}")
    assert err < 1e-4                                          # the bound of test_torch_traces_match_the_oracle
    for key, ref in norms_ref.items():
        assert cpu.maxrel(op.instance_norms(*key), ref) < 1e-4, key
    # a chunk smaller than the groups: several launch groups per loss group
    small = ntk.LayeredNTKOp(prog, fl, m.lambdas, chunk=16)
    assert len(small.launches) > len(op.launches)
    assert float(((small.traces().double() - T_ref).abs() / T_ref).max()) < 1e-4
    for key, ref in norms_ref.items():
        assert cpu.maxrel(small.instance_norms(*key), ref) < 1e-4, key


def test_build_on_the_cpu_keeps_the_torch_path():
    m = cpu.model("wave")
    assert m._ntk_op().kind == "torch"
    assert ntk.layered_reason(m.program()) is not None
