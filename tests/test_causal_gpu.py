"""Causal training weights on the GPU: the update kernel (``csrc/causal.hip``) against a float64 oracle on
the same float32 inputs, its argument checks, one optimizer step on every step path against the float64
torch jet, the captured steps against eager ones, the torch mirror against the kernel and a solver run.

End-to-end tolerances: the compared quantity is ``log W_b`` relative to ``max_b |log W_ref|``, a linear
functional of the per-point adjoints ``c f_i^2`` that the SA-gradient bounds of tests/test_fused_kernels.py
cover (5e-2 bf16, 1e-4 bf16x3: the ceilings).  The bounds below are 3x the errors measured on an MI355X
(profiles/r20_causal_errors.txt)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CEILING = {"bf16": 5e-2, "bf16x3": 1e-4}
# 3x the measured errors (profiles/r20_causal_errors.txt), per path and precision
E2E_BOUND = {
    ("fused", "bf16"): 3.6e-2, ("fused", "bf16x3"): 5.1e-5,        # measured 1.202e-2, 1.700e-5
    ("ranges", "bf16"): 3.6e-2, ("ranges", "bf16x3"): 5.1e-5,      # measured 1.191e-2, 1.700e-5
    ("w32", "bf16"): 7.5e-4, ("w32", "bf16x3"): 1.8e-5,            # measured 2.501e-4, 6.029e-6
    ("unfused", "bf16"): 3.6e-2, ("unfused", "bf16x3"): 5.1e-5,    # measured 1.191e-2, 1.700e-5
}


def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------
# a. the kernel
# ------------------------------------------------------------------------------------------
def oracle(r2, inv_c, bins_of, M, eps):
    """``(W_ref, arg)`` in float64 on the CPU: ``arg_b = eps * sum_{b' < b} L_b'``."""
    r2 = r2.detach().double().cpu().reshape(-1) * float(inv_c)
    bins_of = bins_of.cpu()
    counts = torch.bincount(bins_of, minlength=M).double()
    sums = torch.zeros(M, dtype=torch.float64).index_add_(0, bins_of, r2)
    mean = torch.where(counts > 0, sums / counts.clamp(min=1), torch.zeros_like(sums))
    arg = float(eps) * (torch.cumsum(mean, 0) - mean)
    return torch.exp(-arg), arg


def bins_case(n, M, layout, seed=0):
    """Bin of every point, in the user's (shuffled) order.  ``mixed``: bin 0 empty, bin 1 one point, one bin
    of 700 points (more than one pass of the 256-lane block) where ``n`` and ``M`` allow, the rest random;
    ``last``: every point in bin ``M - 1``."""
    g = torch.Generator().manual_seed(seed)
    if layout == "last" or M == 1:
        return torch.full((n,), M - 1, dtype=torch.int64)
    b = torch.randint(min(2, M - 1), M, (n,), generator=g)
    b[b == 1] = M - 1
    perm = torch.randperm(n, generator=g)
    if M > 3 and n > 1400:
        b[b == 2] = 3
        b[perm[:700]] = 2
    if n > 1:
        b[perm[-1]] = 1
    return b


@pytest.fixture(scope="module")
def lib():
    from tensordiffeq_amd.ops import _lib
    return _lib.load(required=True)


@pytest.mark.parametrize("layout", ["mixed", "last"])
@pytest.mark.parametrize("M", [1, 33, 1024])
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_kernel_matches_fp64(n, M, layout):
    from tensordiffeq_amd.ops import causal
    d = dev()
    bins_of = bins_case(n, M, layout)
    if layout == "mixed" and M == 33 and n == 5000:
        c = torch.bincount(bins_of, minlength=M)
        assert c[0] == 0 and c[1] == 1 and c[2] == 700
    order, start = causal.bin_layout(bins_of, M)
    g = torch.Generator().manual_seed(n + M)
    r2 = torch.rand(n, generator=g) * 10.0 ** torch.randint(-6, 7, (n,), generator=g).float()
    r2[torch.rand(n, generator=g) < 0.2] = 0.0
    r2[int(torch.randint(0, n, (1,), generator=g))] = 1e6
    inv_c, eps = 3.0, torch.tensor(1e-6, dtype=torch.float32)   # bin means ~1e5: |log W| from ~0.1 to ~100
    tail = 64
    r2_buf = torch.full((n + tail,), float("nan"), device=d)
    r2_buf[:n] = r2.to(d)
    ord_buf = torch.full((n + tail,), 2 ** 30, dtype=torch.int32, device=d)
    ord_buf[:n] = order.to(d)
    lam_buf = torch.full((n + tail,), float("nan"), device=d)
    w_bins = torch.full((M,), float("nan"), device=d)
    stats = torch.full((2,), float("nan"), device=d)
    work = torch.full((M,), float("nan"), dtype=torch.float64, device=d)
    args = (r2_buf[:n], inv_c, ord_buf[:n], start.to(d), start, eps.to(d), work, lam_buf[:n], w_bins, stats)
    causal.causal_update(*args)
    lam1, w1, s1 = lam_buf.clone(), w_bins.clone(), stats.clone()
    W_ref, arg = oracle(r2, inv_c, bins_of, M, float(eps))
    bound = 2.0 ** -22 * (2.0 + arg.abs()) * W_ref + 1e-38
    err = (w1.double().cpu() - W_ref).abs()
    print(f"CAUSAL_KERNEL n={n} M={M} {layout}: max err/bound {float((err / bound).max()):.3f}, "
          f"arg max {float(arg.max()):.3e}")
    assert bool(torch.isfinite(w1).all()) and bool((err <= bound).all())
    assert torch.equal(lam1[:n].cpu(), w1.cpu()[bins_of])              # every point carries its bin's weight
    assert bool(torch.isnan(lam1[n:]).all())                           # nothing written behind lam
    assert float(s1[0]) == float(w1.min())
    last = r2.double()[bins_of == M - 1] * inv_c
    L_sum = float(oracle(r2, inv_c, bins_of, M, 1.0)[1][-1]) + (float(last.mean()) if last.numel() else 0.0)
    assert float(s1[1]) == pytest.approx(L_sum, rel=1e-6, abs=1e-30)
    lam_buf[:n] = float("nan")
    w_bins.fill_(float("nan"))
    causal.causal_update(*args)
    assert torch.equal(lam_buf[:n], lam1[:n]) and torch.equal(w_bins, w1) and torch.equal(stats, s1)


def test_kernel_refuses_bad_geometry(lib):
    from tensordiffeq_amd.ops import _lib
    d = dev()
    n = 300
    r2 = torch.rand(n, device=d)
    order = torch.arange(n, dtype=torch.int32, device=d)
    eps = torch.ones((), device=d)
    work = torch.zeros(1025, dtype=torch.float64, device=d)
    w_bins = torch.full((1025,), 7.0, device=d)
    stats = torch.full((2,), 7.0, device=d)
    lam = torch.full((n,), 7.0, device=d)

    def call(M, n_arg, start):
        host = torch.tensor(start, dtype=torch.int32)
        on_dev = host.to(d)
        rc = lib.tdq_causal_update(_lib.ptr(r2), 1.0, _lib.ptr(order), _lib.ptr(on_dev), _lib.ptr(host), M, n_arg,
                                   _lib.ptr(eps), _lib.ptr(work), _lib.ptr(lam), _lib.ptr(w_bins), _lib.ptr(stats),
                                   _lib.stream_ptr(d))
        torch.cuda.synchronize()
        return rc

    even = [0, 100, 200, 300]
    assert call(3, n, even) == 0
    assert bool((lam == 1.0).any()) and not bool((lam == 7.0).any())
    assert not bool((stats == 7.0).any()) and not bool((w_bins[:3] == 7.0).any())
    lam.fill_(7.0)
    w_bins.fill_(7.0)
    stats.fill_(7.0)
    for M, n_arg, start in ((0, n, [0]), (1025, n, list(range(1025)) + [n]), (3, -1, even),
                            (3, n, [0, 200, 100, 300]), (3, n, [0, 100, 200, 299]), (3, n, [1, 100, 200, 300])):
        assert call(M, n_arg, start) != 0, (M, n_arg, start[:4])
    assert bool((lam == 7.0).all()) and bool((w_bins == 7.0).all()) and bool((stats == 7.0).all())


# ------------------------------------------------------------------------------------------
# b. the solver's step paths
# ------------------------------------------------------------------------------------------
def ac_causal(n_f, layers, precision, backend="hip", seed=1234, **kw):
    """Allen-Cahn with the AC-SA boundary set and causal weights."""
    import tensordiffeq_amd as tdq
    from tensordiffeq_amd.boundaries import DomainND, IC, periodicBC
    tdq.set_seed(seed)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 512)
    D.add("t", [0.0, 1.0], 201)
    D.generate_collocation_points(n_f)

    def deriv_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        return u, tdq.grad(u, x)

    def f_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        u_xx = tdq.grad(tdq.grad(u, x), x)
        return tdq.grad(u, t) - 0.0001 * u_xx + 5.0 * u * u * u - 5.0 * u

    init = IC(D, [lambda x: x ** 2 * np.cos(math.pi * x)], var=[["x"]])
    m = tdq.CollocationSolverND(verbose=False)
    kw.setdefault("causal_eps", 0.1)
    kw.setdefault("causal_bins", 16)
    kw.setdefault("causal_bc_weights", [100.0, 1.0])
    m.compile(list(layers), f_model, D, [init, periodicBC(D, ["x"], [deriv_model])], Adaptive_type="causal",
              backend=backend, device=dev(), precision=precision, **kw)
    return m


AC_LAYERS = (2, 128, 128, 128, 128, 1)


def log_w_oracle(m, ref, flat0):
    """``log W_ref`` per bin from the float64 torch jet's ``f`` at ``flat0`` (the adjoint of the weight
    array of the same program on the ``jet`` backend, evaluated in float64)."""
    from tensordiffeq_amd.ops import causal
    p64 = flat0.detach().double()
    lams = [ref.lambdas[0].detach().double().requires_grad_(True)] + [l.detach().double() for l in ref.lambdas[1:]]
    tot, _ = ref.program().evaluate(p64, lams)
    r2 = torch.autograd.grad(tot, lams[0])[0].reshape(-1)      # f^2 / N_f
    bins_of = causal.bin_index(m.X_f_local[:, 1], 0.0, 1.0, m.causal_bins)
    _, arg = oracle(r2, float(m.N_f), bins_of, m.causal_bins, float(np.float32(m.causal_eps[0])))
    return -arg


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("path", ["fused", "ranges", "w32", "unfused"])
def test_one_step_matches_fp64(path, precision, monkeypatch):
    from tensordiffeq_amd.ops import fused_step
    monkeypatch.setenv("TDQ_NO_GRAPH", "1")
    if path == "ranges":
        monkeypatch.setenv("TDQ_FUSED_STEP", "0")
    if path == "unfused":
        monkeypatch.setenv("TDQ_FUSED_LOSS", "0")
    layers = (2, 32, 32, 1) if path == "w32" else AC_LAYERS
    m = ac_causal(517, layers, precision)
    ref = ac_causal(517, layers, precision, backend="jet")
    assert torch.equal(m.X_f_local, ref.X_f_local)
    flat0 = m.u_model.flat.detach().clone()
    eng = m._get_engine(None, 1)
    prog = m.program()
    if path == "unfused":
        assert prog.fused_op is None and not eng._tail_eligible()
    else:
        assert prog.fused_op is not None and eng._tail_eligible()
        fs = fused_step.for_program(prog)
        if path == "fused":
            assert fs is not None and eng._tail_one() == (precision == "bf16")
        else:
            assert fs is None, path
    m.lambdas[0].fill_(float("nan"))   # the priming evaluation and the step write every weight
    m.fit(tf_iter=1)
    assert not torch.equal(m.u_model.flat, flat0)
    W = m.causal_weights().double()
    lam = m.lambdas[0].reshape(-1).cpu()
    from tensordiffeq_amd.ops import causal
    bins_of = causal.bin_index(m.X_f_local[:, 1], 0.0, 1.0, m.causal_bins)
    assert torch.equal(lam, W.float()[bins_of])
    ref_log = log_w_oracle(m, ref, flat0)
    err = float((torch.log(W) - ref_log).abs().max() / ref_log.abs().max())
    print(f"CAUSAL_E2E path={path} precision={precision}: log W error {err:.3e} "
          f"(max |log W_ref| {float(ref_log.abs().max()):.3e})")
    bound = E2E_BOUND[(path, precision)]
    assert bound <= CEILING[precision]
    assert err < bound, err


def _state(m):
    return (m.u_model.flat.detach().clone(), m.lambdas[0].detach().clone(), m._causal_op().w_bins.clone())


def test_graphs_equal_eager_bitwise(monkeypatch):
    """1 warm-up step, then 8 steps: by one 8-step graph, by 8 replays of the 1-step graph, eagerly."""
    out = {}
    for name, env in (("k8", {"TDQ_STEP_UNROLL": "8"}), ("k1", {"TDQ_STEP_UNROLL": "1"}),
                      ("eager", {"TDQ_NO_GRAPH": "1"})):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m = ac_causal(517, AC_LAYERS, "bf16")
            eng = m._get_engine(None, 9)
            assert eng._tail_eligible() and eng._tail_one()
            m.fit(tf_iter=9)
            if name == "k8":
                assert eng.graph_k is not None
            if name == "k1":
                assert eng.graph_a is not None and eng.graph_k is None
            if name == "eager":
                assert eng.graph_a is None
            out[name] = _state(m)
    for name in ("k1", "eager"):
        for a, b, what in zip(out["k8"], out[name], ("theta", "lam", "w_bins")):
            assert torch.equal(a, b), (name, what)
    assert bool((out["k8"][2][1:] < 1.0).all())


def test_mirror_switch_matches_kernel(monkeypatch):
    from tensordiffeq_amd.ops import causal
    res = {}
    for name, val in (("kernel", "1"), ("mirror", "0")):
        with monkeypatch.context() as mp:
            mp.setenv("TDQ_CAUSAL_KERNEL", val)
            m = ac_causal(517, AC_LAYERS, None, causal_eps=1.0)
            assert m._causal_op().hip == (name == "kernel")
            m.fit(tf_iter=3)
            res[name] = m.causal_weights().double()
    Wk, Wm = res["kernel"], res["mirror"]
    arg = -torch.log(Wm)
    bound = 2.0 ** -22 * (2.0 + arg) * Wm + 1e-38
    print(f"CAUSAL_MIRROR max err/bound {float(((Wk - Wm).abs() / bound).max()):.3f}")
    assert bool(((Wk - Wm).abs() <= bound).all())
    del causal


def test_solver_run():
    m = ac_causal(517, AC_LAYERS, "bf16", causal_every=4, causal_eps=[1e-2, 1e-1])
    m.fit(tf_iter=12, newton_iter=4)
    assert [h[0] for h in m.causal_history] == [0, 4, 8]
    assert all(math.isfinite(v) for h in m.causal_history for v in h)
    assert all(math.isfinite(h["Total Loss"]) for h in m.losses) and len(m.losses) == 12
    assert m.fit_info["lbfgs"]["n_iter"] >= 1
    b = ac_causal(517, AC_LAYERS, "bf16", causal_every=4, causal_eps=[1e-2, 1e-1])
    b.fit(tf_iter=12)
    assert torch.equal(m.lambdas[0], b.lambdas[0])          # L-BFGS left the weights as Adam wrote them
    assert not torch.equal(m.u_model.flat, b.u_model.flat)
    assert bool(torch.isfinite(m.lambdas[0]).all())
