"""Causal training weights (``Adaptive_type="causal"``, ops/causal.py) on the CPU: the torch mirror of the
update kernel against a hand-written float64 formula, every refusal, the solver against a float64 training
loop with the same one-step lag, the eps schedule and the checkpoint round trip."""
import math

import numpy as np
import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd.boundaries import DomainND, IC, dirichletBC
from tensordiffeq_amd.models.collocation import parse_adaptive_type
from tensordiffeq_amd.ops import causal


# ------------------------------------------------------------------------------------------
# the mirror against the formula
# ------------------------------------------------------------------------------------------
def formula64(t, r2, inv_c, t0, t1, M, eps):
    """``(lam, W)`` by the definition, one point and one bin at a time, in float64."""
    t, r2 = [float(v) for v in t], [float(v) for v in r2]
    bins = [min(M - 1, int(math.floor((ti - t0) / (t1 - t0) * M))) for ti in t]
    W, cum = [], 0.0
    for b in range(M):
        W.append(math.exp(-eps * cum))
        members = [r2[i] * inv_c for i in range(len(t)) if bins[i] == b]
        cum += sum(members) / len(members) if members else 0.0
    return [W[b] for b in bins], W, bins


def layout_case(M, n=40, seed=0):
    """Times in ``[0, 2]`` with (for M > 1) bin 0 empty, bin 1 holding a single point, one point at
    ``t = t1`` and every remaining point in the last bin."""
    g = torch.Generator().manual_seed(seed)
    t0, t1 = 0.0, 2.0
    if M == 1:
        t = t0 + (t1 - t0) * torch.rand(n, generator=g, dtype=torch.float64)
        t[3] = t1
        return t, t0, t1
    w = (t1 - t0) / M
    t = t1 - w * 0.9 * torch.rand(n, generator=g, dtype=torch.float64)   # the last bin
    t[5] = t0 + 1.5 * w                                                  # the only point of bin 1
    t[7] = t1
    return t, t0, t1


@pytest.mark.parametrize("M", [1, 8, 33])
def test_mirror_matches_fp64_formula(M):
    t, t0, t1 = layout_case(M)
    n = t.numel()
    g = torch.Generator().manual_seed(1)
    r2 = (torch.rand(n, generator=g) * 3.0).float()
    r2[0] = 0.0
    inv_c, eps = 7.0, 0.37
    bins_of = causal.bin_index(t, t0, t1, M)
    lam_ref, W_ref, bins_ref = formula64(t, r2, inv_c, t0, t1, M, float(np.float32(eps)))
    assert bins_of.tolist() == bins_ref
    assert int(bins_of[7]) == M - 1                     # t = t1 lands in the last bin
    if M > 1:
        counts = torch.bincount(bins_of, minlength=M)
        assert counts[0] == 0 and counts[1] == 1 and counts[M - 1] == n - 1
    order, start = causal.bin_layout(bins_of, M)
    assert start[0] == 0 and start[M] == n and sorted(order.tolist()) == list(range(n))
    lam = torch.full((n, 1), float("nan"))
    w_bins = torch.full((M,), float("nan"))
    stats = torch.full((2,), float("nan"))
    causal.causal_update_torch(r2, inv_c, order, start, torch.tensor(eps), lam, w_bins, stats)
    # double sums and one float exp of an argument rounded to fp32 (the kernel's bound)
    W_ref = torch.tensor(W_ref, dtype=torch.float64)
    arg = -torch.log(W_ref)
    bound = 2.0 ** -22 * (2.0 + arg) * W_ref + 1e-38
    assert bool(((w_bins.double() - W_ref).abs() <= bound).all())
    assert torch.equal(lam.reshape(-1), w_bins[bins_of])
    assert float(stats[0]) == float(w_bins.min())
    # eps = 0: weights exactly 1
    causal.causal_update_torch(r2, inv_c, order, start, torch.tensor(0.0), lam, w_bins, stats)
    assert bool((lam == 1.0).all()) and bool((w_bins == 1.0).all()) and float(stats[0]) == 1.0


# ------------------------------------------------------------------------------------------
# the solver
# ------------------------------------------------------------------------------------------
def burgers(n_f=200, seed=0, time_var="t"):
    tdq.set_seed(seed)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 32)
    D.add("t", [0.0, 1.0], 16)
    D.generate_collocation_points(n_f)
    init = IC(D, [lambda x: -np.sin(x * math.pi)], var=[["x"]])
    bcs = [init, dirichletBC(D, val=0.0, var="x", target="upper"), dirichletBC(D, val=0.0, var="x", target="lower")]

    def f_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        u_x = tdq.grad(u, x)
        u_xx = tdq.grad(u_x, x)
        u_t = tdq.grad(u, t)
        return u_t + u * u_x - (0.01 / math.pi) * u_xx
    D.time_var = time_var   # (the conditions above were built with the time axis declared)
    return D, bcs, f_model


def compiled(layers=(2, 16, 16, 1), backend="jet", **kw):
    D, bcs, f = burgers(time_var=kw.pop("time_var", "t"))
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile(list(layers), f, D, bcs, Adaptive_type=kw.pop("Adaptive_type", "causal"), backend=backend,
              device="cpu", **kw)
    return m


def test_parse_needs_opt_in():
    with pytest.raises(NotImplementedError):
        parse_adaptive_type("causal")
    with pytest.raises(NotImplementedError):
        parse_adaptive_type(4)
    assert parse_adaptive_type("causal", causal=True) == 4


@pytest.mark.parametrize("kw, exc, word", [
    (dict(time_var=None), ValueError, "time_var"),
    (dict(dict_adaptive={"residual": [True], "BCs": [False, False, False]}), Exception, "weight vectors"),
    (dict(init_weights={"residual": [torch.ones(200, 1)], "BCs": [None, None, None]}), Exception, "weight vectors"),
    (dict(g=lambda lam: lam ** 2), Exception, "weight function g"),
    (dict(backend="autograd"), ValueError, "autograd"),
    (dict(causal_bins=0), ValueError, "causal_bins"),
    (dict(causal_bins=1025), ValueError, "causal_bins"),
    (dict(causal_eps=[1.0, 0.5]), ValueError, "causal_eps"),
    (dict(causal_bc_weights=[1.0]), ValueError, "causal_bc_weights"),
])
def test_compile_refusals(kw, exc, word):
    with pytest.raises(exc, match=word):
        compiled(**kw)


def test_refuses_two_residual_outputs():
    D, bcs, f = burgers()

    def f2(u_model, x, t):
        r = f(u_model, x, t)
        return r, 2.0 * r
    m = tdq.CollocationSolverND(verbose=False)
    with pytest.raises(ValueError, match="one residual output"):
        m.compile([2, 8, 1], f2, D, bcs, Adaptive_type="causal", backend="jet", device="cpu")


def test_refuses_dist(monkeypatch):
    from tensordiffeq_amd.parallel import dist as pdist
    D, bcs, f = burgers()
    monkeypatch.setattr(pdist, "init_distributed", lambda auto_launch=True: pdist.get_context("cpu"))
    m = tdq.CollocationSolverND(verbose=False)
    with pytest.raises(ValueError, match="dist=True"):
        m.compile([2, 8, 1], f, D, bcs, Adaptive_type="causal", backend="jet", device="cpu", dist=True)


def test_refuses_batch_sz_at_fit():
    m = compiled()
    with pytest.raises(ValueError, match="batch_sz"):
        m.fit(tf_iter=2, batch_sz=50)


def test_discovery_model_does_not_take_the_mode():
    import inspect
    from tensordiffeq_amd.models.discovery import DiscoveryModel
    assert "Adaptive_type" not in inspect.signature(DiscoveryModel.compile).parameters


def fp64_loop(m, steps, bins, eps, bc_weights):
    """Adam on the causal loss in float64 with the solver's lag rule: the weights of step ``k`` come from
    the residuals of step ``k - 1``'s loss pass, those of the first step from the starting parameters.
    Returns ``(losses, lam)``."""
    net = m.u_model
    p = net.flat.detach().double().clone()
    X = m.X_f_local.double()
    t = X[:, 1]
    bins_of = causal.bin_index(t, 0.0, 1.0, bins)
    pts = [(torch.as_tensor(np.asarray(bc.input), dtype=torch.float64),
            torch.as_tensor(np.asarray(bc.val), dtype=torch.float64).reshape(-1, 1)) for bc in m.bcs]

    def mlp(P):
        ws = net.weights(P)

        def call(x):
            h = x
            for i, (k, b) in enumerate(ws):
                h = torch.addmm(b, h, k)
                h = torch.tanh(h) if i < len(ws) - 1 else h
            return h
        return call

    def residual(P):
        x, tt = (X[:, j:j + 1].clone().requires_grad_(True) for j in range(2))
        return m.f_model(mlp(P), x, tt)

    def weights(f):
        r2 = f.detach().reshape(-1) ** 2
        W, cum = [], 0.0
        for b in range(bins):
            W.append(math.exp(-eps * cum))
            sel = r2[bins_of == b]
            cum += float(sel.mean()) if sel.numel() else 0.0
        return torch.tensor(W, dtype=torch.float64)[bins_of].reshape(-1, 1)

    lam = weights(residual(p))                      # the priming evaluation
    mom, var = torch.zeros_like(p), torch.zeros_like(p)
    lr, b1, b2, e = 0.005, 0.99, 0.999, 1e-7
    losses = []
    for k in range(1, steps + 1):
        P = p.clone().requires_grad_(True)
        f = residual(P)
        loss = (lam * f ** 2).mean()
        for w, (xb, vb) in zip(bc_weights, pts):
            loss = loss + w * ((mlp(P)(xb) - vb) ** 2).mean()
        g = torch.autograd.grad(loss, P)[0]
        losses.append(float(loss.detach()))
        lam = weights(f)                            # for the next step
        mom = b1 * mom + (1 - b1) * g
        var = b2 * var + (1 - b2) * g * g
        p = p - lr * math.sqrt(1 - b2 ** k) / (1 - b1 ** k) * mom / (var.sqrt() + e)
    return losses, lam, p


def test_solver_matches_fp64_loop():
    bcw = [3.0, 1.0, 1.0]
    m = compiled(causal_eps=1.0, causal_bins=8, causal_bc_weights=bcw)
    assert m.active_backend == "jet" and m.variables[1:] == []
    ref_losses, ref_lam, ref_p = fp64_loop(m, 6, 8, 1.0, bcw)
    m.fit(tf_iter=6)
    got = torch.tensor([h["Total Loss"] for h in m.losses], dtype=torch.float64)
    # (the tolerance of tests/test_solver.py's fp32-vs-fp64 comparisons)
    np.testing.assert_allclose(got.numpy(), np.asarray(ref_losses), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(m.lambdas[0].double().numpy(), ref_lam.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(m.u_model.flat.detach().double().numpy(), ref_p.numpy(), rtol=1e-4, atol=1e-5)
    W = m.causal_weights()
    assert W.shape == (8,) and float(W[0]) == 1.0 and bool((W[1:] < 1.0).all())
    assert [float(l) for l in m.lambdas[1:]] == bcw


def zero_output_layer(m):
    wo, bo, fi, fo = m.u_model.offsets[-1]
    with torch.no_grad():
        m.u_model.flat[wo:bo + fo] = 0.0


def test_eps_schedule_advances_on_a_tiny_residual():
    m = compiled(causal_eps=[1e-2, 1e-1, 1.0], causal_bins=8, causal_every=3)
    zero_output_layer(m)   # u = 0 solves Burgers: f = 0, every weight 1 > delta
    m.fit(tf_iter=3)
    assert m.causal_history[0] == (0, pytest.approx(1e-1), 1.0)
    assert float(m._causal_op().eps) == pytest.approx(1e-1)
    m.fit(tf_iter=4)
    assert [h[0] for h in m.causal_history] == [0, 3, 6]
    assert all(math.isfinite(h[1]) and math.isfinite(h[2]) for h in m.causal_history)


def test_causal_stop_ends_adam():
    m = compiled(causal_eps=[1e-2], causal_bins=4, causal_every=2, causal_stop=True, causal_delta=-1.0)
    m.fit(tf_iter=6)   # min W > delta at the first check, and 1e-2 is the last eps
    assert len(m.losses) == 0 and [h[:2] for h in m.causal_history] == [(0, 1e-2)]


def test_lbfgs_leaves_the_weights():
    m = compiled(causal_bins=8)
    m.fit(tf_iter=3)
    lam = m.lambdas[0].clone()
    m.fit(newton_iter=3)
    assert torch.equal(m.lambdas[0], lam) and bool((lam < 1.0).any())


def test_example_runs(monkeypatch):
    import importlib.util
    import os
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.syspath_prepend(ex)
    spec = importlib.util.spec_from_file_location("AC_causal", os.path.join(ex, "AC-causal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(["--iters", "3", "--newton", "1", "--n-f", "300", "--device", "cpu", "--quiet", "--bins", "8",
                    "--causal-every", "2"])
    assert all(math.isfinite(v) for v in res.values() if isinstance(v, float))
    assert [h[0] for h in res["causal_history"]] == [0, 2] and res["causal_checks"] == 2
    assert 0.0 < res["min_weight"] <= 1.0
    del sys


def test_checkpoint_resume_is_bitwise(tmp_path):
    kw = dict(causal_eps=[1e-3, 1.0], causal_bins=8, causal_every=2, causal_delta=0.5)
    a = compiled(**kw)
    a.fit(tf_iter=3)
    a.fit(tf_iter=3)
    b = compiled(**kw)
    b.fit(tf_iter=3)
    path = str(tmp_path / "ck.pt")
    b.save(path)
    c = compiled(**kw)
    with torch.no_grad():
        c.u_model.flat.zero_()
    c.resume(path)
    assert torch.equal(c.lambdas[0], b.lambdas[0]) and c.causal_history == b.causal_history
    assert float(c._causal_op().eps) == float(b._causal_op().eps)
    c.fit(tf_iter=3)
    assert torch.equal(c.u_model.flat, a.u_model.flat)
    assert torch.equal(c.lambdas[0], a.lambdas[0])
    assert c.causal_history == a.causal_history and len(a.causal_history) == 3
    assert [h["Total Loss"] for h in c.losses[-3:]] == [h["Total Loss"] for h in a.losses[-3:]]
