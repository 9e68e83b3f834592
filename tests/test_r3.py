"""R3 resampling of the collocation points (``compile(resample="r3")``, ops/r3.py) on the CPU: the mirror's
Philox against the Random123 known answers, the mirror against a plain float64 / Python-integer re-statement
of the rule, the concentration of the population on a frozen fitness, and the solver on the ``jet`` backend
(which rows move, the copies that must follow, the checkpoint round trip, every refusal)."""
import math

import numpy as np
import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd.boundaries import DomainND, IC, dirichletBC
from tensordiffeq_amd.ops import r3

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------
# the re-statement: Python integers and floats only
# ------------------------------------------------------------------------------------------
def philox_py(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def restate(r2, inv_c, box, step, seed, X):
    """``(tau, released, X_new)`` by the definition, one point and one coordinate at a time."""
    n, d_in = len(r2), len(box)
    a = [math.sqrt(float(v) * inv_c) for v in r2]
    tau = sum(a) / n
    released = [not (ai > tau) for ai in a]
    out = X.clone()
    for i in range(n):
        if not released[i]:
            continue
        for j in range(d_in):
            w = philox_py([i, j // 4, step & M32, step >> 32], [seed & M32, seed >> 32])[j % 4]
            u = float(w >> 8) * 2.0 ** -24
            lo, hi = box[j]
            prod = u * (hi - lo)
            out[i, j] = float(np.float32(lo + prod))
    return tau, torch.tensor(released), out


KNOWN = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([M32] * 4, [M32] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("ctr, key, want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert philox_py(ctr, key) == want
    got = r3.philox4x32_10([torch.tensor([c, c], dtype=torch.int64) for c in ctr], key)
    assert [int(g[0]) for g in got] == want and [int(g[1]) for g in got] == want
    # the key as tensors too (what a broadcast over points would pass)
    got = r3.philox4x32_10([torch.tensor([c], dtype=torch.int64) for c in ctr],
                           [torch.tensor([k], dtype=torch.int64) for k in key])
    assert [int(g[0]) for g in got] == want


BOX = [(-1.0, 1.0), (0.0, 1.0), (-3.0, 0.5), (2.0, 10.0), (-0.25, 0.0)]


def buffers(n, d_in, ld, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, ld, generator=g) * 0.5 + 0.125
    r2 = torch.rand(n, generator=g) * 10.0 ** torch.randint(-6, 7, (n,), generator=g).float()
    r2[torch.rand(n, generator=g) < 0.2] = 0.0
    r2[int(torch.randint(0, n, (1,), generator=g))] = 1e6
    return X, r2


def run_mirror(r2, inv_c, box, step, seed, X, d_in):
    n = r2.numel()
    state = torch.tensor(step, dtype=torch.int64)
    stats = torch.full((2,), float("nan"), dtype=torch.float64)
    counts = torch.full(((n + 255) // 256,), -1, dtype=torch.int32)
    bx = torch.tensor(box, dtype=torch.float64)
    r3.r3_update_torch(r2, inv_c, bx, state, seed, [X[:, :d_in]], stats, counts)
    return state, stats, counts


@pytest.mark.parametrize("d_in", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_mirror_matches_restatement(n, d_in):
    box = BOX[:d_in]
    ld = d_in + 1                                   # one column more than the rule may touch
    X, r2 = buffers(n, d_in, ld, seed=n + d_in)
    X0 = X.clone()
    inv_c, seed, step = 3.0, 0x9E3779B97F4A7C15, (7 << 32) + 5
    tau, released, want = restate(r2.tolist(), inv_c, box, step, seed, X0[:, :d_in])
    a = torch.sqrt(r2.double() * inv_c)
    if n > 1:   # the re-statement's left-to-right sum and the mirror's decide every row alike
        assert float(((a - tau).abs() / tau).min()) > 1e-12
    state, stats, counts = run_mirror(r2, inv_c, box, step, seed, X, d_in)
    assert int(state) == step + 1
    assert float(stats[0]) == pytest.approx(tau, rel=1e-14) and float(stats[1]) == float(step)
    got = X[:, :d_in]
    changed = (got != X0[:, :d_in]).any(1)
    assert torch.equal(changed, released)                        # every released row moved, no retained one
    assert torch.equal(got[~released], X0[:, :d_in][~released])  # retained rows: bit for bit
    assert torch.equal(got, want)                                # released rows: the re-statement's bits
    assert torch.equal(X[:, d_in:], X0[:, d_in:])                # the column beside the coordinates
    lo = torch.tensor([b[0] for b in box], dtype=torch.float32)
    hi = torch.tensor([b[1] for b in box], dtype=torch.float32)
    assert bool(((got[released] >= lo) & (got[released] <= hi)).all())
    assert int(counts.sum()) == int(released.sum())
    blocks = torch.cat([released, torch.zeros((-n) % 256, dtype=torch.bool)]).reshape(-1, 256).sum(1)
    assert torch.equal(counts.long(), blocks)
    if n == 1:
        assert bool(released.all())                              # a lone point equals the mean
    else:
        assert 0 < int(released.sum()) < n
    # a second call on the same residuals: the counter has advanced, so the released rows draw again
    X1 = X.clone()
    r3.r3_update_torch(r2, inv_c, torch.tensor(box, dtype=torch.float64), state, seed, [X[:, :d_in]], stats, counts)
    assert int(state) == step + 2 and float(stats[1]) == float(step + 1)
    _, _, want2 = restate(r2.tolist(), inv_c, box, step + 1, seed, X1[:, :d_in])
    assert torch.equal(X[:, :d_in], want2)
    assert bool((X[:, :d_in][released] != X1[:, :d_in][released]).any(1).all())


@pytest.mark.parametrize("n", [1, 257])
def test_mirror_tie_and_nan_release_everything(n):
    box = BOX[:2]
    for case in ("tie", "nan"):
        X = torch.full((n, 2), 0.3)
        r2 = torch.full((n,), 0.25)
        if case == "nan":
            r2 = torch.rand(n) + 0.5
            r2[n // 2] = float("nan")
        state, stats, counts = run_mirror(r2, 1.0, box, 0, 11, X, 2)
        assert int(counts.sum()) == n and int(state) == 1, case
        assert not bool((X == 0.3).all(1).any()), case
        if case == "tie":
            assert float(stats[0]) == 0.5
        else:
            assert math.isnan(float(stats[0]))
        _, rel, want = restate(r2.tolist(), 1.0, box, 0, 11, torch.full((n, 2), 0.3))
        assert bool(rel.all()) and torch.equal(X, want)


def test_population_concentrates_on_a_frozen_fitness():
    """``f(x) = exp(-50 (x - 0.3)^2)`` on ``[-1, 1]``, 2000 points, 40 updates with ``r2`` recomputed from the
    current points: at least half of the population within 0.1 of the peak (a uniform draw: a tenth)."""
    n = 2000
    c = 1.0 / n
    g = torch.Generator().manual_seed(0)
    X = (torch.rand(n, 1, generator=g) * 2.0 - 1.0).float()
    state = torch.zeros((), dtype=torch.int64)
    stats = torch.zeros(2, dtype=torch.float64)
    counts = torch.zeros((n + 255) // 256, dtype=torch.int32)
    box = torch.tensor([[-1.0, 1.0]], dtype=torch.float64)
    for _ in range(40):
        f = torch.exp(-50.0 * (X.double()[:, 0] - 0.3) ** 2)
        r3.r3_update_torch((c * f * f).float(), 1.0 / c, box, state, 2023, [X], stats, counts)
    share = float(((X[:, 0] - 0.3).abs() < 0.1).float().mean())
    print(f"R3_CONCENTRATION share within 0.1 of the peak after 40 updates: {share:.3f}")
    assert int(state) == 40
    assert share >= 0.5


# ------------------------------------------------------------------------------------------
# the solver
# ------------------------------------------------------------------------------------------
def burgers(n_f=500, seed=0):
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
    return D, bcs, f_model


def compiled(layers=(2, 16, 16, 1), backend="jet", resample="r3", problem=None, **kw):
    D, bcs, f = problem if problem is not None else burgers()
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile(list(layers), f, D, bcs, backend=backend, device="cpu", resample=resample, **kw)
    return m


def residual_rows(m, prog):
    si = m._r3_residual_segment(prog)
    return prog.segment_rows(si)


def test_one_step_moves_exactly_the_rows_below_the_mean():
    m = compiled(resample_seed=7)
    assert m.isR3 and m.active_backend == "jet" and m.variables[1:] == []
    assert len(m.lambdas) == 1 and bool((m.lambdas[0] == 1.0).all())
    X0 = m.collocation_points()
    assert torch.equal(X0, m.X_f_local)
    assert m.resample_stats()["step"] == 0
    f = m.program().residual_on(m.f_model, m.X_f_local)[0].reshape(-1).double().abs()
    tau = f.mean()
    near = (f - tau).abs() <= 1e-3 * tau
    assert float(near.float().mean()) <= 0.02
    m.fit(tf_iter=1)
    X1 = m.collocation_points()
    changed = (X1 != X0).any(1)
    assert torch.equal(changed[~near], (f <= tau)[~near])
    st = m.resample_stats()
    assert st["step"] == 1 and st["released"] == int(changed.sum()) and 0 < st["released"] < 500
    assert st["threshold"] == pytest.approx(float(tau), rel=1e-4)
    prog = m.program()
    assert torch.equal(X1, residual_rows(m, prog))
    seg = prog.segments[m._r3_residual_segment(prog)]
    assert seg.X.data_ptr() == residual_rows(m, prog).data_ptr()     # what the user's callables are handed
    assert bool((m.lambdas[0] == 1.0).all())
    lo, hi = torch.tensor([-1.0, 0.0]), torch.tensor([1.0, 1.0])
    assert bool(((X1 >= lo) & (X1 <= hi)).all())
    # the loss is today's unweighted loss: the first step ran on the same points as a solver without the mode
    ref = compiled(resample=None)
    ref.fit(tf_iter=1)
    for k, v in ref.losses[0].items():
        assert m.losses[0][k] == pytest.approx(v, rel=1e-6), k


@pytest.mark.parametrize("prebuilt", [False, True])
def test_lbfgs_runs_on_the_final_adam_population(prebuilt):
    m = compiled(resample_seed=3, precision="bf16", newton_precision="bf16x3")
    if prebuilt:   # the L-BFGS objective's program exists before the points move (as on a GPU)
        assert m.program(precision="bf16x3") is not m.program()
    m.fit(tf_iter=5, newton_iter=3)
    twin = compiled(resample_seed=3, precision="bf16", newton_precision="bf16x3")
    twin.fit(tf_iter=5)
    final = twin.collocation_points()
    assert m.resample_stats()["step"] == 5 and m.fit_info["lbfgs"]["n_iter"] >= 1
    assert torch.equal(m.collocation_points(), final)
    assert torch.equal(m.X_f_local, final)
    assert torch.equal(torch.cat(m.X_f_in, 1), final)
    lb = m._get_lbfgs_engine().program
    assert lb is not m.program()
    assert torch.equal(residual_rows(m, lb), final)
    assert torch.equal(lb.segments[m._r3_residual_segment(lb)].X, final)
    # a second fit continues from the population and the counter
    m.fit(tf_iter=2)
    assert m.resample_stats()["step"] == 7
    assert torch.equal(residual_rows(m, lb), m.collocation_points())


def test_checkpoint_resume_is_bitwise(tmp_path):
    a = compiled(resample_seed=5)
    a.fit(tf_iter=3)
    a.fit(tf_iter=3)
    b = compiled(resample_seed=5)
    b.fit(tf_iter=3)
    path = str(tmp_path / "ck.pt")
    b.save(path)
    c = compiled(resample_seed=99)          # the checkpoint's seed wins
    with torch.no_grad():
        c.u_model.flat.zero_()
    c.resume(path)
    assert c.resample_seed == 5 and c.resample_stats()["step"] == 3
    assert torch.equal(c.collocation_points(), b.collocation_points())
    c.fit(tf_iter=3)
    assert torch.equal(c.u_model.flat, a.u_model.flat)
    assert torch.equal(c.collocation_points(), a.collocation_points())
    assert c.resample_stats() == a.resample_stats() and a.resample_stats()["step"] == 6
    assert [h["Total Loss"] for h in c.losses[-3:]] == [h["Total Loss"] for h in a.losses[-3:]]


@pytest.mark.parametrize("kw, exc, word", [
    (dict(resample="rad"), ValueError, "resample must be"),
    (dict(Adaptive_type=1), ValueError, "Adaptive_type"),
    (dict(Adaptive_type=2), ValueError, "Adaptive_type"),
    (dict(Adaptive_type="ntk"), ValueError, "Adaptive_type"),
    (dict(Adaptive_type="causal"), ValueError, "Adaptive_type"),
    (dict(dict_adaptive={"residual": [True], "BCs": [False, False, False]}), Exception, "weight vectors"),
    (dict(g=lambda lam: lam ** 2), Exception, "weight function g"),
    (dict(backend="autograd"), ValueError, "autograd"),
])
def test_compile_refusals(kw, exc, word):
    with pytest.raises(exc, match=word):
        compiled(**kw)


def test_refuses_two_residual_outputs():
    D, bcs, f = burgers()

    def f2(u_model, x, t):
        r = f(u_model, x, t)
        return r, 2.0 * r
    with pytest.raises(ValueError, match="one residual output"):
        compiled(layers=(2, 8, 1), problem=(D, bcs, f2))


def test_refuses_dist(monkeypatch):
    from tensordiffeq_amd.parallel import dist as pdist
    monkeypatch.setattr(pdist, "init_distributed", lambda auto_launch=True: pdist.get_context("cpu"))
    with pytest.raises(ValueError, match="dist=True"):
        compiled(layers=(2, 8, 1), dist=True)


def test_refuses_an_unbounded_variable():
    D, bcs, f = burgers()
    D.get_dict("x")["range"] = [-math.inf, 1.0]
    with pytest.raises(ValueError, match="finite range"):
        compiled(layers=(2, 8, 1), problem=(D, bcs, f))


def test_refuses_batch_sz_at_fit():
    m = compiled()
    with pytest.raises(ValueError, match="batch_sz"):
        m.fit(tf_iter=2, batch_sz=50)


def test_refuses_a_high_order_residual_segment():
    """(On the CPU no segment runs on the high-order plan, so the flag is set by hand; tests/test_r3_gpu.py
    compiles a KdV residual.)"""
    m = compiled()
    prog = m.program()
    si = m._r3_residual_segment(prog)
    prog.segments[si].hi = True
    with pytest.raises(ValueError, match="order 3 or 4"):
        m._r3_residual_segment(prog)
    with pytest.raises(ValueError, match="high-order plan"):
        prog.refresh_points(si)


def test_stats_need_the_mode():
    m = compiled(resample=None)
    with pytest.raises(ValueError, match="resample='r3'"):
        m.resample_stats()
    assert torch.equal(m.collocation_points(), m.X_f_local)


def test_resample_none_changes_nothing():
    import inspect
    sig = inspect.signature(tdq.CollocationSolverND.compile).parameters
    assert sig["resample"].default is None and sig["resample_seed"].default is None
    m = compiled(resample=None)
    assert not m.isR3 and m.lambdas == [] and m.g is None and m.lambdas_map == {"residual": [], "bcs": []}
    prog = m.program()
    assert all(t.lam is None for t in prog.terms) and prog.g is None
    si = next(t for t in prog.terms if t.kind == "residual").seg
    assert prog.segments[si].X.data_ptr() != prog.segment_rows(si).data_ptr()   # the segment keeps its own copy
    X0 = m.X_f_local.clone()
    m.fit(tf_iter=3, newton_iter=2)
    assert torch.equal(m.X_f_local, X0) and torch.equal(prog.segment_rows(si), X0)
    eng = m._get_engine(None, 1)
    assert eng.after_loss is None


def test_example_runs(monkeypatch):
    import importlib.util
    import os
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.syspath_prepend(ex)
    spec = importlib.util.spec_from_file_location("AC_r3", os.path.join(ex, "AC-r3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(["--iters", "3", "--newton", "1", "--n-f", "300", "--device", "cpu", "--quiet"])
    assert all(math.isfinite(v) for v in res.values() if isinstance(v, float))
    assert res["r3_step"] == 3 and 0 < res["r3_released"] <= 300
