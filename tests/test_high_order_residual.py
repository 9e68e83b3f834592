"""Residuals with third / fourth derivatives on every collocation point (KdV, Kuramoto-Sivashinsky,
beam) on the HIP path: the planner makes such a program mixed (order <= 2 streams of every point on the
fused jet kernels, the high-order streams on ops/jet_hi.py's tile kernels), the step keeps the fused
loss, the fused tail and the K-step graphs, and loss / gradients agree with the torch jet backend.

Measured values: profiles/r14_kdv_errors.txt.
"""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd.boundaries import IC, DomainND, FunctionDirichletBC
from tensordiffeq_amd.jet import JetPlan
from tensordiffeq_amd.ops import jet_hi

EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
C, X0 = 2.0, -1.0


def _soliton(x, t):
    return 0.5 * C / np.cosh(0.5 * math.sqrt(C) * (x - C * t - X0)) ** 2


def _u(u_model, x, t):
    return u_model(torch.cat([x, t], 1))


def kdv(u_model, x, t):
    u = _u(u_model, x, t)
    u_x = tdq.grad(u, x)
    return tdq.grad(u, t) + 6.0 * u * u_x + tdq.grad(tdq.grad(u_x, x), x)


def ks(u_model, x, t):
    u = _u(u_model, x, t)
    u_x = tdq.grad(u, x)
    u_xx = tdq.grad(u_x, x)
    return tdq.grad(u, t) + u * u_x + u_xx + tdq.grad(tdq.grad(u_xx, x), x)


def beam(u_model, x, t):
    u = _u(u_model, x, t)
    u_xx = tdq.grad(tdq.grad(u, x), x)
    return tdq.grad(tdq.grad(u, t), t) + tdq.grad(tdq.grad(u_xx, x), x)


PLANS = {"kdv": (kdv, 5), "ks": (ks, 6), "beam": (beam, 7)}


def _model(f_model, n_f, backend, precision, device, sizes, sa=False, nx=128, nt=64, seed=0):
    """Residual on n_f points, IC on nx and Dirichlet values on 2 x nt points from the soliton."""
    tdq.set_seed(seed)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-5.0, 5.0], nx)
    D.add("t", [0.0, 1.0], nt)
    D.generate_collocation_points(n_f)
    bcs = [IC(D, [lambda x: _soliton(x, 0.0)], var=[["x"]]),
           FunctionDirichletBC(D, fun=[lambda t: _soliton(5.0, t)], var="x", target="upper", func_inputs=["t"]),
           FunctionDirichletBC(D, fun=[lambda t: _soliton(-5.0, t)], var="x", target="lower", func_inputs=["t"])]
    kw = {}
    if sa:
        g = torch.Generator().manual_seed(1)
        kw = {"Adaptive_type": "self-adaptive", "dict_adaptive": {"residual": [True], "BCs": [False, False, False]},
              "init_weights": {"residual": [torch.rand(n_f, 1, generator=g)], "BCs": [None, None, None]}}
    m = tdq.CollocationSolverND(verbose=False)
    m.compile(sizes, f_model, D, bcs, backend=backend, device=device, precision=precision, **kw)
    return m


def _fused(m):
    """``(loss, [gradient per variable])`` of the step's own path: forward, high-order forward, fused
    loss, backward, high-order backward (``AdamEngine._phase_a``) - ``model.grad()`` composes the loss
    with autograd and serves the high-order rows from the torch jet."""
    total, grads, _ = m._get_engine(None, 1)._phase_a()
    torch.cuda.synchronize()
    return total, [g.detach().clone() for g in grads]


def _errors(tag, a, b):
    """Loss, theta-gradient and (if any) SA-weight-gradient errors of the fused path of ``a`` against
    ``b.grad()`` (torch jet backend, same seed: same points, weights and SA weights)."""
    la, ga = _fused(a)
    lb, gb = b.grad()
    assert len(ga) == len(gb)
    e_loss = abs(la.item() - lb.item()) / abs(lb.item())
    e = [((x.reshape(-1) - y.reshape(-1)).norm() / y.norm().clamp_min(1e-30)).item() for x, y in zip(ga, gb)]
    print(f"HOR {tag}: loss {la.item():.6e} vs {lb.item():.6e} rel {e_loss:.2e}, grad theta {e[0]:.2e}"
          + (f", SA weights {e[1]:.2e}" if len(e) > 1 else ""))
    return e_loss, e[0], (e[1] if len(e) > 1 else None)


def _assert_hip_mixed(m, n_hi):
    p = m.program()
    assert m.active_backend == "hip", (m.active_backend, p.reasons)
    assert p.mixed and p.hi_op is not None and p.fused_op is not None, p.reasons
    assert p.n_hi == n_hi
    return p


# bf16x3 bounds against the torch jet backend: three times the largest value measured on an MI355X
# (profiles/r14_kdv_errors.txt: loss <= 3.89e-06, theta gradient <= 4.46e-06, SA-weight gradient 9.39e-06).
# The issue's starting bounds were those of test_ac_baseline_fused_high_order_path (1e-4 / 1e-3), where
# the high-order rows are a fiftieth of the loss; here they are all of it and came out far below.
LOSS_BOUND, GRAD_BOUND, SA_BOUND = 1.2e-5, 1.4e-5, 2.8e-5


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("sa", [False, True], ids=["plain", "self-adaptive"])
def test_kdv_solver_runs_on_the_hip_kernels(sa):
    """KdV residual on 4,096 collocation points, [2,64,64,64,1], IC 128 + 2 x 64 Dirichlet points, bf16x3:
    the program is mixed on the HIP backend with the high-order kernels and the fused loss (on the code
    before this path it planned as ``jet``); loss, theta gradient and SA-weight gradient within LOSS_BOUND /
    GRAD_BOUND / SA_BOUND of the torch jet backend (measured 3.75e-06 / 4.38e-06 / 9.39e-06); in bf16 (only the
    order <= 2 rows change precision) within the bf16 factors of tests/test_hip_kernels.py (3e-3 / 3e-2;
    measured 1.1e-3 / 2.5e-3, SA weights 3.2e-3); 24 Adam steps under K-step graphs end within 2e-2 of the
    jet run's loss (measured 3e-6); 20 L-BFGS iterations are finite and not above the Adam end.  4,096
    points are below ops/jet_hi.py's AUTO_TILE_N: the 4-point kernels (the tile kernels run through the
    solver in test_kdv_9000_points_run_as_one_range)."""
    sizes = [2, 64, 64, 64, 1]
    a = _model(kdv, 4096, "auto", "bf16x3", "cuda", sizes, sa)
    b = _model(kdv, 4096, "jet", None, "cuda", sizes, sa)
    pa = _assert_hip_mixed(a, 4096)
    assert pa.X_all.shape[0] == 4096 + 128 + 2 * 64 and b.active_backend == "jet"
    assert pa.hi_op.entry == "hi" and pa.plan_hi.S == 5 and pa.plan.order == 0
    e_loss, e_grad, e_sa = _errors(f"kdv bf16x3 sa={sa}", a, b)
    assert e_loss < LOSS_BOUND and e_grad < GRAD_BOUND, (e_loss, e_grad)
    if sa:
        assert e_sa < SA_BOUND, e_sa
    h = _model(kdv, 4096, "auto", "bf16", "cuda", sizes, sa)
    _assert_hip_mixed(h, 4096)
    e_loss, e_grad, e_sa = _errors(f"kdv bf16 sa={sa}", h, b)
    assert e_loss < 1e-5 * 300 and e_grad < 1e-4 * 300, (e_loss, e_grad)
    if sa:
        assert e_sa < 1e-4 * 300, e_sa
    a.fit(tf_iter=24)
    b.fit(tf_iter=24)
    eng = a._get_engine(None, 1)
    assert eng._tail_eligible() and getattr(eng, "graph_k", None) is not None
    ha, hb = [r["Total Loss"] for r in a.losses], [r["Total Loss"] for r in b.losses]
    print(f"HOR kdv sa={sa} fit24: {ha[-1]:.6e} vs {hb[-1]:.6e}")
    assert abs(ha[-1] - hb[-1]) / hb[-1] < 2e-2
    a.fit(newton_iter=20)
    print(f"HOR kdv sa={sa} l-bfgs 20: {a.min_loss['l-bfgs']:.6e}")
    assert np.isfinite(a.min_loss["l-bfgs"]) and a.min_loss["l-bfgs"] <= ha[-1]


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("tile", ["auto", "8"])
def test_kdv_9000_points_run_as_one_range(tile, monkeypatch):
    """9,000 collocation points, TDQ_SPLIT at auto: the 0.62 cut of mixed programs (point 5,760 of 9,256)
    cannot hold the high-order block [0, 9000), so point_ranges gives one range and the step, the K-step
    graphs and the L-BFGS objective run without raising - on the 4-point kernels (auto at this size) and
    with the 8-point tile kernels forced (TDQ_HI_TILE).  Same bounds as the 4,096-point program."""
    from tensordiffeq_amd.fit import point_ranges
    monkeypatch.delenv("TDQ_SPLIT", raising=False)
    monkeypatch.setenv("TDQ_HI_TILE", tile)
    sizes = [2, 64, 64, 64, 1]
    a = _model(kdv, 9000, "auto", "bf16x3", "cuda", sizes)
    b = _model(kdv, 9000, "jet", None, "cuda", sizes)
    pa = _assert_hip_mixed(a, 9000)
    assert pa.X_all.shape[0] >= 8192 and point_ranges(pa, pa.fused_op) is None
    assert (pa.hi_op.entry, pa.hi_op.tile, pa.hi_op.tile_bwd) == (("hi", 4, 4) if tile == "auto" else ("hi_tile", 8, 8))
    e_loss, e_grad, _ = _errors(f"kdv 9000 tile {tile}", a, b)
    assert e_loss < LOSS_BOUND and e_grad < GRAD_BOUND, (e_loss, e_grad)
    a.fit(tf_iter=24)
    b.fit(tf_iter=24)
    la, lb = a.losses[-1]["Total Loss"], b.losses[-1]["Total Loss"]
    print(f"HOR kdv 9000 fit24: {la:.6e} vs {lb:.6e}")
    assert abs(la - lb) / lb < 2e-2
    a.fit(newton_iter=20)
    assert np.isfinite(a.min_loss["l-bfgs"]) and a.min_loss["l-bfgs"] <= la


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ks", "beam"])
def test_other_high_order_plans(name, monkeypatch):
    """Kuramoto-Sivashinsky (S = 6) and beam (S = 7) residuals, 2,500 points on [2,32,32,1]: one
    evaluation each with the 8-point tile kernels forced, same backend assertions and bounds as the KdV
    program (measured: loss 3.1e-06, gradient 3.2e-06)."""
    monkeypatch.setenv("TDQ_HI_TILE", "8")
    f, S = PLANS[name]
    a = _model(f, 2500, "auto", "bf16x3", "cuda", [2, 32, 32, 1])
    b = _model(f, 2500, "jet", None, "cuda", [2, 32, 32, 1])
    pa = _assert_hip_mixed(a, 2500)
    assert pa.plan_hi.S == S and pa.hi_op.entry == "hi_tile"
    e_loss, e_grad, _ = _errors(name, a, b)
    assert e_loss < LOSS_BOUND and e_grad < GRAD_BOUND, (e_loss, e_grad)


@pytest.mark.gpu
def test_discovery_model_kdv_coefficients():
    """DiscoveryModel with the KdV residual's two coefficients as variables on 2,000 points of the
    soliton: HIP backend with the high-order kernels; theta, collocation-weight and coefficient
    gradients of the step's path against the jet backend at the KdV program's bounds (measured: loss
    2.1e-06, theta 2.8e-06, collocation weights 7.5e-06, coefficients 5.2e-06 / 2.8e-06)."""
    from tensordiffeq_amd.models import DiscoveryModel

    def f_model(u_model, var, x, t):
        u = _u(u_model, x, t)
        u_x = tdq.grad(u, x)
        return tdq.grad(u, t) + var[0] * u * u_x + var[1] * tdq.grad(tdq.grad(u_x, x), x)

    rng = np.random.default_rng(0)
    x, t = rng.uniform(-5, 5, (2000, 1)), rng.uniform(0, 1, (2000, 1))
    u = _soliton(x, t)

    def build(backend, precision):
        tdq.set_seed(0)
        cw = torch.rand(2000, 1, generator=torch.Generator().manual_seed(1))
        m = DiscoveryModel(verbose=False)
        m.compile([2, 32, 32, 1], f_model, [x, t], u, [tdq.Variable(4.0), tdq.Variable(0.5)], col_weights=cw,
                  backend=backend, device="cuda", precision=precision)
        return m

    a, b = build("auto", "bf16x3"), build("jet", None)
    pa = a.program()
    assert pa.backend == "hip" and pa.mixed and pa.hi_op is not None and pa.fused_op is not None, pa.reasons
    assert pa.n_hi == 2000 and b.program().backend == "jet"
    total, ga, _ = a._get_engine(1)._phase_a()
    torch.cuda.synchronize()
    lb, gb = b.grad()
    assert len(ga) == len(gb) == 4
    e_loss = abs(total.item() - lb.item()) / abs(lb.item())
    e = [((p.reshape(-1) - q.reshape(-1)).norm() / q.norm().clamp_min(1e-30)).item() for p, q in zip(ga, gb)]
    print(f"HOR discovery: loss rel {e_loss:.2e}, theta {e[0]:.2e}, col weights {e[1]:.2e}, c1 {e[2]:.2e}, c2 {e[3]:.2e}")
    assert e_loss < LOSS_BOUND and max(e[0], e[2], e[3]) < GRAD_BOUND and e[1] < SA_BOUND, (e_loss, e)
    a.fit(tf_iter=8)
    assert np.isfinite(float(a.vars[0].detach())) and np.isfinite(float(a.vars[1].detach()))


@pytest.mark.gpu
def test_tile_selection_by_point_count():
    """None -> the 4-point entry points below 2,048 points (402, 2,047), a large tile at 20,000 (the
    threshold of the sweep, AUTO_TILE_N); at 402 points the gradient is bit-equal to an op forced to tile 4."""
    from tests.test_jet_hi_oracle import _make_net
    dev = torch.device("cuda", 0)
    net = _make_net([2, 128, 128, 1], dev)
    plan = JetPlan([(0, 0, 0), (1,)], 2)
    rows = {m: i for i, m in enumerate(plan.streams)}
    X = (2 * torch.rand(20000, 2, device=dev) - 1).contiguous()
    ops = {n: jet_hi.HiJetOp(net, plan, rows, X, n, dev) for n in (402, 2047, 20000)}
    assert ops[402].entry == "hi" and ops[2047].entry == "hi" and (ops[402].tile, ops[2047].tile_bwd) == (4, 4)
    assert ops[20000].entry == "hi_tile" and ops[20000].tile in (8, 16) and ops[20000].tile_bwd in (8, 16)
    four = jet_hi.HiJetOp(net, plan, rows, X, 402, dev, tile=4)
    assert four.entry == "hi"
    dJ = torch.randn(plan.S, 20000, 1, device=dev)
    out = []
    for op in (ops[402], four):
        J = torch.zeros(plan.S, 20000, 1, device=dev)
        op.forward(J, net.flat)
        out.append((J, op.backward(dJ, net.flat).clone()))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    J = torch.zeros(plan.S, 20000, 1, device=dev)
    ops[20000].forward(J, net.flat)
    assert torch.isfinite(ops[20000].backward(dJ, net.flat)).all() and torch.isfinite(J).all()


@pytest.mark.gpu
def test_scratch_cap_keeps_the_jet_backend(monkeypatch):
    """With the cap at 1 MiB the KdV program (4,096 points x 8 streams x 3 layers: 151 MB of scratch)
    stays on the torch jet, the reason names the cap; without it the same program is mixed."""
    monkeypatch.setenv("TDQ_HI_SCRATCH_BYTES", str(1 << 20))
    m = _model(kdv, 4096, "auto", "bf16x3", "cuda", [2, 64, 64, 64, 1])
    p = m.program()
    assert p.backend == "jet" and not p.mixed and p.hi_op is None
    assert any("TDQ_HI_SCRATCH_BYTES" in r for r in p.reasons), p.reasons
    loss, grads = m.grad()
    assert torch.isfinite(loss) and torch.isfinite(grads[0]).all()
    monkeypatch.delenv("TDQ_HI_SCRATCH_BYTES")
    assert _model(kdv, 4096, "auto", "bf16x3", "cuda", [2, 64, 64, 64, 1]).program().mixed


def test_scratch_cap_arithmetic(monkeypatch):
    """Three fp32 buffers of layers x points x streams x 128: by the plan's S from AUTO_TILE_N points on,
    by MAX_S below (the 4-point entry points' sizing); the cap defaults to 32 GiB."""
    assert jet_hi.scratch_bytes(20000, 4, 5) == 3 * 4 * 20000 * 5 * 128 * 4
    assert jet_hi.scratch_bytes(402, 4, 5) == 3 * 4 * 402 * 8 * 128 * 4
    assert jet_hi.AUTO_TILE_N >= jet_hi.SMALL_N == 2048
    monkeypatch.delenv("TDQ_HI_SCRATCH_BYTES", raising=False)
    assert jet_hi.scratch_cap() == 32 << 30
    monkeypatch.setenv("TDQ_HI_SCRATCH_BYTES", "1048576")
    assert jet_hi.scratch_cap() == 1 << 20
    # a million points of the beam plan on four layers: 43 GB, above the default cap
    assert jet_hi.scratch_bytes(10 ** 6, 4, 7) > 32 << 30 > jet_hi.scratch_bytes(10 ** 6, 4, 5)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_high_order_programs_on_the_cpu_stay_on_the_jet(name):
    """device="cpu": the KdV / KS / beam programs plan as ``jet`` (no split) and evaluate."""
    f, S = PLANS[name]
    m = _model(f, 64, "auto", None, "cpu", [2, 16, 16, 1], nx=16, nt=8)
    p = m.program()
    assert p.backend == "jet" and not p.mixed and p.plan.S == S and p.plan.order == (3 if name == "kdv" else 4)
    si, sc = jet_hi.build_spec(p.plan, {})
    assert si[0] == S and len(sc) == {"kdv": 7, "ks": 12, "beam": 14}[name]
    loss, grads = m.grad()
    assert torch.isfinite(loss) and torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0


def _load_example():
    if EX not in sys.path:
        sys.path.insert(0, EX)
    spec = importlib.util.spec_from_file_location("kdv_example", os.path.join(EX, "kdv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_kdv_example_runs_on_the_cpu():
    res = _load_example().main(["--iters", "3", "--newton", "2", "--n-f", "200", "--device", "cpu", "--quiet"])
    assert res["backend"] == "jet" and math.isfinite(res["l2_error"]) and math.isfinite(res["loss"])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_kdv_example_converges_like_the_jet_backend(monkeypatch):
    """examples/kdv.py on a reduced schedule (Adam 2000 + L-BFGS 1000, 5,000 points), same seed, on
    ``auto`` (HIP) and ``--backend jet``: the HIP run's L2 against the exact soliton is at most twice the
    jet run's (the trajectories part ways in precision; this project's seed-to-seed spread on AC-SA is
    1.6x), and the jet run reaches L2 < 0.1 on this schedule.  Measured: HIP 7.13e-04, jet 6.99e-04
    (profiles/r14_kdv_errors.txt)."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = ["--iters", "2000", "--newton", "1000", "--n-f", "5000", "--device", "cuda", "--quiet"]
    hip = _load_example().main(argv)
    jet = _load_example().main(argv + ["--backend", "jet"])
    print(f"HOR example kdv l2: hip {hip['l2_error']:.3e} (adam {hip['adam_ms_per_step']:.3f} ms/step), "
          f"jet {jet['l2_error']:.3e} (adam {jet['adam_ms_per_step']:.3f} ms/step)")
    assert hip["backend"] == "hip" and jet["backend"] == "jet"
    assert jet["l2_error"] < 0.1, jet["l2_error"]
    assert hip["l2_error"] <= 2 * jet["l2_error"], (hip["l2_error"], jet["l2_error"])
