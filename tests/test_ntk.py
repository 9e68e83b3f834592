"""NTK adaptive loss weights (``Adaptive_type=3`` / ``"ntk"``) on the CPU: the torch path of
``ops/ntk.py`` against a float64 oracle, the weights, the solver's update schedule, the argument checks
and data parallelism over gloo.

Oracle: plain per-instance ``torch.autograd.grad`` of ``f_{o,i}`` with respect to a float64 copy of the
parameter vector, one instance at a time, through ``jet.jet_forward`` - no Gram formula anywhere.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tensordiffeq_amd as tdq
from tensordiffeq_amd import fusion
from tensordiffeq_amd.boundaries import IC, DomainND, FunctionDirichletBC, dirichletBC, periodicBC
from tensordiffeq_amd.jet import JetPlan, jet_forward
from tensordiffeq_amd.models.collocation import parse_adaptive_type
from tensordiffeq_amd.ops import ntk


# ------------------------------------------------------------------------------------------
# programs (<= 40 points per segment)
# ------------------------------------------------------------------------------------------
def _domain(n_f, nx=16, nt=12, xlim=(-1.0, 1.0)):
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", list(xlim), nx)
    D.add("t", [0.0, 1.0], nt)
    D.generate_collocation_points(n_f)
    return D


def _u(u_model, x, t):
    return u_model(torch.cat([x, t], 1))


def burgers(n_f=40):
    """Residual with u_xx, an IC and two Dirichlet BCs."""
    D = _domain(n_f)

    def f_model(u_model, x, t):
        u = _u(u_model, x, t)
        u_x = tdq.grad(u, x)
        return tdq.grad(u, t) + u * u_x - (0.01 / math.pi) * tdq.grad(u_x, x)

    bcs = [IC(D, [lambda x: -np.sin(x * math.pi)], var=[["x"]]),
           dirichletBC(D, val=0.0, var="x", target="upper"), dirichletBC(D, val=0.0, var="x", target="lower")]
    return [2, 12, 12, 1], f_model, D, bcs


def periodic(n_f=40):
    """Allen-Cahn with a periodic BC whose ``deriv_model`` returns (u, u_x)."""
    D = _domain(n_f, nt=11)

    def deriv_model(u_model, x, t):
        u = _u(u_model, x, t)
        return u, tdq.grad(u, x)

    def f_model(u_model, x, t):
        u = _u(u_model, x, t)
        return tdq.grad(u, t) - 0.0001 * tdq.grad(tdq.grad(u, x), x) + 5.0 * u ** 3 - 5.0 * u

    bcs = [IC(D, [lambda x: x ** 2 * np.cos(math.pi * x)], var=[["x"]]), periodicBC(D, ["x"], [deriv_model])]
    return [2, 12, 12, 1], f_model, D, bcs


def system(n_f=40):
    """Two outputs: two residual outputs and a two-column IC."""
    D = _domain(n_f, xlim=(-5.0, 5.0))

    def f_model(u_model, x, t):
        h = _u(u_model, x, t)
        u, v = h[:, 0:1], h[:, 1:2]
        sq = u * u + v * v
        return (-tdq.grad(v, t) + 0.5 * tdq.grad(tdq.grad(u, x), x) + sq * u,
                tdq.grad(u, t) + 0.5 * tdq.grad(tdq.grad(v, x), x) + sq * v)

    bcs = [IC(D, [lambda x: 1.0 / np.cosh(x), lambda x: 0.1 * np.sin(x)], var=[["x"], ["x"]])]
    return [2, 12, 12, 2], f_model, D, bcs


def kdv(n_f=40):
    """An order-3 residual (u_xxx)."""
    D = _domain(n_f, xlim=(-5.0, 5.0))

    def f_model(u_model, x, t):
        u = _u(u_model, x, t)
        u_x = tdq.grad(u, x)
        return tdq.grad(u, t) + 6.0 * u * u_x + tdq.grad(tdq.grad(u_x, x), x)

    sol = lambda x, t: 1.0 / np.cosh(x - 2.0 * t + 1.0) ** 2   # noqa: E731
    bcs = [IC(D, [lambda x: sol(x, 0.0)], var=[["x"]]),
           FunctionDirichletBC(D, fun=[lambda t: sol(5.0, t)], var="x", target="upper", func_inputs=["t"])]
    return [2, 12, 12, 1], f_model, D, bcs


PROGRAMS = {"burgers": burgers, "periodic": periodic, "system": system, "kdv": kdv}


def model(name, device="cpu", backend="jet", adaptive="ntk", seed=0, layers=None, n_f=40, **kw):
    tdq.set_seed(seed)
    sizes, f_model, D, bcs = PROGRAMS[name](n_f)
    torch.manual_seed(seed)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile(layers or sizes, f_model, D, bcs, Adaptive_type=adaptive, backend=backend, device=device, **kw)
    return m


# ------------------------------------------------------------------------------------------
# float64 oracle
# ------------------------------------------------------------------------------------------
def oracle(m, flat=None):
    """``(T (n_terms,), {(group, output): per-instance norms})`` in float64 on the CPU: every
    ``f_{o,i}`` of the solver's traced program differentiated on its own."""
    prog = m.program()
    fl = prog.fused_op.fl if prog.fused_op is not None else fusion.build(prog, m.lambdas)
    assert fl is not None, prog.reasons
    idx, rows = prog.fused_streams()
    plan = JetPlan(set(idx) - {()}, prog.d_in)
    p = (m.u_model.flat if flat is None else flat).detach().double().cpu().requires_grad_(True)
    X = prog.X_all.detach().double().cpu()
    Jp = jet_forward(X, prog.net.weights(p), plan)
    J = torch.stack([Jp[plan.index[mi]] for mi, _ in sorted(idx.items(), key=lambda kv: kv[1])])
    lams = [lam.detach().double().cpu() for lam in m.lambdas]
    scal = fusion.scalar_values(fl, lams, None)
    T = torch.zeros(len(fl.term_names), dtype=torch.float64)
    norms = {}
    for gi, gr in enumerate(fl.groups):
        n = gr.n
        off = [prog.segments[s].offset for s in gr.segs]
        vals = fusion.eval_group(gr.program, n, lambda a, r, c: J[r, off[a]:off[a] + n, c],
                                 lambda a, j: X[off[a]:off[a] + n, j], lambda a: fl.val_arrays[a].double().cpu(),
                                 lambda a: lams[fl.lam_slots[a]].reshape(-1), lambda a: scal[a], "cpu", torch.float64)
        for oi, (fr, _, t, c) in enumerate(gr.program.outputs):
            f = vals[fr]
            n2 = torch.stack([torch.autograd.grad(f[i], p, retain_graph=True)[0].square().sum() for i in range(n)])
            norms[(gi, oi)] = n2
            T[t] += c * n2.sum()
    return T, norms


_ORACLE = {}


def shared_oracle(name):
    """The oracle of ``model(name)`` (seed 0), computed once per session."""
    if name not in _ORACLE:
        _ORACLE[name] = oracle(model(name))
    return _ORACLE[name]


def maxrel(x, ref):
    return float((x.double().cpu() - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------
# 1. torch-path traces against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_torch_traces_match_the_oracle(name):
    m = model(name)
    op = m._ntk_op()
    assert op.kind == "torch"
    T_ref, norms_ref = shared_oracle(name)
    assert (T_ref > 0).all()
    # the same formula in float64: round-off of a different summation order only
    T64 = op.traces(m.u_model.flat.detach().double())
    assert maxrel(T64, T_ref) < 1e-11
    for key, ref in norms_ref.items():
        assert maxrel(op.instance_norms(*key), ref) < 1e-10, key
    # float32 parameters (what the solver runs): fp32 round-off of the jet and the Gram sums
    T32 = op.traces()
    assert T32.dtype == torch.float32
    assert float(((T32.double() - T_ref).abs() / T_ref).max()) < 1e-4
    assert m.ntk_traces() == pytest.approx({t: float(v) for t, v in zip(op.fl.term_names, T_ref)}, rel=1e-4)


def test_kdv_program_reads_third_order_streams():
    m = model("kdv")
    assert m.program().plan.order == 3 and (0, 0, 0) in m._ntk_op().plan.streams


# ------------------------------------------------------------------------------------------
# 2. the weights
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["burgers", "system"])
def test_weights_balance_the_traces(name):
    m = model(name)
    assert all(float(lam) == 1.0 for lam in m.lambdas)
    m._ntk_update(0)
    epoch, T, lam = m.ntk_history[-1]
    assert epoch == 0 and set(T) == set(lam) == {t.name for t in m.program().terms}
    total = sum(T.values())
    for k in T:
        assert lam[k] == pytest.approx(total / T[k], rel=1e-6)
        assert lam[k] * T[k] == pytest.approx(total, rel=1e-6)
    # residual weights first, then the BCs, as in lambdas_map
    names = [t.name for t in sorted(m.program().terms, key=lambda t: t.lam)]
    n_res = len(m.lambdas_map["residual"])
    assert names[:n_res] == [f"Residual_{k}" for k in range(n_res)]
    assert [float(m.lambdas[t.lam]) for t in m.program().terms] == [pytest.approx(lam[t.name]) for t in m.program().terms]


def test_unusable_trace_keeps_its_weight():
    lam, ok = ntk.weights(torch.tensor([2.0, 0.0, float("nan"), 6.0]), torch.tensor([1.0, 3.0, 5.0, 7.0]))
    assert ok.tolist() == [True, False, False, True]
    assert lam.tolist() == [4.0, 3.0, 5.0, 8.0 / 6.0]


# ------------------------------------------------------------------------------------------
# 3. the update schedule
# ------------------------------------------------------------------------------------------
def test_fit_updates_every_ntk_every_steps():
    m = model("burgers", ntk_every=10)
    m.fit(tf_iter=25)
    assert [h[0] for h in m.ntk_history] == [0, 10, 20]
    terms = m.program().terms
    # nothing touched the weights since the last update
    assert [float(m.lambdas[t.lam]) for t in terms] == [m.ntk_history[-1][2][t.name] for t in terms]
    lam20 = [lam.clone() for lam in m.lambdas]
    ptrs = [lam.data_ptr() for lam in m.lambdas]
    m.fit(tf_iter=4)          # epochs 25 .. 28: no update
    assert len(m.ntk_history) == 3
    assert all(torch.equal(a, b) for a, b in zip(lam20, m.lambdas))
    m.fit(tf_iter=2)          # epoch 30: an update, in place
    assert [h[0] for h in m.ntk_history] == [0, 10, 20, 30]
    assert ptrs == [lam.data_ptr() for lam in m.lambdas]
    assert any(not torch.equal(a, b) for a, b in zip(lam20, m.lambdas))
    hist = m.losses
    assert len(hist) == 31 and all(math.isfinite(v) for h in hist for v in h.values())
    # the loss is sum_k lambda_k * (unweighted term)
    ref = model("burgers", adaptive=0)
    with torch.no_grad():
        ref.u_model.flat.copy_(m.u_model.flat)
    ref.update_loss()
    by_hand = sum(float(m.lambdas[t.lam]) * float(ref.loss_terms[t.name]) for t in terms)
    assert float(m.update_loss().detach()) == pytest.approx(by_hand, rel=1e-5)
    assert {k: float(v) for k, v in m.loss_terms.items()} == pytest.approx(
        {t.name: float(m.lambdas[t.lam]) * float(ref.loss_terms[t.name]) for t in terms}, rel=1e-5)


def test_minibatch_traces_use_the_full_batch_program():
    m = model("burgers", ntk_every=2)
    m.fit(tf_iter=3, batch_sz=10)
    assert [h[0] for h in m.ntk_history] == [0, 2]
    assert m._ntk_op().prog is m.program()


def test_lbfgs_keeps_the_last_weights():
    m = model("burgers", ntk_every=5)
    m.fit(tf_iter=6, newton_iter=3)
    assert [h[0] for h in m.ntk_history] == [0, 5]
    assert [float(m.lambdas[t.lam]) for t in m.program().terms] == list(m.ntk_history[-1][2].values())


# ------------------------------------------------------------------------------------------
# 4. arguments
# ------------------------------------------------------------------------------------------
def test_argument_errors():
    assert parse_adaptive_type("ntk", ntk=True) == 3 and parse_adaptive_type(3, ntk=True) == 3
    with pytest.raises(NotImplementedError):
        parse_adaptive_type("ntk")
    with pytest.raises(Exception, match="weight vectors"):
        model("burgers", dict_adaptive={"residual": [True], "BCs": [False] * 3},
              init_weights={"residual": [torch.ones(40, 1)], "BCs": [None] * 3})
    with pytest.raises(Exception, match="weight function g"):
        model("burgers", g=lambda lam: lam ** 2)
    with pytest.raises(ValueError, match="autograd"):
        model("burgers", backend="autograd")
    with pytest.raises(ValueError, match="ntk_every"):
        model("burgers", ntk_every=0)


def test_untraceable_loss_is_refused():
    tdq.set_seed(0)
    sizes, _, D, bcs = burgers()

    def f_model(u_model, x, t):     # a data-dependent branch: the tracer cannot fuse it
        u = _u(u_model, x, t)
        return tdq.grad(u, t) + (u if float(u.sum()) > 0 else -u)

    with pytest.raises(ValueError, match="NTK adaptive weighting needs"):
        tdq.CollocationSolverND(verbose=False).compile(sizes, f_model, D, bcs, Adaptive_type="ntk", backend="jet",
                                                       device="cpu")


def test_data_term_gets_the_last_weight():
    tdq.set_seed(0)
    sizes, f_model, D, bcs = burgers()
    m = tdq.CollocationSolverND(assimilate=True, verbose=False)
    m.compile(sizes, f_model, D, bcs, Adaptive_type=3, backend="jet", device="cpu")
    g = np.random.default_rng(0)
    m.compile_data(g.uniform(-1, 1, 20), g.uniform(0, 1, 20), g.normal(size=20))
    data = [t for t in m.program().terms if t.kind == "data"][0]
    assert data.lam == len(m.lambdas) - 1 == m.lambdas_map["data"][0]
    m._ntk_update(0)
    T = m.ntk_history[-1][1]
    assert "Data" in T and float(m.lambdas[data.lam]) == pytest.approx(sum(T.values()) / T["Data"], rel=1e-6)


def test_print_screen_names_the_mode(capsys):
    from tensordiffeq_amd.output import print_screen
    print_screen(model("burgers", ntk_every=7))
    assert "NTK" in capsys.readouterr().out


def test_wave_example_runs():
    import importlib.util
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location("wave_ntk", os.path.join(ex, "wave-ntk.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(["--iters", "4", "--n-f", "200", "--width", "12", "--ntk-every", "2", "--device", "cpu", "--quiet"])
    assert res["ntk_updates"] == 2 and res["ntk_path"] == "torch"
    assert all(math.isfinite(v) for v in res.values() if isinstance(v, float))


# ------------------------------------------------------------------------------------------
# 5. data parallel (gloo, two ranks)
# ------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from tensordiffeq_amd.parallel import dist as pdist
    pdist.reset_context()
    ctx = pdist.init_distributed(backend="gloo", device="cpu")
    m = model("periodic", n_f=41, dist=True)      # shards of 21 and 20 points
    m._ntk_update(0)
    q.put({"rank": rank, "lam": [float(lam) for lam in m.lambdas], "T": m.ntk_history[-1][1]})
    ctx.barrier()
    pdist.destroy()


@pytest.mark.timeout(300)
def test_dp_weights_match_single_process():
    from tensordiffeq_amd.parallel.dist import free_port
    ref = model("periodic", n_f=41)
    ref._ntk_update(0)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=280) for _ in procs), key=lambda r: r["rank"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0]["lam"] == res[1]["lam"]
    assert res[0]["lam"] == pytest.approx([float(lam) for lam in ref.lambdas], rel=1e-5)
    assert res[0]["T"] == pytest.approx(ref.ntk_history[-1][1], rel=1e-5)
