"""Systems of PDEs: networks with several outputs on the jet backends and the fused loss (CPU legs).

The shared program is the nonlinear Schroedinger equation ``i h_t + 1/2 h_xx + |h|^2 h = 0`` with
``h = u + i v`` as the two outputs of one network: ``f_model`` returns the two residuals, a
periodic pair on ``(u, v, u_x, v_x)``, a two-function IC (``u = sech x``, ``v = 0``), SA weights on
the first residual and on the IC.  With 3 and 4 outputs the extra ones enter the second residual,
and the ``(0, 0)`` stream of the last output is never read (the fused loss must write its zeros).

What is checked here: planning on the jet backend for every supported way to pick a component
(before: the nested-autograd backend), the fallback for unsupported ones, ``evaluate`` on the jet
against the autograd backend in float64, the traced program (``fusion.build`` was ``None``), one
output unchanged (STREAM operands, and the generated kernel source by its hash on the parent
commit), per-output targets, and the example.  tests/test_systems_gpu.py has the GPU legs.
"""
import hashlib
import math
import warnings

import numpy as np
import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd import fusion
from tensordiffeq_amd.boundaries import DomainND, IC, FunctionDirichletBC, dirichletBC, periodicBC

IDIOMS = ["slice", "ellipsis", "int", "split", "method_split", "unbind"]
UNSUPPORTED = ["fancy", "arith"]


def _pick(h, idiom, d_out):
    """The components of the network output, each ``(n, 1)``."""
    if idiom == "slice":
        return [h[:, k:k + 1] for k in range(d_out)]
    if idiom == "ellipsis":
        return [h[..., k:k + 1] for k in range(d_out)]
    if idiom == "int":
        return [h[:, k].reshape(-1, 1) for k in range(d_out)]
    if idiom == "split":
        return list(torch.split(h, 1, dim=1))
    if idiom == "method_split":
        return list(h.split(1, 1))
    if idiom == "unbind":
        return [c.unsqueeze(1) for c in torch.unbind(h, dim=1)]
    if idiom == "fancy":        # a permutation of the columns: not a stream any more
        g = h[:, list(range(d_out))[::-1]]
        return [g[:, d_out - 1 - k:d_out - k] for k in range(d_out)]
    if idiom == "arith":        # arithmetic on the multi-column value before the selection
        g = h * 1.0
        return [g[:, k:k + 1] for k in range(d_out)]
    raise ValueError(idiom)


def nls_model(device, backend, d_out=2, width=16, n_f=300, idiom="slice", precision=None, dirichlet=False,
              ic_funs=None):
    """A compiled solver of the shared NLS program (module docstring).  ``dirichlet``: also a
    Dirichlet condition restricted to one output (``outputs=[1]``)."""
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-5.0, 5.0], 16)
    D.add("t", [0.0, math.pi / 2], 16)
    D.generate_collocation_points(n_f)

    def f_model(u_model, x, t):
        c = _pick(u_model(torch.cat([x, t], 1)), idiom, d_out)
        u, v = c[0], c[1]
        u_t, v_t = tdq.grad(u, t), tdq.grad(v, t)
        u_xx = tdq.grad(tdq.grad(u, x), x)
        v_xx = tdq.grad(tdq.grad(v, x), x)
        sq = u * u + v * v
        r1 = -v_t + 0.5 * u_xx + sq * u
        r2 = u_t + 0.5 * v_xx + sq * v
        if d_out == 4:          # third output: value, u_t-like and u_xx-like streams
            r2 = r2 + 0.3 * c[2] * tdq.grad(c[2], t) - 0.1 * tdq.grad(tdq.grad(c[2], x), x)
        if d_out >= 3:          # last output: its (0, 0) stream is never read
            w = c[d_out - 1]
            r2 = r2 + 0.2 * w * tdq.grad(w, x) + 0.1 * tdq.grad(w, t)
        return r1, r2

    def deriv_model(u_model, x, t):
        c = _pick(u_model(torch.cat([x, t], 1)), idiom, d_out)
        return c[0], c[1], tdq.grad(c[0], x), tdq.grad(c[1], x)

    funs = ic_funs if ic_funs is not None else \
        [lambda x: 1.0 / np.cosh(x), lambda x: 0.0 * x, lambda x: 0.1 * np.sin(x), lambda x: 0.2 * np.cos(x)][:d_out]
    bcs = [IC(D, funs, var=[["x"]] * len(funs)), periodicBC(D, ["x"], [deriv_model])]
    flags, init = [True, False], [None, None]
    if dirichlet:
        bcs.append(dirichletBC(D, val=0.25, var="x", target="upper", outputs=[1]))
        flags, init = flags + [False], init + [None]
    g = torch.Generator().manual_seed(0)
    init[0] = 100 * torch.rand(16, 1, generator=g)
    kw = {} if precision is None else {"precision": precision}
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, width, width, d_out], f_model, D, bcs, backend=backend, device=device,
              Adaptive_type="self-adaptive", dict_adaptive={"residual": [True, False], "BCs": flags},
              init_weights={"residual": [torch.rand(n_f, 1, generator=g), None], "BCs": init}, **kw)
    return m


def autograd_fp64(ref, flat, lambdas):
    """``(total, {term: value}, d theta, [d lambda])`` of the solver ``ref`` (compiled with
    ``backend="autograd"``) evaluated in float64 at the weights ``flat`` / ``lambdas``: its points and
    targets (float32 values) are promoted, so every operation of the nested-autograd loss is float64."""
    prog = ref.program()
    assert prog.backend == "autograd"
    for s in prog.segments:
        s.X = s.X.double()
    for t in prog.terms:
        if torch.is_tensor(getattr(t, "val", None)):
            t.val = t.val.double()
    p = flat.detach().to(prog.device, torch.float64).requires_grad_(True)
    lams = [lam.detach().to(prog.device, torch.float64).requires_grad_(True) for lam in lambdas]
    total, vals = prog.evaluate(p, lams)
    g = torch.autograd.grad(total, [p] + lams, allow_unused=True)
    return total.detach(), {k: v.detach() for k, v in vals.items()}, g[0], list(g[1:])


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


def _maxrel(x, ref):
    ref = ref.double().reshape(-1)
    return ((x.double().reshape(-1) - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# --------------------------------------------------------------------------- 1. planning ------
@pytest.mark.parametrize("idiom", IDIOMS)
def test_system_plans_on_the_jet(idiom):
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # the slow-path warning would fail here
        m = nls_model("cpu", "auto", idiom=idiom)
        prog = m.program()
    assert prog.backend == "jet", prog.reasons
    assert set(prog.plan.streams) == {(), (0,), (1,), (0, 0)}
    ref = nls_model("cpu", "autograd", idiom=idiom)
    assert _rel(m.update_loss().detach(), ref.update_loss().detach()) < 1e-4     # float32 both


def test_multi_column_slice_sums_its_columns():
    """``tdq.grad(h[:, 0:2], x)`` is the sum of the two columns' derivatives (tf.gradients), a
    contiguous slice of a 3-output network staying a stream with those columns."""
    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        return tdq.grad(h[:, 0:2], x) - tdq.grad(h[:, 2:3], t) + tdq.grad(tdq.grad(h, x), x)

    def build(backend):
        tdq.set_seed(0)
        D = DomainND(["x", "t"], time_var="t")
        D.add("x", [-1.0, 1.0], 8)
        D.add("t", [0.0, 1.0], 8)
        D.generate_collocation_points(50)
        torch.manual_seed(0)
        m = tdq.CollocationSolverND(verbose=False)
        m.compile([2, 8, 3], f_model, D, [dirichletBC(D, val=0.0, var="x", target="lower")], backend=backend,
                  device="cpu")
        return m
    m, ref = build("auto"), build("autograd")
    assert m.program().backend == "jet", m.program().reasons
    tot, _, g, _ = autograd_fp64(ref, m.u_model.flat, [])
    p = m.u_model.flat.detach().double().requires_grad_(True)
    got, _ = m.program().evaluate(p, [])
    assert _rel(got.detach(), tot) <= 1e-7
    assert _maxrel(torch.autograd.grad(got, p)[0], g) <= 1e-7
    fl = fusion.build(m.program(), [])
    assert fl is not None, m.program().reasons
    losses = fusion.run_reference(fl, m.program(), m.program().jet(p), [], [])
    assert _rel(sum(losses[1:], losses[0]).detach(), tot) <= 1e-7


# --------------------------------------------------------------------------- 2. fallback ------
@pytest.mark.parametrize("idiom", UNSUPPORTED)
def test_unsupported_selection_runs_on_autograd(idiom):
    with pytest.warns(RuntimeWarning, match="nested-autograd"):
        from tensordiffeq_amd.models import loss as loss_mod
        loss_mod._WARNED.clear()
        m = nls_model("cpu", "auto", idiom=idiom)
        prog = m.program()
    assert prog.backend == "autograd" and prog.plan is None
    assert any("not a derivative stream" in r for r in prog.reasons), prog.reasons
    ref = nls_model("cpu", "autograd", idiom="slice")
    a, b = m.update_loss().detach(), ref.update_loss().detach()
    assert _rel(a, b) < 1e-5, (a, b)            # the same float32 autograd computation, other op order


# --------------------------------------------------------------------------- 3. evaluate ------
@pytest.mark.parametrize("d_out,dirichlet", [(2, False), (3, False), (4, False), (2, True)])
def test_jet_evaluate_matches_autograd_fp64(d_out, dirichlet):
    m = nls_model("cpu", "jet", d_out=d_out, dirichlet=dirichlet)
    ref = nls_model("cpu", "autograd", d_out=d_out, dirichlet=dirichlet)
    tot, vals, g, glam = autograd_fp64(ref, m.u_model.flat, m.lambdas)
    p = m.u_model.flat.detach().double().requires_grad_(True)
    lams = [lam.detach().double().requires_grad_(True) for lam in m.lambdas]
    got, gvals = m.program().evaluate(p, lams)
    gg = torch.autograd.grad(got, [p] + lams)
    errs = {k: _rel(gvals[k].detach(), v) for k, v in vals.items()}
    errs["total"] = _rel(got.detach(), tot)
    errs["theta"] = _maxrel(gg[0], g)
    for k, (a, b) in enumerate(zip(gg[1:], glam)):
        errs[f"lambda{k}"] = _maxrel(a, b)
    print(f"SYSTEMS_CPU evaluate d_out={d_out} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-7, errs


# --------------------------------------------------------------------------- 4. fusion --------
@pytest.mark.parametrize("d_out,dirichlet", [(2, False), (3, False), (4, False), (2, True)])
def test_traced_program_matches_evaluate_fp64(d_out, dirichlet):
    from tests.test_loss_ops_oracle import _traced_vs_evaluate
    m = nls_model("cpu", "jet", d_out=d_out, dirichlet=dirichlet)
    prog = m.program()
    fl = fusion.build(prog, m.lambdas)
    assert fl is not None, prog.reasons
    assert fl.d_out == d_out
    errs = _traced_vs_evaluate(m, fl)
    print(f"SYSTEMS_CPU traced d_out={d_out} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-7, errs
    mask = (1 << fusion.COL_SHIFT) - 1
    ops = [c for gr in fl.groups for c in gr.program.code if c[0] == fusion.OP["STREAM"]]
    assert all((c[3] & mask) < fl.n_streams and (c[3] >> fusion.COL_SHIFT) < d_out for c in ops)
    assert {c[3] >> fusion.COL_SHIFT for c in ops} == set(range(d_out))
    if d_out >= 3:      # the last output's (0, 0) stream is in the plan and never read
        s00 = prog.plan.index[(0, 0)]
        assert not any(c[3] == (s00 | (d_out - 1) << fusion.COL_SHIFT) for c in ops)
    if dirichlet:       # the restricted condition reads output 1 only
        gr = [g for g in fl.groups if prog.segments[g.segs[0]].name == "BC_2"][0]
        assert [c[3] >> fusion.COL_SHIFT for c in gr.program.code if c[0] == fusion.OP["STREAM"]] == [1]


@pytest.mark.parametrize("idiom", IDIOMS)
def test_traced_program_every_idiom(idiom):
    """Every supported selection traces to the same bytecode as the slices."""
    code = {}
    for k in ("slice", idiom):
        m = nls_model("cpu", "jet", idiom=k)
        fl = fusion.build(m.program(), m.lambdas)
        assert fl is not None, m.program().reasons
        code[k] = [gr.program.code for gr in fl.groups]
    assert code[idiom] == code["slice"]


def test_untraceable_system_keeps_the_composed_loss():
    """Arithmetic between the columns of a multi-column stream is refused by the tracer with a
    reason (the program itself still runs: on the jet if only values are combined)."""
    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        s = (h * h).sum(dim=1, keepdim=True)
        return tdq.grad(h[:, 0:1], t) + s, tdq.grad(h[:, 1:2], x)
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 8)
    D.add("t", [0.0, 1.0], 8)
    D.generate_collocation_points(50)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 8, 2], f_model, D, [dirichletBC(D, val=0.0, var="x", target="lower")], backend="auto", device="cpu")
    prog = m.program()
    assert prog.backend == "jet", prog.reasons
    assert fusion.build(prog, []) is None
    assert any("loss fusion disabled" in r for r in prog.reasons), prog.reasons


def test_more_than_four_outputs_are_not_fused():
    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        return tdq.grad(h[:, 0:1], t) + h[:, 4:5]
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 8)
    D.add("t", [0.0, 1.0], 8)
    D.generate_collocation_points(50)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 8, 5], f_model, D, [dirichletBC(D, val=0.0, var="x", target="lower")], backend="jet", device="cpu")
    prog = m.program()
    assert fusion.build(prog, []) is None
    assert any("5 network outputs" in r for r in prog.reasons), prog.reasons


def test_more_than_32_stream_output_pairs_are_not_fused():
    """A second-order plan in three variables (10 streams) with 4 outputs: planned on the jet, loss
    composed, with the reason."""
    def f_model(u_model, x, y, t):
        u = u_model(torch.cat([x, y, t], 1))[:, 0:1]
        u_x, u_y, u_t = tdq.grad(u, x), tdq.grad(u, y), tdq.grad(u, t)
        return (tdq.grad(u_x, x) + tdq.grad(u_x, y) + tdq.grad(u_x, t) + tdq.grad(u_y, y) + tdq.grad(u_y, t)
                + tdq.grad(u_t, t))
    tdq.set_seed(0)
    D = DomainND(["x", "y", "t"], time_var="t")
    for v in ("x", "y", "t"):
        D.add(v, [0.0, 1.0], 4)
    D.generate_collocation_points(40)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([3, 8, 4], f_model, D, [dirichletBC(D, val=0.0, var="x", target="lower")], backend="jet", device="cpu")
    prog = m.program()
    assert prog.plan.S == 10
    assert fusion.build(prog, []) is None
    assert any("10 streams x 4 outputs" in r for r in prog.reasons), prog.reasons


# --------------------------------------------------------------------------- 5. one output ----
# sha256 of ops.loss_jit.generate() for two zoo programs, computed on the parent commit
PARENT_SOURCE_SHA = {
    "tanh": "59ab202b824cabfd4922027ff92d0282070c0f4995a9f97fb8706e2d4e415581",
    "burgers": "9d74efa42649ae6464f2edc55b48a1d700b9427bd8a8f3bfd22fa29df40c9dbc",
}


def test_one_output_programs_unchanged():
    from tensordiffeq_amd.ops import loss_jit
    from tensordiffeq_amd.ops.loss_fused import FusedLossOp
    from tests.test_loss_ops_oracle import ZOO, zoo_model
    for name in ZOO:
        m = zoo_model(name, "cpu", "jet")
        prog = m.program()
        fl = fusion.build(prog, m.lambdas)
        assert fl is not None and fl.d_out == 1
        for gr in fl.groups:
            for c in gr.program.code:
                if c[0] == fusion.OP["STREAM"]:
                    assert 0 <= c[3] < fl.n_streams, (name, c)
        if name in PARENT_SOURCE_SHA:
            op = FusedLossOp(fl, prog, m.lambdas, fusion.scalar_values(fl, m.lambdas, None), fl.lam_offsets)
            assert tuple(op.dJ.shape) == (fl.n_streams, prog.X_all.shape[0], 1)
            assert hashlib.sha256(loss_jit.generate(op).encode()).hexdigest() == PARENT_SOURCE_SHA[name], name


@pytest.mark.parametrize("d_out", [2, 3, 4])
def test_generated_system_kernel(d_out):
    """The specialised kernel of the system: one 8- / 16-byte access per (stream, point) for 2 / 4
    outputs, scalar accesses for 3; it compiles for gfx950."""
    import ctypes
    from tensordiffeq_amd.ops import _lib, loss_jit
    from tensordiffeq_amd.ops.loss_fused import FusedLossOp
    m = nls_model("cpu", "jet", d_out=d_out)
    prog = m.program()
    fl = fusion.build(prog, m.lambdas)
    op = FusedLossOp(fl, prog, m.lambdas, fusion.scalar_values(fl, m.lambdas, None), fl.lam_offsets)
    assert tuple(op.dJ.shape) == (fl.n_streams, prog.X_all.shape[0], d_out)
    src = loss_jit.generate(op)
    vec = {2: "float2", 3: None, 4: "float4"}[d_out]
    n_slots = sum(len(gr.segs) for gr in fl.groups)
    if vec is None:
        assert "float2" not in src and "float4" not in src
        assert src.count("dJ[") == n_slots * fl.n_streams * d_out
    else:
        assert src.count(f"*reinterpret_cast<{vec}*>(dJ") == n_slots * fl.n_streams   # zeros included
        loads = sum(len({(s, c & 255) for (_, _, s, c) in
                         [c for c in gr.program.code if c[0] == fusion.OP["STREAM"]]}) for gr in fl.groups)
        assert src.count(f"*reinterpret_cast<const {vec}*>(J") == loads
        assert " = J[" not in src and "dJ[" not in src
    if not _lib.available():
        pytest.skip("native library not built")
    lib = _lib.load()
    code, size = ctypes.c_void_p(0), ctypes.c_longlong(0)
    log = ctypes.create_string_buffer(8192)
    rc = lib.tdq_rtc_compile(src.encode(), b"t.hip", b"gfx950", ctypes.byref(code), ctypes.byref(size), log, 8192)
    assert rc == 0, log.value.decode()
    lib.tdq_rtc_free(code)


# --------------------------------------------------------------------------- 6. targets -------
def test_targets_per_output():
    m = nls_model("cpu", "jet")
    prog = m.program()
    ic = [t for t in prog.terms if t.kind == "ic"][0]
    assert tuple(ic.val.shape) == (16, 2)
    x = np.linspace(-5.0, 5.0, 16)
    assert np.allclose(ic.val[:, 0].numpy(), 1.0 / np.cosh(x), atol=1e-6) and float(ic.val[:, 1].abs().max()) == 0.0
    assert math.isfinite(float(m.update_loss().detach()))
    # the definition: the mean over the n * d_out elements of (lam (u_q - val_q))^2
    u = m.u_model(prog.segments[ic.seg].X).detach()
    want = ((m.lambdas[ic.lam].detach() * (u - ic.val)) ** 2).mean()
    assert _rel(m.loss_terms[ic.name], want) < 1e-5
    X = np.random.RandomState(0).uniform(-1, 1, (37, 2))
    u_pred, f_pred = m.predict(X)
    assert u_pred.shape == (37, 2) and len(f_pred) == 2 and f_pred[0].shape == (37, 1)


def test_one_function_broadcasts_over_outputs():
    m = nls_model("cpu", "jet", ic_funs=[lambda x: 1.0 / np.cosh(x)])
    ic = [t for t in m.program().terms if t.kind == "ic"][0]
    assert tuple(ic.val.shape) == (16, 1)
    ref = nls_model("cpu", "autograd", ic_funs=[lambda x: 1.0 / np.cosh(x)])
    assert _rel(m.update_loss().detach(), ref.update_loss().detach()) < 1e-4
    fl = fusion.build(m.program(), m.lambdas)
    assert fl is not None and len(fl.val_arrays) == 1     # one value array, read for both outputs


def test_wrong_function_count_is_refused_at_compile():
    with pytest.raises(ValueError, match="BC_0.*IC"):
        nls_model("cpu", "jet", d_out=3, ic_funs=[lambda x: x, lambda x: x])
    with pytest.raises(ValueError, match="BC_0.*IC"):
        nls_model("cpu", "jet", d_out=2, ic_funs=[lambda x: x, lambda x: x, lambda x: x])
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 8)
    D.add("t", [0.0, 1.0], 8)
    D.generate_collocation_points(20)
    f = lambda u_model, x, t: tdq.grad(u_model(torch.cat([x, t], 1))[:, 0:1], t)    # noqa: E731
    two = FunctionDirichletBC(D, [lambda t: t, lambda t: -t], "x", "upper", [["t"], ["t"]], outputs=[2])
    with pytest.raises(ValueError, match="BC_0.*FunctionDirichletBC"):
        tdq.CollocationSolverND(verbose=False).compile([2, 8, 3], f, D, [two], device="cpu")
    with pytest.raises(ValueError, match="outputs"):
        tdq.CollocationSolverND(verbose=False).compile([2, 8, 3], f, D,
                                                       [dirichletBC(D, 0.0, "x", "upper", outputs=3)], device="cpu")
    ok = FunctionDirichletBC(D, [lambda t: t, lambda t: -t], "x", "upper", [["t"], ["t"]], outputs=[2, 0])
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 8, 3], f, D, [ok], device="cpu")
    t = m.program().terms[0]
    assert t.cols == [2, 0] and tuple(t.val.shape) == (8, 2)


def test_compile_data_per_output():
    from tests.test_solver import burgers
    D, bcs, _ = burgers(n_f=100)

    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        return tdq.grad(h[:, 0:1], t) + h[:, 1:2] * tdq.grad(h[:, 0:1], x)
    rs = np.random.RandomState(0)
    x, t = rs.uniform(-1, 1, (30, 1)), rs.uniform(0, 1, (30, 1))
    m = tdq.CollocationSolverND(assimilate=True, verbose=False)
    m.compile([2, 8, 2], f_model, D, bcs, device="cpu")
    m.compile_data(x, t, rs.randn(30, 2))
    data = [tm for tm in m.program().terms if tm.kind == "data"][0]
    assert tuple(data.val.shape) == (30, 2) and math.isfinite(float(m.update_loss().detach()))
    with pytest.raises(ValueError, match="compile_data"):
        m.compile_data(x, t, rs.randn(30, 3))


# --------------------------------------------------------------------------- 7. example -------
def test_schrodinger_example_runs(monkeypatch):
    from tests.test_examples import _load
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res = _load("schrodinger").main(["--iters", "20", "--newton", "10", "--n-f", "300", "--device", "cpu", "--quiet"])
    assert res["backend"] == "jet"
    for k, v in res.items():
        if isinstance(v, float):
            assert math.isfinite(v), (k, v)
