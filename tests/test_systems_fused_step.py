"""Systems of PDEs on the one-launch step: networks with 2-4 outputs on the persistent forward ->
per-point loss -> backward kernels (csrc/jet_fused.h: the bf16 Adam step, csrc/jet_fused3.h: the
bf16x3 L-BFGS objective).

The program is the NLS system of tests/test_systems.py (same f_model, periodic pair on
``(u, v, u_x, v_x)``, two-function IC, SA weights, 16 x 16 domain) with the hidden layers as an
argument: the kernels take width 128 with 3 or 4 hidden layers.  Its fused point set is 16 IC + 32
pair + n_f points: n_f = 40 / 300 give 88 / 348 points (a partial last tile at 16 and at 32 points per
tile), n_f = 8400 gives 8,448 points = 264 / 528 tiles, at least 2 per workgroup on 256 CUs, so the
weight-gradient registers, the bias and loss sums and the refill of the tile's dJ run across tiles.

CPU: the kernels of every served shape compile for gfx950 (host-only hipRTC), the generated loss
names every output column the program reads, and the generated loss of a one-output program has
the statements it had before systems were served.  GPU: routing, one evaluation against float64
(whole vectors, and the output layer's blocks one by one), against the separate launches, every
value written, determinism, training.
"""
import contextlib
import math
import os

import numpy as np
import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd import fusion
from tensordiffeq_amd.boundaries import DomainND, IC, periodicBC
from tests.test_systems import autograd_fp64

L3 = [128, 128, 128]
L4 = [128, 128, 128, 128]


def nls_net(device, backend, hidden, d_out=2, n_f=300, precision=None, reads01=False, **kw):
    """The NLS program of ``tests.test_systems.nls_model`` on ``[2, *hidden, d_out]``.  ``reads01``:
    the loss reads outputs 0 and 1 only (no extra residual terms, a two-function IC restricted to
    those outputs), whatever ``d_out``."""
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-5.0, 5.0], 16)
    D.add("t", [0.0, math.pi / 2], 16)
    D.generate_collocation_points(n_f)

    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        c = [h[:, k:k + 1] for k in range(d_out)]
        u, v = c[0], c[1]
        u_t, v_t = tdq.grad(u, t), tdq.grad(v, t)
        u_xx = tdq.grad(tdq.grad(u, x), x)
        v_xx = tdq.grad(tdq.grad(v, x), x)
        sq = u * u + v * v
        r1 = -v_t + 0.5 * u_xx + sq * u
        r2 = u_t + 0.5 * v_xx + sq * v
        if d_out == 4 and not reads01:      # third output: value, u_t-like and u_xx-like streams
            r2 = r2 + 0.3 * c[2] * tdq.grad(c[2], t) - 0.1 * tdq.grad(tdq.grad(c[2], x), x)
        if d_out >= 3 and not reads01:      # last output: its (0, 0) stream is never read
            w = c[d_out - 1]
            r2 = r2 + 0.2 * w * tdq.grad(w, x) + 0.1 * tdq.grad(w, t)
        return r1, r2

    def deriv_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        return h[:, 0:1], h[:, 1:2], tdq.grad(h[:, 0:1], x), tdq.grad(h[:, 1:2], x)

    funs = [lambda x: 1.0 / np.cosh(x), lambda x: 0.0 * x, lambda x: 0.1 * np.sin(x), lambda x: 0.2 * np.cos(x)]
    if reads01 and d_out > 2:
        ic = IC(D, funs[:2], var=[["x"]] * 2, outputs=[0, 1])
    else:
        ic = IC(D, funs[:d_out], var=[["x"]] * d_out)
    bcs = [ic, periodicBC(D, ["x"], [deriv_model])]
    g = torch.Generator().manual_seed(0)
    init = [100 * torch.rand(16, 1, generator=g), None]
    if precision is not None:
        kw["precision"] = precision
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2] + list(hidden) + [d_out], f_model, D, bcs, backend=backend, device=device,
              Adaptive_type="self-adaptive", dict_adaptive={"residual": [True, False], "BCs": [True, False]},
              init_weights={"residual": [torch.rand(n_f, 1, generator=g), None], "BCs": init}, **kw)
    return m


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _prog_op(m):
    from tensordiffeq_amd.ops.loss_fused import FusedLossOp
    prog = m.program()
    fl = fusion.build(prog, m.lambdas)
    assert fl is not None, prog.reasons
    return prog, FusedLossOp(fl, prog, m.lambdas, fusion.scalar_values(fl, m.lambdas, None), fl.lam_offsets)


# --------------------------------------------------------------------------- CPU -------------
@pytest.mark.parametrize("hidden,d_out", [(L3, 2), (L3, 3), (L3, 4), (L4, 2)])
def test_system_kernels_compile(hidden, d_out):
    """``recipe`` serves the shape in both precisions inside 160 KB of LDS, both kernels compile for
    gfx950, and the generated loss names every (stream, output) the program reads.  (Before systems
    were served ``recipe`` raised for every d_out > 1.)"""
    from tensordiffeq_amd.ops import _lib, fused_step
    from tests.test_fused_step import _compile_ok
    if not _lib.available():
        pytest.skip("native library not built")
    prog, op = _prog_op(nls_net("cpu", "jet", hidden, d_out))
    layout, _, N = fused_step.point_layout(prog, fused_step.fused_groups(prog, op))
    assert N == 16 + 32 + 300
    mask = (1 << fusion.COL_SHIFT) - 1
    for precision in ("bf16", "bf16x3"):
        rec = fused_step.recipe(prog, op, layout, precision)
        assert 0 < rec.lds <= 160 * 1024, rec.lds
        assert rec.cfg["d_out"] == d_out and rec.source is not None
        gen = rec.source[len(fused_step.header_source()):]
        assert f"static constexpr int DOUT = {d_out};" in gen
        cols = set()
        for (P, _, ns, _) in layout:
            for c in P.code:
                if c[0] == fusion.OP["STREAM"]:
                    s, q = c[3] & mask, c[3] >> fusion.COL_SHIFT
                    cols.add(q)
                    assert f"JV({s}, t + {c[2]}, {q})" in gen, (s, c[2], q)
                    assert f"dj{c[2]}_{s}_{q} += " in gen
            for sl in range(ns):        # every output of every (slot, stream) is stored
                for s in range(rec.S):
                    for q in range(d_out):
                        assert f"UB({s}, t + {sl}, {q}) = dj{sl}_{s}_{q};" in gen
        assert cols == set(range(d_out))
        _compile_ok(rec.source)


def test_four_outputs_four_layers_bf16_left_out():
    """bf16 / 4 hidden layers / S = 4 / 4 outputs does not fit the LDS (the partial output dots of 4
    waves x 4 streams x 32 points x 4 outputs): ``recipe`` raises, the program keeps the separate
    launches."""
    from tensordiffeq_amd.ops import _lib, fused_step
    if not _lib.available():
        pytest.skip("native library not built")
    prog, op = _prog_op(nls_net("cpu", "jet", L4, 4))
    layout, _, _ = fused_step.point_layout(prog, fused_step.fused_groups(prog, op))
    with pytest.raises(ValueError):
        fused_step.recipe(prog, op, layout, "bf16")


# the statements of each loss group of the AC program ([2, 128 x 4, 1], tests/test_fused_step.py
# ``_deep("ac", ...)``) from its first J load up to its dJ stores, as generated before systems were served
PARENT_BODIES = [
    """\
      v0 = JV(0, t + 0);
      v1 = pv;   // prefetched (pre)
    v2 = v0 - v1;
      v3 = ptr.lam[0][i];
    v4 = v3 * v3;
      { const float f = v2, w = v4;
        acc[0] += 0x1.0000000000000p-6f * w * f * f;
        a2 += 2.f * 0x1.0000000000000p-6f * w * f; a4 += 0x1.0000000000000p-6f * f * f; }
    { const float g = a4; const float x = v3, y = v3; a3 += g * y; a3 += g * x; }
      ptr.dlam[0][i] = a3;
    { const float g = a2; a0 += g; a1 -= g; }
      dj0_0 += a0;""",
    """\
      v0 = JV(0, t + 0);
      v1 = JV(1, t + 0);
      v2 = JV(0, t + 1);
      v3 = JV(1, t + 1);
    v4 = v0 - v2;
    v5 = 0x1.0000000000000p+0f;
    v6 = v1 - v3;
      { const float f = v4, w = v5;
        acc[1] += 0x1.8618620000000p-5f * w * f * f;
        a4 += 2.f * 0x1.8618620000000p-5f * w * f; a5 += 0x1.8618620000000p-5f * f * f; }
      { const float f = v6, w = v5;
        acc[1] += 0x1.8618620000000p-5f * w * f * f;
        a6 += 2.f * 0x1.8618620000000p-5f * w * f; a5 += 0x1.8618620000000p-5f * f * f; }
    { const float g = a6; a1 += g; a3 -= g; }
    { const float g = a4; a0 += g; a2 -= g; }
      dj1_1 += a3;
      dj1_0 += a2;
      dj0_1 += a1;
      dj0_0 += a0;""",
    """\
      v0 = JV(0, t + 0);
      v1 = JV(3, t + 0);
      v2 = JV(2, t + 0);
    v3 = 0x1.a36e2e0000000p-14f;
    v4 = v3 * v1;
    v5 = v2 - v4;
    { const float x = v0; float p = 1.f; p *= x; p *= x; p *= x; v6 = p; }
    v7 = 0x1.4000000000000p+2f;
    v8 = v7 * v6;
    v9 = v5 + v8;
    v10 = v7 * v0;
    v11 = v9 - v10;
      v12 = pv;   // prefetched (pre)
    v13 = v12 * v12;
      { const float f = v11, w = v13;
        acc[2] += 0x1.47ae140000000p-9f * w * f * f;
        a11 += 2.f * 0x1.47ae140000000p-9f * w * f; a13 += 0x1.47ae140000000p-9f * f * f; }
    { const float g = a13; const float x = v12, y = v12; a12 += g * y; a12 += g * x; }
      ptr.dlam[1][i] = a12;
    { const float g = a11; a9 += g; a10 -= g; }
    { const float g = a10; const float x = v7, y = v0; a7 += g * y; a0 += g * x; }
    { const float g = a9; a5 += g; a8 += g; }
    { const float g = a8; const float x = v7, y = v6; a7 += g * y; a6 += g * x; }
    { const float g = a6; const float x = v0; float p = 1.f; p *= x; p *= x; a0 += g * (float)3 * (3 > 0 ? p : 0.f); }
    { const float g = a5; a2 += g; a4 -= g; }
    { const float g = a4; const float x = v3, y = v1; a3 += g * y; a1 += g * x; }
      dj0_2 += a2;
      dj0_3 += a1;
      dj0_0 += a0;""",
]


# sha256 of ``fused_step.gen_loss`` and of ``loss_jit.generate`` for the NLS system on [2, 128 x 3, d_out],
# computed on the commit before the two emitters folded their one-output / several-output forks
PARENT_SYSTEM_SHA = {
    2: ("c71a97b6930fc9dced3585c54cceda44e6b9544af33237a9e16759e6a846a5d6",
        "8fb3246d8582ce00c4d1bb98b81fb7bc16f566967f86950698dd1ee4ac67e579"),
    3: ("801ac6f1abe48b6547ac3ed3dfb1e596084ca9c486c455c440ff38846e686ce7",
        "b2b2256fe49bae54966c21081837fed12b06517d4421145fa50b3b3e373ae7bf"),
    4: ("b6b09c20abec23370cc8a3fb57401381cb8ff0576121373ba3f16a480c1ab2e4",
        "e1b8338bcbdbb5ce0b84d6b7c6be3e49744459d82b5e949e4eabb3403f70b142"),
}


@pytest.mark.parametrize("d_out", [2, 3, 4])
def test_system_generated_text_unchanged(d_out):
    """The generated loss of the one-launch step and the specialised loss kernel of a system are
    byte for byte what the parent commit emitted (2 / 4 outputs: vector J accesses, 3: scalar)."""
    import hashlib
    from tensordiffeq_amd.ops import fused_step, jet_hip, loss_jit
    prog, op = _prog_op(nls_net("cpu", "jet", L3, d_out))
    layout, _, _ = fused_step.point_layout(prog, fused_step.fused_groups(prog, op))
    gen = fused_step.gen_loss(layout, op.n_terms, op.n_terms + op.n_scal, prog.plan.S,
                              spec=jet_hip.stream_spec(prog.plan), d_in=2, d_out=d_out)
    sha = lambda s: hashlib.sha256(s.encode()).hexdigest()  # noqa: E731
    assert (sha(gen), sha(loss_jit.generate(op))) == PARENT_SYSTEM_SHA[d_out]


def _group_bodies(gen):
    out, cur = [], None
    for ln in gen.splitlines():
        if cur is None and "JV(" in ln and "#define" not in ln:
            cur = []
        if cur is not None:
            if ln.lstrip().startswith("UB("):
                out.append("\n".join(cur))
                cur = None
            else:
                cur.append(ln)
    return out


def test_one_output_generated_loss_unchanged():
    from tensordiffeq_amd.ops import fused_step, jet_hip
    from tests.test_fused_step import _deep
    prog, op = _prog_op(_deep("ac", [2, 128, 128, 128, 128, 1]))
    layout, _, _ = fused_step.point_layout(prog, fused_step.fused_groups(prog, op))
    gen = fused_step.gen_loss(layout, op.n_terms, op.n_terms + op.n_scal, prog.plan.S,
                              spec=jet_hip.stream_spec(prog.plan), d_in=2)
    assert "#define JV(s_, k_) fz_jsum<S, PT, NW>(jv, (s_), (k_), bo)" in gen
    assert "#define UB(s_, k_) ubs[((s_) * PT + (k_)) * 4]" in gen
    assert "float pv, float bo)" in gen
    assert _group_bodies(gen) == PARENT_BODIES


# --------------------------------------------------------------------------- GPU -------------
gpu = pytest.mark.gpu
_RESULTS = {}


def _head_blocks(g, d_out, W=128):
    """``{name: slice of theta}``: column q of the output layer's kernel and its bias, one by one
    (theta ends with Ko [W][d_out] row-major, then bo [d_out])."""
    n = g.numel()
    ko = g[n - W * d_out - d_out:n - d_out].reshape(W, d_out)
    out = {}
    for q in range(d_out):
        out[f"Ko[:, {q}]"] = ko[:, q]
        out[f"bo[{q}]"] = g[n - d_out + q:n - d_out + q + 1]
    return out


def _evaluate(precision, hidden, d_out, n_f, fused, reads01=False, nan_fill=False, twice=False):
    """One evaluation (``LossGradEngine.evaluate_fg``) with the one-launch step on or off: ``[gradient |
    loss]``, every ``dlam``, the loss terms (float64 copies on the host), the solver."""
    from tensordiffeq_amd.fit import LossGradEngine
    from tensordiffeq_amd.ops import fused_step
    with _env(TDQ_FUSED_STEP="1" if fused else "0", TDQ_FUSED_STEP_SYSTEMS="1"):
        m = nls_net("cuda", "hip", hidden, d_out, n_f, precision, reads01=reads01)
        prog = m.program()
        assert prog.backend == "hip", prog.reasons
        fop = prog.fused_op
        assert fop is not None, prog.reasons
        fs = fused_step.for_program(prog)
        if fused:
            assert fs is not None, prog.fused_step_reason
            assert fs.cfg["d_out"] == d_out and fs.lo == (precision == "bf16x3")
        else:
            assert fs is None
        eng = LossGradEngine(m, prog, m.lambdas)
        if nan_fill:
            _, _, work = eng.points.buffers()
            work.fill_(float("nan"))
            for d in fop.dlam:
                d.fill_(float("nan"))
        fg = eng.evaluate_fg()
        torch.cuda.synchronize()
        res = {"fg": fg.double().cpu(), "dlam": [d.double().cpu().reshape(-1).clone() for d in fop.dlam],
               "losses": fop.losses.double().cpu().clone(), "m": m, "slots": list(fop.fl.lam_slots)}
        if twice:
            raw = [fg.clone()] + [d.clone() for d in fop.dlam]
            fg2 = eng.evaluate_fg()
            torch.cuda.synchronize()
            res["bitwise"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                 for a, b in zip(raw, [fg2] + list(fop.dlam)))
    return res


def _case(precision, hidden, d_out, n_f):
    """The fused and the separate-launch evaluation of a case and its float64 reference, computed
    once and shared by the tests."""
    key = (precision, tuple(hidden), d_out, n_f)
    if key not in _RESULTS:
        one = _evaluate(precision, hidden, d_out, n_f, True)
        sep = _evaluate(precision, hidden, d_out, n_f, False)
        m = one["m"]
        assert torch.equal(m.u_model.flat, sep["m"].u_model.flat)
        ref = nls_net("cuda", "autograd", hidden, d_out, n_f)
        tot, _, g64, glam64 = autograd_fp64(ref, m.u_model.flat, m.lambdas)
        _RESULTS[key] = (one, sep, (float(tot), g64.cpu(), [g.reshape(-1).cpu() for g in glam64]))
        for r in (one, sep):
            del r["m"]
    return _RESULTS[key]


CASES = [(p, L3, d, 300) for p in ("bf16", "bf16x3") for d in (2, 3, 4)] + \
        [(p, L4, 2, 40) for p in ("bf16", "bf16x3")] + [(p, L3, 2, 8400) for p in ("bf16", "bf16x3")]
_ids = [f"{p}-{len(h)}x128-d{d}-nf{n}" for (p, h, d, n) in CASES]


@gpu
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("hidden", [L3, L4], ids=["3x128", "4x128"])
def test_routing(precision, hidden, monkeypatch):
    from tensordiffeq_amd.ops import fused_step
    monkeypatch.delenv("TDQ_FUSED_STEP", raising=False)
    monkeypatch.setenv("TDQ_FUSED_STEP_SYSTEMS", "1")
    prog = nls_net("cuda", "hip", hidden, 2, 40, precision).program()
    assert fused_step.ineligible(prog, prog.fused_op) is None
    fs = fused_step.for_program(prog)
    assert fs is not None, prog.fused_step_reason
    assert fs.cfg["d_out"] == 2 and fs.pt == (16 if precision == "bf16x3" else 32)
    monkeypatch.setenv("TDQ_FUSED_STEP_SYSTEMS", "0")
    prog = nls_net("cuda", "hip", hidden, 2, 40, precision).program()
    assert fused_step.ineligible(prog, prog.fused_op) == "d_out != 1"
    assert fused_step.for_program(prog) is None and prog.fused_step_reason == "d_out != 1"


@gpu
def test_routing_outside_the_envelope(monkeypatch):
    """Five outputs have no fused loss (the one-launch step's first requirement); 4 outputs on 4
    hidden layers in bf16 are inside the geometry and answer with the LDS; a narrower network keeps
    ``"d_out != 1"``."""
    from tensordiffeq_amd.ops import fused_step
    monkeypatch.delenv("TDQ_FUSED_STEP", raising=False)
    monkeypatch.setenv("TDQ_FUSED_STEP_SYSTEMS", "1")

    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        return tdq.grad(h[:, 0:1], t) + h[:, 4:5]
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 8)
    D.add("t", [0.0, 1.0], 8)
    D.generate_collocation_points(50)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 128, 128, 128, 5], f_model, D, [tdq.boundaries.dirichletBC(D, val=0.0, var="x", target="lower")],
              backend="hip", device="cuda", precision="bf16")
    prog = m.program()
    assert prog.fused_op is None
    assert fused_step.ineligible(prog, prog.fused_op) == "needs the fused loss on a GPU"
    assert fused_step.for_program(prog) is None
    prog = nls_net("cuda", "hip", L4, 4, 40, "bf16").program()
    why = fused_step.ineligible(prog, prog.fused_op)
    assert why is not None and "LDS" in why, why
    prog = nls_net("cuda", "hip", L4, 4, 40, "bf16x3").program()
    assert fused_step.ineligible(prog, prog.fused_op) is None
    prog = nls_net("cuda", "hip", [64, 64, 64], 2, 40, "bf16").program()
    assert fused_step.ineligible(prog, prog.fused_op) == "d_out != 1"


def _norm_rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@gpu
@pytest.mark.parametrize("precision,hidden,d_out,n_f", CASES, ids=_ids)
def test_system_one_launch_vs_autograd_fp64(precision, hidden, d_out, n_f):
    """Loss, theta gradient and SA gradients of the one-launch evaluation against the float64
    ``backend="autograd"`` solver at the same weights: ``TOL_FWD`` / ``TOL_BWD`` / ``20 TOL_BWD`` of
    tests/test_hip_kernels.py on the whole vectors, as tests/test_systems_gpu.py.  The output layer's
    blocks one by one (a norm over all of theta hides a wrong head): column q of Ko and bo[q], error
    relative to that block's largest float64 value, bounded by the larger of ``TOL_BWD`` and 3x the
    same block's error on the separate launches (existing code at the same precision, measured
    here with ``TDQ_FUSED_STEP=0``; 3 is the project's usual margin over a measured error).

    Measured on MI355X (loss / theta gradient / SA gradients; worst head block: one launch / separate):
      bf16   3x128 d_out 2 n_f 300    2.1e-03 / 3.7e-03 / 1.1e-02   Ko[:, 1] 5.7e-03 / 5.7e-03
      bf16   3x128 d_out 3 n_f 300    5.7e-04 / 3.1e-03 / 7.9e-03   bo[1]    1.1e-02 / 5.6e-03
      bf16   3x128 d_out 4 n_f 300    3.1e-04 / 6.1e-03 / 9.5e-03   bo[1]    5.1e-02 / 5.0e-02
      bf16x3 3x128 d_out 2 n_f 300    4.1e-06 / 5.6e-06 / 3.1e-05   Ko[:, 1] 6.8e-06 / 6.7e-06
      bf16x3 3x128 d_out 3 n_f 300    5.3e-08 / 4.1e-06 / 1.7e-05   bo[1]    3.1e-05 / 3.1e-05
      bf16x3 3x128 d_out 4 n_f 300    1.5e-06 / 5.8e-06 / 2.0e-05   bo[1]    2.0e-05 / 2.1e-05
      bf16   4x128 d_out 2 n_f 40     1.2e-03 / 5.9e-03 / 5.1e-03   Ko[:, 0] 9.2e-03 / 7.7e-03
      bf16x3 4x128 d_out 2 n_f 40     6.9e-07 / 5.0e-06 / 1.2e-05   Ko[:, 0] 6.6e-06 / 6.6e-06
      bf16   3x128 d_out 2 n_f 8400   2.1e-03 / 3.8e-03 / 1.2e-02   Ko[:, 0] 6.3e-03 / 6.3e-03
      bf16x3 3x128 d_out 2 n_f 8400   4.0e-06 / 5.6e-06 / 2.9e-05   Ko[:, 1] 6.8e-06 / 6.7e-06
    (bounds: 8e-2 / 1.4e-2 / 0.28 in bf16, 2.5e-4 / 2.5e-5 / 5e-4 in bf16x3)."""
    from tests.test_hip_kernels import TOL_BWD, TOL_FWD
    one, sep, (tot, g64, glam64) = _case(precision, hidden, d_out, n_f)
    fg = one["fg"]
    assert torch.isfinite(fg).all()
    lerr = abs(float(fg[-1]) - tot) / abs(tot)
    gerr = _norm_rel(fg[:-1], g64)
    sa = max(_norm_rel(d, glam64[k]) for k, d in zip(one["slots"], one["dlam"]))
    tag = f"SYSTEMS_ONE_LAUNCH_FP64 {precision} {len(hidden)}x128 d_out={d_out} n_f={n_f}"
    print(f"{tag} loss {lerr:.3e} grad {gerr:.3e} SA {sa:.3e}")
    bad = []
    ref_b = _head_blocks(g64, d_out)
    sep_b = _head_blocks(sep["fg"][:-1], d_out)
    for name, blk in _head_blocks(fg[:-1], d_out).items():
        scale = ref_b[name].abs().max().clamp_min(1e-300)
        err = ((blk - ref_b[name]).abs().max() / scale).item()
        err_sep = ((sep_b[name] - ref_b[name]).abs().max() / scale).item()
        bound = max(TOL_BWD[precision], 3.0 * err_sep)
        print(f"{tag} {name} one launch {err:.3e} separate {err_sep:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((name, err, err_sep, bound))
    assert lerr < TOL_FWD[precision], lerr
    assert gerr < TOL_BWD[precision], gerr
    assert sa < 20 * TOL_BWD[precision], sa
    assert not bad, bad


@gpu
@pytest.mark.parametrize("precision,hidden,d_out,n_f", CASES, ids=_ids)
def test_system_one_launch_matches_separate_launches(precision, hidden, d_out, n_f):
    """Every loss term, the theta gradient and every ``dlam`` against the separate launches, with the
    tolerances of tests/test_fused_step.py ``test_fused_step_matches_separate_launches``."""
    one, sep, _ = _case(precision, hidden, d_out, n_f)
    rel = _norm_rel(one["fg"][:-1], sep["fg"][:-1])
    terms = [(a.item(), b.item()) for a, b in zip(one["losses"], sep["losses"])]
    print(f"SYSTEMS_ONE_LAUNCH_SEP {precision} {len(hidden)}x128 d_out={d_out} n_f={n_f} terms "
          f"{[(f'{a:.5e}', f'{b:.5e}') for a, b in terms]} grad rel {rel:.3e}")
    tl, tg = (2e-2, 3e-2) if precision == "bf16" else (5e-5, 1e-4)
    assert len(terms) >= 3
    for a, b in terms:
        assert abs(a - b) <= tl * abs(b) + 1e-6, terms
    assert rel < tg, rel
    assert len(one["dlam"]) == len(sep["dlam"]) == 2
    for a, b in zip(one["dlam"], sep["dlam"]):
        assert _norm_rel(a, b) < tg


@gpu
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("n_f", [300, 8400])
def test_everything_is_written(precision, n_f):
    """``dlam`` and the gradient-slab buffer pre-filled with NaN: everything read afterwards is
    finite.  With 3 outputs of which the loss reads 0 and 1, the gradients of ``Ko[:, 2]`` and
    ``bo[2]`` are exactly 0 - the dJ of the unread output is written as zeros in every tile."""
    r = _evaluate(precision, L3, 2, n_f, True, nan_fill=True)
    assert torch.isfinite(r["fg"]).all() and all(torch.isfinite(d).all() for d in r["dlam"])
    r = _evaluate(precision, L3, 3, n_f, True, reads01=True, nan_fill=True)
    assert torch.isfinite(r["fg"]).all() and all(torch.isfinite(d).all() for d in r["dlam"])
    b = _head_blocks(r["fg"][:-1], 3)
    assert float(b["Ko[:, 2]"].abs().max()) == 0.0 and float(b["bo[2]"].abs().max()) == 0.0
    assert float(b["Ko[:, 0]"].abs().max()) > 0.0 and float(b["Ko[:, 1]"].abs().max()) > 0.0
    assert float(b["bo[0]"].abs().max()) > 0.0 and float(b["bo[1]"].abs().max()) > 0.0


@gpu
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("n_f", [300, 8400])
def test_two_evaluations_bitwise_equal(precision, n_f):
    assert _evaluate(precision, L3, 2, n_f, True, twice=True)["bitwise"]


@gpu
def test_system_trains_on_the_one_launch_step(monkeypatch):
    """64 Adam steps in bf16 on [2, 128 x 3, 2] with 8,448 points on the one-launch step (1-step and
    K-step graphs), then 32 device L-BFGS iterations on the bf16x3 one-launch objective whose weight
    images the update kernel writes; at the last iterate the evaluation from those images equals
    bitwise the one after ``pack_images``.
    Measured on MI355X: Adam 7.2090e+02 -> 3.4566e+02, L-BFGS minimum 1.9396e-01 (32 iterations)."""
    from tensordiffeq_amd.optimizers import lbfgs_device as LD
    for k in ("TDQ_FUSED_STEP", "TDQ_FUSED_TAIL", "TDQ_LOSS_JIT", "TDQ_SPLIT", "TDQ_FUSED_LOSS", "TDQ_LBFGS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TDQ_FUSED_STEP_SYSTEMS", "1")
    m = nls_net("cuda", "hip", L3, 2, 8400, "bf16", newton_precision="bf16x3")
    m.fit(tf_iter=64)
    torch.cuda.synchronize()
    eng = m._get_engine(None, 64)
    assert eng.points.fused_step() is not None, m.program().fused_step_reason
    assert eng.graph_a is not None and eng.graph_k is not None
    losses = [h["Total Loss"] for h in m.losses]
    assert len(losses) == 64 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    leng = m._get_lbfgs_engine()
    assert leng.program.precision == "bf16x3"
    assert leng.image_target() is not None, getattr(leng.program, "fused_step_reason", None)
    assert leng.points.fused_step().cfg["d_out"] == 2
    m.fit(newton_iter=32)
    torch.cuda.synchronize()
    assert m.fit_info["lbfgs"]["impl"] == "device"
    end = float(m.min_loss["l-bfgs"])
    print(f"SYSTEMS_ONE_LAUNCH_TRAIN adam {losses[0]:.4e} -> {losses[-1]:.4e}, l-bfgs min {end:.4e} "
          f"({m.fit_info['lbfgs']['n_iter']} iterations)")
    assert math.isfinite(end) and end <= losses[-1], (end, losses[-1])
    # the update kernel's scatter of the two-output head against pack_images: a few more iterations
    # driven here, so the flat vector stays at the optimizer's last iterate
    tgt = leng.image_target()
    opt = LD.minimize(leng.evaluate_fg, m.u_model.flat, 8, images=tgt)
    torch.cuda.synchronize()
    assert opt.fused and opt.img_target is not None and not opt.images_stale, opt.reason
    from_images = tgt[1]().clone()
    packed = leng.evaluate_fg().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(packed).all()
    assert torch.equal(from_images.view(torch.int32), packed.view(torch.int32))
