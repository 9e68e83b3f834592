"""One-launch training step (ops/fused_step.py, csrc/jet_fused.h: the fused step).

CPU: the generated kernels (headers + the program's loss as ``GenLoss``; the bf16 step and the
bf16x3 objective) compile with hipRTC for gfx950 for several traced programs, and eligibility is
decided from the program's layout.
GPU: the fused step's loss, SA-weight gradients and parameter gradient match the separate-launch
step (saved-activation kernels + specialized loss kernel) at the bf16 level, and a short training
run follows the same trajectory.
"""
import ctypes

import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd import fusion
from tests.test_loss_jit import _model
from tests.test_solver import allen_cahn, burgers


def _deep(problem, layers):
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    if problem == "burgers":
        D, bcs, f = burgers(n_f=400)
        m.compile(layers, f, D, bcs, backend="jet", device="cpu")
    else:
        D, bcs, f, kw = allen_cahn(n_f=400)
        if problem == "ac_g":
            kw["g"] = lambda lam: lam ** 2 + 0.5 * torch.exp(-lam)
        m.compile(layers, f, D, bcs, backend="jet", device="cpu", **kw)
    return m


def _compile_ok(src):
    from tensordiffeq_amd.ops import _lib, fused_step
    lib = _lib.load()
    code, size = ctypes.c_void_p(0), ctypes.c_longlong(0)
    log = ctypes.create_string_buffer(16384)
    rc = lib.tdq_rtc_compile_ex(src.encode(), b"t.hip", b"gfx950", fused_step.RTC_OPTS.encode(), ctypes.byref(code),
                                ctypes.byref(size), log, len(log))
    assert rc == 0, log.value.decode()[:3000]
    assert size.value > 0
    lib.tdq_rtc_free(code)


def _prog_op(m):
    from tensordiffeq_amd.ops.loss_fused import FusedLossOp
    prog = m.program()
    fl = fusion.build(prog, m.lambdas)
    return prog, FusedLossOp(fl, prog, m.lambdas, fusion.scalar_values(fl, m.lambdas, None), fl.lam_offsets)


@pytest.mark.parametrize("problem,layers", [("ac", [2, 128, 128, 128, 128, 1]), ("ac_g", [2, 128, 128, 128, 1]),
                                            ("burgers", [2, 128, 128, 128, 128, 1]), ("ac", [2, 128, 128, 1])])
def test_fused_step_source_compiles(problem, layers):
    from tensordiffeq_amd.ops import _lib, fused_step
    if not _lib.available():
        pytest.skip("native library not built")
    prog, op = _prog_op(_deep(problem, layers))
    # the residual group is the last group, alone on the last segment
    last = len(prog.segments) - 1
    assert op.fl.groups[-1].segs == [last]
    layout, _, _ = fused_step.point_layout(prog, fused_step.fused_groups(prog, op))
    if len(layers) - 3 < 2:   # a 1-MFMA-layer net ([2, 128, 128, 1]): the fused step needs two
        with pytest.raises(ValueError):
            fused_step.recipe(prog, op, layout, "bf16")
        return
    rec = fused_step.recipe(prog, op, layout, "bf16")
    gen = rec.source[len(fused_step.header_source()):]
    assert "JV(" in gen and "UB(" in gen
    if problem == "ac":   # the periodic pair group reads its partner point
        assert "t + 1" in gen
    _compile_ok(rec.source)
    rec3 = fused_step.recipe(prog, op, layout, "bf16x3")
    assert 0 < rec3.lds <= 160 * 1024, rec3.lds
    _compile_ok(rec3.source)


@pytest.mark.parametrize("pack", ["A", "B", "C", "D"])
def test_fused_step_source_compiles_opcode_zoo(pack):
    """The packed opcode programs of tests/test_loss_ops_oracle.py (every opcode, COORD loads, the
    SCAL adjoint, a VAL-first prefetch, groups without a partner) as ``GenLoss``: the bf16 and the
    bf16x3 kernel compile for gfx950 on the network the GPU leg uses."""
    from tensordiffeq_amd.ops import _lib, fused_step
    from tests.test_loss_ops_oracle import LAYERS4, zoo_model
    if not _lib.available():
        pytest.skip("native library not built")
    prog, op = _prog_op(zoo_model(pack, "cpu", "jet", n_f=400, layers=LAYERS4))
    layout, _, _ = fused_step.point_layout(prog, fused_step.fused_groups(prog, op))
    for precision in ("bf16", "bf16x3"):
        rec = fused_step.recipe(prog, op, layout, precision)
        gen = rec.source[len(fused_step.header_source()):]
        if pack == "A":
            assert "xs[(t + 0) * TDQ_MAXD + 0]" in gen             # COORD from the tile
        if pack == "C":
            assert f"acc[{op.n_terms}] +=" in gen                  # SCAL adjoint
        if pack == "D":
            assert "t + 1" not in gen and "return ptr.val[" in gen  # no pair group, VAL prefetched
        _compile_ok(rec.source)


def test_point_layout():
    """Pair groups start on even offsets with their two segments' points alternating; ``idx`` is -1
    exactly at the padding points; ``N`` counts every slot and pad."""
    from types import SimpleNamespace as NS
    from tensordiffeq_amd.ops import fused_step

    def check(prog, groups):
        layout, idx, N = fused_step.point_layout(prog, groups)
        assert N == len(idx) and [la[0] for la in layout] == [g[1] for g in groups]
        covered = set()
        for (gr, _, _), (_, start, ns, n) in zip(groups, layout):
            assert ns == len(gr.segs) and n == gr.n
            offs = [prog.segments[sg].offset for sg in gr.segs]
            if ns == 2:
                assert start % 2 == 0
            for k in range(n):
                assert idx[start + ns * k:start + ns * (k + 1)] == [o + k for o in offs]
            covered.update(range(start, start + ns * n))
        pads = [i for i in range(N) if i not in covered]
        assert [i for i, v in enumerate(idx) if v == -1] == pads
        assert N == sum(ns * n for (_, _, ns, n) in layout) + len(pads)
        return layout, pads

    prog, op = _prog_op(_deep("ac", [2, 128, 128, 128, 128, 1]))
    layout, _ = check(prog, fused_step.fused_groups(prog, op))
    assert any(ns == 2 for (_, _, ns, _) in layout)
    prog, op = _prog_op(_deep("burgers", [2, 128, 128, 128, 128, 1]))
    layout, pads = check(prog, fused_step.fused_groups(prog, op))
    assert all(ns == 1 for (_, _, ns, _) in layout) and not pads
    # a pair group behind an odd number of points: one pad in front of it
    prog = NS(segments=[NS(offset=0), NS(offset=3), NS(offset=5), NS(offset=7)])
    _, pads = check(prog, [(NS(segs=[0], n=3), "a", None), (NS(segs=[1, 2], n=2), "b", None),
                           (NS(segs=[3], n=1), "c", None)])
    assert pads == [3]


@pytest.mark.parametrize("problem", ["ac", "burgers"])
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_prebuild_source_is_the_ops_source(problem, precision):
    """What ``prebuild`` compiles in the background (``program_recipe``) is, for a plain program,
    the source of every group laid out whole - the kernel ``FusedStepOp`` then asks for."""
    from tensordiffeq_amd.ops import _lib, fused_step
    if not _lib.available():
        pytest.skip("native library not built")
    prog, op = _prog_op(_deep(problem, [2, 128, 128, 128, 128, 1]))
    rec, groups, idx, N = fused_step.program_recipe(prog, op, precision)
    whole = [(gr, gr.program, None) for gr in op.fl.groups]
    assert groups == whole
    ref = fused_step.recipe(prog, op, fused_step.point_layout(prog, whole)[0], precision)
    assert rec.source == ref.source and rec.name == ref.name == fused_step.kernel_name(precision == "bf16x3")
    assert rec.lo == (precision == "bf16x3") and rec.pt == (16 if rec.lo else 32)


def test_mixed_mode_values(monkeypatch):
    from tensordiffeq_amd.ops import fused_step
    monkeypatch.delenv("TDQ_FUSED_STEP_MIXED", raising=False)
    assert fused_step.mixed_mode() == "split"
    for v in ("split", "0"):
        monkeypatch.setenv("TDQ_FUSED_STEP_MIXED", v)
        assert fused_step.mixed_mode() == v
    monkeypatch.setenv("TDQ_FUSED_STEP_MIXED", "1")
    with pytest.raises(ValueError, match="'split' and '0'"):
        fused_step.mixed_mode()


def test_fused_step_not_on_cpu():
    from tensordiffeq_amd.ops import fused_step
    m = _model("ac", "cpu", "jet")
    prog = m.program()
    assert fused_step.ineligible(prog, getattr(prog, "fused_op", None)) is not None


# --------------------------------------------------------------------------- GPU ---------
def _acsa(n_f, seed=0, problem="ac-sa", precision="bf16"):
    import bench
    torch.manual_seed(seed)
    return bench.PROBLEMS[problem]["build"](n_f, 1, "hip", torch.device("cuda", 0), False, precision,
                                            layers=(2, 128, 128, 128, 128, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("problem,n_f,mixed,precision", [("ac-sa", 50000, "split", "bf16"),
                                                         ("ac-sa", 3001, "split", "bf16"),
                                                         ("ac-baseline", 20000, "split", "bf16"),
                                                         ("ac-sa", 50000, "split", "bf16x3"),
                                                         ("ac-sa", 3001, "split", "bf16x3")])
def test_fused_step_matches_separate_launches(problem, n_f, mixed, precision, monkeypatch):
    """One evaluation: every loss term, the theta gradient and the SA-weight gradients of the fused
    step vs the separate launches (saved-activation kernels + specialized loss kernel).  AC-SA runs
    every group in the fused launch (IC with SA weights, the periodic pairs, the residual);
    AC-baseline (order-4 periodic streams): split layout - every main-plan output fused, the
    u_xxx / u_xxxx outputs on the jet_hi side chain."""
    monkeypatch.setenv("TDQ_FUSED_STEP_MIXED", mixed)
    from tensordiffeq_amd.fit import LossGradEngine
    from tensordiffeq_amd.ops import fused_step
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("TDQ_FUSED_STEP", flag)
        m = _acsa(n_f, problem=problem, precision=precision)
        prog = m.program()
        fop = prog.fused_op
        fs = fused_step.for_program(prog)
        if flag == "1":
            assert fs is not None, prog.fused_step_reason
            assert fs.mixed == (problem == "ac-baseline")
            if fs.mixed:
                assert fs.layout == "split"
            assert fs.lo == (precision == "bf16x3")
        else:
            assert fs is None
        eng = LossGradEngine(m, prog, m.lambdas)
        fg = eng.evaluate_fg()
        torch.cuda.synchronize()
        out[flag] = (fg.double().cpu(), [d.double().cpu().clone() for d in fop.dlam], fop.losses.double().cpu().clone())
    g1, g0 = out["1"][0][:-1], out["0"][0][:-1]
    rel = ((g1 - g0).norm() / g0.norm()).item()
    terms = [(a.item(), b.item()) for a, b in zip(out["1"][2], out["0"][2])]
    print(f"FUSED_STEP {problem} n_f={n_f} {precision} terms {[(f'{a:.5e}', f'{b:.5e}') for a, b in terms]} grad rel {rel:.3e}")
    # bf16: the two kernel designs round different operands (layer 0's tanh form, slab precision);
    # bf16x3: both at the split-bf16 level
    tl, tg = (2e-2, 3e-2) if precision == "bf16" else (5e-5, 1e-4)
    for a, b in terms:
        assert abs(a - b) <= tl * abs(b) + 1e-6, terms
    assert rel < tg, rel
    for a, b in zip(out["1"][1], out["0"][1]):
        assert ((a - b).norm() / b.norm().clamp_min(1e-30)).item() < tg


@pytest.mark.gpu
def test_fused_step_training_trajectory(monkeypatch):
    """AC-SA 20k: 200 Adam steps (graphs + fused tail) with and without the fused step end at the
    same loss within the bf16 level."""
    hist = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("TDQ_FUSED_STEP", flag)
        m = _acsa(20000)
        m.fit(tf_iter=200)
        assert (getattr(m.program(), "_fused_step", None) is not None) == (flag == "1")
        hist[flag] = [h["Total Loss"] for h in m.losses]
    a, b = hist["1"], hist["0"]
    print(f"FUSED_STEP_TRAJ first {a[0]:.5e} / {b[0]:.5e} last {a[-1]:.5e} / {b[-1]:.5e}")
    assert abs(a[0] - b[0]) <= 2e-2 * abs(b[0])
    assert abs(a[-1] - b[-1]) <= 0.1 * abs(b[-1])


@pytest.mark.gpu
def test_fused_step_deterministic(monkeypatch):
    monkeypatch.setenv("TDQ_FUSED_STEP", "1")
    m = _acsa(20000)
    from tensordiffeq_amd.fit import LossGradEngine
    eng = LossGradEngine(m, m.program(), m.lambdas)
    a = eng.evaluate_fg().clone()
    b = eng.evaluate_fg().clone()
    assert torch.equal(a, b)
