"""Systems of PDEs on the GPU: the fused loss kernels for 2, 3 and 4 network outputs, one evaluation
end to end against float64, the training invariants and the one-launch step staying out.

The program is the NLS system of tests/test_systems.py at width 32 (two feature tiles, so bf16x3
is real) with n_f = 300 (the residual segment starts at point 48, off a multiple of 128).
"""
import pytest
import torch

from tests.test_loss_ops_oracle import _launch, _maxrel, _oracle_J
from tests.test_systems import autograd_fp64, nls_model

pytestmark = pytest.mark.gpu

W, N_F = 32, 300


# --------------------------------------------------------------------------- 8. loss kernels --
@pytest.mark.parametrize("d_out", [2, 3, 4])
def test_system_loss_kernels_vs_fp64(d_out):
    """The specialised kernel (8-byte accesses for 2 outputs, scalar for 3, 16-byte for 4) and the
    interpreter on an injected J against ``run_reference`` + autograd in float64 of the same
    bytecode, as tests/test_loss_ops_oracle.py ``test_loss_kernels_vs_fp64`` does for one output:
    per-term losses, total, the whole dJ (``dJ``, ``dlam`` and ``partials`` pre-filled with NaN, so
    every (stream, point, output) must be written - with 3 and 4 outputs the (0, 0) stream of the last
    output is never read), dJ per loss group, every dlam.  Metric: max |error| / max |fp64 value| per
    tensor; bound: the larger of 8x the same figure of ``run_reference`` in float32 and 2^-20.  JIT
    and interpreter give the same bits, and two range launches cut at n_blocks // 3 the single
    launch's.

    Measured on MI355X (kernel / fp32 reference per kind of tensor, the worst of its tensors; JIT and
    interpreter agree bit for bit, so one figure serves both):
      d_out 2  total 7.6e-08/7.6e-08 dJ 1.1e-07/1.1e-07 loss 5.6e-08/5.6e-08 dlam 2.4e-07/2.4e-07
      d_out 3  total 3.4e-08/1.4e-07 dJ 1.2e-07/1.2e-07 loss 6.5e-08/2.2e-08 dlam 1.6e-07/1.6e-07
      d_out 4  total 5.6e-09/5.6e-09 dJ 1.3e-07/1.3e-07 loss 1.1e-07/8.8e-09 dlam 1.0e-07/1.0e-07
    """
    m = nls_model("cuda", "hip", d_out=d_out, width=W, n_f=N_F)
    prog = m.program()
    assert prog.backend == "hip", prog.reasons
    op = prog.fused_op
    assert op is not None and op.engine == "jit", prog.reasons
    fl = op.fl
    assert fl.d_out == d_out and tuple(op.dJ.shape) == (fl.n_streams, prog.X_all.shape[0], d_out)
    assert any(meta[1] != 0 for meta in op.group_meta)          # a group with phase != 0
    torch.manual_seed(1)
    J = prog.jet(m.u_model.flat).detach().contiguous()
    assert tuple(J.shape) == tuple(op.dJ.shape)
    J = J + 0.01 * torch.randn_like(J)
    ref64 = _oracle_J(fl, prog, J, m.lambdas, torch.float64)
    ref32 = _oracle_J(fl, prog, J, m.lambdas, torch.float32)
    jit = op.jit
    results = {}
    bits_jit, results["jit"] = _launch(op, J)
    nb = op.n_blocks
    assert nb >= 3
    cut = [(0, nb // 3), (nb // 3, nb - nb // 3)]
    bits_rng, _ = _launch(op, J, cut)
    op.jit = None
    try:
        bits_int, results["interpreter"] = _launch(op, J)
        bits_int_rng, _ = _launch(op, J, cut)
    finally:
        op.jit = jit
    for a, b, c, d in zip(bits_jit, bits_rng, bits_int, bits_int_rng):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    bad = []
    for engine, got in results.items():
        assert set(got) == set(ref64)
        worst = {}
        for key, ref in ref64.items():
            assert torch.isfinite(got[key]).all(), (engine, key)
            err, ref_err = _maxrel(got[key], ref), _maxrel(ref32[key], ref)
            bound = max(8.0 * ref_err, 2.0 ** -20)
            kind = key.split()[0].rstrip("0123456789")      # dJ, total, loss, dlam
            worst[kind] = max(worst.get(kind, (0.0, 0.0)), (err, ref_err))
            if not err <= bound:
                bad.append((engine, key, err, ref_err, bound))
        print(f"SYSTEMS_LOSS_FP64 d_out={d_out} {engine} (kernel/fp32 reference) "
              + " ".join(f"{k} {e:.1e}/{r:.1e}" for k, (e, r) in worst.items()))
    assert not bad, bad


# --------------------------------------------------------------------------- 9. end to end ----
def system_errors(precision, d_out=2):
    """``(loss, theta gradient, SA gradients, fused)``: relative errors of one evaluation of the
    system on the HIP kernels (``LossGradEngine.evaluate_fg`` + the fused loss's ``dlam``; with
    ``TDQ_FUSED_LOSS=0`` the composed loss on the same HIP jet) against the ``backend="autograd"``
    solver in float64 holding the same weights."""
    from tensordiffeq_amd.fit import LossGradEngine
    m = nls_model("cuda", "hip", d_out=d_out, width=W, n_f=N_F, precision=precision)
    prog = m.program()
    assert prog.backend == "hip", prog.reasons
    ref = nls_model("cuda", "autograd", d_out=d_out, width=W, n_f=N_F)
    tot, _, g64, glam64 = autograd_fp64(ref, m.u_model.flat, m.lambdas)
    fop = prog.fused_op
    if fop is not None:
        fg = LossGradEngine(m, prog, m.lambdas).evaluate_fg().double()
        torch.cuda.synchronize()
        loss, g = fg[-1], fg[:-1]
        dlam = {fop.fl.lam_slots[a]: d.double().reshape(-1) for a, d in enumerate(fop.dlam)}
    else:
        p = m.u_model.flat.detach().requires_grad_(True)
        lams = [lam.detach().requires_grad_(True) for lam in m.lambdas]
        loss, _ = prog.evaluate(p, lams)
        gs = torch.autograd.grad(loss, [p] + lams)
        loss, g = loss.detach().double(), gs[0].double()
        dlam = {k: d.double().reshape(-1) for k, d in enumerate(gs[1:])}
    assert torch.isfinite(g).all() and set(dlam) == set(range(len(m.lambdas)))
    lerr = abs(float(loss) - float(tot)) / abs(float(tot))
    gerr = ((g - g64).norm() / g64.norm()).item()
    sa = max(((d - glam64[k].reshape(-1)).norm() / glam64[k].norm().clamp_min(1e-30)).item() for k, d in dlam.items())
    return lerr, gerr, sa, fop is not None


@pytest.mark.parametrize("precision,d_out", [("fp32", 2), ("bf16x3", 2), ("bf16", 2), ("bf16x3", 3), ("bf16x3", 4)])
def test_system_evaluation_vs_autograd_fp64(precision, d_out):
    """Loss, flat theta gradient and SA gradients of ``LossGradEngine`` (jet forward -> fused loss ->
    jet backward -> tail) against the float64 ``backend="autograd"`` solver with the same weights.
    Bounds: those tests/test_hip_kernels.py applies to its d_out = 2 jet cases - ``TOL_FWD`` on the
    relative loss error, ``TOL_BWD`` on the relative gradient-norm error, ``20 TOL_BWD`` on the SA
    gradients; the loss kernel adds fp32 rounding only.

    Measured on MI355X (loss / theta gradient / SA gradients), every case inside its bounds:
      fp32   d_out 2   5.0e-08 / 2.4e-07 / 4.0e-07     (bounds 8e-6 / 1.5e-6 / 3e-5)
      bf16x3 d_out 2   3.5e-06 / 2.9e-06 / 1.2e-05     (bounds 2.5e-4 / 2.5e-5 / 5e-4)
      bf16   d_out 2   6.7e-05 / 2.1e-03 / 7.5e-03     (bounds 8e-2 / 1.4e-2 / 0.28)
      bf16x3 d_out 3   7.0e-07 / 5.0e-06 / 1.9e-05
      bf16x3 d_out 4   3.1e-06 / 5.3e-06 / 1.8e-05
    (Should a precision ever exceed its bound: ``system_errors`` under ``TDQ_FUSED_LOSS=0`` measures
    the autograd-composed loss on the same HIP jet the same way, and a defect of the fused loss shows
    as a difference between the two above fp32 level.)
    """
    from tests.test_hip_kernels import TOL_BWD, TOL_FWD
    lerr, gerr, sa, fused = system_errors(precision, d_out)
    print(f"SYSTEMS_EVAL_FP64 {precision} d_out={d_out} fused={fused} loss {lerr:.3e} grad {gerr:.3e} SA {sa:.3e}")
    assert fused
    assert lerr < TOL_FWD[precision], lerr
    assert gerr < TOL_BWD[precision], gerr
    assert sa < 20 * TOL_BWD[precision], sa


# --------------------------------------------------------------------------- 10. training -----
N_F_TRAIN = 8400        # with the 48 boundary points above the 8192 that point ranges need


def _train(steps=64):
    m = nls_model("cuda", "hip", width=W, n_f=N_F_TRAIN, precision="bf16x3")
    m.fit(tf_iter=steps)
    torch.cuda.synchronize()
    return m


def _state(m):
    return [m.u_model.flat.detach().cpu().clone()] + [lam.detach().cpu().clone() for lam in m.lambdas]


def test_system_training_invariants(monkeypatch):
    """64 Adam steps of the system on [2, 32, 32, 2] in bf16x3: the HIP backend with the fused loss
    and captured graphs, a falling loss, and the trajectory (weights and every SA weight) bitwise
    that of the unfused tail, of the loss interpreter and of a single point range; then 32 device
    L-BFGS iterations.  Measured on MI355X: Adam 1.90e+03 -> 4.61e+01, L-BFGS minimum 2.25e-02."""
    for k in ("TDQ_FUSED_TAIL", "TDQ_LOSS_JIT", "TDQ_SPLIT", "TDQ_FUSED_LOSS"):
        monkeypatch.delenv(k, raising=False)
    m = _train()
    prog = m.program()
    assert m.active_backend == "hip" and prog.fused_op is not None and prog.fused_op.engine == "jit", prog.reasons
    eng = m._get_engine(None, 64)
    assert eng.graph_a is not None and eng.graph_k is not None          # 1-step and K-step graphs
    assert eng.points.ranges() is not None and len(eng.points.ranges()) == 2
    losses = [h["Total Loss"] for h in m.losses]
    assert len(losses) == 64 and all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    base = _state(m)
    for var, check in (("TDQ_FUSED_TAIL", lambda e, p: e.graph_k is None),
                       ("TDQ_LOSS_JIT", lambda e, p: p.fused_op.engine == "interpreter"),
                       ("TDQ_SPLIT", lambda e, p: e.points.ranges() is None)):
        monkeypatch.setenv(var, "0")
        other = _train()
        assert other.program().fused_op is not None
        assert check(other._get_engine(None, 64), other.program()), var
        for a, b in zip(base, _state(other)):
            assert torch.equal(a, b), (var, (a - b).abs().max().item())
        monkeypatch.delenv(var)
    m.fit(newton_iter=32)
    torch.cuda.synchronize()
    assert m.fit_info["lbfgs"]["impl"] == "device"
    end = float(m.min_loss["l-bfgs"])
    print(f"SYSTEMS_TRAIN adam {losses[0]:.4e} -> {losses[-1]:.4e}, l-bfgs min {end:.4e} "
          f"({m.fit_info['lbfgs']['n_iter']} iterations)")
    assert torch.isfinite(torch.tensor(end)) and end <= losses[-1], (end, losses[-1])
    assert torch.isfinite(m.u_model.flat).all()


# --------------------------------------------------------------------------- 11. one launch ---
def test_one_launch_step_stays_out():
    import bench
    from tensordiffeq_amd.ops import fused_step
    m = nls_model("cuda", "hip", width=W, n_f=N_F, precision="bf16")
    prog = m.program()
    assert prog.fused_op is not None
    assert fused_step.ineligible(prog, prog.fused_op) == "d_out != 1"
    assert fused_step.for_program(prog) is None
    ac = bench.build_problem(2048, 1, "hip", torch.device("cuda", 0), False, "bf16")
    prog = ac.program()
    assert fused_step.ineligible(prog, prog.fused_op) is None
    assert fused_step.for_program(prog) is not None
    ac.fit(tf_iter=2)
    assert ac._get_engine(None, 2).points.fused_step() is not None
