"""The fused step kernels' weight-fragment loads against the float64 torch-jet oracle: the bf16 step
fetches the first k-blocks of each GEMM's fragments before the barrier in front of it
(csrc/jet_fused.h fz_pre_w / fz_gemm); the bf16x3 objective (csrc/jet_fused3.h fz3_load_w) loads
them behind the barrier - the placements measured for it were not taken - and runs the same cases.

In the bf16 step the fragments are loaded at four kinds of site - after the layer-0 stores, at the end of a forward
layer, after the output-layer reverse, at the end of a backward step (after the h_0 rebuild where
there is one) - and the remaining k-blocks inside the GEMM, so the cases vary what those sites
depend on: the layer count (LM = 2: the h_0 rebuild sits behind an extra barrier in the step that
loads K_1's fragments; LM = 3: the flagship net) and partial last tiles (n_f = 40 / 517 with the
512 IC and 402 periodic points: 954 / 1431 points, no multiple of 16 or 32).  Both precisions.
Each case also checks that two consecutive launches are bitwise equal (the loads cross a barrier: a
scheduling-dependent hazard would show as run-to-run differences,
profiles/r6s_bf16_nondeterminism.md).

``[2,64,64,64,1]`` (WT = 4, KB = 2) is not a case: the fused step takes width 128 only
(``tdq_jet_fused_lds``, csrc/jet_fused.hip), ``fused_step.for_program`` is ``None`` for it in both
precisions (profiles/r8a_parent_errors.txt, ROUTE lines).

Bounds (gradient, loss, SA gradients; relative).  ``[2,128,128,128,128,1]``: ``BOUNDS`` of
tests/test_fused_kernels.py.  ``[2,128,128,128,1]``: 3x the errors measured on the commit before
this change (``NET3_PARENT``, from profiles/r8a_parent_errors.txt), case by case:
    n_f   precision  gradient    loss        SA gradients
    40    bf16       2.0296e-03  1.6201e-04  3.3049e-03
    40    bf16x3     2.6595e-06  7.3815e-07  1.4378e-05
    517   bf16       1.9833e-03  1.1904e-04  5.2428e-03
    517   bf16x3     2.7849e-06  2.4997e-07  1.3090e-05
(the kernels after the change are bit-identical to the parent's, profiles/r8e_bit_identity.txt, so
they measure the same.)
"""
import functools

import pytest
import torch

from tests.test_fused_kernels import BOUNDS

pytestmark = pytest.mark.gpu

NET3 = (2, 128, 128, 128, 1)
NET4 = (2, 128, 128, 128, 128, 1)
# (n_f, precision) -> errors of [2,128,128,128,1] measured on the parent commit
NET3_PARENT = {
    (40, "bf16"): (2.0296e-03, 1.6201e-04, 3.3049e-03),
    (40, "bf16x3"): (2.6595e-06, 7.3815e-07, 1.4378e-05),
    (517, "bf16"): (1.9833e-03, 1.1904e-04, 5.2428e-03),
    (517, "bf16x3"): (2.7849e-06, 2.4997e-07, 1.3090e-05),
}


def _bounds(layers, n_f, precision):
    if layers == NET4:
        return BOUNDS[precision]
    return tuple(3.0 * e for e in NET3_PARENT[(n_f, precision)])


@functools.lru_cache(maxsize=None)
def _reference(layers, n_f):
    """float64 torch-jet loss and gradients (theta, SA weights) of the AC-SA program - computed once
    per (net, n_f), shared by the two precisions (same seed: same weights, points and SA weights)."""
    import bench
    dev = torch.device("cuda", 0)
    ref = bench.build_problem(n_f, 1, "jet", dev, False, "bf16x3", layers=layers)
    flat = ref.u_model.flat.detach().clone()
    p64 = flat.double().requires_grad_(True)
    lams = [lam.detach().double().requires_grad_(True) for lam in ref.lambdas]
    tot, _ = ref.program().evaluate(p64, lams)
    g64 = torch.autograd.grad(tot, [p64] + lams, allow_unused=True)
    return flat, tot.detach(), [None if g is None else g.detach() for g in g64]


def _oracle(layers, n_f, precision):
    """As tests/test_fused_kernels.py ``_oracle``, with ``layers``: the fused op, its relative errors
    (theta gradient, loss, SA-weight gradients) against float64, and whether a second launch was
    bitwise equal to the first."""
    import bench
    from tensordiffeq_amd.fit import LossGradEngine
    from tensordiffeq_amd.ops import fused_step
    dev = torch.device("cuda", 0)
    m = bench.build_problem(n_f, 1, "hip", dev, False, precision, layers=layers)
    prog = m.program()
    fs = fused_step.for_program(prog)
    assert fs is not None, prog.fused_step_reason
    eng = LossGradEngine(m, prog, m.lambdas)
    fg1 = eng.evaluate_fg().clone()
    dlam = [d.double().clone() for d in prog.fused_op.dlam]
    fg2 = eng.evaluate_fg().clone()
    same = torch.equal(fg1, fg2) and all(torch.equal(a, d.double()) for a, d in zip(dlam, prog.fused_op.dlam))
    flat, tot, g64 = _reference(layers, n_f)
    assert torch.equal(flat, m.u_model.flat.detach()), "reference and kernel start from the same weights"
    fg = fg1.double()
    gerr = ((fg[:-1] - g64[0]).norm() / g64[0].norm()).item()
    lerr = abs(fg[-1].item() - tot.item()) / abs(tot.item())
    lam_err = 0.0
    for a, d in enumerate(dlam):
        gr = g64[1 + prog.fused_op.fl.lam_slots[a]]
        lam_err = max(lam_err, ((d.reshape(-1) - gr.reshape(-1)).norm() / gr.norm().clamp_min(1e-30)).item())
    return fs, gerr, lerr, lam_err, same


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("n_f", [40, 517])
@pytest.mark.parametrize("layers", [NET3, NET4], ids=["3x128", "4x128"])
def test_weight_prefetch_vs_fp64(layers, n_f, precision):
    fs, gerr, lerr, lam_err, same = _oracle(layers, n_f, precision)
    assert fs.lo == (precision == "bf16x3")
    assert fs.N % 16 != 0, fs.N   # a partial last tile in both kernels
    print(f"WEIGHT_PREFETCH_FP64 layers={list(layers)} n_f={n_f} {precision} N={fs.N} G={fs.G} grad {gerr:.3e} "
          f"loss {lerr:.3e} SA {lam_err:.3e} bitwise {same}")
    gb, lb, sb = _bounds(layers, n_f, precision)
    assert gerr < gb, gerr
    assert lerr < lb, lerr
    assert lam_err < sb, lam_err
    assert same, "two consecutive launches differ"
