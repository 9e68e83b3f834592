"""Every opcode of the traced loss program on every executor, against float64.

The per-point loss program (``fusion.py``: 14 arithmetic and 6 input opcodes, each with a forward
and a reverse rule) is executed by ``fusion.run_reference`` (torch), the bytecode interpreter
(``csrc/loss_fused.hip``), the hipRTC-specialised kernel (``ops/loss_jit.py``) and ``GenLoss::eval``
inside the one-launch fused step (``ops/fused_step.gen_loss``; bf16 and bf16x3 kernels).  The zoo
below runs every opcode - TANH, LOG, COS, NEG, SQUARE, POWI at 0 / 1 / 5 / 16, POWF with negative
and integer-valued exponents, DIV by a stream-dependent denominator, COORD, SCAL with its block-
reduced gradient, VAL as the first per-point input - through each of them:

  CPU   ``run_reference`` in float64 vs ``LossProgram.evaluate`` (the user's callables on the torch
        jet): terms, total, theta and lambda gradients at 1e-7 (the only difference is the fp32
        rounding of value arrays, 2^-24); the zoo covers ``fusion.OP`` exactly.
  GPU   interpreter and JIT on an injected ``J`` vs ``run_reference`` + autograd in float64 of the
        same bytecode (``test_loss_kernels_vs_fp64``), and ``GenLoss`` end to end in the fused step
        vs the program on the float64 torch jet (``test_fused_step_zoo_vs_fp64``).

Two defects this turned up are fixed in ``fusion.py`` and tested here: a per-point SA-weight array
read by two loss groups (every GPU executor assigns ``dlam``, so one group's adjoint was lost) and
keyword arguments of traced torch calls (``alpha``, ``rounding_mode``) that were dropped.  A third
showed in tests/test_loss_jit.py once it ran LOG: the interpreter's ``logf`` differed from the
specialised kernel's in the last bit (csrc/build.py ``FILE_FLAGS``).
"""
import math

import numpy as np
import pytest
import torch

import tensordiffeq_amd as tdq
from tensordiffeq_amd import fusion
from tests.test_solver import allen_cahn, burgers


# --------------------------------------------------------------------------- the zoo ---------
def _terms_tanh(u, u_x, u_t, base, x, t):
    return torch.tanh(2.0 * u) - u.tanh() * u_x


def _terms_log(u, u_x, u_t, base, x, t):
    return torch.log(1.5 + u * u) * u_x


def _terms_cos(u, u_x, u_t, base, x, t):
    return torch.cos(3.0 * x) * u - torch.cos(u_x)


def _terms_powi(u, u_x, u_t, base, x, t):
    return u ** 0 + u ** 1 + u_x ** 3 + u ** 5 + u ** 16


def _terms_powf(u, u_x, u_t, base, x, t):
    return (1 + u * u) ** -1.5 + (2 + u_x ** 2) ** 0.5 + u ** 17.0 + (1.5 + u) ** -2


def _terms_div(u, u_x, u_t, base, x, t):
    return u_x / (2 + u * u) + 1 / (1.5 + torch.sin(u)) - (3 - u) / (2 - x * t)


def _res_neg_square(u, u_x, u_t, base, x, t):
    return -(base) + torch.square(u_x) - (-u) * u


def _res_rops(u, u_x, u_t, base, x, t):
    return 2.0 - base + 3.0 * u - (0.5 - u_x) + 2.0 ** u + torch.sqrt(4 + u_t * u_t) + torch.exp(-u * u)


def _res_torchfn(u, u_x, u_t, base, x, t):
    r = torch.add(base, torch.mul(u, u_x))
    r = torch.sub(r, torch.div(u_x, torch.add(torch.pow(u, 2), 2.0)))
    r = torch.add(r, torch.neg(torch.pow(u, 3)))
    r = torch.add(r, u_t, alpha=0.5)
    return torch.sub(r, torch.rsub(u, 1.0), alpha=0.25)


def _added(terms):
    return lambda u, u_x, u_t, base, x, t: base + terms(u, u_x, u_t, base, x, t)


def _sum_of(*fns):
    def expr(*a):
        r = fns[0](*a)
        for f in fns[1:]:
            r = r + f(*a)
        return r
    return expr


FAMILIES = {"tanh": _added(_terms_tanh), "log": _added(_terms_log), "cos": _added(_terms_cos),
            "neg_square": _res_neg_square, "powi": _added(_terms_powi), "powf": _added(_terms_powf),
            "div": _added(_terms_div), "rops": _res_rops, "torchfn": _res_torchfn}
# the fused step costs one hipRTC build per program and precision: the families packed into four
PACKS = {"A": _sum_of(FAMILIES["tanh"], FAMILIES["log"], FAMILIES["cos"], FAMILIES["neg_square"]),
         "B": _sum_of(FAMILIES["powi"], FAMILIES["powf"], FAMILIES["div"]),
         "C": FAMILIES["rops"]}
ZOO_NEW = list(FAMILIES) + ["g", "scal"]          # programs the other test modules do not have
ZOO = ZOO_NEW + ["burgers", "neumann"]
PACK_NAMES = ["A", "B", "C", "D"]
G_FUN = lambda lam: lam ** 2 + 0.5 * torch.exp(-lam)   # noqa: E731


def _residual(expr):
    def f_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        u_x = tdq.grad(u, x)
        u_t = tdq.grad(u, t)
        base = u_t - 0.01 * tdq.grad(u_x, x)
        return expr(u, u_x, u_t, base, x, t)
    return f_model


def zoo_model(name, device, backend, width=8, n_f=400, layers=None, precision=None):
    """A compiled solver of zoo program ``name`` on the small Allen-Cahn set-up (SA weights on the
    residual and the IC, a periodic pair on (u, u_x)); ``burgers`` / ``D``: single-segment groups
    only, Dirichlet constants and an IC value array (VAL is the first per-point input);
    ``neumann``: the Neumann / sin program of tests/test_loss_jit.py."""
    if name == "neumann":
        from tests.test_loss_jit import _neumann_sin
        return _neumann_sin(device, backend, width)
    layers = list(layers) if layers is not None else [2, width, width, 1]
    kw = {} if precision is None else {"precision": precision}
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    if name in ("burgers", "D"):
        D, bcs, f = burgers(n_f=n_f)
        m.compile(layers, f, D, bcs, backend=backend, device=device, **kw)
        return m
    D, bcs, f, sa = allen_cahn(n_f=n_f)
    if name in FAMILIES or name in PACKS:
        f = _residual(FAMILIES[name] if name in FAMILIES else PACKS[name])
    if name in ("g", "C"):
        sa["g"] = G_FUN
    if name in ("scal", "C"):   # one scalar SA weight on the IC: a SCAL input with a dscal gradient
        sa["init_weights"]["BCs"][0] = torch.tensor(1.3)
    m.compile(layers, f, D, bcs, backend=backend, device=device, **kw, **sa)
    return m


def _rel(a, b):
    a, b = float(torch.as_tensor(a).detach()), float(torch.as_tensor(b).detach())
    return abs(a - b) / max(abs(b), 1e-300)


def _maxrel(x, ref):
    """max |x - ref| / max |ref|"""
    ref = ref.double().reshape(-1)
    return ((x.double().reshape(-1) - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _fp64_args(m):
    p = m.u_model.flat.detach().double().requires_grad_(True)
    lams = [lam.detach().double().requires_grad_(True) for lam in m.lambdas]
    return p, lams


def _traced_vs_evaluate(m, fl):
    """Largest relative difference (terms, total, theta and lambda gradients) between the traced
    program on the float64 jet and ``prog.evaluate`` in float64."""
    prog = m.program()
    p, lams = _fp64_args(m)
    tot_e, vals = prog.evaluate(p, lams)
    g_e = torch.autograd.grad(tot_e, [p] + lams, allow_unused=True)
    got = fusion.run_reference(fl, prog, prog.jet(p), lams, fusion.scalar_values(fl, lams, None))
    tot_r = sum(got[1:], got[0])
    g_r = torch.autograd.grad(tot_r, [p] + lams, allow_unused=True)
    errs = {name: _rel(l, vals[name]) for name, l in zip(fl.term_names, got)}
    errs["total"] = _rel(tot_r, tot_e)
    for k, (a, b) in enumerate(zip(g_r, g_e)):
        assert (a is None) == (b is None)
        if b is not None:
            errs["theta" if k == 0 else f"lambda{k - 1}"] = _maxrel(a, b)
    return errs


# --------------------------------------------------------------------------- CPU legs --------
def test_zoo_covers_every_opcode():
    """A new opcode without a zoo case fails here."""
    seen = set()
    for name in ZOO:
        m = zoo_model(name, "cpu", "jet")
        fl = fusion.build(m.program(), m.lambdas)
        assert fl is not None, (name, m.program().reasons)
        for gr in fl.groups:
            assert gr.program.n_regs <= fusion.MAX_REGS
            seen |= {c[0] for c in gr.program.code}
    assert seen == set(fusion.OP.values()), sorted(set(fusion.OP.values()) ^ seen)


def test_zoo_exponents_and_inputs():
    """The edge cases the zoo is there for are really in the bytecode."""
    def ops(name):
        m = zoo_model(name, "cpu", "jet")
        fl = fusion.build(m.program(), m.lambdas)
        return fl, [(c, gr.program) for gr in fl.groups for c in gr.program.code]
    _, code = ops("powi")
    assert {c[3] for c, _ in code if c[0] == fusion.OP["POWI"]} >= {0, 1, 3, 5, 16}
    _, code = ops("powf")
    assert {P.consts[c[3]] for c, P in code if c[0] == fusion.OP["POWF"]} == {-1.5, 0.5, 17.0, -2.0}
    fl, code = ops("scal")
    assert fl.scal_slots == [("lam", 1)] and any(c[0] == fusion.OP["SCAL"] for c, _ in code)
    fl, _ = ops("burgers")
    assert all(len(gr.segs) == 1 for gr in fl.groups) and fl.val_arrays and not fl.lam_slots


@pytest.mark.parametrize("name", ZOO + PACK_NAMES)
def test_reference_matches_evaluate_fp64(name):
    m = zoo_model(name, "cpu", "jet")
    fl = fusion.build(m.program(), m.lambdas)
    assert fl is not None, m.program().reasons
    errs = _traced_vs_evaluate(m, fl)
    print(f"LOSS_OPS_CPU {name} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-7, errs


# --------------------------------------------------------------------------- fixes -----------
def _two_pair_periodic(device, backend, width=8, precision=None):
    """``periodicBC(D, ["x", "y"])`` with one per-point SA weight array: two pair groups read it."""
    from tensordiffeq_amd.boundaries import DomainND, periodicBC
    tdq.set_seed(0)
    D = DomainND(["x", "y"])
    D.add("x", [0.0, 1.0], 16)
    D.add("y", [0.0, 1.0], 16)
    D.generate_collocation_points(200)

    def deriv_model(u_model, x, y):
        u = u_model(torch.cat([x, y], 1))
        return u, tdq.grad(u, x)

    def f_model(u_model, x, y):
        u = u_model(torch.cat([x, y], 1))
        return tdq.grad(tdq.grad(u, x), x) + tdq.grad(tdq.grad(u, y), y) - torch.sin(math.pi * x) * u

    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    kw = {} if precision is None else {"precision": precision}
    m.compile([2, width, width, 1], f_model, D, [periodicBC(D, ["x", "y"], [deriv_model])], backend=backend,
              device=device, Adaptive_type="self-adaptive", dict_adaptive={"residual": [False], "BCs": [True]},
              init_weights={"residual": [None], "BCs": [torch.rand(16, 1, generator=g)]}, **kw)
    return m


def _two_face_neumann(device, backend, width=8):
    """``FunctionNeumannBC(var=["x", "y"])``: one value array and one per-point SA weight array
    over two faces (the API allows it: the term's ``lam`` spans every face of the BC)."""
    from tensordiffeq_amd.boundaries import DomainND, FunctionNeumannBC, dirichletBC
    tdq.set_seed(0)
    D = DomainND(["x", "y"])
    D.add("x", [0.0, 1.0], 11)
    D.add("y", [0.0, 1.0], 11)
    D.generate_collocation_points(100)

    def dx(u_model, x, y):
        return tdq.grad(u_model(torch.cat([x, y], 1)), x)

    def f_model(u_model, x, y):
        u = u_model(torch.cat([x, y], 1))
        return tdq.grad(tdq.grad(u, x), x) + tdq.grad(tdq.grad(u, y), y) + u

    bcs = [dirichletBC(D, val=0.0, var="x", target="lower"),
           FunctionNeumannBC(D, fun=[lambda y: np.cos(y), lambda x: np.sin(x)], var=["x", "y"], target="upper",
                             deriv_model=[dx], func_inputs=["y", "x"])]
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, width, width, 1], f_model, D, bcs, backend=backend, device=device,
              Adaptive_type="self-adaptive", dict_adaptive={"residual": [False], "BCs": [False, True]},
              init_weights={"residual": [None], "BCs": [None, torch.rand(11, 1, generator=g)]})
    return m


@pytest.mark.parametrize("build", [_two_pair_periodic, _two_face_neumann])
def test_weight_shared_by_two_groups(build):
    """A per-point weight array loaded by two loss groups: the program does not fuse and says why.
    (Should the executors ever accumulate across groups instead, the traced program must sum every
    group's part - and as long as they assign ``dlam``, a fused program has one reader per slot.)"""
    m = build("cpu", "jet")
    prog = m.program()
    assert len(m.lambdas) == 1 and m.lambdas[0].numel() > 1
    fl = fusion.build(prog, m.lambdas)
    if fl is None:
        assert any("loss fusion disabled" in r and "lambda 0" in r for r in prog.reasons), prog.reasons
        return
    errs = _traced_vs_evaluate(m, fl)
    assert max(errs.values()) <= 1e-7, errs
    # the GPU executors assign dlam: fused, every weight slot must have exactly one reader
    readers = [a for gr in fl.groups for a in fusion._lam_ids(gr.program)]
    assert len(readers) == len(set(readers)), readers


KWARG_CASES = {
    "add_alpha": lambda a, u, v: torch.add(a, u, alpha=3.0),
    "sub_alpha": lambda a, u, v: a + torch.sub(u, v, alpha=0.5),
    "div_floor": lambda a, u, v: a + u * torch.div(1.0 + v * v, 0.3 + u * u, rounding_mode="floor"),
    "div_trunc": lambda a, u, v: a + u * torch.div(v, 0.3 + u * u, rounding_mode="trunc"),
    "div_none": lambda a, u, v: a + torch.div(v, 0.3 + u * u, rounding_mode=None),
}


@pytest.mark.parametrize("case", list(KWARG_CASES))
def test_traced_torch_keyword_arguments(case):
    """``torch.add(a, u, alpha=3)`` & co.: the program does not fuse (reason recorded) or its traced
    loss is the callable's."""
    D, bcs, _, sa = allen_cahn(n_f=400)
    expr = KWARG_CASES[case]
    f = _residual(lambda u, u_x, u_t, base, x, t: expr(base, u, u_x))
    torch.manual_seed(0)
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 8, 8, 1], f, D, bcs, backend="jet", device="cpu", **sa)
    prog = m.program()
    assert prog.backend == "jet", prog.reasons
    fl = fusion.build(prog, m.lambdas)
    if fl is None:
        assert any("keyword argument" in r for r in prog.reasons), prog.reasons
        assert case.startswith("div_") and case != "div_none"   # alpha and rounding_mode=None are expressible
        return
    errs = _traced_vs_evaluate(m, fl)
    assert max(errs.values()) <= 1e-7, errs


# --------------------------------------------------------------------------- GPU: loss kernels
def _oracle_J(fl, prog, J, lambdas, dtype):
    """Per-term losses, total and the gradients wrt J, every per-point lambda and every scalar of
    the bytecode, by ``run_reference`` + autograd in ``dtype``."""
    Jd = J.detach().to(dtype).requires_grad_(True)
    lams = [lam.detach().to(dtype).requires_grad_(True) for lam in lambdas]
    losses = fusion.run_reference(fl, prog, Jd, lams, fusion.scalar_values(fl, lams, None))
    total = sum(losses[1:], losses[0])
    g = torch.autograd.grad(total, [Jd] + lams, allow_unused=True)
    g = [torch.zeros_like(w) if x is None else x for x, w in zip(g, [Jd] + lams)]
    out = {"total": total.detach().reshape(1), "dJ": g[0]}
    _dJ_by_group(out, fl, prog, g[0])
    for name, l in zip(fl.term_names, losses):
        out["loss " + name] = l.detach().reshape(1)
    for a, k in enumerate(fl.lam_slots):
        out[f"dlam{a}"] = g[1 + k].reshape(-1)
    for a, (kind, k) in enumerate(fl.scal_slots):
        assert kind == "lam"
        out[f"dscal{a}"] = g[1 + k].reshape(1)
    return {k: v.double() for k, v in out.items()}


def _dJ_by_group(out, fl, prog, dJ):
    """``dJ`` of every loss group's points on its own: the whole-tensor metric is normalised by the
    largest adjoint of the program (the IC's, with SA weights ~100), which would hide an error in
    another group."""
    for gi, gr in enumerate(fl.groups):
        idx = torch.cat([torch.arange(prog.segments[s].offset, prog.segments[s].offset + gr.n) for s in gr.segs])
        out[f"dJ group{gi}"] = dJ[:, idx.to(dJ.device)]


def _launch(op, J, ranges=None):
    op.dJ.fill_(float("nan"))     # every entry must be written, the zeros included
    for d in op.dlam:
        d.fill_(float("nan"))
    op.partials.fill_(float("nan"))
    if ranges is None:
        total, losses, dJ, dlam, dscal = op(J, with_total=True, reduce=True)
    else:
        for b0, nb in ranges:
            op.run_range(J, b0, nb)
    torch.cuda.synchronize()
    bits = [op.dJ.clone(), op.partials.clone()] + [d.clone() for d in op.dlam]
    if ranges is not None:
        return bits, None
    out = {"total": total.reshape(1), "dJ": dJ}
    _dJ_by_group(out, op.fl, op.prog, dJ)
    for name, l in zip(op.fl.term_names, losses):
        out["loss " + name] = l.reshape(1)
    for a, d in enumerate(dlam):
        out[f"dlam{a}"] = d.reshape(-1)
    for a in range(op.n_scal):
        out[f"dscal{a}"] = dscal[a].reshape(1)
    return bits, {k: v.double().clone() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ZOO)
def test_loss_kernels_vs_fp64(name):
    """The specialised kernel and the interpreter on an injected J (width 32, n_f = 300: the
    residual segment starts off a multiple of 128, so ``LFGroup.phase != 0``, groups end inside a
    block and inactive threads take part in the block sums) against ``run_reference`` + autograd in
    float64 of the same bytecode: per-term losses, total, the whole dJ (pre-filled with NaN), every
    dlam, dscal - and dJ once more per loss group.  Metric: max |error| / max |fp64 value| per
    tensor; bound: the larger of 8x the same figure of ``run_reference`` in float32 (torch, same
    inputs) and 2^-20.  Two range launches cut at n_blocks // 3 give the single launch's bits.

    Measured on MI355X (worst tensor per program: kernel figure / fp32-reference figure; JIT and
    interpreter agree bit for bit, so one figure serves both):
    (kernel / fp32 reference per kind of tensor, the worst of its tensors; ``dJ`` includes the
    per-group figures)
      tanh       total 7.5e-08/7.5e-08 dJ 1.4e-07/1.4e-07 loss 3.6e-08/6.8e-08 dlam 1.7e-07/1.7e-07
      log        total 4.6e-08/4.6e-08 dJ 1.1e-07/1.2e-07 loss 7.1e-08/5.3e-08 dlam 1.8e-07/1.8e-07
      cos        total 6.7e-08/6.7e-08 dJ 8.6e-08/1.4e-07 loss 3.6e-08/3.6e-08 dlam 1.5e-07/1.5e-07
      neg_square total 6.2e-08/6.2e-08 dJ 1.4e-07/1.4e-07 loss 5.2e-08/5.2e-08 dlam 2.0e-07/2.0e-07
      powi       total 7.4e-08/7.4e-08 dJ 1.2e-07/1.6e-07 loss 2.8e-08/2.8e-08 dlam 1.9e-07/1.9e-07
      powf       total 8.1e-08/8.1e-08 dJ 2.0e-07/2.0e-07 loss 2.8e-08/2.8e-08 dlam 2.3e-07/2.3e-07
      div        total 3.1e-08/3.1e-08 dJ 2.6e-07/1.9e-07 loss 2.8e-08/2.8e-08 dlam 2.4e-07/2.4e-07
      rops       total 5.3e-08/5.3e-08 dJ 1.2e-07/1.3e-07 loss 6.1e-08/2.2e-08 dlam 2.0e-07/2.0e-07
      torchfn    total 5.6e-08/5.6e-08 dJ 1.8e-07/2.2e-07 loss 2.8e-08/2.8e-08 dlam 3.6e-07/3.6e-07
      g          total 2.1e-08/2.1e-08 dJ 1.7e-07/1.9e-07 loss 2.8e-08/2.8e-08 dlam 1.7e-07/1.6e-07
      scal       total 2.6e-08/2.6e-08 dJ 1.2e-07/1.2e-07 loss 5.9e-08/5.9e-08 dlam 1.5e-07/1.5e-07
                 dscal 9.8e-09/9.8e-09
      burgers    total 4.4e-08/4.4e-08 dJ 1.0e-07/1.0e-07 loss 4.5e-08/4.5e-08
      neumann    total 1.0e-07/1.0e-07 dJ 1.6e-07/1.7e-07 loss 1.5e-07/7.4e-08
    Sensitivity (rules broken in a scratch copy): the COS adjoint's sign flipped in
    ``loss_jit._reverse_code`` fails ``cos`` on the JIT (dJ 7.4e-6 of the whole tensor, bound 9.5e-7);
    ``p`` for ``k p`` in the interpreter's POWI adjoint fails powi, powf, torchfn, g, scal and neumann
    on the interpreter (dJ 1.9e-6 ... 0.32, dlam 0.56) and the bitwise JIT comparison of
    tests/test_loss_jit.py for nine programs.
    """
    m = zoo_model(name, "cuda", "hip", width=32, n_f=300)
    prog = m.program()
    op = prog.fused_op
    assert op is not None and op.engine == "jit", prog.reasons
    fl = op.fl
    assert any(meta[1] != 0 for meta in op.group_meta)          # a group with phase != 0
    torch.manual_seed(1)
    J = prog.jet(m.u_model.flat).detach().contiguous()
    J = J + 0.01 * torch.randn_like(J)
    ref64 = _oracle_J(fl, prog, J, m.lambdas, torch.float64)
    ref32 = _oracle_J(fl, prog, J, m.lambdas, torch.float32)
    jit = op.jit
    results = {}
    bits_jit, results["jit"] = _launch(op, J)
    nb = op.n_blocks
    assert nb >= 3
    bits_rng, _ = _launch(op, J, [(0, nb // 3), (nb // 3, nb - nb // 3)])
    op.jit = None
    try:
        bits_int, results["interpreter"] = _launch(op, J)
        bits_int_rng, _ = _launch(op, J, [(0, nb // 3), (nb // 3, nb - nb // 3)])
    finally:
        op.jit = jit
    for x, y in zip(bits_jit, bits_rng):
        assert torch.equal(x, y)
    for x, y in zip(bits_int, bits_int_rng):
        assert torch.equal(x, y)
    bad = []
    for engine, got in results.items():
        assert set(got) == set(ref64)
        worst = {}
        for key, ref in ref64.items():
            assert torch.isfinite(got[key]).all(), (engine, key)
            err, ref_err = _maxrel(got[key], ref), _maxrel(ref32[key], ref)
            bound = max(8.0 * ref_err, 2.0 ** -20)
            kind = key.split()[0].rstrip("0123456789")      # dJ, total, loss, dlam, dscal
            worst[kind] = max(worst.get(kind, (0.0, 0.0)), (err, ref_err))
            if not err <= bound:
                bad.append((engine, key, err, ref_err, bound))
        print(f"LOSS_OPS_FP64 {name} {engine} (kernel/fp32 reference) "
              + " ".join(f"{k} {e:.1e}/{r:.1e}" for k, (e, r) in worst.items()))
    assert not bad, bad


@pytest.mark.gpu
def test_shared_weight_gradient_gpu():
    """The two-pair periodic program on the GPU: the solver's lambda gradient of the BC (by the path
    the program now takes) against float64.  Metric and bound as in ``test_loss_kernels_vs_fp64``,
    the float32 reference being the program on the torch jet in float32.  Before the fix the fused
    kernels kept one pair's part only.  Measured on MI355X: 2.1e-7 (float32 reference 3.2e-7); with
    the parent's ``fusion.py`` 0.31."""
    m = _two_pair_periodic("cuda", "hip", width=32, precision="fp32")
    prog = m.program()
    assert prog.backend == "hip"
    eng = m._get_engine(None, 1)
    _, grads, _ = eng._phase_a()
    got = grads[1].detach().double().reshape(-1)
    ref = _two_pair_periodic("cuda", "jet", width=32)
    with torch.no_grad():
        ref.u_model.flat.copy_(m.u_model.flat)
    out = {}
    for dtype in (torch.float64, torch.float32):
        p = m.u_model.flat.detach().to(dtype).requires_grad_(True)
        lam = [m.lambdas[0].detach().to(dtype).requires_grad_(True)]
        tot, _ = ref.program().evaluate(p, lam)
        out[dtype] = torch.autograd.grad(tot, lam)[0].double().reshape(-1)
    err, ref_err = _maxrel(got, out[torch.float64]), _maxrel(out[torch.float32], out[torch.float64])
    print(f"LOSS_OPS_SHARED_LAMBDA fused={prog.fused_op is not None} kernel path {err:.3e} "
          f"fp32 reference {ref_err:.3e}")
    assert err <= max(8.0 * ref_err, 2.0 ** -20), (err, ref_err)


# --------------------------------------------------------------------------- GPU: fused step --
LAYERS4 = [2, 128, 128, 128, 1]     # the shallowest network the fused step accepts
N_F4 = 517                          # a multiple of neither 16 nor 32


def fused_step_errors(pack, precision):
    """``(fused step or None, theta gradient, loss, SA gradients)``: relative errors of
    ``LossGradEngine.evaluate_fg`` (+ ``fused_op.dlam`` / ``dscal``) against the same program on the
    torch jet in float64, measured as in tests/test_fused_kernels.py."""
    from tensordiffeq_amd.fit import LossGradEngine
    from tensordiffeq_amd.ops import fused_step
    m = zoo_model(pack, "cuda", "hip", n_f=N_F4, layers=LAYERS4, precision=precision)
    prog = m.program()
    fop = prog.fused_op
    assert fop is not None, prog.reasons
    fs = fused_step.for_program(prog)
    fg = LossGradEngine(m, prog, m.lambdas).evaluate_fg().double()
    torch.cuda.synchronize()
    dlam = [d.double().clone() for d in fop.dlam]
    dscal = fop.dscal.double().clone()
    ref = zoo_model(pack, "cuda", "jet", n_f=N_F4, layers=LAYERS4)
    p64, lams = _fp64_args(m)
    tot, _ = ref.program().evaluate(p64, lams)
    g64 = torch.autograd.grad(tot, [p64] + lams, allow_unused=True)
    gerr = ((fg[:-1] - g64[0]).norm() / g64[0].norm()).item()
    lerr = abs(fg[-1].item() - tot.item()) / abs(tot.item())
    sa = 0.0
    for a, d in enumerate(dlam):
        gr = g64[1 + fop.fl.lam_slots[a]]
        sa = max(sa, ((d.reshape(-1) - gr.reshape(-1)).norm() / gr.norm().clamp_min(1e-30)).item())
    for a, (_, k) in enumerate(fop.fl.scal_slots):
        sa = max(sa, _rel(dscal[a], g64[1 + k]))
    return fs, gerr, lerr, sa


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("pack", PACK_NAMES)
def test_fused_step_zoo_vs_fp64(pack, precision):
    """``GenLoss::eval`` in the one-launch step (``tdq_fused_step`` bf16, 32-point tiles;
    ``tdq_fused_step3`` bf16x3, 16-point tiles) on the packed zoo programs - A: tanh + log + cos +
    neg_square (COORD loads from the tile); B: powi + powf + div; C: g(lambda), a scalar SA weight
    (the SCAL adjoint ``acc[n_terms + a] += g``) and rops; D: Burgers (no pair group, VAL first: the
    ``pre`` prefetch of a value array) - network [2, 128, 128, 128, 1], n_f = 517, against the same
    program on the float64 torch jet.  Bounds: tests/test_fused_kernels.py ``BOUNDS``.

    Measured on MI355X (theta gradient / loss / SA gradients):
                fused step                        separate launches (TDQ_FUSED_STEP=0)
      A bf16    2.79e-3 / 7.2e-6 / 1.88e-3        2.75e-3 / 6.9e-6 / 1.88e-3
      A bf16x3  3.20e-6 / 4.5e-7 / 2.94e-6        3.20e-6 / 4.5e-7 / 2.92e-6
      B bf16    2.79e-3 / 9.2e-6 / 1.88e-3        2.74e-3 / 9.0e-6 / 1.88e-3
      B bf16x3  3.20e-6 / 4.6e-7 / 2.61e-6        3.20e-6 / 4.6e-7 / 2.58e-6
      C bf16    1.63e-3 / 9.8e-5 / 7.39e-4        1.76e-3 / 9.7e-5 / 7.36e-4
      C bf16x3  2.51e-6 / 1.4e-7 / 1.19e-6        2.51e-6 / 2.5e-7 / 1.19e-6
      D bf16    4.34e-3 / 7.4e-4 / -              4.32e-3 / 7.4e-4 / -
      D bf16x3  4.20e-6 / 9.8e-8 / -              4.16e-6 / 9.8e-8 / -
    Every program is inside ``BOUNDS``, so no program has a bound of its own.  Sensitivity (rules
    broken in a scratch copy): the SCAL adjoint halved in ``gen_loss`` fails C in both precisions
    (SA error 0.50); the COS adjoint's sign flipped in ``loss_jit._reverse_code`` fails A in bf16x3
    (gradient 9.9e-5 > 3e-5) but stays inside the bf16 bound (2.85e-3 < 8e-3): a small term's
    adjoint is below the bf16 rounding of the network, and the bf16x3 kernel - the same generated
    ``GenLoss`` - is the one that sees it.
    """
    from tests.test_fused_kernels import BOUNDS
    fs, gerr, lerr, sa = fused_step_errors(pack, precision)
    assert fs is not None
    assert fs.lo == (precision == "bf16x3")
    print(f"FUSED_FP64 zoo {pack} n_f={N_F4} {precision} layout={fs.layout} G={fs.G} grad {gerr:.3e} "
          f"loss {lerr:.3e} SA {sa:.3e}")
    gb, lb, sb = BOUNDS[precision]
    assert gerr < gb, gerr
    assert lerr < lb, lerr
    assert sa < sb, sa
