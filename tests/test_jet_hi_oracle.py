"""Every variant and edge of the high-order jet kernels (csrc/jet_hi.hip, ops/jet_hi.py) against float64.

tests/test_jet_hi.py runs the kernels at three shapes that reach chain<5> and table<8> with aligned,
4-divisible widths, variable 0, one staging batch of the weight-gradient kernel and every stream
owned.  This file is the oracle for whoever changes those kernels next:

* a case table that names each of the ten reachable (S, chain / table) instantiations, the
  element-wise weight loads, one and sixteen hidden layers, chains on a variable other than 0,
  d_in 1 / 8, d_out 3 / 4, a partial workgroup, two and three staging batches of the weight-gradient
  kernel (a partial one, an odd row count) and the accumulator wrap of the vector reduction;
* each case with every stream owned and in the production shape (only the top orders owned, permuted
  rows, ldJ > n, NaN in everything the kernels must not read);
* the forward per stream and the gradient per parameter block (K0 rows, hidden kernels, biases, Ko,
  bo), not as one global norm; NaN-filled grad / scratch / work buffers; bitwise determinism and the
  split backward (part 1 then part 2);
* both sides of the depth (HI_X3_DEPTH = 4 hidden layers) beyond which the layer GEMMs split their
  operands into three bf16 terms instead of two - the change the 16-layer case of the table led to;
* j0 != 0 through the C entry points; large pre-activations against a torch emulation of the same
  arithmetic; the host table (build_spec) interpreted in float64 against jet_forward on the CPU for
  every stream set of at most 8 streams over d_in <= 3; the native argument validation.

table<2> (HI_CASES' X(2, false)) is unreachable: a 2-stream plan is (), (v), which hi_spec marks a
chain; it stays in the library and no case can name it.

Measured errors: profiles/r13_jet_hi_oracle_errors.txt.
"""
import ctypes
import itertools

import pytest
import torch

from tensordiffeq_amd.jet import JetPlan, _tanh_jet, closure, jet_forward, tanh_derivs
from tensordiffeq_amd.models.networks import TanhMLP
from tensordiffeq_amd.ops import _lib, jet_hi

# (sizes, requests, n, S, variant): S and the variant are asserted, so that the table cannot drift
# away from the instantiation it names
CASES = [
    ([2, 24, 24, 1], [(1,)], 7, 2, "chain"),                 # chain<2>, variable 1
    ([2, 40, 36, 1], [(1, 1)], 65, 3, "chain"),              # chain<3>, variable 1; off the 32-tile; 2 splits
    ([1, 30, 30, 1], [(0, 0, 0)], 3, 4, "chain"),            # chain<4>; d_in 1; wout % 4 != 0; partial workgroup
    ([2, 33, 1], [(0, 0, 0, 0)], 5, 5, "chain"),             # one hidden layer: no GEMM, no tile-reduce blocks
    ([2, 128, 128, 3], [(1, 1, 1, 1)], 257, 5, "chain"),     # chain<5>, variable 1; d_out 3; 65 workgroups; 5 splits
    ([8, 32, 32, 4], [(7, 7, 7)], 12, 4, "chain"),           # d_in 8, d_out 4, variable 7
    ([2] + [24] * 16 + [1], [(0, 0, 0, 0)], 21, 5, "chain"),  # 16 hidden layers
    ([2, 128, 128, 128, 1], [(0, 0, 0, 0)], 1100, 5, "chain"),  # 3 staging batches (partial, odd); 275 workgroups
    ([2, 21, 1], [(0,), (1,)], 2, 3, "table"),               # table<3>; one hidden layer
    ([2, 17, 20, 20, 1], [(0, 0), (1,)], 13, 4, "table"),    # table<4>; off_layer(1) = 51 unaligned
    ([2, 96, 100, 4], [(0, 0, 0), (1,)], 130, 5, "table"),   # table<5>; d_out 4; 3 splits
    ([2, 44, 44, 1], [(0, 0, 0), (0, 1)], 10, 6, "table"),   # table<6>
    ([2, 64, 48, 1], [(0, 0, 0), (0, 1), (1, 1)], 10, 7, "table"),  # table<7>
    ([2, 128, 128, 1], [(0, 0, 0, 1)], 300, 8, "table"),     # table<8>, 32 GEMM rows live; two batches
    ([3, 31, 32, 1], [(0, 1, 2)], 11, 8, "table"),           # S = 8 in three variables; width 31
]
CASE_IDS = ["x".join(map(str, c[0][:2] + c[0][-1:])) + f"L{len(c[0]) - 2}-" +
            "+".join("".join(map(str, m)) for m in c[1]) + f"-n{c[2]}" for c in CASES]
BOUND = 1e-4  # the split-bf16 family's documented bound (tests/test_jet_hi.py)


def _host_variant(spec_i):
    """hi_spec's rule (csrc/jet_hi.hip): the straight-line chain code for S in 2..5 with
    order[s] == s for every stream, the interpreted partition table otherwise."""
    S = spec_i[0]
    order = spec_i[1:1 + S]
    return "chain" if 2 <= S <= 5 and all(order[s] == s for s in range(S)) else "table"


def _owned_production(plan):
    """The streams the fused kernels do not carry: the plan's highest order (orders 3 and 4 of an
    order-4 plan)."""
    keep = {3, 4} if plan.order == 4 else {plan.order}
    return [m for m in plan.streams if len(m) in keep]


def _production_rows(owned):
    """Non-adjacent, permuted rows of a J with len(owned) + 2 rows."""
    R = len(owned) + 2
    pos = list(range(R - 1, -1, -2))[:len(owned)]
    if len(pos) >= 3:
        pos[0], pos[1] = pos[1], pos[0]
    assert len(pos) == len(owned) and all(abs(a - b) > 1 for a, b in itertools.combinations(pos, 2))
    return dict(zip(owned, pos)), R


def _blocks(net):
    """(name, start, end) of every parameter block of the flat buffer: K0 row by row, every hidden
    kernel, every bias, Ko, bo."""
    out, last = [], len(net.offsets) - 1
    for i, (wo, bo, fi, fo) in enumerate(net.offsets):
        if i == 0:
            out += [(f"K0[{v}]", wo + v * fo, wo + (v + 1) * fo) for v in range(fi)]
            out.append(("b0", bo, bo + fo))
        elif i == last:
            out += [("Ko", wo, bo), ("bo", bo, bo + fo)]
        else:
            out += [(f"K{i}", wo, bo), (f"b{i}", bo, bo + fo)]
    assert out[-1][2] == net.flat.numel() and all(a[2] == b[1] for a, b in zip(out, out[1:]))
    return out


def _make_net(sizes, dev, scale=1.0):
    torch.manual_seed(0)
    net = TanhMLP(sizes, device=dev)
    with torch.no_grad():
        net.flat.add_(0.05 * torch.randn_like(net.flat))
        if scale != 1.0:
            net.flat.mul_(scale)
    return net


def _ref_fp64(net, X, plan, dJ):
    p = net.flat.detach().double().clone().requires_grad_(True)
    J = jet_forward(X.double(), net.weights(p), plan)
    g = torch.autograd.grad((J * dJ.double()).sum(), p)[0]
    return J.detach(), g


def _rel(a, ref, floor=1e-30):
    return ((a.double() - ref).norm() / ref.norm().clamp_min(floor)).item()


def _block_errors(net, g, gr):
    whole = gr.norm().item()
    errs = {name: ((g[a:b].double() - gr[a:b]).norm() / max(gr[a:b].norm().item(), 1e-6 * whole)).item()
            for name, a, b in _blocks(net)}
    return errs, _rel(g, gr)


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _fwd_direct(op, J, P, ldJ, j0):
    rc = op.lib.tdq_jet_hi_fwd(_lib.ptr(op.X), op.n_hi, _lib.ptr(P), *op._args(), _lib.ptr(J), ldJ, j0,
                               _lib.ptr(op.Z), _lib.stream_ptr(op.X.device))
    _lib.check(rc, "tdq_jet_hi_fwd")


def _bwd_direct(op, dJ, P, ldJ, j0, part):
    rc = op.lib.tdq_jet_hi_bwd_part(_lib.ptr(op.X), op.n_hi, _lib.ptr(P), *op._args(), _lib.ptr(dJ), ldJ, j0,
                                    _lib.ptr(op.Z), _lib.ptr(op.work), _lib.ptr(op.grad), int(part),
                                    _lib.stream_ptr(op.X.device))
    _lib.check(rc, "tdq_jet_hi_bwd_part")
    return op.grad


SENTINEL = -12345.6789


def _measure(tag, sizes, reqs, n, production, S=None, variant=None, j0=None, scale=1.0):
    """One forward + backward of the kernels against the fp64 torch jet, with everything the kernels
    must not touch or read poisoned.  Asserts the structural properties (rows and points outside the
    kernels' share untouched, gradient finite from NaN-filled buffers, bitwise determinism, split
    backward) and returns ({stream: forward error}, {block: gradient error}, global gradient error,
    net, plan, X, full-stream dJ) for the caller's bounds.

    ``j0`` None: through HiJetOp (ldJ = the X_all rows; production: n + 37 rows, NaN tail); an int:
    through the C entry points, the points' J rows at ``[j0, j0 + n)`` of ``ldJ = n + 9``."""
    dev = torch.device("cuda", 0)
    net = _make_net(sizes, dev, scale)
    d_in, d_out = sizes[0], sizes[-1]
    plan = JetPlan(reqs, d_in)
    if S is not None:
        assert plan.S == S
        assert _host_variant(jet_hi.build_spec(plan, {})[0]) == variant
    X = (2 * torch.rand(n, d_in, device=dev) - 1).contiguous()
    if production:
        rows, R = _production_rows(_owned_production(plan))
    else:
        rows, R = {m: i for i, m in enumerate(plan.streams)}, plan.S
    if j0 is None:
        lo, ldJ = 0, n + 37 if production else n
        X_all = torch.full((ldJ, d_in), float("nan"), device=dev)
        X_all[:n] = X
    else:
        lo, ldJ = j0, n + 9
        X_all = X
    op = jet_hi.HiJetOp(net, plan, rows, X_all, n, dev)
    for buf in (op.grad, op.Z, op.work):
        buf.fill_(float("nan"))
    J = torch.full((R, ldJ, d_out), SENTINEL, device=dev)
    dJ = torch.full((R, ldJ, d_out), float("nan"), device=dev)
    live = torch.zeros(R, ldJ, dtype=torch.bool, device=dev)
    for m, r in rows.items():
        dJ[r, lo:lo + n] = torch.randn(n, d_out, device=dev)
        live[r, lo:lo + n] = True
    if j0 is None:
        fwd = lambda: op.forward(J, net.flat)
        bwd = lambda part=0: op.backward(dJ, net.flat, part=part)
    else:
        fwd = lambda: _fwd_direct(op, J, net.flat, ldJ, j0)
        bwd = lambda part=0: _bwd_direct(op, dJ, net.flat, ldJ, j0, part)
    fwd()
    g = bwd().clone()
    torch.cuda.synchronize()

    # forward: every unowned row and every point outside [lo, lo + n) bit-for-bit untouched
    assert torch.equal(_bits(J)[~live], _bits(torch.full_like(J, SENTINEL))[~live]), tag
    assert torch.isfinite(J[live]).all(), tag
    # every gradient element written, no unwritten scratch / work / dJ / X element read
    assert torch.isfinite(g).all(), (tag, (~torch.isfinite(g)).nonzero().flatten()[:8].tolist())
    # deterministic, and the split backward gives the same bits from re-poisoned buffers
    assert torch.equal(_bits(bwd()), _bits(g)), tag
    op.grad.fill_(float("nan"))
    op.work.fill_(float("nan"))
    bwd(1)
    assert torch.equal(_bits(bwd(2)), _bits(g)), tag

    full = torch.zeros(plan.S, n, d_out, device=dev)
    for m, r in rows.items():
        full[plan.index[m]] = dJ[r, lo:lo + n]
    Jr, gr = _ref_fp64(net, X, plan, full)
    ferr = {m: _rel(J[r, lo:lo + n], Jr[plan.index[m]]) for m, r in rows.items()}
    berr, gerr = _block_errors(net, g, gr)
    for m, e in ferr.items():
        print(f"HIO {tag} fwd {m}: {e:.2e} (norm {Jr[plan.index[m]].norm().item():.2e})")
    for name, e in berr.items():
        print(f"HIO {tag} grad {name}: {e:.2e}")
    print(f"HIO {tag} grad all: {gerr:.2e}")
    return ferr, berr, gerr, net, plan, X, full


@pytest.mark.gpu
@pytest.mark.parametrize("production", [False, True], ids=["all-owned", "production"])
@pytest.mark.parametrize("sizes,reqs,n,S,variant", CASES, ids=CASE_IDS)
def test_case_table_matches_fp64_jet(sizes, reqs, n, S, variant, production):
    """Forward per owned stream and gradient per parameter block below 1e-4 of the fp64 torch jet,
    for every reachable instantiation and edge of the case table, with every stream owned and in
    the production shape; rows / points outside the kernels' share untouched, NaN-filled buffers,
    bitwise determinism, part 1 + part 2 == part 0 (_measure).

    Measured on an MI355X (profiles/r13_jet_hi_oracle_errors.txt).  Fourteen of the fifteen cases, in
    both shapes: forward <= 4.0e-05 ([2,40,36,1] u_yy), gradient block <= 2.9e-05 (K0[1] of the same
    case), whole gradient <= 9.0e-06.

    The 16-hidden-layer case missed the gradient bound with the two-term bf16 split at every depth:
    gradient blocks up to 1.44e-04 (b14) with every stream owned and 2.50e-04 (b3) in the production
    shape, whole gradient 8.38e-05 / 1.26e-04, forward 5.75e-05 - the accumulated rounding of fifteen
    split-bf16 GEMMs each way (the torch emulation of that arithmetic, _emu_forward below, was as far
    from fp64 on the same inputs: blocks 1.56e-04 / 3.35e-04).  Networks of more than four hidden
    layers now split into three bf16 terms (HI_X3_DEPTH, csrc/jet_hi.hip); the case is at forward
    8.5e-07, blocks 1.7e-06 / 1.17e-05 (b15), whole gradient 7.7e-07 / 4.1e-06."""
    tag = f"{CASE_IDS[[c[0] for c in CASES].index(sizes)]} {'prod' if production else 'all'}"
    ferr, berr, gerr, *_ = _measure(tag, sizes, reqs, n, production, S, variant)
    for m, e in ferr.items():
        assert e < BOUND, (tag, "forward", m, e)
    for name, e in berr.items():
        assert e < BOUND, (tag, "gradient block", name, e)
    assert gerr < BOUND, (tag, gerr)


# The layer GEMMs split their operands into two bf16 terms up to HI_X3_DEPTH = 4 hidden layers and into
# three beyond (csrc/jet_hi.hip): both sides of that threshold, chain and table, and the largest LDS
# layout of the three-term kernels (8 streams, d_in 8, d_out 4)
DEPTH_CASES = [
    ([2] + [24] * 4 + [1], [(0, 0, 0, 0)], 21, 5, "chain"),   # last depth of the two-term split
    ([2] + [24] * 5 + [1], [(0, 0, 0, 0)], 21, 5, "chain"),   # first depth of the three-term split
    ([2, 20, 33, 128, 20, 20, 1], [(0, 0, 0, 1)], 9, 8, "table"),  # three-term, table<8>, widths off the tile
    ([8] + [16] * 5 + [4], [(0, 1, 7)], 6, 8, "table"),       # three-term, largest LDS layout
]


@pytest.mark.gpu
@pytest.mark.parametrize("production", [False, True], ids=["all-owned", "production"])
@pytest.mark.parametrize("sizes,reqs,n,S,variant", DEPTH_CASES, ids=[f"L{len(c[0]) - 2}-S{c[3]}" for c in DEPTH_CASES])
def test_depth_threshold_of_the_three_term_split(sizes, reqs, n, S, variant, production):
    """Same checks and bound as the case table on both sides of the depth at which the layer GEMMs
    change from two to three bf16 terms per operand.  Measured: four layers (two terms) forward
    1.05e-05, gradient block 2.9e-05; five layers (three terms) forward <= 1.9e-06, block <= 2.6e-06."""
    tag = f"depth L{len(sizes) - 2} S{S} {'prod' if production else 'all'}"
    ferr, berr, gerr, *_ = _measure(tag, sizes, reqs, n, production, S, variant)
    assert max(ferr.values()) < BOUND and max(berr.values()) < BOUND and gerr < BOUND, (tag, ferr, berr, gerr)


@pytest.mark.gpu
def test_j0_offset_through_the_c_entry_points():
    """The high-order points' J rows at [5, 5 + n) of ldJ = n + 9 (tdq_jet_hi_fwd / _bwd_part called
    directly, production ownership): same checks, the rows [0, 5) and [5 + n, ldJ) untouched."""
    ferr, berr, gerr, *_ = _measure("j0=5", [2, 40, 36, 2], [(0, 0, 0, 0)], 23, True, 5, "chain", j0=5)
    assert max(ferr.values()) < BOUND and max(berr.values()) < BOUND and gerr < BOUND, (ferr, berr, gerr)


def _mm3(a, b):
    """a @ b as the kernels' split-bf16 product: hi hi + hi lo + lo hi of the bf16 splits, fp32 sums."""
    ah, bh = a.bfloat16().float(), b.bfloat16().float()
    al, bl = (a - ah).bfloat16().float(), (b - bh).bfloat16().float()
    return ah @ bh + ah @ bl + al @ bh


class _Split3(torch.autograd.Function):
    """Hidden-to-hidden product of the kernels: split-bf16 forward (hi_mma<false>) and adjoint
    (hi_mma<true>), fp32 weight gradient (jet_hi_wgrad_kernel)."""

    @staticmethod
    def forward(ctx, a, w):
        ctx.save_for_backward(a, w)
        return _mm3(a, w)

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        return _mm3(g, w.t().contiguous()), a.t() @ g


def _emu_forward(X, weights, plan):
    """jet_forward in the kernels' arithmetic: fp32 everywhere, the hidden-to-hidden products split-bf16."""
    streams, N = plan.streams, X.shape[0]
    K1, b1 = weights[0]
    z = {(): torch.addmm(b1, X, K1)}
    for mi in streams[1:]:
        z[mi] = K1[mi[0]].unsqueeze(0).expand(N, -1) if len(mi) == 1 else None
    for li, (K, b) in enumerate(weights[1:], start=1):
        h = _tanh_jet(z, streams, plan.order)
        mm = (lambda a, w: a @ w) if li == len(weights) - 1 else _Split3.apply
        z = {mi: None if h[mi] is None else mm(h[mi].contiguous(), K) + (b if mi == () else 0.0) for mi in streams}
    d_out = weights[-1][0].shape[1]
    return torch.stack([z[mi] if z[mi] is not None else X.new_zeros(N, d_out) for mi in streams], 0)


@pytest.mark.gpu
def test_large_preactivations_against_same_arithmetic_emulation():
    """Weights x 3 ([2,64,64,1], u_xxxx, 64 points): |z| up to 1.7 in layer 0 and more in layer 1, where
    q3..q5 change sign and hi_sigmas leaves its small-z branch; stream norms up to 1e3.  The 1e-4
    bound was written for small z, so the bound here comes from a torch emulation of the kernels'
    arithmetic (fp32, split-bf16 hidden-to-hidden products, jet._tanh_jet): its own error against
    fp64, e_emu, per stream and per parameter block; the kernels stay below 4 e_emu + 1e-6 (the
    factor covers summation order and __expf).

    Measured on an MI355X (profiles/r13_jet_hi_oracle_errors.txt; layer-0 |z| up to 2.06, u_xxxx norm
    2.3e+03): forward, kernel 3.5e-06 .. 1.03e-05 against e_emu 3.5e-06 .. 1.18e-05 (largest: u_xxxx);
    gradient blocks, kernel <= 1.84e-05 against e_emu <= 1.69e-05 (K0[1]); whole gradient 1.35e-05
    against 1.31e-05 - the kernels sit on the emulation, a quarter of the bound."""
    sizes, reqs, n = [2, 64, 64, 1], [(0, 0, 0, 0)], 64
    ferr, berr, gerr, net, plan, X, full = _measure("big-z", sizes, reqs, n, False, 5, "chain", scale=3.0)
    Jr, gr = _ref_fp64(net, X, plan, full)
    cpu = TanhMLP(sizes, device="cpu")
    p = net.flat.detach().cpu().clone().requires_grad_(True)
    Je = _emu_forward(X.cpu(), cpu.weights(p), plan)
    ge = torch.autograd.grad((Je * full.cpu()).sum(), p)[0]
    Jr, gr = Jr.cpu(), gr.cpu()
    z0 = X.double() @ net.kernel(0).double() + net.bias(0).double()
    print(f"HIO big-z layer-0 |z| max {z0.abs().max().item():.2f}")
    assert z0.abs().max().item() > 1.0
    e_f = {m: _rel(Je[plan.index[m]].detach(), Jr[plan.index[m]]) for m in plan.streams}
    e_b, e_g = _block_errors(cpu, ge, gr)
    bad = []
    for m in plan.streams:
        print(f"HIO big-z fwd {m}: kernel {ferr[m]:.2e} e_emu {e_f[m]:.2e}")
        if not ferr[m] < 4 * e_f[m] + 1e-6:
            bad.append(("forward", m, ferr[m], e_f[m]))
    for name in e_b:
        print(f"HIO big-z grad {name}: kernel {berr[name]:.2e} e_emu {e_b[name]:.2e}")
        if not berr[name] < 4 * e_b[name] + 1e-6:
            bad.append(("gradient block", name, berr[name], e_b[name]))
    print(f"HIO big-z grad all: kernel {gerr:.2e} e_emu {e_g:.2e}")
    if not gerr < 4 * e_g + 1e-6:
        bad.append(("gradient", "all", gerr, e_g))
    assert not bad, bad


# ---- host table on the CPU ----

def _interp_spec(spec_i, spec_c, X, weights):
    """fp64 interpreter of build_spec's table, as the kernels read it: layer 0 from order / var, linear
    layers with the net's weights (bias on stream 0), tanh from the term list with jet.tanh_derivs."""
    S = spec_i[0]
    order, var = spec_i[1:1 + S], spec_i[1 + S:1 + 2 * S]
    nt = spec_i[1 + 3 * S]
    terms = [spec_i[2 + 3 * S + 7 * k:9 + 3 * S + 7 * k] for k in range(nt)]
    assert len(spec_c) == nt and len(spec_i) == 2 + 3 * S + 7 * nt
    K0, b0 = weights[0]
    zero = torch.zeros(X.shape[0], K0.shape[1], dtype=X.dtype)
    z = [X @ K0 + b0] + [K0[var[s]].expand_as(zero) if order[s] == 1 else zero for s in range(1, S)]
    for K, b in weights[1:]:
        sg = tanh_derivs(torch.tanh(z[0]), 4)
        h = [sg[0]] + [torch.zeros_like(z[0]) for _ in range(1, S)]
        for (s, k, nb, *fac), c in zip(terms, spec_c):
            v = c * sg[k]
            for f in fac[:nb]:
                v = v * z[f]
            h[s] = h[s] + v
        z = [hs @ K + (b if s == 0 else 0.0) for s, hs in enumerate(h)]
    return torch.stack(z, 0)


def _down_closed_sets(d, max_s=jet_hi.MAX_S, max_order=4):
    """Every stream set (closed under sub-multisets) over d variables with 2..max_s streams and order
    <= max_order: each is the closure of a request set, and every request set's closure is one."""
    mis = [m for r in range(1, max_order + 1) for m in itertools.combinations_with_replacement(range(d), r)]
    root = frozenset({()})
    seen, frontier = {root}, [root]
    while frontier:
        nxt = []
        for cur in frontier:
            for m in mis:
                if m in cur or not set(closure([m])) - {m} <= cur:
                    continue
                new = cur | {m}
                if len(new) <= max_s and new not in seen:
                    seen.add(new)
                    nxt.append(new)
        frontier = nxt
    return sorted((sorted(s - root, key=lambda m: (len(m), m)) for s in seen if len(s) > 1), key=lambda r: (len(r), r))


def _check_host_table(sizes, reqs):
    torch.manual_seed(0)
    net = TanhMLP(sizes, device="cpu")
    with torch.no_grad():
        net.flat.add_(0.05 * torch.randn_like(net.flat))
    plan = JetPlan(reqs, sizes[0])
    X = 2 * torch.rand(5, sizes[0], dtype=torch.float64) - 1
    w = net.weights(net.flat.detach().double())
    want = {tuple(sorted(m)): 3 + 2 * i for i, m in enumerate(reqs)}
    si, sc = jet_hi.build_spec(plan, want)
    S = si[0]
    assert S == plan.S and si[1:1 + S] == [len(m) for m in plan.streams]
    # `out` carries exactly the requested rows
    assert si[1 + 2 * S:1 + 3 * S] == [want.get(m, -1) for m in plan.streams]
    got, ref = _interp_spec(si, sc, X, w), jet_forward(X, w, plan)
    for s, m in enumerate(plan.streams):
        scale = ref[s].abs().max().item()
        assert (got[s] - ref[s]).abs().max().item() <= 1e-10 * scale, (reqs, m)
    return _host_variant(si), S


def test_host_table_interpreted_matches_jet_forward_case_table():
    """build_spec's table, interpreted in fp64, is jet_forward (1e-10 of each stream's scale) for every
    plan of the case table; the host rule picks the variant each case names, and the table names all
    ten reachable instantiations (table<2> is unreachable: a 2-stream plan is always a chain)."""
    named = set()
    for sizes, reqs, _, S, variant in CASES:
        assert _check_host_table(sizes, reqs) == (variant, S), (sizes, reqs)
        named.add((variant, S))
    assert named == {("chain", s) for s in range(2, 6)} | {("table", s) for s in range(3, 9)}


def test_host_table_interpreted_matches_jet_forward_all_small_plans():
    """The same for every stream set of 2..8 streams and order <= 4 over d_in <= 3 (5 + 51 + 304 sets)."""
    count = 0
    for d in (1, 2, 3):
        sets = _down_closed_sets(d)
        for reqs in sets:
            variant, S = _check_host_table([d, 6, 5, 1], reqs)
            one_var = len({v for m in reqs for v in m}) == 1
            assert (variant == "chain") == (one_var and S <= 5), reqs
            count += 1
    assert count == 4 + 51 + 304


def test_build_spec_limits():
    with pytest.raises(ValueError):
        jet_hi.build_spec(JetPlan([(0, 0, 1, 1)], 2), {})       # 9 streams
    assert JetPlan([(0, 0, 1, 1)], 2).S == 9
    with pytest.raises(ValueError):
        jet_hi.build_spec(JetPlan([(0, 0, 0, 0, 0)], 2), {})    # order 5, 6 streams
    jet_hi.build_spec(JetPlan([(0, 0, 0, 1)], 2), {})           # 8 streams, order 4: accepted


def test_eligible_flips_at_the_envelope():
    """Width 128 / 129, d_in 8 / 9, d_out 4 / 5, 16 / 17 hidden layers."""
    plan = JetPlan([(0, 0, 0)], 2)
    ok = lambda sizes, p=plan: jet_hi.eligible(TanhMLP(sizes, device="cpu"), p)[0]
    assert ok([2, 128, 128, 1]) and not ok([2, 128, 129, 1]) and not ok([2, 129, 1])
    assert ok([8, 16, 1], JetPlan([(7, 7, 7)], 8)) and not ok([9, 16, 1], JetPlan([(8, 8, 8)], 9))
    assert ok([2, 16, 4]) and not ok([2, 16, 5])
    assert ok([2] + [8] * 16 + [1]) and not ok([2] + [8] * 17 + [1])


@pytest.mark.gpu
def test_native_argument_validation_rejects_before_any_launch():
    """Width 129, a 9-stream spec, a term whose factor is stream 0 and order[0] != 0 return a non-zero
    code from tdq_jet_hi_fwd and tdq_jet_hi_bwd_part and leave J / grad untouched (hi_dims / hi_spec
    reject before any launch)."""
    dev = torch.device("cuda", 0)
    lib = _lib.load(required=True)
    n, d_in, d_out = 4, 2, 1
    good_w = [128, 128]
    si, sc = jet_hi.build_spec(JetPlan([(0, 0)], 2), {(0, 0): 0})
    S = si[0]
    nine = [9] + [0] + [1] * 8 + [0] * 9 + [-1] * 9 + [0]
    fac0 = list(si)
    first = 2 + 3 * S            # term 0: (stream, k, nb, b0, ..)
    assert fac0[first + 2] >= 1
    fac0[first + 3] = 0
    ord0 = list(si)
    ord0[1] = 1
    bad = [("width 129", [128, 129], si, sc), ("S = 9", good_w, nine, [1.0]),
           ("factor stream 0", good_w, fac0, sc), ("order[0] != 0", good_w, ord0, sc)]
    X = torch.rand(n, d_in, device=dev)
    P = torch.randn(4 * 129 * 129, device=dev)
    # buffers as large as the valid geometry needs: nothing may be launched, and nothing could run out of bounds
    gw = (ctypes.c_int * 2)(*good_w)
    Z = torch.zeros(int(lib.tdq_jet_hi_scratch_floats(n, 2)), device=dev)
    work = torch.zeros(int(lib.tdq_jet_hi_work_floats(n, d_in, gw, d_out, 2)) + 4 * 129 * 129, device=dev)
    st = _lib.stream_ptr(dev)
    # the unmodified arguments are accepted (so each rejection below is due to its one change)
    J = torch.full((S, n, d_out), SENTINEL, device=dev)
    assert lib.tdq_jet_hi_fwd(_lib.ptr(X), n, _lib.ptr(P), d_in, gw, d_out, 2, (ctypes.c_int * len(si))(*si),
                              (ctypes.c_float * len(sc))(*sc), _lib.ptr(J), n, 0, _lib.ptr(Z), st) == 0
    torch.cuda.synchronize()
    assert (J[0] != SENTINEL).all() and (J[1:] == SENTINEL).all()
    for name, widths, spec_i, spec_c in bad:
        w = (ctypes.c_int * len(widths))(*widths)
        ci, cc = (ctypes.c_int * len(spec_i))(*spec_i), (ctypes.c_float * len(spec_c))(*spec_c)
        J = torch.full((9, n, d_out), SENTINEL, device=dev)
        dJ = torch.ones(9, n, d_out, device=dev)
        grad = torch.full((4 * 129 * 129,), SENTINEL, device=dev)
        rc = lib.tdq_jet_hi_fwd(_lib.ptr(X), n, _lib.ptr(P), d_in, w, d_out, 2, ci, cc, _lib.ptr(J), n, 0,
                                _lib.ptr(Z), st)
        assert rc != 0, name
        for part in (0, 1, 2):
            rc = lib.tdq_jet_hi_bwd_part(_lib.ptr(X), n, _lib.ptr(P), d_in, w, d_out, 2, ci, cc, _lib.ptr(dJ), n, 0,
                                         _lib.ptr(Z), _lib.ptr(work), _lib.ptr(grad), part, st)
            assert rc != 0, (name, part)
        torch.cuda.synchronize()
        assert (J == SENTINEL).all() and (grad == SENTINEL).all(), name
