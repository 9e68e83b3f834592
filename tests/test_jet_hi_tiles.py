"""The high-order jet kernels (csrc/jet_hi.hip: jet_hi_fwd_kernel, jet_hi_chain_kernel) at 8 and 16 points
per workgroup, and every tile through the tdq_jet_hi_tile_* entry points, against float64.

Same oracle as tests/test_jet_hi_oracle.py (its ``_measure``: forward per stream and gradient per
parameter block against ``jet_forward`` in fp64 at the family's 1e-4, every stream owned and the
production shape, NaN-filled buffers, bitwise determinism, part 1 + part 2 == part 0), with the tile
forced through ``HiJetOp(tile=)``.  The production shape here also runs through the C entry points
with ``j0 != 0``.  The cases are the edges of the larger tiles: a partial last workgroup for both
tiles, S = 8 with every GEMM row tile live, unaligned layer offsets, fewer points than one tile, one
hidden layer, both sides of the three-term split, several weight-gradient splits with a partial
staging batch and more than 256 vector-slab rows, tile 4 through the tile entry points (alone and as
the chain's half of a mixed pair: what the automatic choice gives where 8 points do not fit the
chain), and the rows of tile 4 for comparison.
"""
import ctypes
import functools

import pytest
import torch

from tensordiffeq_amd.jet import JetPlan
from tensordiffeq_amd.ops import _lib, jet_hi

from . import test_jet_hi_oracle as oracle
from .test_jet_hi_oracle import BOUND, SENTINEL

# (tile, sizes, requests, n, S, variant)
CASES = [
    (8, [2, 128, 128, 1], [(0, 0, 0), (1,)], 19, 5, "table"),      # KdV plan; partial last workgroup
    (16, [2, 128, 128, 1], [(0, 0, 0), (1,)], 19, 5, "table"),
    (8, [2, 128, 128, 128, 3], [(1, 1, 1, 1)], 257, 5, "chain"),   # chain<5> on variable 1; d_out 3
    # d_out 3: the chain's vector-parameter area (7 slots) leaves no room for 16 points x 5 streams, the
    # forward has it - the pair the automatic choice makes there
    ((16, 8), [2, 128, 128, 128, 3], [(1, 1, 1, 1)], 257, 5, "chain"),
    (8, [2, 128, 128, 1], [(0, 0, 0, 1)], 300, 8, "table"),        # S = 8: the largest tile there, 4 row tiles live
    (8, [2, 17, 20, 20, 1], [(0, 0), (1,)], 13, 4, "table"),       # unaligned layer offsets
    (8, [1, 30, 30, 1], [(0, 0, 0)], 3, 4, "chain"),               # wout % 4 != 0; fewer points than one tile
    (16, [2, 33, 1], [(0, 0, 0, 0)], 5, 5, "chain"),               # one hidden layer: no GEMM
    (8, [2] + [24] * 5 + [1], [(0, 0, 0, 0)], 21, 5, "chain"),     # three-term split
    (8, [2] + [24] * 4 + [1], [(0, 0, 0, 0)], 21, 5, "chain"),     # two-term side of the depth threshold
    (16, [2, 128, 128, 128, 1], [(0, 0, 0, 0)], 4100, 5, "chain"),  # 17 splits, partial batch, 257 vslab rows
    (16, [2, 24, 24, 24, 24, 24, 1], [(0, 0, 0)], 37, 4, "chain"),  # LDS boundary: 16 points, three-term, S = 4
    # tile 4 through the tile entry points (S-sized scratch, 256-point splits): the fallback of the
    # automatic choice (three-term split, S = 8: all 32 GEMM rows live); HiJetOp(tile=4) means the small
    # entry points, so only the direct-call shape reaches them (SHAPES below)
    (4, [2] + [24] * 5 + [1], [(0, 0, 0, 1)], 21, 8, "table"),
    ((8, 4), [2, 128, 128, 1], [(0, 0, 0), (1,)], 19, 5, "table"),  # mixed pair; partial last workgroup for both
]
IDS = [f"t{c[0] if isinstance(c[0], int) else '+'.join(map(str, c[0]))}-" + "x".join(map(str, c[1][:2] + c[1][-1:])) + f"L{len(c[1]) - 2}-S{c[4]}-n{c[3]}" for c in CASES]


@pytest.fixture
def force_tile(monkeypatch):
    """Make the oracle's ``_measure`` build its op with a forced tile and, on its direct (``j0``) path,
    call the tile entry points."""
    def _force(tile):
        monkeypatch.setattr(jet_hi, "HiJetOp", functools.partial(jet_hi.HiJetOp, tile=tile))

        def fwd(op, J, P, ldJ, j0):
            pair = tile if isinstance(tile, tuple) else (tile, tile)
            assert op.entry == ("hi" if pair == (4, 4) else "hi_tile") and (op.tile, op.tile_bwd) == pair
            rc = op.lib.tdq_jet_hi_tile_fwd(_lib.ptr(op.X), op.n_hi, _lib.ptr(P), *op._args(), _lib.ptr(J), ldJ, j0,
                                            _lib.ptr(op.Z), op.tile, _lib.stream_ptr(op.X.device))
            _lib.check(rc, "tdq_jet_hi_tile_fwd")

        def bwd(op, dJ, P, ldJ, j0, part):
            rc = op.lib.tdq_jet_hi_tile_bwd_part(_lib.ptr(op.X), op.n_hi, _lib.ptr(P), *op._args(), _lib.ptr(dJ), ldJ,
                                                 j0, _lib.ptr(op.Z), _lib.ptr(op.work), _lib.ptr(op.grad), int(part),
                                                 op.tile_bwd, _lib.stream_ptr(op.X.device))
            _lib.check(rc, "tdq_jet_hi_tile_bwd_part")
            return op.grad

        monkeypatch.setattr(oracle, "_fwd_direct", fwd)
        monkeypatch.setattr(oracle, "_bwd_direct", bwd)
    return _force


def _assert_bounds(tag, ferr, berr, gerr):
    for m, e in ferr.items():
        assert e < BOUND, (tag, "forward", m, e)
    for name, e in berr.items():
        assert e < BOUND, (tag, "gradient block", name, e)
    assert gerr < BOUND, (tag, gerr)


# the two HiJetOp shapes and the direct call of the C tile entry points; tile 4 alone only the latter
SHAPES = [pytest.param(*c, shape, id=f"{i}-{shape}") for shape in ("all-owned", "production", "production-j0")
          for c, i in zip(CASES, IDS) if c[0] != 4 or shape == "production-j0"]


@pytest.mark.gpu
@pytest.mark.parametrize("tile,sizes,reqs,n,S,variant,shape", SHAPES)
def test_tile_kernels_match_fp64_jet(force_tile, tile, sizes, reqs, n, S, variant, shape):
    """Forward per owned stream and gradient per parameter block below 1e-4 of the fp64 torch jet with
    the tile forced: every stream owned; the production shape through HiJetOp (top orders owned,
    permuted rows, ldJ = n + 37, NaN in everything that must not be read); and the production shape
    through the C entry points with j0 = 5."""
    force_tile(tile)
    tag = f"tile{tile} {IDS[CASES.index((tile, sizes, reqs, n, S, variant))]} {shape}"
    ferr, berr, gerr, *_ = oracle._measure(tag, sizes, reqs, n, shape != "all-owned", S, variant,
                                           j0=5 if shape == "production-j0" else None)
    _assert_bounds(tag, ferr, berr, gerr)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [8, 16])
def test_tile_forward_rows_are_the_four_point_kernels_rows(tile):
    """[2,128,128,1], the KdV plan, 1024 points: per row the kernels run the same arithmetic at every
    tile (k order, the three products, hi_sigmas, the output layer's sum); the forward rows agree
    within 2e-6 of each stream's norm, a few fp32 ulps (printed, with whether they are bit-equal: the
    compiler may contract the elementwise code of two instantiations differently).  The gradient takes
    other split counts and slab rows, another summation order: printed, and checked against fp64 at
    1e-4 like the forward."""
    dev = torch.device("cuda", 0)
    sizes, reqs, n = [2, 128, 128, 1], [(0, 0, 0), (1,)], 1024
    net = oracle._make_net(sizes, dev)
    plan = JetPlan(reqs, 2)
    X = (2 * torch.rand(n, 2, device=dev) - 1).contiguous()
    rows = {m: i for i, m in enumerate(plan.streams)}
    dJ = torch.randn(plan.S, n, 1, device=dev)
    out = {}
    for t in (4, tile):
        op = jet_hi.HiJetOp(net, plan, rows, X, n, dev, tile=t)
        assert op.entry == ("hi" if t == 4 else "hi_tile") and op.tile == t
        J = torch.full((plan.S, n, 1), float("nan"), device=dev)
        op.forward(J, net.flat)
        out[t] = (J, op.backward(dJ, net.flat).clone())
    torch.cuda.synchronize()
    (J4, g4), (Jt, gt) = out[4], out[tile]
    for s, m in enumerate(plan.streams):
        d = ((Jt[s] - J4[s]).norm() / J4[s].norm()).item()
        print(f"HIT tile{tile} vs 4-point fwd {m}: {d:.2e}")
    assert torch.equal(oracle._bits(Jt), oracle._bits(J4))
    for name, a, b in oracle._blocks(net):
        d = ((gt[a:b] - g4[a:b]).norm() / g4[a:b].norm()).item()
        print(f"HIT tile{tile} vs 4-point grad {name}: {d:.2e}")
    Jr, gr = oracle._ref_fp64(net, X, plan, dJ)
    assert max(oracle._rel(Jt[s], Jr[s]) for s in range(plan.S)) < BOUND
    berr, gerr = oracle._block_errors(net, gt, gr)
    assert max(berr.values()) < BOUND and gerr < BOUND


@pytest.mark.gpu
def test_forced_tile_that_does_not_fit_raises():
    """16 points x 8 streams need 128 GEMM rows: beyond LDS.  16 points x 5 streams fit with one output
    and not with three (the chain's vector-parameter area)."""
    dev = torch.device("cuda", 0)
    net = oracle._make_net([2, 32, 32, 1], dev)
    X = torch.rand(40, 2, device=dev)
    p8, p5 = JetPlan([(0, 0, 0, 1)], 2), JetPlan([(0, 0, 0, 0)], 2)
    with pytest.raises(ValueError):
        jet_hi.HiJetOp(net, p8, {}, X, 40, dev, tile=16)
    with pytest.raises(ValueError):
        jet_hi.HiJetOp(net, p5, {}, X, 40, dev, tile=5)
    assert jet_hi.HiJetOp(net, p8, {}, X, 40, dev, tile=8).tile == 8
    assert jet_hi.HiJetOp(net, p5, {}, X, 40, dev, tile=16).tile_bwd == 16
    with pytest.raises(ValueError):
        jet_hi.HiJetOp(oracle._make_net([2, 32, 32, 3], dev), p5, {}, X, 40, dev, tile=16)


@pytest.mark.gpu
def test_tile_entry_points_reject_before_any_launch():
    """Tile 5, a tile that does not fit (16 points x 8 streams), width 129 and a 9-stream spec return a
    non-zero code from tdq_jet_hi_tile_fwd / tdq_jet_hi_tile_bwd_part (every part) and leave J / grad
    untouched; the size functions return -1 for them."""
    dev = torch.device("cuda", 0)
    lib = _lib.load(required=True)
    n, d_in, d_out = 20, 2, 1
    good_w = [128, 128]
    si, sc = jet_hi.build_spec(JetPlan([(0, 0)], 2), {(0, 0): 0})
    s8, c8 = jet_hi.build_spec(JetPlan([(0, 0, 0, 1)], 2), {(0, 0, 0, 1): 0})
    nine = [9] + [0] + [1] * 8 + [0] * 9 + [-1] * 9 + [0]
    bad = [("tile 5", 5, good_w, si, sc), ("tile 16 x 8 streams", 16, good_w, s8, c8),
           ("width 129", 8, [128, 129], si, sc), ("S = 9", 8, good_w, nine, [1.0])]
    X = torch.rand(n, d_in, device=dev)
    P = torch.randn(4 * 129 * 129, device=dev)
    gw = (ctypes.c_int * 2)(*good_w)
    Z = torch.zeros(int(lib.tdq_jet_hi_tile_scratch_floats(n, 2, 8)), device=dev)
    work = torch.zeros(int(lib.tdq_jet_hi_tile_work_floats(n, d_in, gw, d_out, 2, 4)) + 4 * 129 * 129, device=dev)
    st = _lib.stream_ptr(dev)
    assert lib.tdq_jet_hi_tile_scratch_floats(n, 2, 9) == -1 and lib.tdq_jet_hi_tile_scratch_floats(n, 2, 0) == -1
    assert lib.tdq_jet_hi_tile_work_floats(n, d_in, gw, d_out, 2, 5) == -1
    assert lib.tdq_jet_hi_tile_work_floats(n, d_in, (ctypes.c_int * 2)(128, 129), d_out, 2, 8) == -1
    assert lib.tdq_jet_hi_tile_scratch_floats(n, 2, 3) == 3 * 2 * n * 3 * 128   # sized by S
    # the unmodified arguments are accepted at tile 8
    J = torch.full((si[0], n, d_out), SENTINEL, device=dev)
    assert lib.tdq_jet_hi_tile_fwd(_lib.ptr(X), n, _lib.ptr(P), d_in, gw, d_out, 2, (ctypes.c_int * len(si))(*si),
                                   (ctypes.c_float * len(sc))(*sc), _lib.ptr(J), n, 0, _lib.ptr(Z), 8, st) == 0
    torch.cuda.synchronize()
    assert (J[0] != SENTINEL).all() and (J[1:] == SENTINEL).all()
    for name, tile, widths, spec_i, spec_c in bad:
        w = (ctypes.c_int * len(widths))(*widths)
        ci, cc = (ctypes.c_int * len(spec_i))(*spec_i), (ctypes.c_float * len(spec_c))(*spec_c)
        J = torch.full((9, n, d_out), SENTINEL, device=dev)
        dJ = torch.ones(9, n, d_out, device=dev)
        grad = torch.full((4 * 129 * 129,), SENTINEL, device=dev)
        rc = lib.tdq_jet_hi_tile_fwd(_lib.ptr(X), n, _lib.ptr(P), d_in, w, d_out, 2, ci, cc, _lib.ptr(J), n, 0,
                                     _lib.ptr(Z), tile, st)
        assert rc != 0, name
        for part in (0, 1, 2):
            rc = lib.tdq_jet_hi_tile_bwd_part(_lib.ptr(X), n, _lib.ptr(P), d_in, w, d_out, 2, ci, cc, _lib.ptr(dJ), n,
                                              0, _lib.ptr(Z), _lib.ptr(work), _lib.ptr(grad), part, tile, st)
            assert rc != 0, (name, part)
        torch.cuda.synchronize()
        assert (J == SENTINEL).all() and (grad == SENTINEL).all(), name
