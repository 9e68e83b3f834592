"""Host side of the high-order jet kernels (``csrc/jet_hi.hip``).

A loss program whose callables need derivatives beyond the fused kernels' order 2 (the reference's
AC-baseline / AC-dist-new periodic BC on u_xxx and u_xxxx, ``examples/AC-baseline.py:23-29``)
keeps every point in the fused step: the fused jet kernels compute the order <= 2 streams of
ALL points, :class:`HiJetOp` computes the extra streams of the few high-order points into extra
rows of the same jet buffer ``J`` (the fused loss reads them like any other stream), and after the
loss the parameter gradient of their adjoints, which the fused step tail adds to theta's gradient.

A residual that itself takes a third or fourth derivative (KdV u_xxx, Kuramoto-Sivashinsky and beam
u_xxxx) makes every collocation point a high-order point: the same composition, with ``n_hi`` in the
tens of thousands.  The same kernel pair (``jet_hi_fwd_kernel`` / ``jet_hi_chain_kernel``) serves
both at 4, 8 or 16 points per workgroup; the large sets go through the tile entry points
(``tdq_jet_hi_tile_*``: scratch sized by the plan's stream count, weight-gradient splits that grow
with the point count; ``HiJetOp(tile=)``, ``AUTO_TILE_N``).

Stream table (``spec_i`` / ``spec_c``): the high-order plan's streams in canonical order with their
order / variable / output row, then the Faa di Bruno terms of every stream
(``jet.faa_terms``: tanh derivative order, coefficient, factor streams).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ..jet import faa_terms

MAX_S, MAX_T, MAX_W = 8, 48, 128

# Points per workgroup.  Tile 4 is for a few hundred boundary points; from AUTO_TILE_N points on (a
# KdV-type residual: the high-order points are the collocation set) the kernels serve 8 points per
# workgroup where that fits their LDS.  Below SMALL_N points ``tile=None`` always means the 4-point
# entry points (``tdq_jet_hi_*``), so every shape of before keeps its tile, scratch and splits.
# KdV Adam step on MI355X, bf16x3, tile 4 / 8 / 16 (profiles/r14_jet_hi_tile_sweep.jsonl; run range
# 0.03 ms): 2,048 points 0.218 / 0.205 / 0.286 ms, 5,000 0.413 / 0.395 / 0.490, 20,000 1.486 / 1.250 /
# 1.310, 50,000 3.497 / 2.928 / 3.104.  20,000 is the smallest swept size at which a larger tile wins
# by more than three run ranges; 16 points never beat 8 (its adjoint chain spills up to 95 VGPRs,
# profiles/r14_jet_hi_tile_resources.txt), so 16 stays a forced choice.
TILES = (8, 4)       # the automatic choice, largest first
SMALL_N = 2048
AUTO_TILE_N = 20000  # >= SMALL_N
DEFAULT_SCRATCH_CAP = 32 << 30


def scratch_cap():
    """Byte cap of the high-order scratch (``TDQ_HI_SCRATCH_BYTES``, default 32 GiB): a program whose
    high-order segments would need more keeps the torch jet backend."""
    import os
    return int(float(os.environ.get("TDQ_HI_SCRATCH_BYTES", DEFAULT_SCRATCH_CAP)))


def scratch_bytes(n_hi, n_hidden, S):
    """Bytes of the activation scratch (Z | H | B: three fp32 buffers of ``n_hidden x n_hi x streams x
    128``) that :class:`HiJetOp` allocates for ``n_hi`` points: the tile entry points size it by the
    plan's ``S``, the 4-point ones by ``MAX_S``."""
    streams = S if n_hi >= AUTO_TILE_N else MAX_S
    return 3 * n_hidden * int(n_hi) * streams * MAX_W * 4


def build_spec(plan_hi, out_rows):
    """``(spec_i, spec_c)`` lists for ``plan_hi``; ``out_rows[mi]`` = J row of stream ``mi`` (only the
    streams written / seeded by the kernels).  Raises ValueError outside the kernel's table limits."""
    streams = plan_hi.streams
    S = len(streams)
    if S > MAX_S:
        raise ValueError(f"high-order plan has {S} streams > {MAX_S}")
    idx = plan_hi.index
    order = [len(m) for m in streams]
    if max(order) > 4:
        raise ValueError("derivative order > 4")
    var = [m[0] if len(m) == 1 else 0 for m in streams]
    out = [int(out_rows.get(m, -1)) for m in streams]
    terms, coefs = [], []
    for s, mi in enumerate(streams):
        if s == 0:
            continue
        for k, blocks, c in faa_terms(mi):
            bl = [idx[b] for b in blocks]
            terms.append([s, k, len(bl)] + bl + [0] * (4 - len(bl)))
            coefs.append(float(c))
    if len(terms) > MAX_T:
        raise ValueError(f"{len(terms)} Faa di Bruno terms > {MAX_T}")
    spec_i = [S] + order + var + out + [len(terms)] + [v for t in terms for v in t]
    return spec_i, coefs


def eligible(net, plan_hi):
    """Whether the kernels take this network / high-order plan (split-bf16 MFMA layer GEMMs, widths <= 128)."""
    from ..models.networks import TanhMLP
    if not isinstance(net, TanhMLP):
        return False, "network is not a TanhMLP"
    sizes = net.layer_sizes
    if max(sizes[1:-1]) > MAX_W or sizes[0] > 8 or sizes[-1] > 4 or len(sizes) - 2 > 16:
        return False, "network outside the high-order kernel's envelope"
    try:
        build_spec(plan_hi, {})
    except ValueError as e:
        return False, str(e)
    try:
        lib = _lib.load()
    except _lib.NativeUnavailable:
        lib = None
    if lib is not None and not lib.tdq_jet_hi_lds_ok(len(plan_hi.streams), sizes[0], sizes[-1], len(sizes) - 2):
        return False, "streams x input / output width beyond the high-order kernels' LDS"
    return True, ""


class HiJetOp:
    """Extra (high-order) streams of the points ``[0, n_hi)`` of ``X_all``.

    ``rows``: J rows of the streams the kernels write (and whose adjoints they seed) - the
    high-order streams the fused kernels do not carry.  ``grad``: the parameter gradient of the
    last :meth:`backward` (persistent buffer: captured graphs replay the same pointers)."""

    def __init__(self, net, plan_hi, out_rows, X_all, n_hi, device, tile=None):
        """``tile``: points per workgroup - ``None`` picks by ``n_hi`` (the 4-point entry points below
        ``AUTO_TILE_N``, else the first of ``TILES`` that fits LDS, forward and adjoint chain each), ``4``
        forces the 4-point entry points, ``8`` / ``16`` those tiles through the tile entry points
        (ValueError if LDS cannot hold it).  :attr:`tile` / :attr:`tile_bwd`: what the forward / the chain run with;
        :attr:`entry`: ``"hi"`` (4-point entry points) or ``"hi_tile"``."""
        self.lib = _lib.load(required=True)
        self.net = net
        self.sizes = list(net.layer_sizes)
        self.widths = self.sizes[1:-1]
        self.n_hi = int(n_hi)
        self.X = X_all
        self.ldJ = X_all.shape[0]
        si, sc = build_spec(plan_hi, out_rows)
        self._si = (ctypes.c_int * len(si))(*si)
        self._sc = (ctypes.c_float * max(1, len(sc)))(*sc)
        self._w = (ctypes.c_int * len(self.widths))(*self.widths)
        self.S = si[0]
        self.tile, self.tile_bwd, self.entry = self._pick_tiles(tile)
        if self.entry == "hi":
            nz = self.lib.tdq_jet_hi_scratch_floats(self.n_hi, len(self.widths))
            nw = self.lib.tdq_jet_hi_work_floats(self.n_hi, self.sizes[0], self._w, self.sizes[-1], len(self.widths))
        else:
            nz = self.lib.tdq_jet_hi_tile_scratch_floats(self.n_hi, len(self.widths), self.S)
            nw = self.lib.tdq_jet_hi_tile_work_floats(self.n_hi, self.sizes[0], self._w, self.sizes[-1],
                                                      len(self.widths), self.tile_bwd)
        if nz < 0 or nw < 0:
            raise ValueError("high-order jet kernels cannot serve this network")
        self.Z = torch.empty(max(1, int(nz)), dtype=torch.float32, device=device)
        self.work = torch.empty(max(1, int(nw)), dtype=torch.float32, device=device)
        self.grad = torch.zeros(net.flat.numel(), dtype=torch.float32, device=device)

    def _pick_tiles(self, tile):
        """``(forward tile, chain tile, entry)``.  A pair ``(forward, chain)`` forces each."""
        geo = (self.S, self.sizes[0], self.sizes[-1], len(self.widths))
        fits = lambda t, chain: bool(self.lib.tdq_jet_hi_tile_ok(t, *geo, chain))
        if tile is None:
            if self.n_hi < max(SMALL_N, AUTO_TILE_N):
                return 4, 4, "hi"
            tf, tb = (next((t for t in TILES if fits(t, chain)), 4) for chain in (0, 1))
            return tf, tb, "hi_tile"
        pair = tuple(tile) if isinstance(tile, (tuple, list)) else (tile, tile)
        if len(pair) != 2 or any(t not in (4, 8, 16) for t in pair):
            raise ValueError(f"tile must be None, 4, 8 or 16 (or a pair of those), not {tile!r}")
        for chain, t in enumerate(pair):
            if not fits(t, chain):
                raise ValueError(f"high-order jet kernels: {t} points per workgroup with {self.S} streams do not "
                                 f"fit the LDS of the {'adjoint chain' if chain else 'forward'} on this network")
        return pair[0], pair[1], "hi" if pair == (4, 4) else "hi_tile"

    def _args(self):
        return (self.sizes[0], self._w, self.sizes[-1], len(self.widths), self._si, self._sc)

    def forward(self, J, P):
        """Extra stream rows of ``J`` (``(S_total, N, d_out)``, N = the X_all rows) for the high-order
        points, on the current stream."""
        if self.entry == "hi":
            rc = self.lib.tdq_jet_hi_fwd(_lib.ptr(self.X), self.n_hi, _lib.ptr(P), *self._args(), _lib.ptr(J), self.ldJ,
                                         0, _lib.ptr(self.Z), _lib.stream_ptr(self.X.device))
            _lib.check(rc, "tdq_jet_hi_fwd")
            return
        rc = self.lib.tdq_jet_hi_tile_fwd(_lib.ptr(self.X), self.n_hi, _lib.ptr(P), *self._args(), _lib.ptr(J),
                                          self.ldJ, 0, _lib.ptr(self.Z), self.tile, _lib.stream_ptr(self.X.device))
        _lib.check(rc, "tdq_jet_hi_tile_fwd")

    def backward(self, dJ, P, part=0):
        """Parameter gradient of the adjoints in the extra rows of ``dJ`` -> :attr:`grad`.  ``part``:
        0 everything; 1 the adjoint chain only; 2 the weight-gradient tiles + reduction only (after a
        part-1 call; ``dJ`` unused) - the halves may run on different graph branches."""
        if self.entry == "hi":
            rc = self.lib.tdq_jet_hi_bwd_part(_lib.ptr(self.X), self.n_hi, _lib.ptr(P), *self._args(), _lib.ptr(dJ),
                                              self.ldJ, 0, _lib.ptr(self.Z), _lib.ptr(self.work), _lib.ptr(self.grad),
                                              int(part), _lib.stream_ptr(self.X.device))
            _lib.check(rc, "tdq_jet_hi_bwd_part")
            return self.grad
        rc = self.lib.tdq_jet_hi_tile_bwd_part(_lib.ptr(self.X), self.n_hi, _lib.ptr(P), *self._args(), _lib.ptr(dJ),
                                               self.ldJ, 0, _lib.ptr(self.Z), _lib.ptr(self.work), _lib.ptr(self.grad),
                                               int(part), self.tile_bwd, _lib.stream_ptr(self.X.device))
        _lib.check(rc, "tdq_jet_hi_tile_bwd_part")
        return self.grad
