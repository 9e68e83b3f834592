"""R3 (retain-resample-release) resampling of the collocation points (Daw, Bu, Wang, Perdikaris and
Karpatne, ICML 2023, "Mitigating propagation failures in PINNs using retain-resample-release sampling").

After every loss pass, with ``a_i = sqrt(r2_i / c) = |f_i|`` from the adjoint ``r2_i = c f_i^2`` of a per-point
weight array of ones that every loss executor writes (``c``: the residual output's coefficient, ``1 / N_f``):

    tau = (1 / n) sum_i a_i                              (float64, fixed order)
    row i is retained iff a_i > tau                      (a tie, any NaN and a lone point release)
    a released row: x_ij = float32(lo_j + u * (hi_j - lo_j)),  u = (w >> 8) * 2^-24,
        w = word j % 4 of Philox4x32-10(counter (i, j // 4, step_lo, step_hi), key (seed_lo, seed_hi))

in float64 with the multiply and the add rounded separately.  Rows keep their place and retained rows are
not written; the step counter advances by one per update.

* :class:`R3Op` - owns the box, the seed, the device counter, ``stats = {tau, step used}``, the released
  counts, the work buffer and the destinations (the residual rows of ``LossProgram.X_all`` and, where the
  program has a one-launch step, of ``FusedStepOp.X``); :meth:`R3Op.update` launches ``tdq_r3_resample``
  (csrc/r3.hip) on the current stream, so it is a node of a captured step.
* :func:`r3_update_torch` - the mirror with the same contract and the same bits in the written rows: the
  CPU and torch-jet paths, and the GPU with ``TDQ_R3_KERNEL=0``.  Tensor ops only (no host read), so it can
  be captured too.
"""
from __future__ import annotations

import os

import torch

MAX_DIN = 8
BLOCK = 256
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def kernel_enabled():
    """``TDQ_R3_KERNEL=0`` keeps the update on the torch mirror on a GPU (the A/B and fallback switch of
    tools/r3_timing.py); on by default."""
    return os.environ.get("TDQ_R3_KERNEL", "1") != "0"


def _mulhilo(m, x):
    """``(hi, lo)`` 32-bit halves of ``m * x`` for a 32-bit constant ``m`` and an int64 tensor ``x`` of
    32-bit values: ``x`` goes in two 16-bit halves, so every product stays below 2^48."""
    p_lo = m * (x & 0xFFFF)
    p_hi = m * (x >> 16)
    lo = (((p_hi & 0xFFFF) << 16) + p_lo) & _MASK
    hi = (p_hi + (p_lo >> 16)) >> 16
    return hi, lo


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror and Shaw, SC 2011; the Random123 constants) on int64 tensors
    that hold 32-bit words: ``counter`` four tensors, ``key`` two (tensors or ints), broadcast together.
    Returns the four output words.  Integer tensor ops only, exact on every device."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def r3_update_torch(r2, inv_c, box, state, seed, dests, stats, counts):
    """The mirror of ``tdq_r3_resample``.  ``r2`` ``(n,)`` / ``(n, 1)`` float32; ``box`` ``(d_in, 2)`` float64
    (``lo_j, hi_j``); ``state`` the 0-dim int64 step counter (advanced in place); ``seed`` a Python int (64
    bit); ``dests`` the ``(n, d_in)`` float32 views that receive the released rows; ``stats`` ``(2,)`` float64
    and ``counts`` ``(ceil(n / 256),)`` int32 as the kernel writes them."""
    r2 = r2.detach().reshape(-1)
    n, dev = r2.numel(), r2.device
    d_in = box.shape[0]
    a = torch.sqrt(r2.double() * float(inv_c))
    tau = a.sum() / n
    released = ~(a > tau)
    step = state.detach().reshape(())
    i = torch.arange(n, dtype=torch.int64, device=dev)
    zero = torch.zeros_like(i)
    s_lo, s_hi = zero + (step & _MASK), zero + ((step >> 32) & _MASK)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = []
    for blk in range((d_in + 3) // 4):
        words.extend(philox4x32_10((i, zero + blk, s_lo, s_hi), (seed & _MASK, seed >> 32)))
    lo, hi = box[:, 0].double(), box[:, 1].double()
    u = (torch.stack(words[:d_in], dim=1) >> 8).double() * 2.0 ** -24
    prod = u * (hi - lo)
    x = (lo + prod).float()
    pad = (-n) % BLOCK
    rel = torch.cat([released, released.new_zeros(pad)]) if pad else released
    with torch.no_grad():
        for X in dests:
            X.copy_(torch.where(released[:, None], x, X))
        counts.copy_(rel.reshape(-1, BLOCK).sum(1))
        stats[0] = tau
        stats[1] = step.double()
        state.add_(1)
    return dests[0]


class R3Op:
    """The R3 update of one loss program.  ``prog``: the finalized program; ``fop``: its
    :class:`~.loss_fused.FusedLossOp` or None (then :meth:`update` takes the adjoint from autograd);
    ``box``: ``[(lo_j, hi_j)]`` of the input variables; ``state``: the 0-dim int64 device counter (the
    solver's, shared by every op it builds); ``dests``: ``[(tensor, first row)]`` - the tensors whose rows
    ``first + i`` hold the residual points, the first one being ``prog.X_all``; ``lam_index``: the index of
    the array of ones in the solver's lambda list; ``inv_c``: ``1 / c`` of the residual output."""

    def __init__(self, prog, fop, n, box, seed, state, dests, device, lam_index, inv_c):
        self.prog, self.fop = prog, fop
        self.device = dev = torch.device(device)
        self.n, self.d_in = int(n), len(box)
        if self.n < 1:
            raise ValueError("R3 resampling: no residual points")
        if not 1 <= self.d_in <= MAX_DIN:
            raise ValueError(f"R3 resampling: {self.d_in} input variables outside 1..{MAX_DIN}")
        self.box = torch.tensor([[float(lo), float(hi)] for lo, hi in box], dtype=torch.float64, device=dev)
        if not bool(torch.isfinite(self.box).all()) or bool((self.box[:, 1] < self.box[:, 0]).any()):
            raise ValueError(f"R3 resampling: the box {box} is not finite and ordered")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if state.dtype != torch.int64 or state.numel() != 1 or state.device.type != dev.type:
            raise ValueError("R3 resampling: the step counter must be one int64 element on the op's device")
        self.state = state
        self.lam_index, self.inv_c = int(lam_index), float(inv_c)
        self.slot = None if fop is None else fop.fl.lam_slots.index(self.lam_index)
        self.dests = []
        for X, first in dests:
            first = int(first)
            if X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] < self.d_in or not X.is_contiguous() \
                    or first < 0 or first + self.n > X.shape[0] or X.device.type != dev.type:
                raise ValueError(f"R3 resampling: destination {tuple(X.shape)} {X.dtype} cannot hold rows "
                                 f"[{first}, {first + self.n}) of {self.d_in} coordinates")
            self.dests.append((X, first))
        if not 1 <= len(self.dests) <= 2:
            raise ValueError(f"R3 resampling: {len(self.dests)} destinations (one or two)")
        self.stats = torch.zeros(2, dtype=torch.float64, device=dev)
        self.counts = torch.zeros((self.n + BLOCK - 1) // BLOCK, dtype=torch.int32, device=dev)
        self.hip = dev.type == "cuda" and kernel_enabled()
        self.work = None
        if self.hip:
            from . import _lib
            lib = _lib.load(required=True)
            self.work = torch.zeros(lib.tdq_r3_work_doubles(self.n), dtype=torch.float64, device=dev)
            if lib.tdq_r3_count_ints(self.n) != self.counts.numel():
                raise RuntimeError("R3 resampling: the library's workgroup count differs from ops/r3.py's")

    def views(self):
        """The ``(n, d_in)`` views of the destinations' residual rows."""
        return [X[first:first + self.n, :self.d_in] for X, first in self.dests]

    def points(self):
        """The current population, an ``(n, d_in)`` view of the first destination."""
        return self.views()[0]

    def update(self, r2):
        """One R3 update from ``r2 = c f^2`` (``(n,)`` or ``(n, 1)`` float32), on the current stream."""
        if r2.numel() != self.n or r2.dtype != torch.float32 or not r2.is_contiguous():
            raise ValueError(f"R3 resampling: r2 must be a contiguous float32 tensor of {self.n} elements, "
                             f"got {tuple(r2.shape)} {r2.dtype}")
        if not self.hip:
            return r3_update_torch(r2, self.inv_c, self.box, self.state, self.seed, self.views(), self.stats,
                                   self.counts)
        (X, first), second = self.dests[0], (self.dests[1] if len(self.dests) > 1 else (None, 0))
        return r3_resample(r2, self.inv_c, self.box, self.state, self.seed, X, first, second[0], second[1], self.n,
                           self.d_in, self.work, self.stats, self.counts)

    def read_stats(self):
        """``{"step", "released", "threshold"}``: the counter, and the released count and ``tau`` of the
        last update (a host read)."""
        return {"step": int(self.state), "released": int(self.counts.sum()), "threshold": float(self.stats[0])}


def r3_resample(r2, inv_c, box, state, seed, X, first, X2, first2, n, d_in, work, stats, counts):
    """``tdq_r3_resample`` (csrc/r3.hip) on the current stream: rows ``first + i`` of ``X`` and, with ``X2``
    not None, rows ``first2 + i`` of ``X2``.  The kernel trusts the extents of its arrays, so they are
    checked here; it refuses bad geometry (``n < 1``, ``d_in`` outside 1..8, a row stride below ``d_in``, a
    null pointer) itself, before any launch, with a ``RuntimeError`` here."""
    from . import _lib
    lib = _lib.load(required=True)
    n, d_in, first, first2 = int(n), int(d_in), int(first), int(first2)
    nw, nc = lib.tdq_r3_work_doubles(n), lib.tdq_r3_count_ints(n)
    for name, t, dt, size in (("r2", r2, torch.float32, n), ("box", box, torch.float64, 2 * d_in),
                              ("state", state, torch.int64, 1), ("work", work, torch.float64, nw),
                              ("stats", stats, torch.float64, 2), ("counts", counts, torch.int32, nc)):
        if t.dtype != dt or t.numel() < size or not t.is_contiguous() or not t.is_cuda or (
                name in ("r2", "box", "state") and t.numel() != size):
            raise ValueError(f"tdq_r3_resample: {name} must be a contiguous {dt} device tensor of {size} elements, "
                             f"got {tuple(t.shape)} {t.dtype}")
    for name, t, f in (("X", X, first), ("X2", X2, first2)):
        if t is None and name == "X2":
            continue
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda or f < 0 \
                or f + n > t.shape[0]:
            raise ValueError(f"tdq_r3_resample: {name} must be a contiguous float32 device matrix with rows "
                             f"[{f}, {f + n}), got {tuple(t.shape)} {t.dtype}")
    ld, ld2 = X.shape[1], (X2.shape[1] if X2 is not None else 0)
    esz = X.element_size()
    import ctypes
    xp = ctypes.c_void_p(X.data_ptr() + first * ld * esz)
    rc = lib.tdq_r3_resample(_lib.ptr(r2), float(inv_c), _lib.ptr(box), _lib.ptr(state),
                             int(seed) & 0xFFFFFFFFFFFFFFFF, xp, int(ld), _lib.ptr(X2), int(ld2), first2, n, d_in,
                             _lib.ptr(work), _lib.ptr(stats), _lib.ptr(counts), _lib.stream_ptr(r2.device))
    _lib.check(rc, "tdq_r3_resample")
    return X
