"""Temporal causality weights of the collocation points (Wang, Sankaran and Perdikaris, arXiv 2203.07404).

With the points binned by their time coordinate into ``M`` slabs of ``[t0, t1]``,
``bin(i) = min(M - 1, floor((t_i - t0) / (t1 - t0) * M))``:

    L_b = (1 / n_b) sum_{i in b} f_i^2                 (0 for an empty bin)
    W_b = exp(-eps * sum_{b' < b} L_b')                (W_0 = 1)
    lambda_i = W_bin(i)

The residual term of the loss is ``(1 / N_f) sum_i lambda_i f_i^2`` (``g_MSE`` with the identity ``g``).  No
gradient flows through the weights and no optimizer owns them: they are overwritten in place after every
loss pass, from the adjoint ``r2_i = c f_i^2`` of the weight array that every loss executor writes (``c``: the
residual output's coefficient, ``1 / N_f``).

* :class:`CausalOp` - owns the bin layout (``order``, ``bin_start``), the device scalar ``eps``, the bin
  weights ``w_bins`` and ``stats = {min_b W_b, sum_b L_b}``; :meth:`CausalOp.update` launches
  ``tdq_causal_update`` (csrc/causal.hip) on the current stream, so it is a node of a captured step.
* :func:`causal_update_torch` - the mirror with the same contract (double sums, float ``exp``): the CPU
  and torch-jet paths, and the GPU with ``TDQ_CAUSAL_KERNEL=0``.
"""
from __future__ import annotations

import os

import torch

MAX_BINS = 1024


def kernel_enabled():
    """``TDQ_CAUSAL_KERNEL=0`` keeps the update on the torch mirror on a GPU (the A/B and fallback switch
    of tools/causal_timing.py); on by default."""
    return os.environ.get("TDQ_CAUSAL_KERNEL", "1") != "0"


def bin_index(t, t0, t1, bins):
    """``bin(i) = min(M - 1, floor((t_i - t0) / (t1 - t0) * M))`` in float64, clamped to ``[0, M - 1]``."""
    t = torch.as_tensor(t).detach().reshape(-1).double().cpu()
    if not t1 > t0:
        raise ValueError(f"causal weights: empty time range [{t0}, {t1}]")
    b = torch.floor((t - float(t0)) / (float(t1) - float(t0)) * int(bins)).to(torch.int64)
    return b.clamp_(0, int(bins) - 1)


def bin_layout(bins_of, M):
    """``(order, bin_start)``: the stable permutation that sorts the points by bin (int32, ``n``) and
    the ``M + 1`` offsets of the bins in it (int32)."""
    order = torch.sort(bins_of, stable=True).indices.to(torch.int32)
    counts = torch.bincount(bins_of, minlength=M)[:M]
    start = torch.zeros(M + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(counts, 0)
    return order, start.to(torch.int32)


def causal_update_torch(r2, inv_c, order, bin_start, eps, lam, w_bins, stats):
    """The mirror of ``tdq_causal_update``: bin sums and the scan in float64 (fixed order),
    ``W_b = exp(float32(-eps * cum_b))`` in float32; writes ``lam[order[j]] = W_bin(j)``, ``w_bins`` and
    ``stats = {min W, sum_b L_b}`` in place.  ``eps``: a 0-dim float32 tensor."""
    M = bin_start.numel() - 1
    n = order.numel()
    idx = order.long()
    start = bin_start.long()
    counts = start[1:] - start[:-1]
    binj = torch.repeat_interleave(torch.arange(M, device=r2.device), counts, output_size=n)
    v = r2.detach().reshape(-1)[idx].double()
    sums = torch.zeros(M, dtype=torch.float64, device=r2.device).index_add_(0, binj, v)
    mean = torch.where(counts > 0, sums * float(inv_c) / counts.clamp(min=1).double(), torch.zeros_like(sums))
    cum = torch.cumsum(mean, 0) - mean
    W = torch.exp((-eps.detach().double() * cum).float())
    with torch.no_grad():
        w_bins.copy_(W)
        lam.reshape(-1)[idx] = W[binj]
        stats[0] = W.min()
        stats[1] = mean.sum().float()
    return lam


class CausalOp:
    """The causal weights of one loss program.  ``prog``: the finalized program; ``fop``: its
    :class:`~.loss_fused.FusedLossOp` or None (then :meth:`update` takes the adjoint from autograd);
    ``t_column``: the time coordinate of the residual points ``(n,)``; ``t_range``: ``(t0, t1)`` of the
    domain; ``eps_list``: the increasing eps schedule; ``lam``: the ``(n, 1)`` weight array, ``lam_index``
    its index in the solver's lambda list; ``inv_c``: ``1 / c`` of the residual output."""

    def __init__(self, prog, fop, t_column, t_range, bins, eps_list, device, lam, lam_index, inv_c):
        bins = int(bins)
        if not 1 <= bins <= MAX_BINS:
            raise ValueError(f"causal weights: {bins} bins outside 1..{MAX_BINS}")
        self.prog, self.fop, self.bins = prog, fop, bins
        self.device = dev = torch.device(device)
        self.eps_list = [float(e) for e in eps_list]
        self.lam, self.lam_index, self.inv_c = lam, int(lam_index), float(inv_c)
        n = lam.numel()
        bins_of = bin_index(t_column, t_range[0], t_range[1], bins)
        if bins_of.numel() != n:
            raise ValueError(f"causal weights: {bins_of.numel()} time coordinates for {n} weights")
        order, start = bin_layout(bins_of, bins)
        self.bin_start_host = start.contiguous()           # the entry point checks the host copy
        self.order, self.bin_start = order.to(dev), start.to(dev)
        self.eps_index = 0
        self.eps = torch.full((), self.eps_list[0], dtype=torch.float32, device=dev)
        self.w_bins = torch.ones(bins, dtype=torch.float32, device=dev)
        self.stats = torch.tensor([1.0, 0.0], dtype=torch.float32, device=dev)
        self.slot = None if fop is None else fop.fl.lam_slots.index(self.lam_index)
        self.hip = dev.type == "cuda" and kernel_enabled()
        self.work = None
        if self.hip:
            from . import _lib
            lib = _lib.load(required=True)
            self.work = torch.zeros(lib.tdq_causal_work_doubles(bins), dtype=torch.float64, device=dev)

    def set_eps(self, index):
        """Write schedule entry ``index`` into the device scalar (in place: captured steps stay valid)."""
        self.eps_index = int(index)
        self.eps.fill_(self.eps_list[self.eps_index])

    def update(self, r2):
        """``lam <- W_bin`` from ``r2 = c f^2`` (``(n,)`` or ``(n, 1)`` float32), on the current stream."""
        if r2.numel() != self.lam.numel() or r2.dtype != torch.float32 or not r2.is_contiguous():
            raise ValueError(f"causal weights: r2 must be a contiguous float32 tensor of {self.lam.numel()} elements, "
                             f"got {tuple(r2.shape)} {r2.dtype}")
        if not self.hip:
            return causal_update_torch(r2, self.inv_c, self.order, self.bin_start, self.eps, self.lam, self.w_bins,
                                       self.stats)
        return causal_update(r2, self.inv_c, self.order, self.bin_start, self.bin_start_host, self.eps, self.work,
                             self.lam, self.w_bins, self.stats)

    def min_weight(self):
        """``min_b W_b`` of the last update (a host read)."""
        return float(self.stats[0])


def causal_update(r2, inv_c, order, bin_start, bin_start_host, eps, work, lam, w_bins, stats):
    """``tdq_causal_update`` (csrc/causal.hip) on the current stream.  The kernel trusts the extents of
    its arrays, so they are checked here; it refuses bad geometry (bins outside 1..1024, a
    non-monotone ``bin_start``) itself, before any launch, with a ``RuntimeError`` here."""
    from . import _lib
    M, n = bin_start_host.numel() - 1, order.numel()
    for name, t, dt, size in (("r2", r2, torch.float32, n), ("order", order, torch.int32, n),
                              ("bin_start", bin_start, torch.int32, M + 1), ("eps", eps, torch.float32, 1),
                              ("work", work, torch.float64, max(1, M)), ("lam", lam, torch.float32, n),
                              ("w_bins", w_bins, torch.float32, M), ("stats", stats, torch.float32, 2)):
        if t.dtype != dt or t.numel() < size or not t.is_contiguous() or not t.is_cuda or (
                name in ("r2", "order", "lam", "bin_start", "w_bins") and t.numel() != size):
            raise ValueError(f"tdq_causal_update: {name} must be a contiguous {dt} device tensor of {size} elements, "
                             f"got {tuple(t.shape)} {t.dtype}")
    if bin_start_host.dtype != torch.int32 or bin_start_host.is_cuda or not bin_start_host.is_contiguous():
        raise ValueError("tdq_causal_update: bin_start_host must be a contiguous int32 CPU tensor")
    rc = _lib.load(required=True).tdq_causal_update(
        _lib.ptr(r2), float(inv_c), _lib.ptr(order), _lib.ptr(bin_start), _lib.ptr(bin_start_host), int(M), int(n),
        _lib.ptr(eps), _lib.ptr(work), _lib.ptr(lam), _lib.ptr(w_bins), _lib.ptr(stats), _lib.stream_ptr(r2.device))
    _lib.check(rc, "tdq_causal_update")
    return lam
