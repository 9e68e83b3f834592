"""NTK traces of a loss program: ``T_k = sum_{outputs o of term k} c_o sum_i ||d f_{o,i} / d theta||^2``.

The traced loss program (:func:`tensordiffeq_amd.fusion.build`) defines the loss as the sum over
groups and outputs ``(f, w, term, c)`` of ``c w sum_i f_i^2``; the trace of a term is that sum with
``f^2`` replaced by the squared parameter-gradient norm of ``f`` and ``w = 1``.  With equal batch sizes
it is proportional to ``Tr(K_kk)`` of Wang, Yu and Perdikaris (arXiv 2007.14527, Algorithm 1), whose
weights are ``lambda_k = sum_j T_j / T_k`` (:func:`weights`).

The per-instance norm is never taken from a materialised gradient.  With the rows ``r = (point,
stream)`` of an instance, ``Z_l[r]`` the adjoint of layer ``l``'s pre-activation stream and
``H_{l-1}[r]`` the activation stream below it (the input jets at layer 0), layer ``l``'s weight gradient
is ``sum_r H[r] Z[r]^T``, so

    ||d f / d theta||^2 = sum_l [ sum_{r, r'} (Z_l[r] . Z_l[r']) (H_{l-1}[r] . H_{l-1}[r'])
                                  + ||sum_{value rows} Z_l[r]||^2 ]

* :class:`NTKTraceOp` - the HIP path: per group chunk one exact-fp32 forward (``tdq_jet_fwd``), per
  output the seed launch (``tdq_loss_seed``: ``d f_o / d J`` from the loss interpreter) and the norm
  launch (``tdq_ntk_norm``, csrc/ntk_trace.hip), then a fixed-order sum.
* :class:`LayeredNTKOp` - the HIP path beyond that kernel's register envelope (5-8 streams at width 128,
  unequal widths): the layer-wise engine's fp32 forward and adjoints-only pass, then per dense layer one
  Gram-product launch (``tdq_ntk_gram``, csrc/ntk_gram.hip) on the ``(H_{l-1}, Z_l)`` planes.
* :class:`TorchNTK` - the same formula on the torch jet (CPU, ``backend="jet"``, and any plan or
  network outside the HIP envelope): the adjoints ``Z`` of all instances come from ONE reverse pass per
  output, because an instance's ``f`` only reads its own rows.
"""
from __future__ import annotations

import ctypes

import torch

from .. import fusion
from ..jet import JetPlan, _tanh_jet

CHUNK = 65536         # points per forward of the HIP path (the saved streams are ~8 KB per point)
TORCH_CHUNK = 8192    # instances per pass of the torch path


def outputs(fl):
    """``[(group index, output index in the group, term index, c)]`` in program order."""
    return [(gi, oi, t, c) for gi, gr in enumerate(fl.groups) for oi, (_, _, t, c) in enumerate(gr.program.outputs)]


def weights(T, prev):
    """``lambda_k = sum_j T_j / T_k`` over the usable traces (finite and > 0); a term with an unusable
    trace keeps ``prev[k]``.  Returns ``(lambdas, usable mask)`` (float64 tensors on the CPU)."""
    T = torch.as_tensor(T, dtype=torch.float64).cpu()
    prev = torch.as_tensor(prev, dtype=torch.float64).cpu()
    ok = torch.isfinite(T) & (T > 0)
    total = T[ok].sum()
    return torch.where(ok, total / torch.where(ok, T, torch.ones_like(T)), prev), ok


# ------------------------------------------------------------------------------------------
# torch path
# ------------------------------------------------------------------------------------------
def _tapped_jet(X, weights_, plan):
    """The torch jet of :func:`tensordiffeq_amd.jet.jet_forward` with every dense layer tapped:
    returns ``(z_out, taps)``, ``z_out[mi]`` the output stream ``(N, d_out)`` or None (identically 0)
    and ``taps = [(H, Z)]`` per dense layer, dicts stream -> ``(N, in)`` input / ``(N, out)``
    pre-activation.  Every ``Z`` tensor takes a gradient: d(sum_i f_i)/dZ holds every point's adjoint."""
    streams = plan.streams
    N = X.shape[0]
    eye = torch.eye(X.shape[1], dtype=X.dtype, device=X.device)
    h = {(): X}
    for mi in streams[1:]:
        h[mi] = eye[mi[0]].expand(N, -1) if len(mi) == 1 else None
    taps, z = [], None
    for li, (K, b) in enumerate(weights_):
        if li > 0:
            h = _tanh_jet(z, streams, plan.order)
        z, H, Z = {}, {}, {}
        for mi in streams:
            hm = h[mi]
            if hm is None:
                z[mi] = None
                continue
            zm = torch.addmm(b, hm, K) if mi == () else hm @ K
            if not zm.requires_grad:
                zm.requires_grad_(True)
            z[mi], H[mi], Z[mi] = zm, hm, zm
        taps.append((H, Z))
    return z, taps


def _gram_norms(taps, grads, m, slots):
    """Per-instance squared gradient norm from the tapped streams: instance ``i`` owns the points
    ``i + k m`` (slot ``k``) of the tapped point list."""
    total = None
    for (H, Z), g in zip(taps, grads):
        mis = [mi for mi in Z if g.get(mi) is not None]
        if not mis:
            continue

        def rows(d):  # (m, slots * len(mis), features)
            return torch.stack([d[mi].reshape(slots, m, -1) for mi in mis], dim=1).flatten(0, 1).transpose(0, 1)

        Zr, Hr = rows(g), rows(H)
        term = ((Zr @ Zr.transpose(1, 2)) * (Hr @ Hr.transpose(1, 2))).sum((1, 2))
        if () in g and g[()] is not None:
            term = term + g[()].reshape(slots, m, -1).sum(0).square().sum(1)
        total = term if total is None else total + term
    return total


class TorchNTK:
    """Exact traces on the torch jet: any plan the torch jet serves (high-order streams, wide or
    unequal networks), CPU or GPU."""

    kind = "torch"

    def __init__(self, prog, fl, lambdas, chunk=TORCH_CHUNK):
        self.prog, self.fl, self.lambdas, self.chunk = prog, fl, lambdas, int(chunk)
        idx, _ = prog.fused_streams()
        self.row_mi = {row: mi for mi, row in idx.items()}
        self.plan = JetPlan(set(idx) - {()}, prog.d_in)
        self.norms = {}

    def _group(self, gi, params, want):
        """``{output index: per-instance norms (n,)}`` of group ``gi`` for the outputs in ``want``."""
        prog, fl = self.prog, self.fl
        gr = fl.groups[gi]
        P = gr.program
        dt, dev = params.dtype, params.device
        W = [(k.detach(), b.detach()) for k, b in prog.net.weights(params)]
        offs = [prog.segments[s].offset for s in gr.segs]
        res = {oi: [] for oi in want}
        scalars = fusion.scalar_values(fl, self.lambdas, None)
        for lo in range(0, gr.n, self.chunk):
            hi = min(gr.n, lo + self.chunk)
            m = hi - lo
            X = torch.cat([prog.X_all[o + lo:o + hi] for o in offs], dim=0).to(dt)
            with torch.enable_grad():
                z, taps = _tapped_jet(X, W, self.plan)

                def stream(a, row, col):
                    v = z[self.row_mi[row]]
                    return X.new_zeros(m) if v is None else v[a * m:(a + 1) * m, col]

                def lam(a):
                    k = fl.lam_slots[a]
                    o = fl.lam_offsets.get(k, (0, 0))[0]
                    return self.lambdas[k].detach().reshape(-1)[o + lo:o + hi].to(dt)

                vals = fusion.eval_group(P, m, stream, lambda a, j: X[a * m:(a + 1) * m, j],
                                         lambda a: fl.val_arrays[a].to(dev)[lo:hi].to(dt), lam,
                                         lambda a: scalars[a].detach().to(dt), dev, dt)
                flat = [zt for _, Z in taps for zt in Z.values()]
                for oi in want:
                    f = vals[P.outputs[oi][0]]
                    if not f.requires_grad:      # an output that does not read the network
                        res[oi].append(X.new_zeros(m))
                        continue
                    gs = iter(torch.autograd.grad(f.sum(), flat, retain_graph=True, allow_unused=True))
                    grads = [{mi: next(gs) for mi in Z} for _, Z in taps]
                    res[oi].append(_gram_norms(taps, grads, m, len(offs)).detach())
        return {oi: torch.cat(v) if v else torch.zeros(0, dtype=dt, device=dev) for oi, v in res.items()}

    def traces(self, params=None):
        """``T`` ``(n_terms,)`` at ``params`` (default: the network's flat fp32 vector; a float64 vector
        evaluates everything in float64)."""
        prog, fl = self.prog, self.fl
        params = prog.net.flat.detach() if params is None else params.detach()
        T = torch.zeros(len(fl.term_names), dtype=params.dtype, device=params.device)
        self.norms = {}
        for gi, gr in enumerate(fl.groups):
            got = self._group(gi, params, range(len(gr.program.outputs)))
            for oi, (_, _, t, c) in enumerate(gr.program.outputs):
                self.norms[(gi, oi)] = got[oi]
                T[t] = T[t] + c * got[oi].sum()
        return T

    def instance_norms(self, gi, oi):
        """Per-instance norms of output ``oi`` of group ``gi`` from the last :meth:`traces` call (the
        diagonal of that output's NTK block)."""
        return self.norms[(gi, oi)]


# ------------------------------------------------------------------------------------------
# HIP path
# ------------------------------------------------------------------------------------------
def hip_reason(prog):
    """None when :class:`NTKTraceOp` serves the program, else why not (the exact-fp32 kernels' envelope:
    order <= 2, equal widths <= 128, streams x width tiles <= 32, d_in <= 8, d_out <= 4)."""
    from .jet_hip import is_layered
    from .jet_mlp import hip_config
    if prog.device.type != "cuda" or prog.backend != "hip":
        return "the program does not run on the HIP backend"
    if prog.fused_op is None:
        return "the loss program is not fused"
    if prog.mixed:
        return f"derivative order {prog.plan_hi.order} > 2"
    try:
        cfg = hip_config(prog.net, prog.plan, "fp32")
    except ValueError as e:
        return str(e)
    if is_layered(cfg):
        return cfg["why"]
    if cfg["precision"] != "fp32":
        return f"no exact-fp32 kernels for {cfg}"
    return None


def pad_kp(P, cfg, Kp=None):
    """The zero-padded ``[in][out]`` images of the hidden kernels (``tdq_jet_pad_kp``) in ``Kp``."""
    from . import _lib
    W = 16 * cfg["WT"]
    if Kp is None:
        Kp = torch.zeros(max(1, (cfg["n_hidden"] - 1) * W * W), device=P.device)
    _lib.check(_lib.load().tdq_jet_pad_kp(_lib.ptr(P), _lib.ptr(Kp), cfg["d_in"], cfg["width"], cfg["d_out"],
                                          cfg["n_hidden"], _lib.stream_ptr(P.device)), "tdq_jet_pad_kp")
    return Kp


def instance_norms(saved, dJ, Kp, n_inst, offA=0, offB=None, out=None):
    """``n2[i] = ||d (sum_{s,q} dJ[s, n, q] J[s, n, q]) / d theta||^2`` over the points ``n`` of instance
    ``i < n_inst`` (``tdq_ntk_norm``): point ``offA + i``, or the pair ``(offA + i, offB + i)``.  ``saved``:
    an exact-fp32 :func:`~.jet_hip.forward_raw` over the ``N`` points; ``dJ``: ``(S, N, d_out)``."""
    from . import _lib
    X, P, scratch, cfg, spec, S = saved
    N = X.shape[0]
    if cfg["precision"] != "fp32" or cfg.get("engine") == "layered":
        raise ValueError("the NTK norm kernel reads the saved streams of the exact-fp32 jet forward")
    if tuple(dJ.shape) != (S, N, cfg["d_out"]) or not dJ.is_contiguous() or dJ.dtype != torch.float32:
        raise ValueError(f"dJ must be a contiguous float32 ({S}, {N}, {cfg['d_out']}) tensor, got {tuple(dJ.shape)}")
    if out is None:
        out = torch.zeros(n_inst, device=X.device)
    spec_c = (ctypes.c_int * len(spec))(*spec)
    rc = _lib.load().tdq_ntk_norm(_lib.ptr(X), _lib.ptr(P), _lib.ptr(Kp), _lib.ptr(dJ), _lib.ptr(scratch),
                                  _lib.ptr(out), N, int(offA), -1 if offB is None else int(offB), int(n_inst),
                                  cfg["d_in"], cfg["width"], cfg["d_out"], cfg["n_hidden"], S, spec_c,
                                  _lib.stream_ptr(X.device))
    _lib.check(rc, "tdq_ntk_norm")
    return out


def seeds(fop, gi, oi, J, X, dJ, lo, m, seg_off):
    """``dJ = d f_o / d J`` for the instances ``[lo, lo + m)`` of group ``gi``, output ``oi`` of its program
    (``tdq_loss_seed``, the loss interpreter's seed mode).  ``J`` / ``dJ`` ``(S, N, d_out)`` and ``X``
    ``(N, d_in)`` hold ``N`` points of which slot ``k``'s instance ``i`` is point ``seg_off[k] + i``; the entries
    of those points that the program does not read are zeroed, other points are not touched."""
    from . import _lib
    gr = fop.fl.groups[gi]
    S, N, d_out = J.shape
    if tuple(dJ.shape) != (S, N, d_out) or not (J.is_contiguous() and dJ.is_contiguous() and X.is_contiguous()):
        raise ValueError("seeds: J and dJ must be contiguous (S, N, d_out) tensors of one shape")
    off = list(seg_off) + [0] * (2 - len(seg_off))
    rc = _lib.load().tdq_loss_seed(_lib.ptr(fop.code), _lib.ptr(fop.consts), _lib.ptr(fop.outs), _lib.ptr(fop.groups),
                                   _lib.ptr(fop.ptrs), fop.n_groups, S, X.shape[1], N, d_out, _lib.ptr(J), _lib.ptr(X),
                                   _lib.ptr(dJ), int(gi), int(oi), int(lo), int(m), int(off[0]), int(off[1]), gr.n,
                                   len(gr.segs), len(gr.program.outputs), gr.program.n_regs,
                                   _lib.stream_ptr(J.device))
    _lib.check(rc, "tdq_loss_seed")
    return dJ


class NTKTraceOp:
    """Traces on the HIP kernels.  ``fop``: the program's :class:`~.loss_fused.FusedLossOp` (its
    bytecode tables feed the seed launches).  Persistent buffers: the seeds ``dJ``, the padded weight
    images, the per-instance norms of every output and the per-launch sums; the traces always run the
    exact-fp32 kernels on the fp32 parameter vector, whatever precision the solver trains in.

    The residual set is processed in chunks of at most ``chunk`` points: every launch group is a
    contiguous instance range of one loss group, forwarded on its own point list (a periodic group's upper
    points, then its lower points)."""

    kind = "hip"

    def __init__(self, prog, fop, chunk=CHUNK):
        from . import _lib
        from .jet_mlp import hip_config
        why = hip_reason(prog)
        if why is not None:
            raise ValueError(f"NTK trace kernels cannot serve this program: {why}")
        self.prog, self.fop, self.fl = prog, fop, fop.fl
        self.lib = _lib.load()
        self.cfg = cfg = hip_config(prog.net, prog.plan, "fp32")
        self.S = prog.plan.S
        dev = prog.device
        self.outputs = outputs(self.fl)
        self.launches = []   # (group, lo, m, slots) per forward
        for gi, gr in enumerate(self.fl.groups):
            step = max(1, int(chunk) // len(gr.segs))
            self.launches += [(gi, lo, min(gr.n, lo + step) - lo, len(gr.segs)) for lo in range(0, gr.n, step)]
        n_max = max((m * k for _, _, m, k in self.launches), default=1)
        W = 16 * cfg["WT"]
        self.dJ = torch.zeros(self.S * n_max * cfg["d_out"], device=dev)
        self.Kp = torch.zeros(max(1, (cfg["n_hidden"] - 1) * W * W), device=dev)
        self.norms = {(gi, oi): torch.zeros(self.fl.groups[gi].n, device=dev) for gi, oi, _, _ in self.outputs}
        n_sums = sum(len(self.fl.groups[gi].program.outputs) for gi, _, _, _ in self.launches)
        self.sums = torch.zeros(max(1, n_sums), device=dev)
        self.T = torch.zeros(len(self.fl.term_names), device=dev)
        # T[t] = sum_k coef[t, k] sums[k]: every sum's coefficient in its term's row
        coef = torch.zeros(len(self.fl.term_names), max(1, n_sums))
        k = 0
        for gi, _, _, _ in self.launches:
            for (_, _, t, c) in self.fl.groups[gi].program.outputs:
                coef[t, k] = c
                k += 1
        self._coef = coef.to(dev)

    def traces(self, params=None):
        """``T`` ``(n_terms,)`` on the device.  Two calls at the same parameters give the same bits: every
        per-instance norm is one thread's fixed-order arithmetic and the sums run in a fixed order."""
        from . import _lib, jet_hip
        prog, fl, cfg = self.prog, self.fl, self.cfg
        P = (prog.net.flat if params is None else params).detach().contiguous()
        if P.dtype != torch.float32:
            raise ValueError("the NTK trace kernels take the fp32 parameter vector")
        pad_kp(P, cfg, self.Kp)
        k = 0
        for gi, lo, m, slots in self.launches:
            gr = fl.groups[gi]
            offs = [prog.segments[s].offset for s in gr.segs]
            X = prog.X_all[offs[0] + lo:offs[0] + lo + m] if slots == 1 else \
                torch.cat([prog.X_all[o + lo:o + lo + m] for o in offs], dim=0)
            J, saved = jet_hip.forward_raw(X, P, prog.net, prog.plan, precision="fp32")
            dJ = self.dJ[:J.numel()].view(J.shape)
            for oi in range(len(gr.program.outputs)):
                # slot k's instance i is point k m + (i - lo) of this launch's point list
                seeds(self.fop, gi, oi, J, saved[0], dJ, lo, m, [k_ * m - lo for k_ in range(slots)])
                n2 = instance_norms(saved, dJ, self.Kp, m, 0, m if slots == 2 else None,
                                    out=self.norms[(gi, oi)][lo:lo + m])
                _lib.check(self.lib.tdq_ntk_sum(_lib.ptr(n2), m, _lib.ptr(self.sums[k:k + 1]),
                                                _lib.stream_ptr(P.device)), "tdq_ntk_sum")
                k += 1
        torch.sum(self._coef * self.sums, dim=1, out=self.T)
        return self.T

    def instance_norms(self, gi, oi):
        """Per-instance norms of output ``oi`` of group ``gi`` from the last :meth:`traces` call."""
        return self.norms[(gi, oi)]


# ------------------------------------------------------------------------------------------
# layer-wise HIP path
# ------------------------------------------------------------------------------------------
def _gram_check(H, Z, S, N, n_inst, offA, offB, n2):
    for name, t in (("H", H), ("Z", Z)):
        if t.dim() != 2 or t.shape[0] != S * N or t.dtype != H.dtype or not t.is_floating_point() \
                or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            raise ValueError(f"tdq_ntk_gram: {name} must be a floating ({S * N}, W) row-major plane, got "
                             f"{tuple(t.shape)} strides {tuple(t.stride())}")
    if not 1 <= S <= 8 or n_inst < 0 or offA < 0 or offA + n_inst > N or (offB is not None and (
            offB < 0 or offB + n_inst > N)):
        raise ValueError(f"tdq_ntk_gram: S {S}, instances [{offA}, {offA + n_inst}) / pair offset {offB} outside "
                         f"1..8 streams of {N} points")
    if n2.dtype != H.dtype or not n2.is_contiguous() or n2.numel() != n_inst:
        raise ValueError(f"tdq_ntk_gram: n2 must be a contiguous ({n_inst},) tensor of the planes' dtype")


def gram_norms(H, Z, S, N, n_inst, offA=0, offB=None, out=None, accumulate=False):
    """One dense layer's share of the per-instance norms (``tdq_ntk_gram``, csrc/ntk_gram.hip):
    ``out[i] (+)= sum_{r,r'} (Z[r].Z[r']) (H[r].H[r']) + ||sum_{value rows} Z[r]||^2`` over the rows of
    instance ``i`` - the ``S`` streams of point ``offA + i``, and of ``offB + i`` in pair mode.  ``H`` / ``Z``:
    float32 ``(S*N, W)`` planes (row ``s N + n``), each with its own row stride."""
    from . import _lib
    if out is None:
        out = torch.zeros(max(0, n_inst), device=H.device)
    # the kernel trusts the planes' extent and n2's length; it refuses bad geometry itself
    for name, t in (("H", H), ("Z", Z)):
        if t.dim() != 2 or t.shape[0] != S * N or t.dtype != torch.float32 or t.stride(1) != 1 or not t.is_cuda:
            raise ValueError(f"tdq_ntk_gram: {name} must be a float32 ({S * N}, W) row-major device plane, got "
                             f"{tuple(t.shape)} strides {tuple(t.stride())}")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != max(0, n_inst) or not out.is_cuda:
        raise ValueError(f"tdq_ntk_gram: n2 must be a contiguous float32 ({n_inst},) device tensor")
    rc = _lib.load(required=True).tdq_ntk_gram(
        _lib.ptr(H), H.stride(0), H.shape[1], _lib.ptr(Z), Z.stride(0), Z.shape[1], int(S), int(N), int(offA),
        -1 if offB is None else int(offB), int(n_inst), int(bool(accumulate)), _lib.ptr(out),
        _lib.stream_ptr(H.device))
    _lib.check(rc, "tdq_ntk_gram")
    return out


def gram_norms_torch(H, Z, S, N, n_inst, offA=0, offB=None, out=None, accumulate=False):
    """The torch mirror of :func:`gram_norms` (same contract, the planes' own dtype): the CPU path of
    :class:`LayeredNTKOp` and the formula of the tests."""
    _gram_check(H, Z, S, N, n_inst, offA, offB, out if out is not None else H.new_empty(max(0, n_inst)))
    offs = [offA] if offB is None else [offA, offB]

    def rows(V):  # (n_inst, R, W)
        V = V.view(S, N, V.shape[1]) if V.is_contiguous() else V.reshape(S, N, V.shape[1])
        return torch.cat([V[:, o:o + n_inst] for o in offs], dim=0).transpose(0, 1)

    Zr, Hr = rows(Z), rows(H)
    term = ((Zr @ Zr.transpose(1, 2)) * (Hr @ Hr.transpose(1, 2))).sum((1, 2))
    term = term + Zr[:, ::S].sum(1).square().sum(1)
    if out is None:
        return term
    if accumulate:
        out += term
    else:
        out.copy_(term)
    return out


def layered_enabled():
    """``TDQ_NTK_LAYERED=0`` keeps the programs of :class:`LayeredNTKOp` on the torch path (the A/B switch of
    tools/ntk_timing.py); on by default."""
    import os
    return os.environ.get("TDQ_NTK_LAYERED", "1") != "0"


def layered_reason(prog):
    """None when :class:`LayeredNTKOp` serves the program on the GPU, else why not: the HIP backend, a
    fused, unmixed program of order <= 2 with S <= 8, hidden widths <= 128 (equal or not), <= 16 hidden
    layers, d_in <= 8, d_out <= 4."""
    if prog.device.type != "cuda" or prog.backend != "hip":
        return "the program does not run on the HIP backend"
    if prog.fused_op is None:
        return "the loss program is not fused"
    if prog.mixed:
        return f"derivative order {prog.plan_hi.order} > 2"
    sizes = list(prog.net.layer_sizes)
    if prog.plan.order > 2 or prog.plan.S > 8:
        return f"order {prog.plan.order}, {prog.plan.S} streams"
    # (the kernels take any width; 128 keeps the networks wider than that on the path their tests pin)
    if max(sizes[1:-1]) > 128 or len(sizes) - 2 > 16 or sizes[0] > 8 or sizes[-1] > 4:
        return f"layers {sizes} outside widths <= 128, <= 16 hidden layers, d_in <= 8, d_out <= 4"
    return None


class LayeredNTKOp:
    """Traces on the layer-wise engine, for programs beyond :class:`NTKTraceOp`'s register envelope
    (5-8 streams at width 128, unequal widths).  Per launch group one exact-fp32 layered forward
    (:func:`.jet_layered.forward_raw`), per output the seed launch (``tdq_loss_seed``), the adjoints-only
    pass (:func:`.jet_layered.adjoint_planes`) and one ``tdq_ntk_gram`` per dense layer, then the
    fixed-order ``tdq_ntk_sum``.  Same interface, buffers, chunking and bitwise repeatability as
    :class:`NTKTraceOp`.  Without a GPU (``fop=None``) the seeds come from autograd through the torch
    interpreter and the Gram step from :func:`gram_norms_torch`."""

    kind = "hip-layered"

    def __init__(self, prog, fl, lambdas, fop=None, chunk=CHUNK):
        self.prog, self.fl, self.lambdas, self.fop = prog, fl, lambdas, fop
        self.S = prog.plan.S
        self.d_out = prog.net.layer_sizes[-1]
        dev = prog.device
        self.hip = fop is not None and dev.type == "cuda"
        self.outputs = outputs(fl)
        self.launches = []   # (group, lo, m, slots) per forward
        for gi, gr in enumerate(fl.groups):
            step = max(1, int(chunk) // len(gr.segs))
            self.launches += [(gi, lo, min(gr.n, lo + step) - lo, len(gr.segs)) for lo in range(0, gr.n, step)]
        n_max = max((m * k for _, _, m, k in self.launches), default=1)
        self.dJ = torch.zeros(self.S * n_max * self.d_out, device=dev)
        self.norms = {(gi, oi): torch.zeros(fl.groups[gi].n, device=dev) for gi, oi, _, _ in self.outputs}
        n_sums = sum(len(fl.groups[gi].program.outputs) for gi, _, _, _ in self.launches)
        self.sums = torch.zeros(max(1, n_sums), device=dev)
        self.T = torch.zeros(len(fl.term_names), device=dev)
        coef = torch.zeros(len(fl.term_names), max(1, n_sums))
        k = 0
        for gi, _, _, _ in self.launches:
            for (_, _, t, c) in fl.groups[gi].program.outputs:
                coef[t, k] = c
                k += 1
        self._coef = coef.to(dev)

    def _seeds_torch(self, gi, oi, J, X, dJ, lo, m):
        """``dJ = d f_o / d J`` by autograd through the torch interpreter (the mirror of :func:`seeds`)."""
        fl = self.fl
        P = fl.groups[gi].program
        dt, dev = J.dtype, J.device
        scalars = fusion.scalar_values(fl, self.lambdas, None)

        def lam(a):
            k = fl.lam_slots[a]
            o = fl.lam_offsets.get(k, (0, 0))[0]
            return self.lambdas[k].detach().reshape(-1)[o + lo:o + lo + m].to(dt)

        with torch.enable_grad():
            Jg = J.detach().clone().requires_grad_(True)
            vals = fusion.eval_group(P, m, lambda a, row, col: Jg[row, a * m:(a + 1) * m, col],
                                     lambda a, j: X[a * m:(a + 1) * m, j],
                                     lambda a: fl.val_arrays[a].to(dev)[lo:lo + m].to(dt), lam,
                                     lambda a: scalars[a].detach().to(dt), dev, dt)
            f = vals[P.outputs[oi][0]]
            g = torch.autograd.grad(f.sum(), Jg, allow_unused=True)[0] if f.requires_grad else None
        dJ.copy_(torch.zeros_like(J) if g is None else g)
        return dJ

    def traces(self, params=None):
        """``T`` ``(n_terms,)`` on the device.  Two calls at the same parameters give the same bits: every
        kernel of the chain computes each element in a fixed order and the sums run in a fixed order."""
        from . import _lib, jet_layered
        prog, fl = self.prog, self.fl
        P = (prog.net.flat if params is None else params).detach().contiguous()
        if P.dtype != torch.float32:
            raise ValueError("the NTK trace kernels take the fp32 parameter vector")
        gram = gram_norms if self.hip else gram_norms_torch
        S = self.S
        k = 0
        for gi, lo, m, slots in self.launches:
            gr = fl.groups[gi]
            offs = [prog.segments[s].offset for s in gr.segs]
            X = prog.X_all[offs[0] + lo:offs[0] + lo + m] if slots == 1 else \
                torch.cat([prog.X_all[o + lo:o + lo + m] for o in offs], dim=0)
            X = X.contiguous()
            N = X.shape[0]
            J, saved = jet_layered.forward_raw(X, P, prog.net, prog.plan, precision="fp32")
            dJ = self.dJ[:J.numel()].view(J.shape)
            for oi in range(len(gr.program.outputs)):
                # slot k's instance i is point k m + (i - lo) of this launch's point list
                if self.hip:
                    seeds(self.fop, gi, oi, J, X, dJ, lo, m, [k_ * m - lo for k_ in range(slots)])
                else:
                    self._seeds_torch(gi, oi, J, X, dJ, lo, m)
                n2 = self.norms[(gi, oi)][lo:lo + m]
                for li, (H, Z) in enumerate(jet_layered.adjoint_planes(saved, dJ)):
                    gram(H, Z, S, N, m, 0, m if slots == 2 else None, out=n2, accumulate=li > 0)
                if self.hip:
                    _lib.check(_lib.load().tdq_ntk_sum(_lib.ptr(n2), m, _lib.ptr(self.sums[k:k + 1]),
                                                       _lib.stream_ptr(P.device)), "tdq_ntk_sum")
                else:
                    self.sums[k] = n2.sum()
                k += 1
        torch.sum(self._coef * self.sums, dim=1, out=self.T)
        return self.T

    def instance_norms(self, gi, oi):
        """Per-instance norms of output ``oi`` of group ``gi`` from the last :meth:`traces` call."""
        return self.norms[(gi, oi)]


def build(prog, lambdas):
    """The trace evaluator of a finalized program: :class:`NTKTraceOp` inside the fused kernels' envelope,
    :class:`LayeredNTKOp` inside the layer-wise one (:func:`layered_reason`), else :class:`TorchNTK` (on a
    GPU the reason goes to ``prog.reasons`` and is warned once).  ``ValueError`` when the loss cannot be
    traced into a fused program - that program defines the outputs."""
    if prog.backend not in ("hip", "jet"):
        raise ValueError("NTK adaptive weighting needs the jet path (backend 'jet' or 'hip'): "
                         + "; ".join(prog.reasons or [f"backend {prog.backend!r}"]))
    fl = prog.fused_op.fl if prog.fused_op is not None else fusion.build(prog, lambdas)
    if fl is None:
        raise ValueError("NTK adaptive weighting needs a loss the tracer can fuse: "
                         + "; ".join(prog.reasons or ["loss fusion failed"]))
    if prog.device.type == "cuda":
        why = hip_reason(prog)
        if why is None:
            return NTKTraceOp(prog, prog.fused_op)
        if layered_enabled() and layered_reason(prog) is None:
            return LayeredNTKOp(prog, fl, lambdas, fop=prog.fused_op)
        from ..models.loss import _warn_once
        msg = f"NTK traces on the torch jet: {why}"
        prog.reasons.append(msg)
        _warn_once(msg)
    return TorchNTK(prog, fl, lambdas)
