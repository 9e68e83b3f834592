"""One-launch training step: forward -> loss -> backward of every point (hipRTC).

The persistent point-tile kernel of ``csrc/jet_fused.h`` (the fused step) runs, per 32-point tile,
the Taylor-jet forward of the network, the per-point loss of the fused loss program and its
reverse sweep, and the recompute backward into the tile loop's register-resident weight gradient -
so J and dJ never touch HBM and the step has no forward / loss / backward launch boundaries.  The
loss is the traced program of the fused loss (:mod:`.loss_jit` emits the same statements, here as
the body of a ``GenLoss::eval`` the kernel calls per point: every loss group, with the two points
of a periodic pair side by side in the tile), so the kernel is compiled at run time with hipRTC
once per (network shape, loss program) and cached per process.  A step is then the fused launch
plus the two-launch step tail (``jet_hip.step_tail`` / ``dp_tail_a``: slab reduction, loss
bookkeeping, Adam).

Programs with order-3/4 boundary streams (``jet_hi.hip``) run every loss output on main-plan
streams fused and keep the high-order outputs' chain (jet_hi forward, their loss blocks, jet_hi
adjoint) on a side stream beside it.

The reference's step is tensordiffeq/models.py:90-135 (``train_op_inner`` / ``update_loss``): a
tape over the network, the residual and the boundary MSEs, then the optimizer.

Precision ``bf16x3`` (the L-BFGS objective) runs the same one-launch structure with every GEMM
operand split into bf16 hi + lo (``csrc/jet_fused3.h``: 16-point tiles, since the lo planes double
the LDS images); its tail reduces fp32 slab rows.

Networks with 2-4 outputs (systems of PDEs) run on the same two kernels inside their geometry
(width 128, 2-3 MFMA layers, S <= 4, plain programs): the number of outputs is a compile-time
constant of the generated kernel (``GenLoss::DOUT``) - one output-layer dot per (stream, output), the
loss's ``JV`` / ``UB`` take the output as a third argument, the reverse sums over the outputs.  A
combination whose LDS does not fit (bf16, 3 MFMA layers, S = 4, 4 outputs) and every multi-output
network outside the geometry keep the separate launches.

``TDQ_FUSED_STEP=0`` keeps the separate launches (``fit.run_ranges``);
``TDQ_FUSED_STEP_SYSTEMS=0`` does so for networks with several outputs only.
"""
from __future__ import annotations

import collections
import ctypes
import hashlib
import os
import warnings

import torch

from . import _lib, jet_hip, loss_jit
from .jet_mlp import hip_config

_CACHE = {}   # source sha -> (module, func)
_HEADERS = ("common.h", "jet_common.h", "jet_bf3.h", "jet_fused.h", "jet_fused3.h")
# the library's hipcc flags (csrc/build.py _flags), as hipRTC options
RTC_OPTS = "-O3 -std=c++17 -fno-slp-vectorize -munsafe-fp-atomics"


# the bf16x3 objective's kernel under LLVM's max-ILP machine scheduler: 273.3-274.8 vs 277.3-278.2 us
# per evaluation, L-BFGS 0.3190 vs 0.3220 ms per iteration; the bf16 step is faster on the default
# scheduler (0.1378 vs 0.1421 ms) - profiles/r6ba_sched_strategy_ab.txt
# (and col4_sum on ds_bpermute there: the v_permlane swap form is 0.4 % faster in the bf16 step but
# 0.8 % slower in this kernel, profiles/r6be_col4_permlane_ab.txt)
RTC_OPTS_LO = " -mllvm -amdgpu-sched-strategy=max-ilp -DTDQ_COL4_BPERMUTE"


def _opts(src=""):
    """hipRTC options; ``TDQ_FUSED_STEP_TIMING=1`` adds the phase stamps (tools/fused_step_timing.py)."""
    extra = os.environ.get("TDQ_FUSED_STEP_DEFINES", "")   # A/B builds, e.g. "-DTDQ_PK_TANH=0"
    return RTC_OPTS + (RTC_OPTS_LO if "fz3_body<" in src else "") + \
        (" -DTDQ_PHASE_TIMING" if os.environ.get("TDQ_FUSED_STEP_TIMING") == "1" else "") + \
        (" " + extra if extra else "")


def enabled():
    return os.environ.get("TDQ_FUSED_STEP", "1") != "0"


def systems_enabled():
    """``TDQ_FUSED_STEP_SYSTEMS``: ``0`` keeps networks with several outputs on the separate launches
    (:func:`ineligible` answers ``"d_out != 1"``)."""
    return os.environ.get("TDQ_FUSED_STEP_SYSTEMS", "1") != "0"


def _csrc():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")


def header_source():
    """The kernel headers as one translation unit (hipRTC has no include path of ours)."""
    out = []
    for h in _HEADERS:
        with open(os.path.join(_csrc(), h)) as f:
            lines = f.read().splitlines()
        out.append("\n".join(ln for ln in lines if not ln.strip().startswith('#include "')
                             and ln.strip() != "#pragma once"))
    return "\n".join(out)


def spec_source(spec, S, d_in, d_out=1):
    """``SPEC`` / ``DIN`` / ``DOUT`` members of the generated struct: the plan's stream spec (csrc
    jet_common.h ``make_spec``), the input width and the number of network outputs as compile-time
    constants, so the kernel's one-hot stream selects, first-layer loops and output-layer loops
    fold away (the kernels require them)."""
    if spec is None or d_in is None:
        raise ValueError("gen_loss: the stream spec and d_in are compile-time constants of the kernel")
    M = 8   # TDQ_MAXS
    st, var, ia, ib = [0] * M, [0] * M, [0] * M, [0] * M
    selA = [[0.0] * M for _ in range(M)]
    selB = [[0.0] * M for _ in range(M)]
    for s in range(S):
        ty, a, b = spec[3 * s:3 * s + 3]
        st[s] = ty
        if ty == 1:
            var[s] = a
        if ty == 2:
            ia[s], ib[s] = a, b
            selA[s][a] = 1.0
            selB[s][b] = 1.0
    arr = lambda v: "{" + ", ".join(str(x) for x in v) + "}"  # noqa: E731
    mat = lambda m: "{" + ", ".join("{" + ", ".join(f"{x:.1f}f" for x in r) + "}" for r in m) + "}"  # noqa: E731
    return [f"  static constexpr JetSpec SPEC = {{{arr(st)}, {arr(var)}, {mat(selA)}, {mat(selB)}, {arr(ia)}, "
            f"{arr(ib)}}};",
            f"  static constexpr int DIN = {int(d_in)};",
            f"  static constexpr int DOUT = {int(d_out)};"]


def gen_loss(groups, n_terms, nacc, S, spec=None, d_in=None, d_out=1):
    """``struct GenLoss`` of the loss groups laid out in the fused point set.  ``groups``: one
    ``(program, start, n_slots, n)`` per group - its ``n`` instances occupy points ``start + k``
    (one slot) or the pairs ``start + 2k, start + 2k + 1`` (two slots: a periodic pair side by side,
    ``start`` even, so a pair never straddles a tile of 16 or 32 points).  The statements are those
    of :func:`.loss_jit._group_code` per point: J streams / coordinates from the tile (the partner's
    from the next point-thread), per-point inputs (SA weights, data values, scalars) from global
    memory, loss / scalar-gradient sums into the thread's accumulators, dJ of the instance's points
    into the tile's ``ubs``.  Points outside every group get dJ = 0.  ``eval<S, PT>`` serves both
    tile sizes (``PT`` points per tile).

    ``d_out`` > 1 (a system): a STREAM operand is ``stream | column << COL_SHIFT`` as in
    :func:`.loss_jit._group_code`; J is ``JV(stream, point, output)``, the adjoints are
    ``dj{slot}_{stream}_{output}`` and EVERY output of every (slot, stream) is stored - zero where the
    program reads nothing, so the kernel's reverse never sees a previous tile's value.  With one
    output the output suffix / argument drops (``dj`` / ``jv`` / ``ub`` below) and the bias comes by
    value: the text such a program had before systems were served."""
    D = int(d_out)
    if not 1 <= D <= 4:
        raise ValueError(f"fused step: {D} network outputs")
    cmask = (1 << loss_jit.COL_SHIFT) - 1

    def dj(sl, s, q):   # the adjoint of J(slot, stream, output)
        return f"dj{sl}_{s}" + (f"_{q}" if D > 1 else "")

    def jv(s, k, q):
        return f"JV({s}, {k}" + (f", {q})" if D > 1 else ")")

    def ub(s, k, q):
        return f"UB({s}, {k}" + (f", {q})" if D > 1 else ")")

    L = []
    e = L.append
    e("struct GenLoss {")
    e(f"  static constexpr int NACC = {max(1, nacc)};")
    for ln in spec_source(spec, S, d_in, D):
        e(ln)

    def branches(body):
        kw = "if"
        for (P, start, ns, n) in groups:
            end = start + ns * n
            e(f"    {kw} (n >= {start} && n < {end} && n < N) {{")
            kw = "else if"
            if ns == 2:
                e(f"      if ((n - {start}) & 1) return;   // the pair's first point-thread owns it")
                e(f"      const int i = (n - {start}) >> 1;")
            else:
                e(f"      const int i = n - {start};")
            body(P, ns)
            e("      return;")
            e("    }")

    # the first per-point global input (SA weight / data value) of each group: the kernel loads it
    # for the NEXT tile during this one (pre, into an LDS word per point) - the loss phase then
    # waits for no global load on the common groups (bf16 step 0.1397 -> 0.1382 ms, objective
    # 278.2 -> 277.0 us: profiles/r6ae_loss_input_prefetch_ab.txt)
    first = {}
    for gi, (P, start, ns, n) in enumerate(groups):
        seen = []

        def probe(name, r, a, b, seen=seen):
            if name in ("VAL", "LAM") and not seen:
                seen.append((name, a))
            return ""
        loss_jit._forward_code(P, lambda _ln: None, probe)
        first[gi] = seen[0] if seen else None
    e("  __device__ static float pre(int n, int N, const FzLossPtrs& ptr) {")
    kw = "if"
    for gi, (P, start, ns, n) in enumerate(groups):
        if first[gi] is None:
            continue
        nm, a = first[gi]
        arr = {"VAL": "val", "LAM": "lam"}[nm]
        end = start + ns * n
        idx = f"(n - {start}) >> 1" if ns == 2 else f"n - {start}"
        e(f"    {kw} (n >= {start} && n < {end} && n < N) return ptr.{arr}[{a}][{idx}];")
        kw = "else if"
    e("    return 0.f;")
    e("  }")
    # the kernel's side of the interface (csrc/jet_fused.h): J of (stream, point[, output]) is the NW
    # waves' partial output dots summed here (wave order, + bo on the value stream) instead of in a
    # separate phase behind one more barrier; one output takes its bias by value, several the array
    e("  template <int S, int PT, int NW>")
    e("  __device__ static void eval(const float* jv, const float* xs, int t, int n, int N, "
      "const FzLossPtrs& ptr, float* ubs, float (&acc)[NACC], float pv, "
      + ("float bo" if D == 1 else "const float* bo") + ") {")
    if D == 1:
        e("    #define JV(s_, k_) fz_jsum<S, PT, NW>(jv, (s_), (k_), bo)")
        e("    #define UB(s_, k_) ubs[((s_) * PT + (k_)) * 4]")
    else:
        e(f"    #define JV(s_, k_, q_) fz_jsum_q<S, PT, NW, {D}>(jv, (s_), (k_), (q_), bo)")
        e("    #define UB(s_, k_, q_) ubs[((s_) * PT + (k_)) * 4 + (q_)]")

    cur = {}

    def eval_body(P, ns):
        fp = first[[g[0] for g in groups].index(P)]
        cur["first"], cur["used"] = fp, False
        nr = max(1, P.n_regs)
        e("      float " + ", ".join(f"v{r}" for r in range(nr)) + ";")
        e("      float " + ", ".join(f"a{r} = 0.f" for r in range(nr)) + ";")
        e("      float " + ", ".join(f"{dj(sl, b, q)} = 0.f" for sl in range(ns) for b in range(S)
                                     for q in range(D)) + ";")

        def stream(b):
            s, q = b & cmask, b >> loss_jit.COL_SHIFT
            if s >= S or q >= D:
                raise ValueError("fused step: stream outside the jet plan")
            return s, q

        def load(name, r, a, b):
            if name in ("STREAM", "COORD") and a >= ns:
                raise ValueError("fused step: slot outside the group")
            if name == "STREAM":
                s, q = stream(b)
                return f"      v{r} = {jv(s, f't + {a}', q)};"
            if name == "COORD":
                return f"      v{r} = xs[(t + {a}) * TDQ_MAXD + {b}];"
            if (name, a) == cur["first"] and not cur["used"]:
                cur["used"] = True
                return f"      v{r} = pv;   // prefetched (pre)"
            return {"VAL": f"      v{r} = ptr.val[{a}][i];", "LAM": f"      v{r} = ptr.lam[{a}][i];",
                    "SCAL": f"      v{r} = *ptr.scal[{a}];"}[name]

        loss_jit._forward_code(P, e, load)
        for (f, w, tt, c) in P.outputs:
            cl = loss_jit._lit(c)
            e(f"      {{ const float f = v{f}, w = v{w};")
            e(f"        acc[{tt}] += {cl} * w * f * f;")
            e(f"        a{f} += 2.f * {cl} * w * f; a{w} += {cl} * f * f; }}")

        def store(name, r, a, b, g):
            if name == "STREAM":
                return f"      {dj(a, *stream(b))} += {g};"
            if name == "LAM":
                return f"      ptr.dlam[{a}][i] = {g};"
            return f"      acc[{n_terms + a}] += {g};"

        loss_jit._reverse_code(P, e, store)
        # the outputs of one (slot, stream) on one line (one output: all of them on one)
        rows = [" ".join(f"{ub(b, f't + {sl}', q)} = {dj(sl, b, q)};" for q in range(D))
                for sl in range(ns) for b in range(S)]
        for ln in ([" ".join(rows)] if D == 1 else rows):
            e("      " + ln)

    branches(eval_body)
    e("    #pragma unroll")
    zero = " ".join(f"{ub('s', 't', q)} = 0.f;" for q in range(D))
    e("    for (int s = 0; s < S; ++s) " + (zero if D == 1 else "{ " + zero + " }"))
    e("    #undef JV")
    e("    #undef UB")
    e("  }")
    e("};")
    return "\n".join(L)


def kernel_name(lo=False):
    """``tdq_fused_step`` (bf16 step) / ``tdq_fused_step3`` (bf16x3 objective): distinct names in
    the kernel traces."""
    return "tdq_fused_step3" if lo else "tdq_fused_step"


def kernel_source(S, nso, LM, lds, gen, lo=False):
    """The kernel translation unit: the headers, the generated loss, and ``tdq_fused_step`` over
    ``fz_body`` (bf16, 32-point tiles) or ``fz3_body`` (``lo``: bf16x3, 16-point tiles)."""
    body = "fz3_body" if lo else "fz_body"
    return (header_source() + "\n" + gen + "\n"
            'extern "C" __global__ void __launch_bounds__(64 * FZ_WAVES) '
            f"__attribute__((amdgpu_waves_per_eu(2, 2))) {kernel_name(lo)}(FzParams P) {{\n"
            f"  __shared__ __attribute__((aligned(16))) char lds[{lds}];\n"
            f"  {body}<8, {S}, {nso}, {LM}, GenLoss>(P, lds);\n"
            "}\n")


_PENDING = {}   # source key -> (thread, [code bytes | exception])


def _key(src):
    return hashlib.sha256((loss_jit.device_arch() + _opts(src) + src).encode()).hexdigest()


def _rtc_compile(src):
    """hipRTC compile of ``src`` to code-object bytes (host only: no GPU call)."""
    lib = _lib.load(required=True)
    code, size = ctypes.c_void_p(0), ctypes.c_longlong(0)
    log = ctypes.create_string_buffer(16384)
    rc = lib.tdq_rtc_compile_ex(src.encode(), b"tdq_fused_step.hip", loss_jit.device_arch().encode(),
                                _opts(src).encode(), ctypes.byref(code), ctypes.byref(size), log, len(log))
    if rc != 0:
        raise RuntimeError(f"hipRTC compile failed ({rc}): {log.value.decode(errors='replace')[:2000]}")
    try:
        return ctypes.string_at(code, size.value)
    finally:
        lib.tdq_rtc_free(code)


def compile_async(src):
    """Start the hipRTC compile of ``src`` on a host thread (ctypes releases the GIL), so a later
    :func:`_compile` of the same source only loads the module.  No-op when it is cached or pending."""
    import threading
    k = _key(src)
    if k in _CACHE or k in _PENDING:
        return
    out = []

    def work():
        try:
            out.append(_rtc_compile(src))
        except Exception as e:  # noqa: BLE001 - re-raised by _compile
            out.append(e)
    th = threading.Thread(target=work, name="tdq-rtc", daemon=True)
    _PENDING[k] = (th, out)
    th.start()


def _compile(src, name="tdq_fused_step"):
    """``(module, function)`` of the fused-step kernel ``name`` in ``src`` (compiled once per
    process; a compile started by :func:`compile_async` is joined)."""
    lib = _lib.load(required=True)
    k = _key(src)
    if k not in _CACHE:
        pend = _PENDING.pop(k, None)
        if pend is not None:
            pend[0].join()
            code = pend[1][0]
            if isinstance(code, Exception):
                raise code
        else:
            code = _rtc_compile(src)
        buf = ctypes.create_string_buffer(code, len(code))
        mod, fn = ctypes.c_void_p(0), ctypes.c_void_p(0)
        _lib.check(lib.tdq_rtc_load(buf, name.encode(), ctypes.byref(mod), ctypes.byref(fn)), "hipModuleLoadData")
        _CACHE[k] = (mod, fn)
    return _CACHE[k]


def mixed_mode():
    """``TDQ_FUSED_STEP_MIXED``: how a mixed program (order-3/4 boundary streams from jet_hi.hip)
    runs.  ``split`` (default) - every loss output on main-plan streams runs in the fused launch (the
    boundary groups' low-order outputs included), only the high-order outputs' chain (jet_hi
    forward, their loss blocks, jet_hi adjoint) on a side stream; ``0`` - the point-range path.
    MI355X, AC-baseline 50k: split 0.207 ms/step, point ranges 0.219-0.226 (AC-SA 0.168;
    profiles/r5split3_*, r5acb_*).  The residual-only layout (``1``, 0.251 ms/step) was removed:
    tools/patches/fused_step_residual_layout_REMOVED.patch."""
    mode = os.environ.get("TDQ_FUSED_STEP_MIXED", "split")
    if mode not in ("split", "0"):
        raise ValueError(f"TDQ_FUSED_STEP_MIXED={mode!r}: accepted values are 'split' and '0'")
    return mode


def _mixed(prog):
    return getattr(prog, "hi_op", None) is not None


def fused_groups(prog, fop):
    """``[(group, fused program, side program or None)]`` of the fused point set: every group whose
    outputs read main-plan streams only runs whole in the fused launch; a mixed program's other
    groups are split (:func:`fusion.split_by_streams`) - or the reason that does not apply (an output
    reading main-plan and high-order streams together, or an SA weight read by both halves)."""
    from .. import fusion
    out = []
    for gr in fop.fl.groups:
        if all(s < prog.plan.S for (_, s) in gr.program.stream_regs):
            out.append((gr, gr.program, None))
            continue
        sp = fusion.split_by_streams(fop.fl, gr, prog.plan.S)
        if sp is None:
            return "a loss output reads main-plan and high-order streams together (or both read one SA weight)"
        out.append((gr, sp[0], sp[1]))
    return out


def point_layout(prog, groups):
    """The fused point set of ``groups`` (:func:`fused_groups`): groups in program order, a periodic
    group's two segments interleaved pair by pair, pair groups on even offsets.  Returns
    ``(layout, idx, N)``: the ``[(program, start, n_slots, n)]`` of :func:`gen_loss`, the gather index
    of the ``N`` points into ``prog.X_all`` (-1: the padding point in front of a pair group)."""
    layout, idx = [], []
    for gr, P_f, _ in groups:
        ns = len(gr.segs)
        if ns == 2 and len(idx) % 2:
            idx.append(-1)
        layout.append((P_f, len(idx), ns, gr.n))
        offs = [prog.segments[sg].offset for sg in gr.segs]
        for k in range(gr.n):
            idx.extend(o + k for o in offs)
    return layout, idx, len(idx)


# everything that determines the compiled kernel (:func:`recipe`): geometry, stream spec, the number of
# second-order streams, MFMA layers, bf16x3 (hi + lo operands), points per tile, LDS bytes, kernel name
# and source (None without a layout)
KernelRecipe = collections.namedtuple("KernelRecipe", "cfg S spec nso LM lo pt lds name source")


def recipe(prog, fop, layout, precision=None):
    """The :class:`KernelRecipe` of ``prog`` (in ``precision``, default the program's) with the loss
    groups laid out as ``layout`` (``None``: the geometry alone).  Host only - no GPU call.  Raises
    ``ValueError`` outside the kernels' envelope."""
    cfg = hip_config(prog.net, prog.plan, precision or prog.precision)
    S = cfg["S"]
    spec = jet_hip.stream_spec(prog.plan)
    nso = sum(1 for s in range(S) if spec[3 * s] == 2)
    LM = cfg["n_hidden"] - 1
    lo = cfg["precision"] == "bf16x3"
    lds = _lib.load(required=True).tdq_jet_fused_lds(cfg["d_in"], jet_hip._warg(cfg), cfg["d_out"], cfg["n_hidden"],
                                                     S, int(lo))
    if lds < 0 or lds > 160 * 1024:
        raise ValueError(f"fused step: {lds} bytes of LDS")
    source = None
    if layout is not None:
        gen = gen_loss(layout, fop.n_terms, fop.n_terms + fop.n_scal, S, spec=spec, d_in=cfg["d_in"],
                       d_out=cfg["d_out"])
        source = kernel_source(S, nso, LM, lds, gen, lo=lo)
    return KernelRecipe(cfg, S, spec, nso, LM, lo, 16 if lo else 32, lds, kernel_name(lo), source)


def program_recipe(prog, fop, precision=None):
    """``(recipe, groups, idx, N)`` of a program's fused step: what :func:`prebuild` compiles and
    :class:`FusedStepOp` runs."""
    groups = fused_groups(prog, fop)
    if isinstance(groups, str):
        raise ValueError(groups)
    layout, idx, N = point_layout(prog, groups)
    return recipe(prog, fop, layout, precision), groups, idx, N


def prebuild(prog):
    """Start compiling the fused step of a single-plan program in the background (the L-BFGS
    objective while the Adam phase runs: its hipRTC compile, ~0.35 s, then overlaps the Adam
    steps).  Returns whether a compile was started (or was already cached)."""
    if not torch.cuda.is_available():
        return False
    fop = getattr(prog, "fused_op", None)
    if ineligible(prog, fop) is not None or _mixed(prog):
        return False
    compile_async(program_recipe(prog, fop)[0].source)
    return True


def ineligible(prog, fop):
    """Why the fused step cannot serve this program (``None``: it can)."""
    if not enabled():
        return "TDQ_FUSED_STEP=0"
    mode = mixed_mode()
    if prog.device.type != "cuda" or fop is None:
        return "needs the fused loss on a GPU"
    try:
        cfg = hip_config(prog.net, prog.plan, prog.precision)
    except ValueError as e:
        return str(e)
    if cfg["precision"] not in ("bf16", "bf16x3") or not jet_hip.is_split_bf16(cfg):
        return f"precision {cfg['precision']}"
    if cfg["d_out"] != 1:
        # a system: inside the kernels' geometry (width 128, 2-3 MFMA layers, S <= 4, up to 4 outputs,
        # no high-order boundary streams) unless switched off; every other multi-output network keeps
        # the separate launches with this answer
        if not (systems_enabled() and cfg["d_out"] <= 4 and not _mixed(prog) and cfg["S"] <= 4
                and cfg["n_hidden"] - 1 in (2, 3) and all(w == 128 for w in cfg["widths"])):
            return "d_out != 1"
        try:
            recipe(prog, fop, None)
        except ValueError as e:
            return f"LDS: {e} ({cfg['precision']}, {cfg['n_hidden']} hidden layers, S={cfg['S']}, d_out={cfg['d_out']})"
    try:
        recipe(prog, fop, None)
    except ValueError:
        return f"network {cfg['widths']} / S={cfg['S']} (width-128 MFMA layers 2-3, S <= 4)"
    if not _mixed(prog):
        if any(s >= cfg["S"] for gr in fop.fl.groups for (_, s) in gr.program.stream_regs):
            return "a loss group reads streams outside the jet plan"
        return None
    if cfg["precision"] == "bf16x3":
        # the bf16x3 objective of a mixed program keeps the point-range launches (its boundary
        # chain runs on the bf16x3 jet_hi kernels beside them)
        return "bf16x3: high-order boundary streams keep the separate launches"
    if mode == "0":
        return "high-order boundary streams (TDQ_FUSED_STEP_MIXED=0)"
    sp = fused_groups(prog, fop)
    return sp if isinstance(sp, str) else None


class FusedStepOp:
    """The fused training step of a :class:`~tensordiffeq_amd.models.loss.LossProgram` (built by
    :func:`for_program`).

    Single-plan programs (layout ``plain``): EVERY loss group runs in the one launch - the points
    re-laid out once into a fused point set (:func:`point_layout`), so a step is the fused launch +
    the two-launch step tail.  Precision bf16: 32-point tiles (``jet_fused.h``); bf16x3 (the L-BFGS
    objective): 16-point tiles with hi + lo operands (``jet_fused3.h``) and fp32 slab rows.  Mixed
    programs (order-3/4 boundary streams from jet_hi.hip, bf16 only, :func:`mixed_mode`; layout
    ``split``): every loss output on main-plan streams in the fused launch, the high-order outputs
    (their own loss op, :func:`fusion.split_by_streams`) with the jet_hi forward / adjoint on a side
    stream beside it."""

    def __init__(self, prog, fop):
        lib = _lib.load(required=True)
        self.prog, self.fop = prog, fop
        rec, groups, idx, self.N = program_recipe(prog, fop)
        cfg = self.cfg = rec.cfg
        self.lo, self.pt, self.lds, self.source = rec.lo, rec.pt, rec.lds, rec.source
        self.nacc = fop.n_terms + fop.n_scal
        dev = prog.device
        self.mixed = _mixed(prog)
        self.layout = "split" if self.mixed else "plain"
        self.idx = idx   # (kept on the host: refresh_points / segment_start are rare)
        ix = torch.tensor(idx, dtype=torch.long, device=dev)
        X_f = prog.X_all[ix.clamp_min(0)].clone()
        X_f[ix < 0] = 0.0
        self.X = X_f.contiguous()
        # prow: the loss-partial rows of the side chain's loss blocks lie ahead of the fused rows
        self.fop2, self.prow = None, 0
        if self.mixed:
            # the high-order outputs: a loss op of their own (same term / value / lambda / scalar
            # slots - its pointer table is the main op's)
            import copy
            from ..fusion import Group
            from .loss_fused import FusedLossOp
            fl2 = copy.copy(fop.fl)
            fl2.groups = []
            for gr, _, P_s in groups:
                if P_s is not None:
                    g2 = Group(list(gr.segs), gr.n)
                    g2.program = P_s
                    fl2.groups.append(g2)
            self.fop2 = FusedLossOp(fl2, prog, fop.lams, fop.scalars, fop.fl.lam_offsets)
            self.fop2.ptrs = fop.ptrs
            self.prow = self.fop2.n_blocks
        self.module, self.func = _compile(self.source, rec.name)
        ntiles = -(-self.N // self.pt)
        cus = max(1, lib.tdq_device_cus())
        rounds = -(-ntiles // cus)
        if self.fop2 is not None:
            # split layout: one round more leaves ~57 CUs to the jet_hi side chain - AC-baseline 50k
            # (7 rounds) 0.2070 vs 0.2105 ms/step (+2 rounds: 0.2277), profiles/r5split3_*; with many
            # rounds the extra one costs more than the side chain gains - AC-dist 500k (62 rounds)
            # 1.043-1.048 ms/step without it, 1.058-1.060 with it (profiles/r6ao_ac_dist_rounds.txt)
            rounds += int(os.environ.get("TDQ_FS_SPLIT_ROUNDS", "1" if rounds <= 16 else "0"))
        # the fewest workgroups with the same tiles per workgroup (AC-SA 50k, bf16: 1592 tiles,
        # 228 x 7; bf16x3: 3183 tiles, 245 x 13); one gradient-slab row per workgroup
        self.G = -(-ntiles // rounds)
        self.free_cus = cus - self.G   # CUs the persistent workgroups leave to a side chain
        need = lib.tdq_slab_floats_rows(self.G, cfg["d_in"], jet_hip._warg(cfg), cfg["d_out"], cfg["n_hidden"])
        cap = lib.tdq_jet_bf3_slab_floats(prog.X_all.shape[0], cfg["d_in"], jet_hip._warg(cfg), cfg["d_out"],
                                          cfg["n_hidden"])
        if need < 0 or need > cap:
            raise ValueError(f"fused step: {self.G} slab rows do not fit the backward's buffer")
        # loss partials: the side chain's loss blocks' rows (mixed) then one row per fused workgroup
        self.n_lblocks = self.prow + self.G
        self.lpart = torch.zeros(max(1, self.n_lblocks * self.nacc), dtype=torch.float32, device=dev)
        self._side = None
        if self.fop2 is not None:   # the side chain's loss blocks write rows [0, prow) of the same buffer
            self.fop2.partials = self.lpart[:self.prow * self.nacc]
            self._side = torch.cuda.Stream(device=dev)

    def refresh_points(self):
        """Re-gather the fused point set from ``prog.X_all`` in place (points that moved: resampling)."""
        with torch.no_grad():
            ix = torch.tensor(self.idx, dtype=torch.long, device=self.X.device)
            X_f = self.prog.X_all[ix.clamp_min(0)]
            X_f[ix < 0] = 0.0
            self.X.copy_(X_f)

    def segment_start(self, si):
        """The first row of segment ``si`` in the fused point set when its points are the consecutive
        rows ``start + i`` there (a group of one segment), else None."""
        s = self.prog.segments[si]
        ix = torch.tensor(self.idx, dtype=torch.long)
        pos = torch.nonzero(ix == s.offset).reshape(-1)
        if s.n < 1 or pos.numel() != 1:
            return None
        start = int(pos[0])
        if start + s.n > ix.numel() or not torch.equal(ix[start:start + s.n], torch.arange(s.offset, s.offset + s.n)):
            return None
        return start

    def run(self, saved, J, work, flat, pack=True, prebook=None):
        """The step's gradient slabs and loss partials (the fused launch; mixed programs: plus the
        high-order chain on a side stream, joined before return).  ``saved`` / ``J`` / ``work``: the
        persistent step buffers of ``jet_hip.alloc_forward`` / ``alloc_backward``.  ``prebook``
        (``jet_hip.prebook_struct``; bf16 step only): the fused launch also does the pre-bookkeeping
        of an Adam step that ends in the one-launch tail - never given under DP or for the bf16x3
        objective."""
        lib = _lib.load()
        fop, cfg = self.fop, self.cfg
        if pack:
            jet_hip.pack_images(saved)
        cur = torch.cuda.current_stream(flat.device)
        side = self._side
        hop = self.prog.hi_op
        _, _, scratch, _, spec, S = saved
        spec_arr = (ctypes.c_int * len(spec))(*spec)

        def fused():
            rc = lib.tdq_fused_step_launch(self.func, _lib.ptr(self.X), _lib.ptr(scratch), _lib.ptr(work), self.N,
                                           cfg["d_in"], jet_hip._warg(cfg), cfg["d_out"], cfg["n_hidden"], S,
                                           spec_arr, self.G, _lib.ptr(fop.ptrs), _lib.ptr(self.lpart),
                                           self.prow, self.nacc, int(self.lo), _lib.ptr(prebook),
                                           _lib.stream_ptr(flat.device))
            _lib.check(rc, "tdq_fused_step_launch")

        if side is None:
            fused()
            return
        # which branch is captured first.  With >= 32 CUs left to the side chain (AC-baseline 50k:
        # 56) the fused launch goes first and no longer starts ~11 us into the step behind the
        # fork: 0.1638 vs 0.1736 ms/step (profiles/r6aj_ac_baseline_split_order.txt).  With few free
        # CUs (AC-dist 500k: 7) the jet_hi forward launched second waited for the whole fused launch
        # (964 us) and the chain ran after it (profiles/r6am_*): side chain first
        order = os.environ.get("TDQ_FS_SPLIT_ORDER", "fused_first" if self.free_cus >= 32 else "side_first")
        ev = torch.cuda.Event()
        ev.record(cur)
        if order != "side_first":
            fused()
        side.wait_event(ev)
        with torch.cuda.stream(side):   # the high-order outputs' chain
            hop.forward(J, flat)
            self.fop2.run_range(J, 0, self.fop2.n_blocks)
            hop.backward(self.fop2.dJ, flat)
        if order == "side_first":
            fused()
        cur.wait_stream(side)

    def set_timing_buffer(self, buf):
        """Phase-stamp build only: the int64 buffer of the stamps ([G * 8 waves][64])."""
        _lib.check(_lib.load().tdq_rtc_set_global_ptr(self.module, b"tdq_ts", ctypes.c_void_p(buf.data_ptr())),
                   "tdq_rtc_set_global_ptr")

    def tail_kw(self):
        """Keyword arguments of ``jet_hip.step_tail`` / ``dp_tail_a`` for this step's rows (the slab
        precision follows the program's: bf16 rows for bf16, fp32 rows for bf16x3)."""
        return {"rows": self.G, "lpart": self.lpart, "n_lblocks": self.n_lblocks}


def for_program(prog):
    """The program's :class:`FusedStepOp` (built once), or ``None`` (reason in
    ``prog.fused_step_reason``)."""
    if getattr(prog, "_fused_step_built", False):
        return prog._fused_step
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        # module loads cannot run inside a capture: the engines build the op before capturing
        # (fit.AdamEngine._capture, the L-BFGS drivers' first eager evaluation) - never cache a
        # "not available" decided here
        warnings.warn("fused training step first requested inside a graph capture; using separate launches")
        return None
    prog._fused_step_built = True
    prog._fused_step = None
    fop = getattr(prog, "fused_op", None)
    why = ineligible(prog, fop)
    if why is None:
        try:
            prog._fused_step = FusedStepOp(prog, fop)
        except Exception as e:  # noqa: BLE001 - the separate launches serve every program
            why = f"{type(e).__name__}: {e}"
            warnings.warn(f"fused training step unavailable, using separate launches: {why}")
    prog.fused_step_reason = why
    return prog._fused_step
