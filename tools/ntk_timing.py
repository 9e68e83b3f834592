"""Cost of the NTK weight update at the AC-SA shape ([2, 128 x 4, 1], 50k collocation points + the
initial and periodic boundary points, ``Adaptive_type="ntk"``, bf16 training precision):

    python tools/ntk_timing.py [--n-f 50000] [--reps 9] [--out profiles/NAME.json]

* one full ``NTKTraceOp.traces()`` call (every forward, seed, norm and sum launch of every loss output);
* the norm kernel of the residual output (``tdq_ntk_norm``; with and without the weight-image launch)
  against the existing exact-fp32 backward (``tdq_jet_bwd``: weight images, backward kernel, slab
  reduction) over the same points, seeds and saved streams - the norm kernel runs the backward's adjoint
  chain without the dK GEMMs;
* the Adam step, for the overhead per step at ``ntk_every=100``.

``--shape wave128`` measures the layer-wise path instead (``LayeredNTKOp``: five streams at width 128, outside
the norm kernel's envelope): the 1-D wave program of examples/wave-ntk.py on [2, 128 x 3, 1] with 10,000
collocation points; one ``traces()`` call of ``LayeredNTKOp`` against one of ``TorchNTK`` on the same program,
alternating inside every repetition, and the Adam step at ``ntk_every=100`` on each path
(``TDQ_NTK_LAYERED=0`` selects the torch path).

Every time is a host clock around launches that end in a device synchronise, after warm-up calls; the
two kernels alternate inside each repetition; medians and ranges over the repetitions.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(n_f, device):
    import math
    import numpy as np
    import torch
    import tensordiffeq_amd as tdq
    from tensordiffeq_amd.boundaries import IC, DomainND, periodicBC
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 512)
    D.add("t", [0.0, 1.0], 201)
    D.generate_collocation_points(n_f)

    def deriv_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        return u, tdq.grad(u, x)

    def f_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        return tdq.grad(u, t) - 0.0001 * tdq.grad(tdq.grad(u, x), x) + 5.0 * u ** 3 - 5.0 * u

    bcs = [IC(D, [lambda x: x ** 2 * np.cos(math.pi * x)], var=[["x"]]), periodicBC(D, ["x"], [deriv_model])]
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 128, 128, 128, 128, 1], f_model, D, bcs, Adaptive_type="ntk", ntk_every=100, backend="hip",
              device=device, precision="bf16", newton_precision="bf16x3")
    return m


def build_wave(n_f, device, width=128):
    import math
    import numpy as np
    import torch
    import tensordiffeq_amd as tdq
    from tensordiffeq_amd.boundaries import IC, DomainND, FunctionNeumannBC, dirichletBC
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [0.0, 1.0], 101)
    D.add("t", [0.0, 1.0], 101)
    D.generate_collocation_points(n_f)

    def u_t(u_model, x, t):
        return tdq.grad(u_model(torch.cat([x, t], 1)), t)

    def f_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        return tdq.grad(tdq.grad(u, t), t) - 4.0 * tdq.grad(tdq.grad(u, x), x)

    bcs = [IC(D, [lambda x: np.sin(math.pi * x) + 0.5 * np.sin(4 * math.pi * x)], var=[["x"]]),
           FunctionNeumannBC(D, fun=[lambda x: 0.0 * x], var="t", target="lower", deriv_model=[u_t],
                             func_inputs=["x"]),
           dirichletBC(D, val=0.0, var="x", target="lower"), dirichletBC(D, val=0.0, var="x", target="upper")]
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, width, width, width, 1], f_model, D, bcs, Adaptive_type="ntk", ntk_every=100, backend="hip",
              device=device, precision="bf16")
    return m


def wave128(a):
    """The layer-wise path against the torch path on the wave program (see the module docstring)."""
    import warnings
    import torch
    from tensordiffeq_amd.ops import ntk
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return 1e3 * (time.perf_counter() - t0)

    os.environ["TDQ_NTK_LAYERED"] = "1"
    m = build_wave(a.n_f, "cuda")
    op = m._ntk_op()
    assert op.kind == "hip-layered", m.program().reasons
    prog = op.prog
    top = ntk.TorchNTK(prog, op.fl, m.lambdas)
    ops = {"layered": op, "torch": top}
    for o in ops.values():
        for _ in range(3):
            o.traces()
    ms = {k: [] for k in ops}
    for _ in range(a.reps):
        for k, o in ops.items():        # alternating inside every repetition
            ms[k].append(timed(o.traces))
    T_l, T_t = op.traces().double().cpu(), top.traces().double().cpu()

    def adam(env):
        os.environ["TDQ_NTK_LAYERED"] = env
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mm = build_wave(a.n_f, "cuda")
            kind = mm._ntk_op().kind
            mm.fit(tf_iter=64)
            sync()
            v = []
            for _ in range(3):
                t0 = time.perf_counter()
                mm.fit(tf_iter=a.steps)   # a multiple of ntk_every: includes steps / 100 weight updates
                sync()
                v.append(1e3 * (time.perf_counter() - t0) / a.steps)
        return kind, v

    steps = {}
    for env in ("1", "0", "1", "0"):    # alternating
        kind, v = adam(env)
        steps.setdefault(kind, []).extend(v)
    os.environ["TDQ_NTK_LAYERED"] = "1"
    lay, tor = _stat(ms["layered"]), _stat(ms["torch"])
    out = {"shape": "wave128", "n_f": a.n_f, "points": int(prog.X_all.shape[0]),
           "layers": list(prog.net.layer_sizes), "S": op.S, "outputs": len(op.outputs),
           "forwards_per_traces_call": len(op.launches),
           "traces_ms": {"hip-layered": lay, "torch": tor},
           "torch_over_layered": tor["median"] / lay["median"],
           # the README's rule for defaults: the medians differ by more than three times the torch path's range
           "layered_faster_by_rule": bool(tor["median"] - lay["median"] > 3 * (tor["max"] - tor["min"])),
           "worst_rel_difference_of_traces": float(((T_l - T_t).abs() / T_t).max()),
           "adam_ms_per_step_ntk_every_100": {k: _stat(v) for k, v in steps.items()}}
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return out


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main(argv=None):
    import torch
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", choices=["acsa", "wave128"], default="acsa",
                    help="acsa: the norm kernel at the AC-SA shape (default); wave128: the layer-wise path")
    ap.add_argument("--n-f", type=int, default=None, help="collocation points (acsa 50000, wave128 10000)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5, help="launches per timed window")
    ap.add_argument("--steps", type=int, default=300, help="Adam steps per timed block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/ntk_timing.py measures on the GPU; none found")
    if a.n_f is None:
        a.n_f = 10000 if a.shape == "wave128" else 50000
    if a.shape == "wave128":
        return wave128(a)
    from tensordiffeq_amd.ops import jet_hip, ntk
    m = build(a.n_f, "cuda")
    op = m._ntk_op()
    assert op.kind == "hip", m.program().reasons
    prog, fop = op.prog, op.fop
    sync = torch.cuda.synchronize

    def timed(fn, n=1):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return 1e3 * (time.perf_counter() - t0) / n

    for _ in range(3):
        op.traces()
    traces = [timed(op.traces) for _ in range(a.reps)]

    # the residual output: its group, one forward over its points, its seeds
    gi = [i for i, gr in enumerate(fop.fl.groups) if gr.n == a.n_f][0]
    gr = fop.fl.groups[gi]
    off = prog.segments[gr.segs[0]].offset
    X = prog.X_all[off:off + gr.n]
    P = prog.net.flat.detach()
    J, saved = jet_hip.forward_raw(X, P, prog.net, prog.plan, precision="fp32")
    dJ = ntk.seeds(fop, gi, 0, J, X, torch.zeros_like(J), 0, gr.n, [0])
    Kp = ntk.pad_kp(P, op.cfg)
    n2 = torch.zeros(gr.n, device="cuda")
    grad = torch.empty_like(P)
    runs = {"norm": lambda: ntk.instance_norms(saved, dJ, Kp, gr.n, out=n2),
            "pad_norm": lambda: (ntk.pad_kp(P, op.cfg, Kp), ntk.instance_norms(saved, dJ, Kp, gr.n, out=n2)),
            "jet_bwd": lambda: jet_hip.backward_raw(saved, dJ, grad=grad),
            "jet_fwd": lambda: jet_hip.forward_raw(X, P, prog.net, prog.plan, precision="fp32")}
    for fn in runs.values():
        timed(fn, 3)
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():      # alternating inside every repetition
            ms[k].append(timed(fn, a.inner))

    m.fit(tf_iter=64)
    sync()
    step = []
    for _ in range(3):
        t0 = time.perf_counter()
        m.fit(tf_iter=a.steps)    # a multiple of ntk_every: includes steps / 100 weight updates
        sync()
        step.append(1e3 * (time.perf_counter() - t0) / a.steps)
    m2 = build(a.n_f, "cuda")
    m2.ntk_every = 10 ** 9        # the same program and weights, never updated after epoch 0
    m2.fit(tf_iter=64)
    sync()
    plain = []
    for _ in range(3):
        t0 = time.perf_counter()
        m2.fit(tf_iter=a.steps)
        sync()
        plain.append(1e3 * (time.perf_counter() - t0) / a.steps)

    out = {"n_f": a.n_f, "points": int(prog.X_all.shape[0]), "layers": list(prog.net.layer_sizes), "S": op.S,
           "outputs": len(op.outputs), "forwards_per_traces_call": len(op.launches),
           "traces_ms": _stat(traces), "kernels_ms": {k: _stat(v) for k, v in ms.items()},
           "adam_ms_per_step_ntk_every_100": _stat(step), "adam_ms_per_step_no_update": _stat(plain)}
    nm, bw = out["kernels_ms"]["pad_norm"], out["kernels_ms"]["jet_bwd"]
    out["pad_norm_over_jet_bwd"] = nm["median"] / bw["median"]
    # "no slower" unless the medians differ by more than three times the backward's own range
    out["norm_slower_than_bwd"] = bool(nm["median"] - bw["median"] > 3 * (bw["max"] - bw["min"]))
    out["traces_ms_per_step_at_ntk_every_100"] = out["traces_ms"]["median"] / 100
    out["overhead_per_step_fraction"] = out["traces_ms_per_step_at_ntk_every_100"] / statistics.median(plain)
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == "__main__":
    main()
