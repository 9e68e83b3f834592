"""Cost of R3 resampling in the Adam step at the AC shape ([2, 128 x 4, 1], 50k collocation points + the
initial and periodic boundary points, bf16, the one-launch fused step):

    python tools/r3_timing.py [--n-f 50000] [--steps 2000] [--runs 3] [--out profiles/NAME.json]

Two programs on the same points and boundary set - ``resample="r3"`` and the non-adaptive AC program - are
timed in processes of their own, one process per run, taking turns (r3, none, r3, none, ...), ``--runs`` of
each: a run is ``--steps`` captured Adam steps (a multiple of the 8-step graph) between two device
synchronisations on the host clock, after a warm-up that captures the graphs.  The r3 runs also time the
update alone: ``R3Op.update`` on the adjoint the last step left, eager launches in a timed window.  Medians
and ranges over the runs.  ``--kind r3|none`` is one such run (what the children execute).  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(kind, n_f, device):
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
        return tdq.grad(u, t) - 0.0001 * tdq.grad(tdq.grad(u, x), x) + 5.0 * u * u * u - 5.0 * u

    bcs = [IC(D, [lambda x: x ** 2 * np.cos(math.pi * x)], var=[["x"]]), periodicBC(D, ["x"], [deriv_model])]
    kw = dict(resample="r3", resample_seed=0) if kind == "r3" else {}
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 128, 128, 128, 128, 1], f_model, D, bcs, backend="hip", device=device, precision="bf16",
              newton_precision="bf16x3", **kw)
    return m


def one_run(kind, n_f, steps):
    """One process's measurement: ``{"kind", "adam_ms_per_step", ...}``."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/r3_timing.py measures on the GPU; none found")
    sync = torch.cuda.synchronize
    m = build(kind, n_f, "cuda")
    m.fit(tf_iter=72)          # captures the 1-step and the 8-step graph
    eng = m._get_engine(None, steps)
    out = {"kind": kind, "tail_launches": eng.tail_launches, "one_launch_step": bool(eng._tail_one()),
           "k_step_graph": eng.graph_k is not None}
    sync()
    t0 = time.perf_counter()
    m.fit(tf_iter=steps)
    sync()
    out["adam_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / steps
    if kind == "r3":
        op = m._r3_op()
        r2 = op.fop.dlam[op.slot]
        for _ in range(10):
            op.update(r2)
        sync()
        t0 = time.perf_counter()
        for _ in range(200):
            op.update(r2)
        sync()
        out["update_us_eager_back_to_back"] = 1e6 * (time.perf_counter() - t0) / 200
        out["kernel"] = "hip" if op.hip else "torch mirror (TDQ_R3_KERNEL=0)"
        out["destinations"] = len(op.dests)
        out["stats"] = m.resample_stats()
    return out


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-f", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=2000, help="Adam steps per timed run")
    ap.add_argument("--runs", type=int, default=3, help="runs of each program (alternating, one process each)")
    ap.add_argument("--kind", default=None, choices=["r3", "none"], help="one run in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.kind is not None:
        res = one_run(a.kind, a.n_f, a.steps)
        print("R3_TIMING_RUN " + json.dumps(res))
        return res
    runs = {"r3": [], "none": []}
    for _ in range(max(3, a.runs)):
        for kind in ("r3", "none"):            # alternating, a fresh process each
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kind", kind, "--n-f", str(a.n_f),
                                "--steps", str(a.steps)], capture_output=True, text=True, timeout=600)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("R3_TIMING_RUN ")), None)
            if p.returncode != 0 or line is None:
                sys.exit(f"run {kind} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[kind].append(json.loads(line[len("R3_TIMING_RUN "):]))
    out = {"n_f": a.n_f, "steps_per_run": a.steps, "precision": "bf16",
           "engines": {k: {f: v[0][f] for f in ("tail_launches", "one_launch_step", "k_step_graph")}
                       for k, v in runs.items()},
           "adam_ms_per_step": {k: _stat([r["adam_ms_per_step"] for r in v]) for k, v in runs.items()},
           "update_us_eager_back_to_back": _stat([r["update_us_eager_back_to_back"] for r in runs["r3"]]),
           "kernel": runs["r3"][0]["kernel"], "destinations": runs["r3"][0]["destinations"],
           "last_stats": runs["r3"][-1]["stats"]}
    med = {k: out["adam_ms_per_step"][k]["median"] for k in runs}
    out["r3_minus_none_us"] = 1e3 * (med["r3"] - med["none"])
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == "__main__":
    main()
