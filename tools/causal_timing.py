"""Cost of the causal weight update in the Adam step at the AC shape ([2, 128 x 4, 1], 50k collocation
points + the initial and periodic boundary points, bf16, the one-launch fused step):

    python tools/causal_timing.py [--n-f 50000] [--steps 400] [--runs 3] [--out profiles/NAME.json]

Three solvers of one process on the same points and boundary set - ``Adaptive_type="causal"``, the AC-SA
program (self-adaptive weights on the residual and the IC) and the non-adaptive AC program - take turns:
each run is ``--steps`` captured Adam steps (a multiple of the 8-step graph) between two device
synchronisations on the host clock, after a warm-up that captures the graphs; ``--runs`` rounds of the
three, alternating.  Also the update's own time: ``CausalOp.update`` alone, eager launches in a timed window.
Medians and ranges over the runs.  Needs a GPU."""
import argparse
import json
import os
import statistics
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
    kw = {}
    if kind == "causal":
        kw = dict(Adaptive_type="causal", causal_eps=[1e-2, 1e-1, 1.0, 10.0, 100.0], causal_bins=32,
                  causal_every=10 ** 9, causal_bc_weights=[100.0, 1.0])
    elif kind == "sa":
        g = torch.Generator().manual_seed(0)
        kw = dict(Adaptive_type="self-adaptive", dict_adaptive={"residual": [True], "BCs": [True, False]},
                  init_weights={"residual": [torch.rand(n_f, 1, generator=g)],
                                "BCs": [100 * torch.rand(512, 1, generator=g), None]})
    m = tdq.CollocationSolverND(verbose=False)
    m.compile([2, 128, 128, 128, 128, 1], f_model, D, bcs, backend="hip", device=device, precision="bf16",
              newton_precision="bf16x3", **kw)
    return m


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main(argv=None):
    import torch
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-f", type=int, default=50000)
    ap.add_argument("--steps", type=int, default=400, help="Adam steps per timed run")
    ap.add_argument("--runs", type=int, default=3, help="rounds of the three solvers (alternating)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/causal_timing.py measures on the GPU; none found")
    sync = torch.cuda.synchronize
    kinds = ("causal", "sa", "none")
    models = {k: build(k, a.n_f, "cuda") for k in kinds}
    info = {}
    for k, m in models.items():
        m.fit(tf_iter=72)          # captures the 1-step and the 8-step graph
        eng = m._get_engine(None, a.steps)
        info[k] = {"tail_launches": eng.tail_launches, "one_launch_step": bool(eng._tail_one()),
                   "k_step_graph": eng.graph_k is not None}
    sync()
    ms = {k: [] for k in kinds}
    for _ in range(max(3, a.runs)):
        for k in kinds:            # alternating
            m = models[k]
            sync()
            t0 = time.perf_counter()
            m.fit(tf_iter=a.steps)
            sync()
            ms[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
    # the update alone, on the adjoint the last step left
    op = models["causal"]._causal_op()
    r2 = op.fop.dlam[op.slot]
    for _ in range(10):
        op.update(r2)
    upd = []
    for _ in range(max(3, a.runs)):
        sync()
        t0 = time.perf_counter()
        for _ in range(200):
            op.update(r2)
        sync()
        upd.append(1e6 * (time.perf_counter() - t0) / 200)
    out = {"n_f": a.n_f, "steps_per_run": a.steps, "precision": "bf16", "bins": op.bins, "engines": info,
           "adam_ms_per_step": {k: _stat(v) for k, v in ms.items()},
           "update_us_eager_back_to_back": _stat(upd),
           "kernel": "hip" if op.hip else "torch mirror (TDQ_CAUSAL_KERNEL=0)"}
    med = {k: out["adam_ms_per_step"][k]["median"] for k in kinds}
    out["causal_minus_none_us"] = 1e3 * (med["causal"] - med["none"])
    out["causal_minus_sa_us"] = 1e3 * (med["causal"] - med["sa"])
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == "__main__":
    main()
