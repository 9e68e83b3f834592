"""Adam step and L-BFGS iteration time of examples/kdv.py ([2, 128 x 4, 1], 20k collocation points).

One run (one process, one JSON line):

    python tools/kdv_timing.py [--root TREE] [--precision bf16x3] [--n-f 20000] [--tile auto|4|8|16]

``--root TREE`` imports the package from another checkout (built there) with this tree's example: on
a tree from before the high-order residual path the same program plans as ``jet`` (torch Taylor
jets), here as ``hip`` (fused jet kernels + the high-order kernels' tile variant).  ``--tile`` forces
the high-order kernels' points per workgroup (``TDQ_HI_TILE``).

Drivers (each run a fresh process, alternating):

    python tools/kdv_timing.py --ab PARENT_TREE --out profiles/NAME.json     # 4 + 4 runs per precision
    python tools/kdv_timing.py --sweep --out profiles/NAME.jsonl             # tile x point-count sweep

Step time = host clock around ``fit(tf_iter=steps)`` ending in a device synchronise, after a warm-up
``fit`` that also captures the step graphs; three timed blocks per run (median reported, all kept).
L-BFGS: host clock around ``fit(newton_iter=)`` over the iterations it ran.  Needs a GPU (without one
it only rehearses at a tiny size).
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def one_run(a):
    root = os.path.abspath(a.root or ROOT)
    sys.path.insert(0, root)
    if a.tile != "auto":
        os.environ["TDQ_HI_TILE"] = a.tile
    import torch
    import tensordiffeq_amd  # noqa: F401 - from --root, before the example puts its own tree on the path
    ex = os.path.join(ROOT, "examples")
    sys.path.append(ex)
    spec = importlib.util.spec_from_file_location("kdv", os.path.join(ex, "kdv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from _common import parser
    gpu = torch.cuda.is_available()
    n_f = a.n_f if gpu else 300
    ap = parser("t")
    ap.add_argument("--sa", action="store_true")
    args = ap.parse_args(["--n-f", str(n_f), "--quiet", "--device", "cuda" if gpu else "cpu", "--backend", a.backend]
                         + (["--precision", a.precision] if a.precision else []))
    model, _ = mod.build(args)
    prog = model.program()
    sync = torch.cuda.synchronize if gpu else (lambda: None)
    slow = prog.backend != "hip"
    warm, steps = (8, 40) if slow else (64, a.steps)
    if not gpu:
        warm, steps = 2, 3
    model.fit(tf_iter=warm)
    sync()
    blocks = []
    for _ in range(3):
        t0 = time.perf_counter()
        model.fit(tf_iter=steps)
        sync()
        blocks.append(1e3 * (time.perf_counter() - t0) / steps)
    out = {"root": os.path.relpath(root, ROOT), "backend": prog.backend, "precision": prog.precision,
           "n_f": int(n_f), "points": int(prog.X_all.shape[0]), "n_hi": int(getattr(prog, "n_hi", 0)),
           "fused_loss": prog.fused_op is not None, "steps": steps, "adam_ms_blocks": blocks,
           "adam_ms_per_step": statistics.median(blocks)}
    hop = getattr(prog, "hi_op", None)
    out["hi_tile"] = [getattr(hop, "tile", 4), getattr(hop, "tile_bwd", 4)] if hop is not None else None
    out["Mpts_per_s"] = out["points"] / out["adam_ms_per_step"] / 1e3
    if a.newton:
        model.fit(newton_iter=4 if gpu else 2)   # warm-up: builds (and captures) the objective
        sync()
        t0 = time.perf_counter()
        model.fit(newton_iter=(10 if slow else a.newton) if gpu else 2)
        sync()
        n_it = int((model.fit_info.get("lbfgs") or {}).get("n_iter", 0))
        out["lbfgs_iters"] = n_it
        out["lbfgs_ms_per_iter"] = 1e3 * (time.perf_counter() - t0) / max(1, n_it)
    out["loss"] = float(model.losses[-1]["Total Loss"])
    print("KDV " + json.dumps(out), flush=True)
    return out


def child(extra, timeout=600):
    """One run in a fresh process; its JSON line or None."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, capture_output=True, text=True,
                       timeout=timeout)
    for line in r.stdout.splitlines():
        if line.startswith("KDV "):
            return json.loads(line[4:])
    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
    raise RuntimeError(f"run {extra} failed with exit status {r.returncode}")


def _stat(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "runs": vals}


def ab(a):
    """This tree against ``a.ab``: 4 + 4 alternating runs per precision; medians and ranges."""
    out = {"parent": os.path.relpath(os.path.abspath(a.ab), ROOT), "n_f": a.n_f}
    for prec in ("bf16x3", "bf16"):
        runs = {"new": [], "parent": []}
        for _ in range(4):
            for name, root in (("new", ROOT), ("parent", a.ab)):
                runs[name].append(child(["--root", root, "--precision", prec, "--n-f", str(a.n_f), "--newton",
                                         str(a.newton), "--steps", str(a.steps)]))
                print(prec, name, runs[name][-1], flush=True)
        res = {}
        for name, rr in runs.items():
            res[name] = {"backend": rr[0]["backend"], "hi_tile": rr[0]["hi_tile"],
                         "adam_ms_per_step": _stat([r["adam_ms_per_step"] for r in rr]),
                         "lbfgs_ms_per_iter": _stat([r["lbfgs_ms_per_iter"] for r in rr])}
        for key in ("adam_ms_per_step", "lbfgs_ms_per_iter"):
            p, n = res["parent"][key], res["new"][key]
            gain = p["median"] - n["median"]
            res[key + "_ratio_parent_over_new"] = p["median"] / n["median"]
            # "faster" only when the gain exceeds three times the parent's own run-to-run range
            res[key + "_faster"] = bool(gain > 3 * (p["max"] - p["min"]))
        out[prec] = res
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return out


def sweep(a):
    """Adam step time with the tile forced to 4 / 8 / 16 at 2,048 / 5,000 / 20,000 / 50,000 collocation
    points, two processes each (alternating over the tiles), one JSON line per run."""
    lines = []
    for n_f in (2048, 5000, 20000, 50000):
        for rep in range(2):
            for tile in ("4", "8", "16"):
                r = child(["--precision", a.precision or "bf16x3", "--n-f", str(n_f), "--tile", tile, "--newton", "0",
                           "--steps", str(a.steps)])
                r["rep"] = rep
                lines.append(r)
                print(json.dumps(r), flush=True)
                if a.out:
                    with open(a.out, "w") as fh:
                        fh.write("".join(json.dumps(x) + "\n" for x in lines))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=None, help="checkout whose package runs (default: this tree)")
    ap.add_argument("--precision", default=None)
    ap.add_argument("--backend", default="auto")
    ap.add_argument("--n-f", type=int, default=20000)
    ap.add_argument("--tile", default="auto")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--newton", type=int, default=60, help="timed L-BFGS iterations (0: none)")
    ap.add_argument("--ab", default=None, metavar="PARENT_TREE")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.ab:
        return ab(a)
    if a.sweep:
        return sweep(a)
    return one_run(a)


if __name__ == "__main__":
    main()
