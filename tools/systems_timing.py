"""Adam step time of examples/schrodinger.py ([2, 100 x 4, 2], 20k collocation points) on the jet path
(``backend="auto"``: HIP jet kernels + fused loss) and on ``backend="autograd"`` (nested autograd, what
a system paid before it could be planned on the jet), each twice, alternating, in one process.

    python tools/systems_timing.py [--width 128] [--precision bf16] [--out profiles/NAME.json]

``--width 128`` is the width the one-launch step serves (``TDQ_FUSED_STEP_SYSTEMS=0`` keeps the separate
launches); the route taken is recorded as ``fused_step`` / ``fused_step_reason``.

Step time = host clock around ``fit(tf_iter=steps)`` ending in a device synchronise, after a warm-up
``fit`` that also captures the step graphs.  Needs a GPU (without one it only rehearses at a tiny size
and keeps no numbers).
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
for p in (ROOT, EX):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the JSON result here too")
    ap.add_argument("--width", type=int, default=100, help="hidden width of the four layers")
    ap.add_argument("--precision", default=None, help="bf16x3 | bf16 | fp32 (default: the solver's)")
    a = ap.parse_args(argv)
    spec = importlib.util.spec_from_file_location("schrodinger", os.path.join(EX, "schrodinger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from _common import parser
    gpu = torch.cuda.is_available()
    n_f = "20000" if gpu else "300"
    out = {"net": [2] + [a.width] * 4 + [2], "n_f": int(n_f),
           "device": torch.cuda.get_device_name(0) if gpu else "cpu"}
    for name, backend, warm, steps in (("new", "auto", 64, 2000), ("autograd", "autograd", 8, 100),
                                       ("new_repeat", "auto", 64, 2000), ("autograd_repeat", "autograd", 8, 100)):
        if not gpu:
            warm, steps = 2, 3
        args = parser("t").parse_args(["--n-f", n_f, "--backend", backend, "--quiet",
                                       "--device", "cuda" if gpu else "cpu"]
                                      + (["--precision", a.precision] if a.precision and backend != "autograd" else []))
        args.width = a.width
        model, _ = mod.build(args)
        prog = model.program()
        model.fit(tf_iter=warm)
        if gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.fit(tf_iter=steps)
        if gpu:
            torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        n = prog.X_all.shape[0]
        out[name] = {"backend": prog.backend, "precision": prog.precision, "fused_loss": prog.fused_op is not None,
                     "engine": getattr(prog.fused_op, "engine", None), "steps": steps, "ms_per_step": 1e3 * dt,
                     "points": n, "Mpts_per_s": n / dt / 1e6, "loss": float(model.losses[-1]["Total Loss"]),
                     "fused_step": getattr(prog, "_fused_step", None) is not None,
                     "fused_step_reason": getattr(prog, "fused_step_reason", None)}
        print(name, out[name], flush=True)
        del model
    out["ratio_autograd_over_new"] = out["autograd"]["ms_per_step"] / out["new"]["ms_per_step"]
    if not gpu:
        return None
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == "__main__":
    main()
