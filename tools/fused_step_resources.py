"""Register / LDS / spill report of the generated fused-step kernels (bf16 step and bf16x3
objective) for the AC-SA program and for systems (the NLS program on networks with 2 and 4 outputs:
``nls2_*`` on [2, 128 x 4, 2], ``nls4_*`` on [2, 128 x 3, 4]), compiled offline with hipcc for gfx950
(no GPU needed), each with the options it runs with (``fused_step._opts``: the bf16x3 kernel's
differ):

    python tools/fused_step_resources.py [--out DIR]

Prints hipcc's kernel-resource-usage remarks (VGPRs, AGPRs, spills, LDS, occupancy) and leaves the
source (``.hip``) and its assembly (``.s``) in DIR; ``diff`` two DIRs' ``.s`` (without their
``__hip_cuid`` lines) to see whether a header change altered a kernel."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def nls(layers, n_f=400):
    """The nonlinear Schroedinger system (examples/schrodinger.py) on ``layers``; outputs past the
    second enter the second residual."""
    import math
    import numpy as np
    import torch
    import tensordiffeq_amd as tdq
    from tensordiffeq_amd.boundaries import IC, DomainND, periodicBC
    d_out = layers[-1]
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-5.0, 5.0], 16)
    D.add("t", [0.0, math.pi / 2], 16)
    D.generate_collocation_points(n_f)

    def deriv_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        return h[:, 0:1], h[:, 1:2], tdq.grad(h[:, 0:1], x), tdq.grad(h[:, 1:2], x)

    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        u, v = h[:, 0:1], h[:, 1:2]
        sq = u * u + v * v
        r1 = -tdq.grad(v, t) + 0.5 * tdq.grad(tdq.grad(u, x), x) + sq * u
        r2 = tdq.grad(u, t) + 0.5 * tdq.grad(tdq.grad(v, x), x) + sq * v
        for k in range(2, d_out):
            w = h[:, k:k + 1]
            r2 = r2 + 0.3 * w * tdq.grad(w, t) - 0.1 * tdq.grad(tdq.grad(w, x), x) + 0.2 * tdq.grad(w, x)
        return r1, r2

    funs = [lambda x: 1.0 / np.cosh(x), lambda x: 0.0 * x, lambda x: 0.1 * np.sin(x), lambda x: 0.2 * np.cos(x)]
    m = tdq.CollocationSolverND(verbose=False)
    m.compile(list(layers), f_model, D, [IC(D, funs[:d_out], var=[["x"]] * d_out), periodicBC(D, ["x"], [deriv_model])],
              backend="jet", device="cpu", Adaptive_type="self-adaptive",
              dict_adaptive={"residual": [True, False], "BCs": [True, False]},
              init_weights={"residual": [torch.rand(n_f, 1), None], "BCs": [torch.rand(16, 1), None]})
    return m


def sources():
    import torch
    import bench
    from tensordiffeq_amd import fusion
    from tensordiffeq_amd.ops import fused_step
    from tensordiffeq_amd.ops.loss_fused import FusedLossOp
    out = {}
    for tag, m in (("", bench.build_problem(400, 1, "jet", torch.device("cpu"), False)),
                   ("nls2_", nls([2, 128, 128, 128, 128, 2])), ("nls4_", nls([2, 128, 128, 128, 4]))):
        prog = m.program()
        fl = fusion.build(prog, m.lambdas)
        op = FusedLossOp(fl, prog, m.lambdas, fusion.scalar_values(fl, m.lambdas, None), fl.lam_offsets)
        for prec in ("bf16", "bf16x3"):
            out[tag + prec] = fused_step.program_recipe(prog, op, prec)[0].source
    return out


def main():
    from tensordiffeq_amd.ops import fused_step
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="/tmp/fused_step_src")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name, src in sources().items():
        path = os.path.join(a.out, f"fused_step_{name}.hip")
        with open(path, "w") as f:
            f.write(src.replace('extern "C" __global__', '#include <hip/hip_runtime.h>\nextern "C" __global__', 1))
        r = subprocess.run(["hipcc", "--offload-arch=gfx950"] + fused_step._opts(src).split() +
                           ["--cuda-device-only", "-S", path, "-o", path[:-4] + ".s",
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        print(f"== {name} (rc {r.returncode})")
        for ln in r.stderr.splitlines():
            if "remark" in ln or "error" in ln:
                print("  " + ln.split("remark: ")[-1])


if __name__ == "__main__":
    main()
