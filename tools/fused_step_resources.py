"""Register / LDS / spill report of the generated fused-step kernels (bf16 step and bf16x3
objective) for the AC-SA program, compiled offline with hipcc for gfx950 (no GPU needed), each
with the options it runs with (``fused_step._opts``: the bf16x3 kernel's differ):

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


def sources():
    import torch
    import bench
    from tensordiffeq_amd import fusion
    from tensordiffeq_amd.ops import fused_step
    from tensordiffeq_amd.ops.loss_fused import FusedLossOp
    m = bench.build_problem(400, 1, "jet", torch.device("cpu"), False)
    prog = m.program()
    fl = fusion.build(prog, m.lambdas)
    op = FusedLossOp(fl, prog, m.lambdas, fusion.scalar_values(fl, m.lambdas, None), fl.lam_offsets)
    return {prec: fused_step.program_recipe(prog, op, prec)[0].source for prec in ("bf16", "bf16x3")}


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
