"""Register / LDS / spill table of every instantiated ``ntk_norm_kernel<WT, S, PAIR>`` variant
(``csrc/ntk_trace.hip``), compiled offline with hipcc for gfx950 with the library's flags (no GPU needed):

    python tools/ntk_resources.py [--out FILE]
    python tools/ntk_resources.py --gram [--out FILE]     # ntk_gram_kernel (csrc/ntk_gram.hip) instead

One line per variant: width tiles, streams, pair mode, VGPRs, AGPRs, scratch bytes per lane (spills), the
static LDS and the dynamic LDS the launcher asks for (the wave-private adjoint images, ``4 S WT`` KiB)."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tensordiffeq_amd.csrc import build
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gram", action="store_true", help="the Gram-product kernel of the layer-wise NTK path")
    a = ap.parse_args()
    src = os.path.join(build.HERE, "ntk_gram.hip" if a.gram else "ntk_trace.hip")
    r = subprocess.run([build.hipcc()] + build._flags() + ["--cuda-device-only", "-S", src, "-o", os.devnull,
                                                           "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    rows, cur = [], None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: (.*)$", ln)
        if not m:
            continue
        t = m.group(1).strip()
        k = re.match(r"Function Name: (\S+)", t)
        if k:
            cur = {"name": k.group(1)}
            rows.append(cur)
        elif cur is not None and ":" in t:
            key, val = t.split(":", 1)
            cur[key.strip()] = val.split("[")[0].strip()
    if a.gram:   # one kernel: S, the widths, the load path and pair mode are run-time arguments
        lines = ["# ntk_gram_kernel, hipcc " + " ".join(build._flags()[:3]),
                 f"{'kernel':<16} {'VGPRs':>6} {'AGPRs':>6} {'SGPRs':>6} {'spill VGPRs':>11} {'scratch B/lane':>14} "
                 f"{'LDS static':>10} {'occupancy':>9}"]
        for row in rows:
            if "ntk_gram_kernel" in row["name"]:
                lines.append(f"{'ntk_gram_kernel':<16} {row.get('VGPRs', '?'):>6} {row.get('AGPRs', '?'):>6} "
                             f"{row.get('TotalSGPRs', '?'):>6} {row.get('VGPRs Spill', '?'):>11} "
                             f"{row.get('ScratchSize [bytes/lane]', '?'):>14} "
                             f"{row.get('LDS Size [bytes/block]', '?'):>10} "
                             f"{row.get('Occupancy [waves/SIMD]', '?'):>9}")
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return
    lines = ["# ntk_norm_kernel<WT, S, PAIR>, hipcc " + " ".join(build._flags()[:3]),
             f"{'WT':>3} {'S':>2} {'pair':>4} {'VGPRs':>6} {'AGPRs':>6} {'spill VGPRs':>11} {'scratch B/lane':>14} "
             f"{'LDS static':>10} {'LDS dynamic':>11}"]
    for row in rows:
        m = re.search(r"ntk_norm_kernelILi(\d+)ELi(\d+)ELb([01])E", row["name"])
        if not m:
            continue
        wt, s, pair = int(m.group(1)), int(m.group(2)), int(m.group(3))
        lines.append(f"{wt:>3} {s:>2} {pair:>4} {row.get('VGPRs', '?'):>6} {row.get('AGPRs', '?'):>6} "
                     f"{row.get('VGPRs Spill', '?'):>11} {row.get('ScratchSize [bytes/lane]', '?'):>14} "
                     f"{row.get('LDS Size [bytes/block]', '?'):>10} {4 * s * wt * 256 * 4:>11}")
    lines[2:] = sorted(lines[2:], key=lambda ln: [int(v) for v in ln.split()[:3]])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
