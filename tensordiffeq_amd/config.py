"""Configuration: constructor kwargs stay the primary interface (reference parity, SURVEY.md §5
"Config / flag system"); :class:`SolverConfig` gathers the framework-level knobs with ``TDQ_*``
environment overrides so that a run can be re-tuned without code changes.

=====================  ==========================  =========================================
field                  env var                     meaning
=====================  ==========================  =========================================
backend                TDQ_BACKEND                 auto | hip | jet | autograd
precision              TDQ_PRECISION               bf16x3 (split-bf16 MFMA) | bf16 (bf16 MFMA operands,
                                                   fp32 accumulate / jets / master weights) | fp32
newton_precision       TDQ_NEWTON_PRECISION        jet precision of the L-BFGS phase (default: precision)
newton_schedule        TDQ_NEWTON_SCHEDULE         leading L-BFGS phases "prec:iters,..." before the
                                                   newton_precision phase (e.g. "bf16:7000")
seed                   TDQ_SEED                    global seed applied at compile
periodic_legacy        TDQ_PERIODIC_LEGACY         1: reference periodic-BC quirk (B12)
log_every              TDQ_LOG_EVERY               progress / metrics cadence (steps)
metrics_path           TDQ_METRICS                 JSONL metrics file (rank-suffixed under DP)
graphs                 TDQ_NO_GRAPH=1 disables     HIP-graph capture of the training step
fused_loss             TDQ_FUSED_LOSS=0 disables   single-kernel loss program
allow_torch_fallback   TDQ_ALLOW_TORCH_FALLBACK    1: let GPU runs fall back to torch ops
lbfgs                  TDQ_LBFGS                   auto (device on GPU, host on CPU) | device
                                                   (GPU-resident kernels, graph-replayed) | host
lbfgs_stop             TDQ_LBFGS_STOP              legacy (default: the reference's effective |f| < tolX,
                                                   optimizers.py:273) | fixed (|f - f_old| < tolX)
force_dp               TDQ_FORCE_DP=1              DP machinery (process group, bucket all-reduce)
                                                   even at world 1 (parallel/dist.py)
dp_graph               TDQ_DP_GRAPH=0 disables     RCCL all-reduce captured inside the step graph
nan_check              TDQ_NAN_CHECK=0 disables    device loss-history NaN/Inf scan (fit.py)
(fused_step)           TDQ_FUSED_STEP=0 disables   one-launch forward -> loss -> backward (bf16 Adam
                                                   step, bf16x3 L-BFGS objective; ops/fused_step.py)
(tail_one)             TDQ_TAIL_ONE=0 disables     one-launch step tail after the fused step (a workgroup
                                                   owns 256 theta columns from the slab rows to Adam;
                                                   0: the two launches) and the one-launch slab
                                                   reduction of the L-BFGS objective / DP step (bf16
                                                   slab rows; fp32 rows always take two passes)
(split)                TDQ_SPLIT                   auto (cut at 0.38 for bf16, 0.35 for bf16x3) | off | cut
                                                   fraction: two point ranges on concurrent graph
                                                   branches (fit.point_ranges)
(hi_kernel)            TDQ_HI_KERNEL=0 disables    high-order (order 3 / 4) jet kernels: those points'
                                                   streams on the torch jet (models/loss.py)
(hi_scratch)           TDQ_HI_SCRATCH_BYTES        byte cap of the high-order kernels' activation scratch
                                                   (default 32 GiB); above it a residual with order-3/4
                                                   derivatives keeps the torch jet backend (ops/jet_hi.py)
(hi_tile)              TDQ_HI_TILE                 auto | 4 | 8 | 16: points per workgroup of the
                                                   high-order kernels (auto: 8 from 20,000 points on)
(lbfgs_fused)          TDQ_LBFGS_FUSED=0           five-launch L-BFGS update instead of two
(causal_kernel)        TDQ_CAUSAL_KERNEL=0         causal weights (Adaptive_type 4) updated by the torch
                                                   mirror on the GPU instead of csrc/causal.hip
                                                   (ops/causal.py: the A/B and fallback switch)
(r3_kernel)            TDQ_R3_KERNEL=0             R3 resampling (compile(resample="r3")) by the torch
                                                   mirror on the GPU instead of csrc/r3.hip
                                                   (ops/r3.py: the A/B and fallback switch)
(profiling)            TDQ_PROFILE                 directory: every fit() runs under torch.profiler
                                                   -> trace.json + kernels.txt (profiling.py)
=====================  ==========================  =========================================
"""
from __future__ import annotations

import dataclasses
import os


def _env_bool(name, default):
    v = os.environ.get(name)
    if v is None:
        return default
    return v.strip().lower() in ("1", "true", "yes", "on")


# L-BFGS function-change test used by every entry point (solver, eager_lbfgs, DeviceLBFGS,
# minimize): "legacy" = the reference's effective |f| < tolX (optimizers.py:273)
DEFAULT_LBFGS_STOP = "legacy"


@dataclasses.dataclass(frozen=True)
class SolverConfig:
    backend: str = "auto"
    precision: str = "bf16x3"
    newton_precision: str | None = None
    # L-BFGS precision schedule: leading phases "prec:iters[,prec:iters...]" before the
    # newton_precision phase takes the remaining iterations (e.g. "bf16:7000")
    newton_schedule: str | None = None
    seed: int | None = None
    periodic_legacy: bool = False
    log_every: int = 100
    metrics_path: str | None = None
    graphs: bool = True
    fused_loss: bool = True
    allow_torch_fallback: bool = False
    lbfgs: str = "auto"
    # the reference's effective test (|f| < tolX, i.e. run to maxIter): on AC-SA it reaches L2
    # 2.2/2.7/2.0e-2 (seeds 0-2) against 3.7/2.7/3.4e-2 with |f - f_old| < tolX, which stops
    # L-BFGS after ~5k of 10k iterations (profiles/r3_lbfgs_stop_ab.jsonl)
    lbfgs_stop: str = DEFAULT_LBFGS_STOP

    @classmethod
    def from_env(cls, **overrides):
        """Defaults <- TDQ_* environment <- explicit ``overrides`` (``None`` values are ignored)."""
        e = os.environ
        vals = {
            "backend": e.get("TDQ_BACKEND", cls.backend),
            "precision": e.get("TDQ_PRECISION", cls.precision),
            "newton_precision": e.get("TDQ_NEWTON_PRECISION") or None,
            "newton_schedule": e.get("TDQ_NEWTON_SCHEDULE") or None,
            "seed": int(e["TDQ_SEED"]) if "TDQ_SEED" in e else None,
            "periodic_legacy": _env_bool("TDQ_PERIODIC_LEGACY", False),
            "log_every": int(e.get("TDQ_LOG_EVERY", cls.log_every)),
            "metrics_path": e.get("TDQ_METRICS") or None,
            "graphs": not _env_bool("TDQ_NO_GRAPH", False),
            "fused_loss": _env_bool("TDQ_FUSED_LOSS", True),
            "allow_torch_fallback": _env_bool("TDQ_ALLOW_TORCH_FALLBACK", False),
            "lbfgs": e.get("TDQ_LBFGS", cls.lbfgs),
            "lbfgs_stop": e.get("TDQ_LBFGS_STOP", cls.lbfgs_stop),
        }
        vals.update({k: v for k, v in overrides.items() if v is not None})
        cfg = cls(**vals)
        cfg.validate()
        return cfg

    def validate(self):
        if self.backend not in ("auto", "hip", "jet", "autograd"):
            raise ValueError(f"backend {self.backend!r}")
        if self.precision not in ("bf16x3", "bf16", "fp32"):
            raise ValueError(f"precision {self.precision!r}")
        if self.newton_precision not in (None, "bf16x3", "bf16", "fp32"):
            raise ValueError(f"newton_precision {self.newton_precision!r}")
        parse_newton_schedule(self.newton_schedule)
        if self.log_every < 1:
            raise ValueError("log_every must be >= 1")
        if self.lbfgs not in ("auto", "device", "host"):
            raise ValueError(f"lbfgs {self.lbfgs!r}")
        if self.lbfgs_stop not in ("fixed", "legacy"):
            raise ValueError(f"lbfgs_stop {self.lbfgs_stop!r}")

    def apply_process_env(self):
        """Push the process-wide switches that the kernels / engines read."""
        os.environ["TDQ_FUSED_LOSS"] = "1" if self.fused_loss else "0"
        os.environ["TDQ_NO_GRAPH"] = "0" if self.graphs else "1"
        os.environ["TDQ_ALLOW_TORCH_FALLBACK"] = "1" if self.allow_torch_fallback else "0"


def parse_newton_schedule(spec):
    """``"bf16:7000,bf16x3:1000"`` -> ``[("bf16", 7000), ("bf16x3", 1000)]`` (leading L-BFGS phases)."""
    if not spec:
        return []
    out = []
    for part in str(spec).split(","):
        prec, _, n = part.strip().partition(":")
        if prec not in ("bf16x3", "bf16", "fp32") or not n.strip().isdigit():
            raise ValueError(f"newton_schedule entry {part!r}: want precision:iterations")
        out.append((prec, int(n)))
    return out
