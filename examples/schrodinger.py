"""Nonlinear Schroedinger equation as a system of two PDEs on a two-output network.

i h_t + 1/2 h_xx + |h|^2 h = 0 with h = u + i v on x in [-5, 5], t in [0, pi/2]:
    -v_t + 1/2 u_xx + (u^2 + v^2) u = 0,     u_t + 1/2 v_xx + (u^2 + v^2) v = 0,
h(x, 0) = sech x (u = sech x, v = 0), periodic in x for u, v, u_x, v_x.  The exact solution is the
soliton u = sech x cos(t/2), v = sech x sin(t/2); the relative L2 error of |h| against it is printed,
so the example needs no data file.  Net [2, 100 x 4, 2], N_f = 20,000, Adam 10k + L-BFGS 10k
(``--width 128`` is the width the one-launch step serves; the route is printed).
The components are picked from the network output with ``h[:, 0:1]`` / ``h[:, 1:2]``; the program
runs on the jet kernels (``backend == "hip"`` on a GPU) with the fused loss.
Run:  python examples/schrodinger.py [--iters 10000 --newton 10000]
"""
import math
import time

import numpy as np
import torch

from _common import grid_points, parser, report, solver_kw

import tensordiffeq_amd as tdq
from tensordiffeq_amd.boundaries import IC, DomainND, periodicBC

NX, NT = 256, 201


def exact(x, t):
    """The soliton on the points ``(x, t)``: ``(u, v)``."""
    s = 1.0 / np.cosh(x)
    return s * np.cos(t / 2), s * np.sin(t / 2)


def build(args):
    tdq.set_seed(args.seed)
    Domain = DomainND(["x", "t"], time_var="t")
    Domain.add("x", [-5.0, 5.0], NX)
    Domain.add("t", [0.0, math.pi / 2], NT)
    N_f = args.n_f or 20000
    Domain.generate_collocation_points(N_f)

    def ic_u(x):
        return 1.0 / np.cosh(x)

    def ic_v(x):
        return 0.0 * x

    def deriv_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        u, v = h[:, 0:1], h[:, 1:2]
        return u, v, tdq.grad(u, x), tdq.grad(v, x)

    def f_model(u_model, x, t):
        h = u_model(torch.cat([x, t], 1))
        u, v = h[:, 0:1], h[:, 1:2]
        u_t, v_t = tdq.grad(u, t), tdq.grad(v, t)
        u_xx = tdq.grad(tdq.grad(u, x), x)
        v_xx = tdq.grad(tdq.grad(v, x), x)
        sq = u * u + v * v
        return -v_t + 0.5 * u_xx + sq * u, u_t + 0.5 * v_xx + sq * v

    init = IC(Domain, [ic_u, ic_v], var=[["x"], ["x"]])       # one target function per output
    x_periodic = periodicBC(Domain, ["x"], [deriv_model])
    model = tdq.CollocationSolverND(verbose=not args.quiet)
    width = int(getattr(args, "width", 100))
    model.compile([2, width, width, width, width, 2], f_model, Domain, [init, x_periodic], **solver_kw(args))
    return model, Domain


def main(argv=None):
    ap = parser(__doc__.splitlines()[0], iters=10000, newton=10000)
    ap.add_argument("--width", type=int, default=100, help="hidden width (128: the one-launch step's)")
    args = ap.parse_args(argv)
    model, Domain = build(args)
    backend = model.active_backend
    if model.device.type == "cuda" and args.backend == "auto":
        assert backend == "hip", (backend, model.program().reasons)
    t0 = time.perf_counter()
    model.fit(tf_iter=args.iters)
    t1 = time.perf_counter()
    if args.newton:
        model.fit(newton_iter=args.newton)
    t2 = time.perf_counter()
    x = np.linspace(-5.0, 5.0, NX)
    t = np.linspace(0.0, math.pi / 2, NT)
    X_star, _, _ = grid_points(x, t)
    h_pred, _ = model.predict(X_star)                           # (N, 2): u and v
    u, v = exact(X_star[:, 0], X_star[:, 1])
    err = float(tdq.find_L2_error(np.hypot(h_pred[:, 0:1], h_pred[:, 1:2]), np.hypot(u, v)[:, None]))
    res = report("schrodinger", {"l2_error_abs_h": err, "loss": float(model.losses[-1]["Total Loss"]),
                                 "adam_s": t1 - t0, "lbfgs_s": t2 - t1, "backend": backend,
                                 "fused_loss": model.program().fused_op is not None,
                                 "fused_step_reason": str(getattr(model.program(), "fused_step_reason", "not requested"))},
                 args.quiet, model=model)
    return res


if __name__ == "__main__":
    main()
