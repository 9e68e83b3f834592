"""Korteweg-de Vries soliton: u_t + 6 u u_x + u_xxx = 0 on x in [-5, 5], t in [0, 1].

Exact solution u = (c / 2) sech^2(sqrt(c) / 2 (x - c t - x0)) with c = 2, x0 = -1: the initial
condition and the Dirichlet values at both ends come from it, and the L2 error is taken against it on
a 256 x 100 grid (no data file).  Net [2, 128 x 4, 1], N_f = 20,000, Adam 10k + L-BFGS 10k.

The residual needs u_xxx on every collocation point: on a GPU the order <= 2 streams come from the
fused jet kernels and the third-order streams from the high-order jet kernels' tile variant
(ops/jet_hi.py); ``--backend jet`` keeps the torch Taylor-jet engine.
Run:  python examples/kdv.py [--iters 10000 --newton 10000 --sa]
"""
import math

import numpy as np
import torch

from _common import grid_points, parser, report, solver_kw

import tensordiffeq_amd as tdq
from tensordiffeq_amd.boundaries import IC, DomainND, FunctionDirichletBC

C, X0 = 2.0, -1.0
XR, TR = (-5.0, 5.0), (0.0, 1.0)


def soliton(x, t):
    return 0.5 * C / np.cosh(0.5 * math.sqrt(C) * (x - C * t - X0)) ** 2


def f_model(u_model, x, t):
    u = u_model(torch.cat([x, t], 1))
    u_x = tdq.grad(u, x)
    u_xxx = tdq.grad(tdq.grad(u_x, x), x)
    u_t = tdq.grad(u, t)
    return u_t + 6.0 * u * u_x + u_xxx


def build(args, sizes=None, nx=256, nt=100):
    """``(model, Domain)``; ``args``: the ``_common.parser`` namespace (``sa``: a self-adaptive weight on
    the residual)."""
    tdq.set_seed(args.seed)
    Domain = DomainND(["x", "t"], time_var="t")
    Domain.add("x", list(XR), nx)
    Domain.add("t", list(TR), nt)
    N_f = args.n_f or 20000
    Domain.generate_collocation_points(N_f)
    BCs = [IC(Domain, [lambda x: soliton(x, TR[0])], var=[["x"]]),
           FunctionDirichletBC(Domain, fun=[lambda t: soliton(XR[1], t)], var="x", target="upper", func_inputs=["t"]),
           FunctionDirichletBC(Domain, fun=[lambda t: soliton(XR[0], t)], var="x", target="lower", func_inputs=["t"])]
    kw = {}
    if getattr(args, "sa", False):
        g = torch.Generator().manual_seed(args.seed)
        kw = {"Adaptive_type": "self-adaptive", "dict_adaptive": {"residual": [True], "BCs": [False, False, False]},
              "init_weights": {"residual": [torch.rand(N_f, 1, generator=g)], "BCs": [None, None, None]}}
    model = tdq.CollocationSolverND(verbose=not args.quiet)
    model.compile(sizes or [2, 128, 128, 128, 128, 1], f_model, Domain, BCs, **kw, **solver_kw(args))
    return model, Domain


def l2_exact(model, nx=256, nt=100):
    """Relative L2 of u against the exact soliton on an ``nx x nt`` grid."""
    x, t = np.linspace(*XR, nx), np.linspace(*TR, nt)
    X_star, X, T = grid_points(x, t)
    u_pred, _ = model.predict(X_star)
    return float(tdq.find_L2_error(u_pred, soliton(X, T).flatten()[:, None]))


def main(argv=None):
    ap = parser(__doc__.splitlines()[0], iters=10000, newton=10000)
    ap.add_argument("--sa", action="store_true", help="self-adaptive weight on the residual")
    args = ap.parse_args(argv)
    model, _ = build(args)
    model.fit(tf_iter=args.iters, newton_iter=args.newton)
    res = report("kdv", {"l2_error": l2_exact(model), "loss": float(model.losses[-1]["Total Loss"])}, args.quiet,
                 model=model)
    if args.plot:
        x, t = np.linspace(*XR, 256), np.linspace(*TR, 100)
        _, X, T = grid_points(x, t)
        tdq.plotting.plot_solution_domain1D(model, [x, t], ub=np.array([XR[1], TR[1]]), lb=np.array([XR[0], TR[0]]),
                                            Exact_u=soliton(X, T).T)
    return res


if __name__ == "__main__":
    main()
