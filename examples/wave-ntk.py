"""1-D wave equation with NTK adaptive loss weights (Wang, Yu, Perdikaris, arXiv 2007.14527, section 7).

u_tt = 4 u_xx on [0, 1]^2, u(x, 0) = sin(pi x) + sin(4 pi x) / 2, u_t(x, 0) = 0, u(0, t) = u(1, t) = 0;
exact solution sin(pi x) cos(2 pi t) + sin(4 pi x) cos(8 pi t) / 2.  The loss terms (residual, initial
value, initial velocity, two walls) have gradients of very different size; ``Adaptive_type="ntk"`` gives
each term the weight sum_j T_j / T_k of its NTK trace, recomputed every ``--ntk-every`` Adam steps.
Prints the relative L2 error on a 101 x 101 grid with NTK weights and without (``Adaptive_type=0``) at the
same schedule.
"""
import math

import numpy as np
import torch

from _common import parser, report, solver_kw

import tensordiffeq_amd as tdq
from tensordiffeq_amd.boundaries import IC, DomainND, FunctionNeumannBC, dirichletBC


def exact(x, t):
    return np.sin(math.pi * x) * np.cos(2 * math.pi * t) + 0.5 * np.sin(4 * math.pi * x) * np.cos(8 * math.pi * t)


def build(args, adaptive):
    tdq.set_seed(args.seed)
    Domain = DomainND(["x", "t"], time_var="t")
    Domain.add("x", [0.0, 1.0], 101)
    Domain.add("t", [0.0, 1.0], 101)
    Domain.generate_collocation_points(args.n_f or 10000)

    def u_t(u_model, x, t):
        return tdq.grad(u_model(torch.cat([x, t], 1)), t)

    def f_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        return tdq.grad(tdq.grad(u, t), t) - 4.0 * tdq.grad(tdq.grad(u, x), x)

    BCs = [IC(Domain, [lambda x: exact(x, 0.0)], var=[["x"]]),
           FunctionNeumannBC(Domain, fun=[lambda x: 0.0 * x], var="t", target="lower", deriv_model=[u_t],
                             func_inputs=["x"]),
           dirichletBC(Domain, val=0.0, var="x", target="lower"),
           dirichletBC(Domain, val=0.0, var="x", target="upper")]
    model = tdq.CollocationSolverND(verbose=not args.quiet)
    kw = {"ntk_every": args.ntk_every} if adaptive else {}
    model.compile([2, args.width, args.width, args.width, 1], f_model, Domain, BCs,
                  Adaptive_type="ntk" if adaptive else 0, **kw, **solver_kw(args))
    return model


def l2(model):
    x = np.linspace(0.0, 1.0, 101)
    X, T = np.meshgrid(x, x)
    pts = np.hstack((X.flatten()[:, None], T.flatten()[:, None]))
    u, _ = model.predict(pts)
    return float(tdq.find_L2_error(u, exact(pts[:, 0:1], pts[:, 1:2])))


def main(argv=None):
    ap = parser(__doc__.splitlines()[0], iters=10000, newton=0, n_f=10000)
    ap.add_argument("--ntk-every", type=int, default=100, help="Adam steps between NTK weight updates")
    ap.add_argument("--width", type=int, default=64,
                    help="hidden width, three hidden layers (5 streams: the norm kernel takes widths <= 64, the "
                         "layer-wise trace path widths <= 128)")
    args = ap.parse_args(argv)
    res = {}
    for tag, adaptive in (("ntk", True), ("baseline", False)):
        model = build(args, adaptive)
        model.fit(tf_iter=args.iters, newton_iter=args.newton)
        res[f"l2_{tag}"] = l2(model)
        res[f"loss_{tag}"] = float(model.losses[-1]["Total Loss"])
        if adaptive:
            res["ntk_path"] = model._ntk_op().kind
            res["ntk_updates"] = len(model.ntk_history)
            for name, lam in model.ntk_history[-1][2].items():
                res[f"lambda_{name}"] = lam
    return report("wave-ntk", res, args.quiet, model=model)


if __name__ == "__main__":
    main()
