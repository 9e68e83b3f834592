"""``CollocationSolverND`` - forward collocation PINN solver.

Reference: tensordiffeq/models.py:12-319.  Same public surface: ``compile(layer_sizes, f_model,
domain, bcs, Adaptive_type=0, dict_adaptive=None, init_weights=None, g=None, dist=False)``,
``compile_data``, ``update_loss``, ``grad``, ``fit(tf_iter, newton_iter, batch_sz,
newton_eager)``, ``get_loss_and_flat_grad``, ``predict(X_star, best_model=False)``, ``save``,
``load_model``; attributes ``u_model``, ``tf_optimizer``, ``tf_optimizer_weights`` (replaceable),
``lambdas``, ``lambdas_map``, ``losses``, ``min_loss``, ``best_epoch``, ``best_model``.

Implements the reference's *intent* where it is broken: ``Adaptive_type`` accepts
ints and names, type 3 / ``"ntk"`` being the NTK weighting of ``ops/ntk.py`` (B14) and type 4 / ``"causal"``
the causal training weights of ``ops/causal.py`` (not in the reference); SA works with minibatches and under DP (B5); DP shards points (B3) and
reports the true global loss (B4); repeated ``fit`` calls resume (B6); L-BFGS runs under DP
(B7); best weights are real snapshots (B8); the data-assimilation term is used (B17).  Beyond the reference,
``compile(resample="r3")`` moves the collocation points after every Adam step (R3 resampling, ``ops/r3.py``;
``collocation_points()``, ``resample_stats()``).
"""
from __future__ import annotations

import math
import os
import time

import numpy as np
import torch
from tqdm.auto import tqdm

from .. import checkpoint
from ..fit import AdamEngine, LossGradEngine, ParamGroup
from ..optimizers import Adam, eager_lbfgs
from ..output import print_screen
from ..parallel import dist as pdist
from .loss import LossProgram, Term
from .networks import FlatModule, TanhMLP

_ADAPTIVE = {0: 0, "none": 0, "baseline": 0, "pinn": 0,
             1: 1, "self-adaptive": 1, "self_adaptive": 1, "sa": 1, "sa-pinn": 1,
             2: 2, "loss-weights": 2, "self-adaptive-loss": 2, "weight_outside_sum": 2,
             3: 3, "ntk": 3,
             4: 4, "causal": 4}


def _identity(lam):
    """``g`` of the causal mode: the residual term is ``mean(lambda_i f_i^2)``."""
    return lam


def parse_adaptive_type(a, ntk=False, causal=False):
    """``ntk=True`` / ``causal=True``: the caller implements NTK / causal weighting
    (``CollocationSolverND.compile``)."""
    key = a.lower() if isinstance(a, str) else a
    if key not in _ADAPTIVE:
        raise Exception("Adaptive method invalid!")
    v = _ADAPTIVE[key]
    if v == 3 and not ntk:
        raise NotImplementedError("NTK adaptive weighting (Adaptive_type=3) is not implemented")
    if v == 4 and not causal:
        raise NotImplementedError("causal training weights (Adaptive_type=4) are not implemented")
    return v


def default_device():
    ctx = pdist._CTX
    if ctx is not None:
        return ctx.device
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


class _FlatModel:
    """Callable view of the network evaluated at a frozen flat snapshot (``best_model`` values)."""

    def __init__(self, net, flat):
        self.net, self.flat = net, flat

    def __call__(self, *xs):
        with torch.no_grad():
            return self.net(*xs, params=self.flat)


class CollocationSolverND:
    def __init__(self, assimilate=False, verbose=True):
        self.assimilate = assimilate
        self.verbose = verbose
        self.best_epoch = {"adam": -1, "l-bfgs": -1, "overall": -1}
        self.min_loss = {"adam": np.inf, "l-bfgs": np.inf, "overall": np.inf}
        self.best_model = {"adam": None, "l-bfgs": None, "overall": None}
        self.lambdas = self.dict_adaptive = self.lambdas_map = None
        self.isNTK = False
        self.ntk_every = 100
        self.ntk_history = []   # (epoch, {term: T_k}, {term: lambda_k}) per NTK update
        self.isCausal = False
        self.causal_history = []   # (epoch, eps in force after the check, min_b W_b) per eps check
        self.isR3 = False          # compile(resample="r3"): the collocation points move (ops/r3.py)
        self.data_x = self.data_t = self.data_s = None
        self._engine = None
        self._lbfgs_engine = None
        self._state = None
        self._programs = {}
        self._best_flat = {}
        self.fit_info = {}    # last fit(): per-phase steps / wall time, L-BFGS stop reason
        self.log_every = 100
        self.metrics = None   # MetricsLogger (compile(metrics_path=...) or TDQ_METRICS)

    # ================================================================== compile =========
    def compile(self, layer_sizes, f_model, domain, bcs, Adaptive_type=0, dict_adaptive=None,
                init_weights=None, g=None, dist=False, backend="auto", device=None,
                periodic_legacy=False, seed=None, network=None, precision=None, metrics_path=None,
                log_every=None, newton_precision=None, lbfgs_stop=None, newton_schedule=None, ntk_every=100,
                causal_eps=1.0, causal_bins=32, causal_delta=0.99, causal_every=100, causal_stop=False,
                causal_bc_weights=None, resample=None, resample_seed=None):
        from ..config import SolverConfig
        self.config = SolverConfig.from_env(backend=None if backend == "auto" else backend, precision=precision,
                                            seed=seed, metrics_path=metrics_path, log_every=log_every,
                                            newton_precision=newton_precision, lbfgs_stop=lbfgs_stop,
                                            newton_schedule=newton_schedule)
        backend = self.config.backend
        precision = self.config.precision
        # jet-GEMM precision of the L-BFGS phase (None: same as the Adam phase).  L-BFGS's
        # curvature pairs need the accurate gradient; Adam tolerates bf16 activations
        # (profiles/r2_v2_accuracy_mixed.jsonl)
        self.newton_precision = self.config.newton_precision
        # leading L-BFGS phases in other precisions, e.g. [("bf16", 7000)]: cheaper iterations first,
        # the newton_precision phase (fresh history from the best iterate) polishes
        from ..config import parse_newton_schedule
        self.newton_schedule = parse_newton_schedule(self.config.newton_schedule)
        if precision == "bf16" and (self.newton_precision or precision) == "bf16":
            from .loss import _warn_once
            _warn_once("precision='bf16' also for L-BFGS: its curvature pairs need accurate gradients (AC-SA "
                       "stalls at L2 6-7e-2 vs 2.2e-2 with newton_precision='bf16x3'), and residuals dominated by "
                       "second derivatives with large sources lose accuracy in bf16 (Helmholtz L2 9.4e-2 vs 7.9e-3 "
                       "in bf16x3); consider newton_precision='bf16x3' or precision='bf16x3'")
        seed = self.config.seed
        periodic_legacy = periodic_legacy or self.config.periodic_legacy
        self.log_every = self.config.log_every
        if seed is not None:
            from ..utils.seeding import set_seed
            set_seed(seed)
        self.dist = bool(dist)
        self.dist_ctx = pdist.init_distributed(auto_launch=True) if dist else pdist.get_context(device)
        self.device = torch.device(device) if device is not None else (
            self.dist_ctx.device if dist else default_device())
        self.tf_optimizer = Adam(lr=0.005, beta_1=0.99)
        self.tf_optimizer_weights = Adam(lr=0.005, beta_1=0.99)
        self.layer_sizes = list(layer_sizes)
        self.sizes_w = [layer_sizes[i] * layer_sizes[i - 1] for i in range(1, len(layer_sizes))]
        self.sizes_b = list(layer_sizes[1:])
        self.bcs = list(bcs)
        self.f_model = f_model
        self.g = g
        self.domain = domain
        self.backend = backend
        self.precision = precision
        self.periodic_legacy = periodic_legacy
        if domain.X_f is None:
            raise ValueError("call domain.generate_collocation_points(N_f) before compile")
        X_f = torch.as_tensor(np.asarray(domain.X_f) if not torch.is_tensor(domain.X_f) else domain.X_f,
                              dtype=torch.float32)
        self.N_f = int(X_f.shape[0])
        if self.config.metrics_path:
            from ..metrics import MetricsLogger
            self.metrics = MetricsLogger(self.config.metrics_path, self.dist_ctx.rank, self.dist_ctx.world,
                                         n_points=None)
        ctx = self.dist_ctx
        self._lo, self._hi = pdist.shard_range(self.N_f, ctx.rank, ctx.world)
        self.X_f_local = X_f[self._lo:self._hi].to(self.device)
        self.X_f_in = [self.X_f_local[:, j:j + 1] for j in range(X_f.shape[1])]
        self.X_f_len = np.array([self.N_f])
        if network is not None and not isinstance(network, (TanhMLP, FlatModule)):
            network = FlatModule(network)
        self.u_model = network if network is not None else TanhMLP(self.layer_sizes, device=self.device)
        self.u_model.to(self.device)
        if ctx.is_distributed:
            ctx.broadcast_(self.u_model.flat.data)

        self.Adaptive_type = parse_adaptive_type(Adaptive_type, ntk=True, causal=True)
        self.isAdaptive = self.Adaptive_type in (1, 2)
        self.isNTK = self.Adaptive_type == 3
        self.isCausal = self.Adaptive_type == 4
        # NTK weights multiply the terms like type 2's: lambda_k * mean(f^2); so do the causal mode's
        # fixed BC / IC / data scalars, beside its per-point residual weights (g_MSE, g the identity)
        self.weight_outside_sum = self.Adaptive_type in (2, 3, 4)
        if self.isCausal:
            self._check_causal(dict_adaptive, init_weights, g, backend, causal_eps, causal_bins, causal_delta,
                               causal_every, causal_bc_weights)
            self.causal_stop = bool(causal_stop)
            self.g = _identity
        self.isR3 = self._check_resample(resample, resample_seed, dict_adaptive, init_weights, g, backend)
        if self.isR3:
            self.g = _identity
        if self.isNTK:
            if dict_adaptive is not None or init_weights is not None:
                raise Exception("NTK weights are computed from the network, one per loss term, but weight vectors "
                                "were provided. Set the weight vectors to \"none\" to continue")
            if g is not None:
                raise Exception("NTK weights multiply each loss term; a weight function g was provided. "
                                "Set g to \"none\" to continue")
            if backend == "autograd":
                raise ValueError("NTK adaptive weighting needs the jet path (backend 'jet' or 'hip'), "
                                 "backend 'autograd' was requested")
            if int(ntk_every) < 1:
                raise ValueError(f"ntk_every must be positive, got {ntk_every}")
            self.ntk_every = int(ntk_every)
            self.ntk_history = []
            self._ntk = None
            self._ntk_epoch = 0
        if not self.isAdaptive and dict_adaptive is not None and init_weights is not None:
            raise Exception("Adaptive weights are turned off but weight vectors were provided. "
                            "Set the weight vectors to \"none\" to continue")
        if self.isAdaptive:
            if dict_adaptive is None or init_weights is None:
                raise Exception("Adaptive weights selected but no inputs were specified!")
            if all(not any(v) for v in dict_adaptive.values()):
                raise Exception("Adaptive method was selected but none loss was marked to be adaptive")
            self.dict_adaptive = dict_adaptive
            self._init_lambdas(init_weights, dict_adaptive)
        else:
            self.lambdas, self.lambdas_map, self._lam_kind = [], {"residual": [], "bcs": []}, []
            self._lam_for = {}
        self._programs = {}
        self._engine = None
        self._lbfgs_engine = None
        self._state = None
        if self.isNTK:
            self._init_ntk_lambdas()
            self._ntk_op()   # a loss the tracer cannot fuse is refused here
        if self.isCausal:
            self._init_causal_lambdas()
        if self.isR3:
            self._init_r3_lambdas()
            self._r3_residual_segment(self.program())   # a residual the mode cannot move is refused here
        for i, bc in enumerate(self.bcs):   # a target that does not fit the outputs is refused here
            if bc.isInit or bc.isDirichlect:
                self._value_target(f"BC_{i} ({type(bc).__name__})", bc.val, getattr(bc, "outputs", None))

    def _value_target(self, name, val, outputs=None):
        """``(target, output columns or None)`` of a value condition (Dirichlet / IC / data) on a
        network with ``d_out`` outputs: a scalar or one column ``(n, 1)`` is the target of every
        selected output, ``k`` columns are the targets of the ``k`` selected outputs (all ``d_out``
        without ``outputs=``), in order.  Anything else is a ``ValueError`` naming the condition."""
        d_out = int(self.layer_sizes[-1])
        cols = None if outputs is None else list(outputs)
        if cols is not None and any(c >= d_out for c in cols):
            raise ValueError(f"{name}: outputs={cols} on a network with {d_out} output(s)")
        n_sel = d_out if cols is None else len(cols)
        val = torch.as_tensor(np.asarray(val) if not torch.is_tensor(val) else val.detach().cpu(),
                              dtype=torch.float32, device=self.device)
        if val.numel() == 1:
            return val.reshape(()), cols
        if val.dim() < 2 or val.shape[1] == 1:
            val = val.reshape(-1, 1)
        if val.dim() != 2 or val.shape[1] not in (1, n_sel):
            k = val.shape[1] if val.dim() == 2 else tuple(val.shape)
            raise ValueError(f"{name}: {k} target functions / columns for {n_sel} network output(s)"
                             + (f" (outputs={cols})" if cols is not None else "")
                             + f"; give one (applied to every output) or {n_sel}")
        return val.contiguous(), cols

    def _init_lambdas(self, init_weights, dict_adaptive):
        ctx = self.dist_ctx
        lambdas, lmap, kinds, lam_for = [], {}, [], {}
        for key in ("residual", "BCs"):
            vals = init_weights.get(key, init_weights.get(key.lower(), []))
            flags = dict_adaptive.get(key, dict_adaptive.get(key.lower(), []))
            idx = []
            for j, value in enumerate(vals):
                if value is None or not (j < len(flags) and flags[j]):
                    continue
                t = torch.as_tensor(value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value),
                                    dtype=torch.float32).to(self.device)
                if ctx.is_distributed:
                    ctx.broadcast_(t)
                # per-point residual weights are sharded with the points - except under
                # Adaptive_type 2 ("outside sum": (sum_i w_i) * mean(r^2), reference utils.py:38-44),
                # whose sum over ALL weights multiplies every rank's partial mean: those weights stay
                # replicated and their gradient (the global mean) is all-reduced like theta's
                sharded = (key == "residual" and t.numel() == self.N_f and ctx.is_distributed
                           and not self._outside_sum_weights())
                if sharded:
                    t = t.reshape(-1, 1)[self._lo:self._hi]
                t = t.reshape(-1, 1).contiguous() if t.numel() > 1 else t.reshape(()).contiguous()
                lambdas.append(t.detach().requires_grad_(True))
                kinds.append("residual" if key == "residual" else "bc")
                idx.append(len(lambdas) - 1)
                lam_for[(kinds[-1], j)] = len(lambdas) - 1
            lmap[key.lower()] = idx
        self.lambdas, self.lambdas_map, self._lam_kind = lambdas, lmap, kinds
        self._lam_for = lam_for

    def _init_ntk_lambdas(self):
        """One scalar weight per loss term, 1.0: every residual output, then every BC, then the
        assimilation term.  No optimizer owns them; :meth:`_ntk_update` overwrites them in place."""
        self._n_res = self._residual_count()
        keys = [("residual", k) for k in range(self._n_res)] + [("bc", i) for i in range(len(self.bcs))]
        if self.assimilate:
            keys.append(("data", 0))
        self.lambdas = [torch.ones((), dtype=torch.float32, device=self.device) for _ in keys]
        self._lam_for = {k: i for i, k in enumerate(keys)}
        self._lam_kind = ["residual" if k[0] == "residual" else "bc" for k in keys]
        self.lambdas_map = {"residual": [i for i, k in enumerate(keys) if k[0] == "residual"],
                            "bcs": [i for i, k in enumerate(keys) if k[0] == "bc"]}
        if self.assimilate:
            self.lambdas_map["data"] = [len(keys) - 1]

    # ---------------------------------------------------------------- causal weights ----
    def _check_causal(self, dict_adaptive, init_weights, g, backend, eps, bins, delta, every, bc_weights):
        """The causal mode's refusals, each naming its reason, and its settings."""
        tv = getattr(self.domain, "time_var", None)
        if tv is None or tv not in self.domain.vars:
            raise ValueError("causal training weights bin the collocation points by time, but the domain has no "
                             "time_var")
        if dict_adaptive is not None or init_weights is not None:
            raise Exception("causal weights are computed from the residuals, one per collocation point, but weight "
                            "vectors were provided. Set the weight vectors to \"none\" to continue")
        if g is not None:
            raise Exception("causal weights multiply the squared residuals directly; a weight function g was "
                            "provided. Set g to \"none\" to continue")
        if backend == "autograd":
            raise ValueError("causal training weights need the jet path (backend 'jet' or 'hip'), backend "
                             "'autograd' was requested")
        if self.dist:
            raise ValueError("causal training weights are not available with dist=True: the bins' residual "
                             "means would need an all-reduce in every step")
        if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= 1024:
            raise ValueError(f"causal_bins must be an integer in 1..1024, got {bins}")
        eps_list = [float(e) for e in (eps if isinstance(eps, (list, tuple)) else [eps])]
        if not eps_list or any(not (math.isfinite(e) and e >= 0.0) for e in eps_list) \
                or any(b <= a for a, b in zip(eps_list, eps_list[1:])):
            raise ValueError(f"causal_eps must be a non-negative float or an increasing list of them, got {eps}")
        if int(every) < 1:
            raise ValueError(f"causal_every must be positive, got {every}")
        n_res = self._residual_count()
        if n_res != 1:
            raise ValueError(f"causal training weights take one residual output, f_model returns {n_res}")
        self._n_res = n_res
        n_terms = len(self.bcs) + (1 if self.assimilate else 0)
        bcw = [1.0] * n_terms if bc_weights is None else [float(w) for w in bc_weights]
        if len(bcw) != n_terms:
            raise ValueError(f"causal_bc_weights: {len(bcw)} weights for {n_terms} BC / IC / data terms")
        self.causal_eps = eps_list
        self.causal_bins, self.causal_delta, self.causal_every = int(bins), float(delta), int(every)
        self.causal_bc_weights = bcw
        self.causal_history = []
        self._causal_epoch = 0
        self._causal_eps_index = 0
        self._causal_done = False
        self._causal_ops = {}

    def _init_causal_lambdas(self):
        """The per-point residual weights ``(N_f, 1)``, ones, then one fixed scalar per BC / IC / data
        term (the untrained-scalar slots of :meth:`_init_ntk_lambdas`).  No optimizer owns them; the
        residual weights are overwritten in place after every loss pass (ops/causal.py)."""
        keys = [("residual", 0)] + [("bc", i) for i in range(len(self.bcs))]
        if self.assimilate:
            keys.append(("data", 0))
        self.lambdas = [torch.ones((self.X_f_local.shape[0], 1), dtype=torch.float32, device=self.device)]
        self.lambdas += [torch.full((), w, dtype=torch.float32, device=self.device) for w in self.causal_bc_weights]
        self._lam_for = {k: i for i, k in enumerate(keys)}
        self._lam_kind = ["residual" if k[0] == "residual" else "bc" for k in keys]
        self.lambdas_map = {"residual": [0], "bcs": [i for i, k in enumerate(keys) if k[0] == "bc"]}
        if self.assimilate:
            self.lambdas_map["data"] = [len(keys) - 1]

    def _causal_op(self, prog=None):
        """The weight update of the full-batch program (``ops/causal.py``), rebuilt with the program."""
        from ..ops import causal
        prog = self.program() if prog is None else prog
        op = self._causal_ops.get("op")
        if op is None or op.prog is not prog:
            tv = self.domain.time_var
            j = self.domain.vars.index(tv)
            t0, t1 = (float(v) for v in self.domain.get_dict(tv)["range"])
            term = next(t for t in prog.terms if t.kind == "residual")
            n = prog.segments[term.seg].n
            c = term.scale / (term.denom if term.denom is not None else n)
            op = causal.CausalOp(prog, prog.fused_op, self.X_f_local[:, j], (t0, t1), self.causal_bins,
                                 self.causal_eps, self.device, self.lambdas[0], 0, 1.0 / c)
            op.set_eps(self._causal_eps_index)
            self._causal_ops = {"op": op}
            self._programs.pop(("engine", None), None)   # its captured step calls the old update
        return op

    def causal_weights(self):
        """The ``M`` bin weights ``W_b`` of the last update (a CPU tensor)."""
        if not self.isCausal:
            raise ValueError("causal_weights() needs Adaptive_type='causal'")
        return self._causal_op().w_bins.detach().cpu().clone()

    def _causal_prime(self):
        """One loss evaluation at the current parameters, then the weight update: the weights of the
        first step of a ``fit`` call.  Runs eagerly, before any capture."""
        op = self._causal_op()
        prog = op.prog
        flat = self._flat()
        fop = prog.fused_op
        if fop is not None:
            from ..ops import jet_hip
            J, _ = jet_hip.forward_raw(prog.X_all, flat, prog.net, prog.plan, prog.precision, rows=fop.fl.n_streams)
            if prog.hi_op is not None:
                prog.hi_op.forward(J, flat)
            fop(J)
            op.update(fop.dlam[op.slot])
            return
        lam = self.lambdas[0].detach().requires_grad_(True)
        loss, _ = prog.evaluate(flat.detach(), [lam] + [l.detach() for l in self.lambdas[1:]])
        op.update(torch.autograd.grad(loss, lam)[0].contiguous())

    def _causal_check(self, epoch):
        """The eps schedule: with ``min_b W_b`` above ``causal_delta`` the next eps is written in
        place (captured steps read it through its pointer).  Returns True when ``causal_stop`` ends
        the Adam phase: the last eps has passed ``delta``."""
        op = self._causal_op()
        w = op.min_weight()
        if w > self.causal_delta:
            if op.eps_index + 1 < len(self.causal_eps):
                op.set_eps(op.eps_index + 1)
                self._causal_eps_index = op.eps_index
            else:
                self._causal_done = True
        self.causal_history.append((int(epoch), float(self.causal_eps[op.eps_index]), w))
        return self.causal_stop and self._causal_done

    # ---------------------------------------------------------------- R3 resampling ----
    def _check_resample(self, resample, seed, dict_adaptive, init_weights, g, backend):
        """``compile(resample=...)``: whether the R3 mode is on, after its refusals, each naming its
        reason."""
        if resample is None:
            return False
        if not isinstance(resample, str) or resample.lower() != "r3":
            raise ValueError(f"resample must be None or 'r3' (retain-resample-release), got {resample!r}")
        if self.Adaptive_type != 0:
            raise ValueError(f"R3 resampling moves the collocation points, but Adaptive_type={self.Adaptive_type} "
                             "keeps weights that belong to fixed points (or to their time bins): Adaptive_type "
                             "must be 0")
        if dict_adaptive is not None or init_weights is not None:
            raise Exception("R3 resampling keeps its own per-point array of ones, but weight vectors were "
                            "provided. Set the weight vectors to \"none\" to continue")
        if g is not None:
            raise Exception("R3 resampling reads the squared residuals through a weight array of ones; a weight "
                            "function g was provided. Set g to \"none\" to continue")
        if backend == "autograd":
            raise ValueError("R3 resampling needs the jet path (backend 'jet' or 'hip'), backend 'autograd' "
                             "was requested")
        if self.dist:
            raise ValueError("R3 resampling is not available with dist=True: the mean of |f| over the population "
                             "would need an all-reduce in every step")
        box = []
        for v in self.domain.vars:
            rng = next((d["range"] for d in self.domain.domaindict if d["identifier"] == v), None)
            if rng is None or not all(math.isfinite(float(b)) for b in rng) or not float(rng[1]) >= float(rng[0]):
                raise ValueError(f"R3 resampling draws uniformly from the domain box, but variable {v!r} has no "
                                 f"finite range ({rng})")
            box.append((float(rng[0]), float(rng[1])))
        if not 1 <= len(box) <= 8:
            raise ValueError(f"R3 resampling takes 1..8 input variables, the domain has {len(box)}")
        n_res = self._residual_count()
        if n_res != 1:
            raise ValueError(f"R3 resampling takes one residual output, f_model returns {n_res}")
        self._n_res = n_res
        if seed is None:
            seed = self.config.seed if self.config.seed is not None else 0
        self.resample = "r3"
        self.resample_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._r3_box = box
        self._r3_state = torch.zeros((), dtype=torch.int64, device=self.device)   # the step counter
        self._r3_ops = {}
        return True

    def _init_r3_lambdas(self):
        """The per-point array ``(N_f, 1)`` of ones on the residual term, ``g`` the identity: the loss is the
        unweighted one, and the array's adjoint is ``c f^2``, what ops/r3.py reads.  No optimizer owns it
        and nothing writes it."""
        self.lambdas = [torch.ones((self.X_f_local.shape[0], 1), dtype=torch.float32, device=self.device)]
        self._lam_for = {("residual", 0): 0}
        self._lam_kind = ["residual"]
        self.lambdas_map = {"residual": [0], "bcs": []}

    def _r3_residual_segment(self, prog):
        """Index of the residual segment of ``prog``, after the refusals that need the program."""
        term = next(t for t in prog.terms if t.kind == "residual")
        if prog.backend == "autograd":
            raise ValueError("R3 resampling needs the jet path, but the loss callables run on the nested-autograd "
                             "backend: " + "; ".join(prog.reasons or ["not jet-expressible"]))
        if prog.segments[term.seg].hi:
            raise ValueError("R3 resampling cannot move a residual of order 3 or 4: its points also live in the "
                             "high-order kernels' own point set and scratch layout")
        return term.seg

    def _r3_op(self, prog=None):
        """The resampling update of the full-batch program (``ops/r3.py``), rebuilt with the program: it
        writes the residual rows of ``prog.X_all`` and, where the program has a one-launch step, of
        ``FusedStepOp.X``.  The step counter is the solver's and survives a rebuild."""
        from ..ops import r3
        prog = self.program() if prog is None else prog
        op = self._r3_ops.get("op")
        if op is None or op.prog is not prog:
            si = self._r3_residual_segment(prog)
            prog.refresh_points(si)   # the segment's own X becomes a view of its X_all rows
            seg = prog.segments[si]
            term = next(t for t in prog.terms if t.kind == "residual")
            c = term.scale / (term.denom if term.denom is not None else seg.n)
            dests = [(prog.X_all, seg.offset)]
            if self.device.type == "cuda" and prog.fused_op is not None:
                from ..ops import fused_step
                fs = fused_step.for_program(prog)
                if fs is not None:
                    start = fs.segment_start(si)
                    if start is None:
                        raise ValueError("R3 resampling: the residual points are not consecutive rows of the "
                                         "one-launch step's point set")
                    dests.append((fs.X, start))
            op = r3.R3Op(prog, prog.fused_op, seg.n, self._r3_box, self.resample_seed, self._r3_state, dests,
                         self.device, 0, 1.0 / c)
            self._r3_ops = {"op": op}
            self._programs.pop(("engine", None), None)   # its captured step calls the old update
        return op

    def _r3_sync(self, points=None):
        """Every copy of the residual points outside the running program takes the current population
        (``points``: a population to install everywhere, a checkpoint's): ``X_f_local`` (and so
        ``X_f_in``), and every other built program - the bf16x3 objective of the L-BFGS phase may have been
        built during Adam - through :meth:`LossProgram.refresh_points`, in place."""
        op = self._r3_ops.get("op")
        with torch.no_grad():
            if points is not None:
                self.X_f_local.copy_(points.to(self.X_f_local.device).reshape(self.X_f_local.shape))
            elif op is not None:
                self.X_f_local.copy_(op.points())
        for key, prog in list(self._programs.items()):
            if isinstance(prog, LossProgram) and key[:2] == ("batch", None):
                if points is None and op is not None and prog is op.prog:
                    continue
                prog.refresh_points(self._r3_residual_segment(prog), self.X_f_local)

    def _r3_restore(self, points, seed, step):
        """A checkpoint's population, seed and counter (``resume``): the run continues its trajectory."""
        if tuple(points.shape) != tuple(self.X_f_local.shape):
            raise ValueError(f"checkpoint holds {tuple(points.shape)} collocation points, the solver "
                             f"{tuple(self.X_f_local.shape)}")
        self.resample_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._r3_state.fill_(int(step))
        self._r3_ops = {}                             # the op carries the seed: rebuilt with the engine
        self._programs.pop(("engine", None), None)
        self._r3_sync(points.to(torch.float32))

    def collocation_points(self):
        """The current collocation points ``(N_f, d_in)`` (a CPU tensor): the population R3 resampling has
        reached, or the fixed set."""
        op = self._r3_ops.get("op") if self.isR3 else None
        X = op.points() if op is not None else self.X_f_local
        return X.detach().cpu().clone()

    def resample_stats(self):
        """``{"step", "released", "threshold"}``: the number of R3 updates so far, and the released rows
        and the threshold ``tau = mean |f|`` of the last one (a host read)."""
        if not self.isR3:
            raise ValueError("resample_stats() needs compile(resample='r3')")
        op = self._r3_ops.get("op")
        if op is None:
            return {"step": int(self._r3_state), "released": 0, "threshold": float("nan")}
        return op.read_stats()

    def _ntk_op(self):
        """The trace evaluator of the full-batch program (``ops/ntk.py``), rebuilt with the program."""
        from ..ops import ntk
        prog = self.program()
        if self._ntk is None or self._ntk.prog is not prog:
            self._ntk = ntk.build(prog, self.lambdas)
        return self._ntk

    def _ntk_traces(self):
        """``(terms, T)``: the weighted terms of the full-batch program and their global traces (a
        float64 CPU vector; under DP the all-reduced sum of the ranks' traces - the program's
        coefficients already carry the global means and the 1/world of replicated terms)."""
        op = self._ntk_op()
        prog = op.prog
        T = op.traces().detach().to(torch.float32)
        ctx = self.dist_ctx
        if ctx.is_distributed:
            T = T.clone()
            ctx.all_reduce_(T)
        return [t for t in prog.terms if t.lam is not None], T.double().cpu()

    def ntk_traces(self):
        """``{term name: T_k}``: the NTK trace of every loss term at the current parameters."""
        terms, T = self._ntk_traces()
        names = [t.name for t in self._ntk_op().prog.terms]
        return {t.name: float(T[names.index(t.name)]) for t in terms}

    def _ntk_update(self, epoch):
        """``lambda_k = sum_j T_j / T_k``, written in place: captured step graphs, the one-launch fused
        step and the L-BFGS objective read the weights through their scalar pointers."""
        from ..ops import ntk
        from .loss import _warn_once
        terms, T = self._ntk_traces()
        names = [t.name for t in self._ntk_op().prog.terms]
        Tk = torch.stack([T[names.index(t.name)] for t in terms])
        prev = torch.stack([self.lambdas[t.lam].detach().double().cpu() for t in terms])
        lam, ok = ntk.weights(Tk, prev)
        if not bool(ok.all()):
            bad = [t.name for t, o in zip(terms, ok.tolist()) if not o]
            _warn_once(f"NTK weighting: the trace of {bad} is not positive and finite; the term keeps its weight")
        with torch.no_grad():
            for t, v in zip(terms, lam.tolist()):
                self.lambdas[t.lam].copy_(torch.tensor(v, dtype=torch.float32))
        self.ntk_history.append((int(epoch), {t.name: float(v) for t, v in zip(terms, Tk)},
                                 {t.name: float(self.lambdas[t.lam]) for t in terms}))

    def compile_data(self, x, t, y):
        if not self.assimilate:
            raise Exception("Assimilate needs to be set to 'true' for data assimilation. Re-initialize "
                            "CollocationSolverND with assimilate=True.")
        self.data_x, self.data_t, self.data_s = x, t, y
        if hasattr(self, "layer_sizes"):
            self._data_target()
        self._programs = {}
        self._engine = None

    def _data_target(self):
        """Assimilation targets: ``(n, 1)``, or one column per output ``(n, d_out)``."""
        y = np.asarray(self.data_s)
        n = np.asarray(self.data_x).size
        y = y.reshape(n, -1) if y.ndim > 1 and y.shape[0] == n else y.reshape(-1, 1)
        if y.shape[0] != n:
            raise ValueError(f"compile_data: {y.shape[0]} target rows for {n} data points")
        return self._value_target("compile_data", y)[0]

    # ================================================================== program =========
    def _adaptive_flags(self, key):
        if not self.isAdaptive:
            return []
        d = self.dict_adaptive
        return list(d.get(key, d.get(key.lower(), [])))

    def _residual_count(self):
        from .loss import _Float64View
        is_mlp = isinstance(self.u_model, TanhMLP)
        probe = self.X_f_local[:4].detach()
        probe = probe.double() if is_mlp else probe
        cols = [probe[:, j:j + 1].clone().requires_grad_(True) for j in range(probe.shape[1])]
        net = _Float64View(self.u_model) if is_mlp else self.u_model
        out = self.f_model(net, *cols)
        return len(out) if isinstance(out, (tuple, list)) else 1

    def _build_program(self, batch=None, precision=None):
        ctx = self.dist_ctx
        world = ctx.world if ctx.is_distributed else 1
        rep_scale = 1.0 / world
        prog = LossProgram(self.u_model, len(self.domain.vars), self.device, backend=self.backend,
                           precision=precision or self.precision,
                           world=world, weight_outside_sum=self.weight_outside_sum, g=self.g,
                           periodic_legacy=self.periodic_legacy)
        prog.causal = self.isCausal   # per-point residual weights beside outside-sum scalars (fusion.py)
        for i, bc in enumerate(self.bcs):
            lam = self._lam_for.get(("bc", i))
            name = f"BC_{i}"
            if bc.isPeriodic:
                pairs = []
                for k in range(len(bc.upper_points)):
                    su = prog.add_segment(f"{name}_up{k}", bc.upper_points[k])
                    sl = prog.add_segment(f"{name}_lo{k}", bc.lower_points[k])
                    pairs.append((su, sl))
                    for fn in bc.deriv_model:
                        prog.register_callable(fn, su)
                        prog.register_callable(fn, sl)
                prog.add_term(Term(name, "periodic", pairs=pairs, fns=list(bc.deriv_model), lam=lam,
                                   scale=rep_scale))
            elif bc.isNeumann:
                segs = []
                for k, pts in enumerate(bc.points):
                    s = prog.add_segment(f"{name}_n{k}", pts)
                    segs.append(s)
                    for fn in bc.deriv_model:
                        prog.register_callable(fn, s)
                val = torch.as_tensor(np.asarray(bc.val), dtype=torch.float32, device=self.device).reshape(-1, 1)
                prog.add_term(Term(name, "neumann", segs=segs, fns=list(bc.deriv_model), val=val,
                                   lam=lam, scale=rep_scale))
            elif bc.isInit or bc.isDirichlect:
                s = prog.add_segment(name, bc.input)
                val, cols = self._value_target(f"{name} ({type(bc).__name__})", bc.val, getattr(bc, "outputs", None))
                prog.add_term(Term(name, "ic" if bc.isInit else "dirichlet", seg=s, val=val, lam=lam,
                                   scale=rep_scale, cols=cols))
            else:
                raise Exception("Boundary condition type is not acceptable")
        if self.assimilate and self.data_s is not None:
            Xd = np.hstack([np.reshape(np.asarray(self.data_x), (-1, 1)),
                            np.reshape(np.asarray(self.data_t), (-1, 1))])
            s = prog.add_segment("data", Xd)
            val = self._data_target()
            prog.add_term(Term("Data", "data", seg=s, val=val, scale=rep_scale, lam=self._lam_for.get(("data", 0))))
        Xr = self.X_f_local
        n_glob = self.N_f
        if batch is not None:
            lo, hi = batch
            Xr = Xr[lo:hi]
            n_glob = (hi - lo) * world
        sr = prog.add_segment("residual", Xr)
        prog.register_callable(self.f_model, sr)
        n_res = self._n_res if hasattr(self, "_n_res") else self._residual_count()
        self._n_res = n_res
        for k in range(n_res):
            lam = self._lam_for.get(("residual", k))
            term = Term(f"Residual_{k}", "residual", seg=sr, fn=self.f_model, extra=(), index=k,
                        lam=lam, denom=float(n_glob) if world > 1 or batch is not None else None)
            if batch is not None and lam is not None and self.lambdas[lam].numel() > 1:
                term.lam_range = batch
            prog.add_term(term)
        prog.finalize()
        return prog

    def program(self, batch=None, precision=None):
        self._flat()  # wraps a user-assigned custom network
        if self._state is not None:
            self._train_state(self.device)  # re-validates the best snapshot against the network
        if self._programs.get("net") is not self.u_model:
            self._programs = {"net": self.u_model}
            self._engine = None
            self._lbfgs_engine = None
        if precision == self.precision:
            precision = None
        key = ("batch", batch) if precision is None else ("batch", batch, precision)
        if key not in self._programs:
            prog = self._build_program(batch, precision)
            prog.enable_fusion(self.lambdas)
            self._programs[key] = prog
        return self._programs[key]

    @property
    def active_backend(self):
        return self.program().backend

    # ================================================================== state ===========
    def _train_state(self, device):
        flat = self._flat()
        st = self._state
        if st is not None and (st["best_flat"].numel() != flat.numel() or st["best_flat"].device != flat.device):
            # the network was replaced (load_model with other layer sizes, a custom u_model): the
            # best-weights snapshot belongs to the old parameter vector - restart best tracking
            # (epoch counter and loss history are kept); compiled engines are dropped with it
            st["best_flat"] = flat.detach().clone()
            st["best_loss"] = torch.full((), math.inf, dtype=torch.float32, device=flat.device)
            st["best_epoch"] = torch.full((), -1, dtype=torch.int64, device=flat.device)
            st.pop("improved", None)
            self._programs = {}
            self._engine = None
            self._lbfgs_engine = None
        if self._state is None:
            self._state = {
                "best_loss": torch.full((), math.inf, dtype=torch.float32, device=device),
                "best_flat": flat.detach().clone(),
                "best_epoch": torch.full((), -1, dtype=torch.int64, device=device),
                "epoch": torch.zeros((), dtype=torch.int64, device=device),
                "epoch_host": 0,
                "hist": None,
            }
        return self._state

    def _flat(self):
        if not isinstance(self.u_model, (TanhMLP, FlatModule)):
            self.u_model = FlatModule(self.u_model).to(self.device)  # user replaced u_model
        return self.u_model.flat

    @property
    def variables(self):
        # (NTK and causal weights and the R3 mode's ones are not trained: no gradient is taken with respect to them)
        return [self._flat()] + ([] if self.isNTK or self.isCausal or self.isR3 else list(self.lambdas or []))

    def _outside_sum_weights(self):
        """Per-point residual weights enter through MSE's outside sum (Adaptive_type 2 without
        ``g``): their sum over ALL points multiplies every rank's partial mean, so under DP they stay
        replicated.  With ``g`` the residual term is g_MSE, element-wise g(lam) * f^2 (reference
        utils.py:47-48), and the weights are sharded with their points like type 1's."""
        return self.weight_outside_sum and self.g is None

    def _lam_replicated(self):
        ctx = self.dist_ctx
        return [not (k == "residual" and ctx.is_distributed and l.numel() > 1 and not self._outside_sum_weights())
                for l, k in zip(self.lambdas, self._lam_kind)]

    # ================================================================== loss API =========
    def update_loss(self):
        total, vals = self.program().evaluate(self._flat(), self.lambdas)
        self.loss_terms = {k: v.detach() for k, v in vals.items()}
        return total

    def grad(self):
        loss = self.update_loss()
        grads = torch.autograd.grad(loss, self.variables, allow_unused=True)
        return loss, [torch.zeros_like(v) if g is None else g for g, v in zip(grads, self.variables)]

    def get_loss_and_flat_grad(self):
        eng = self._get_lbfgs_engine()
        return lambda w: eng(torch.as_tensor(w, dtype=torch.float32, device=self.device))

    def _get_lbfgs_engine(self, precision=None):
        """The L-BFGS objective's engine at ``precision`` (default ``newton_precision``)."""
        default = self.newton_precision or self.precision
        prec = precision or default
        if prec != default:
            key = ("lbfgs_engine", prec)
            eng = self._programs.get(key)
            prog = self.program(precision=prec)
            if eng is None or eng.program is not prog:
                eng = self._programs[key] = LossGradEngine(self, prog, self.lambdas)
            return eng
        if self._lbfgs_engine is None:
            self._lbfgs_engine = LossGradEngine(self, self.program(precision=prec), self.lambdas)
        return self._lbfgs_engine

    def _get_engine(self, batch=None, n_hint=0):
        key = ("engine", batch)
        eng = self._programs.get(key)
        prog = self.program(batch)
        if eng is None:
            groups = [ParamGroup([self._flat()], lambda: self.tf_optimizer, 1.0)]
            bind = None
            if self.isNTK or self.isCausal or self.isR3:   # the weights enter the loss but no optimizer owns them
                bind = lambda alias: {"params": alias[0], "lambdas": self.lambdas}  # noqa: E731
            else:
                groups.append(ParamGroup(self.lambdas, lambda: self.tf_optimizer_weights, -1.0,
                                         self._lam_replicated()))
            eng = AdamEngine(self, prog, groups, n_steps_hint=n_hint, lambdas=self.lambdas, bind=bind,
                             causal=self._causal_op(prog) if self.isCausal else None,
                             resample=self._r3_op(prog) if self.isR3 else None)
            self._programs[key] = eng
        return eng

    # ================================================================== fit =============
    def minibatches(self, batch_sz):
        """Per-rank minibatch ranges ``[(lo, hi), ...]`` (local shard indices) or ``[None]`` for
        full batch.  The count comes from the SMALLEST shard (``N_f // world``), so every rank
        runs the same number of steps - and therefore the same number of collectives - per
        epoch even when ``N_f`` does not divide evenly; each step's residual denominator is
        ``batch_sz * world`` on every rank."""
        if batch_sz is None:
            return [None]
        batch_sz = int(batch_sz)
        if batch_sz <= 0:
            raise ValueError(f"batch_sz must be positive, got {batch_sz}")
        ctx = self.dist_ctx
        world = ctx.world if ctx.is_distributed else 1
        n_min = self.N_f // world
        if batch_sz >= n_min:
            return [None]
        nb = n_min // batch_sz
        return [(i * batch_sz, (i + 1) * batch_sz) for i in range(nb)]

    def fit(self, tf_iter=0, newton_iter=0, batch_sz=None, newton_eager=True):
        from ..profiling import maybe_profile
        with maybe_profile(f"CollocationSolverND.fit(tf_iter={tf_iter}, newton_iter={newton_iter})"):
            return self._fit(tf_iter, newton_iter, batch_sz, newton_eager)

    def _fit(self, tf_iter, newton_iter, batch_sz, newton_eager):
        ctx = self.dist_ctx
        if self.isCausal and batch_sz is not None:
            raise ValueError("causal training weights need full-batch steps (the bins' residual means cover every "
                             "collocation point): batch_sz must be None")
        if self.isR3 and batch_sz is not None:
            raise ValueError("R3 resampling needs full-batch steps (the threshold is the mean of |f| over every "
                             "collocation point): batch_sz must be None")
        batches = self.minibatches(batch_sz)
        if self.verbose and ctx.rank == 0:
            print_screen(self)
        self.program()  # build / plan before timing-sensitive loops
        start_epoch = self._train_state(self.device)["epoch_host"]
        if tf_iter > 0:
            if self.verbose and ctx.rank == 0:
                print("Starting Adam training")
            bar = tqdm(total=tf_iter, disable=not (self.verbose and ctx.rank == 0), desc="Adam")

            if self.metrics is not None:
                self.metrics.n_points = self.X_f_local.shape[0]
                self.metrics.mark(start_epoch)
                if ctx.is_distributed:  # which collective carries the DP bucket (and its start-up timing)
                    self.metrics.log_event("allreduce", world=ctx.world, **ctx.allreduce_info)

            def progress(done, loss):
                bar.n = done
                if loss is not None:
                    bar.set_postfix(loss=loss)
                    if self.metrics is not None:
                        self._log_metrics("adam", loss)
                bar.refresh()

            t_adam = time.perf_counter()
            self._prebuild_lbfgs_objective()
            if batches == [None] and self.isNTK:
                # segments between NTK updates: the weights change in place, the captured step stays
                eng = self._get_engine(None, tf_iter)
                done = 0
                while done < tf_iter:
                    if self._ntk_epoch % self.ntk_every == 0:
                        self._ntk_update(self._ntk_epoch)
                    n = min(tf_iter - done, self.ntk_every - self._ntk_epoch % self.ntk_every)
                    eng.run(n, progress=lambda k, loss, base=done: progress(base + k, loss), log_every=self.log_every)
                    done += n
                    self._ntk_epoch += n
            elif batches == [None] and self.isCausal:
                # segments between eps checks: eps and the weights change in place, the captured step stays
                self._causal_prime()
                eng = self._get_engine(None, tf_iter)
                done = 0
                while done < tf_iter:
                    if self._causal_epoch % self.causal_every == 0 and self._causal_check(self._causal_epoch):
                        break
                    n = min(tf_iter - done, self.causal_every - self._causal_epoch % self.causal_every)
                    eng.run(n, progress=lambda k, loss, base=done: progress(base + k, loss), log_every=self.log_every)
                    done += n
                    self._causal_epoch += n
                tf_iter = done
            elif batches == [None]:
                eng = self._get_engine(None, tf_iter)
                eng.run(tf_iter, progress=progress, log_every=self.log_every)
            else:
                engines = [self._get_engine(b, tf_iter * len(batches)) for b in batches]
                for ep in range(tf_iter):
                    if self.isNTK:   # the traces always come from the full-batch program
                        if self._ntk_epoch % self.ntk_every == 0:
                            self._ntk_update(self._ntk_epoch)
                        self._ntk_epoch += 1
                    for eng in engines:
                        loss = eng.run(1, use_graph=False)
                    if (ep + 1) % self.log_every == 0 or ep + 1 == tf_iter:
                        progress(ep + 1, float(loss))
            bar.close()
            if self.isR3:   # the final population, into X_f_local and every other built program
                self._r3_sync()
            st = self._state
            self.min_loss["adam"] = float(st["best_loss"])   # (device sync: the phase is done)
            self.fit_info["adam"] = {"steps": int(tf_iter), "wall_s": time.perf_counter() - t_adam}
            self.best_epoch["adam"] = int(st["best_epoch"])
            self._best_flat["adam"] = st["best_flat"].clone()
            self.best_model["adam"] = _FlatModel(self.u_model, self._best_flat["adam"])
        if newton_iter > 0:
            if self.isR3:   # L-BFGS runs on the frozen population (a program built since then takes it here)
                self._r3_sync()
            self._fit_lbfgs(newton_iter, newton_eager)
        self._select_overall(start_epoch, tf_iter)

    def _log_metrics(self, phase, loss):
        st = self._state
        ep = int(st["epoch_host"])
        terms = None
        if st["hist"] is not None and ep > 0:
            row = st["hist"][ep - 1].detach().cpu().tolist()
            terms = {t.name: v for t, v in zip(self.program().terms, row[1:])}
        self.metrics.log(phase, ep, loss, terms)

    def _use_device_lbfgs(self):
        """Device-resident L-BFGS (``optimizers/lbfgs_device.py``) by default on a GPU; the
        host-driven port elsewhere.  ``TDQ_LBFGS`` / ``SolverConfig.lbfgs`` overrides."""
        impl = getattr(getattr(self, "config", None), "lbfgs", "auto")
        if impl == "auto":
            return self.device.type == "cuda"
        return impl == "device"

    def _prebuild_lbfgs_objective(self):
        """Start the hipRTC compile of the L-BFGS objective's one-launch kernel (ops/fused_step.py
        ``prebuild``) on a host thread, so it overlaps the Adam phase instead of opening the
        L-BFGS phase (~0.35 s for the bf16x3 objective).  Timed inside the Adam phase."""
        if self.device.type != "cuda" or os.environ.get("TDQ_PREBUILD", "1") == "0":
            return
        try:
            from ..ops import fused_step
            prog = self.program(precision=self.newton_precision or self.precision)
            if prog.backend == "hip":
                fused_step.prebuild(prog)
        except Exception:  # noqa: BLE001 - an optimisation only: the L-BFGS phase compiles it itself
            pass

    def _fit_lbfgs(self, newton_iter, newton_eager):
        t0 = time.perf_counter()
        info = self._fit_lbfgs_body(newton_iter, newton_eager)
        info["wall_s"] = time.perf_counter() - t0
        info["max_iter"] = int(newton_iter)
        self.fit_info["lbfgs"] = info
        if self.metrics is not None:
            self.metrics.log_event("lbfgs_stop", **info)
        if self.verbose and self.dist_ctx.rank == 0:
            print(f"L-BFGS stopped after {info['n_iter']} iterations: {info['reason']}")

    def _fit_lbfgs_body(self, newton_iter, newton_eager):
        """Run L-BFGS; returns ``{"impl", "n_iter", "func_evals", "reason", "stop"}``.  With a
        ``newton_schedule`` the leading phases run first (each from the previous phase's best
        iterate, device L-BFGS only), then the ``newton_precision`` phase takes the rest."""
        sched = list(getattr(self, "newton_schedule", None) or [])
        if sched and newton_eager and self._use_device_lbfgs():
            phases = []
            left = int(newton_iter)
            for prec, n in sched:
                n = min(n, left)
                if n <= 0:
                    break
                info = self._fit_lbfgs_phase(n, self._get_lbfgs_engine(prec))
                phases.append({"precision": prec, **{k: info[k] for k in ("n_iter", "reason")}})
                left -= n
            if left > 0:
                info = self._fit_lbfgs_phase(left, self._get_lbfgs_engine())
                phases.append({"precision": self.newton_precision or self.precision,
                               **{k: info[k] for k in ("n_iter", "reason")}})
            info = dict(info)
            info["n_iter"] = sum(p["n_iter"] for p in phases)
            info["phases"] = phases
            return info
        if sched:
            from .loss import _warn_once
            _warn_once("newton_schedule is honoured by the device L-BFGS only (newton_eager=True on a GPU, "
                       "TDQ_LBFGS=device); this L-BFGS path runs one phase at newton_precision")
        return self._fit_lbfgs_phase(newton_iter, None, newton_eager)

    def _fit_lbfgs_phase(self, newton_iter, eng=None, newton_eager=True):
        ctx = self.dist_ctx
        stop = getattr(getattr(self, "config", None), "lbfgs_stop", "legacy")
        if self.verbose and ctx.rank == 0:
            print("Starting L-BFGS training")
        eng = eng if eng is not None else self._get_lbfgs_engine()
        flat = self._flat()
        bar = tqdm(total=newton_iter, disable=not (self.verbose and ctx.rank == 0), desc="L-BFGS")

        def on_eval(it, f):
            if self.metrics is not None and (it % self.log_every == 0 or it == newton_iter):
                self.metrics.log("lbfgs", it, f)
            if it % 10 == 0 or it == newton_iter:
                bar.n = min(it, newton_iter)
                bar.set_postfix(loss=f)
                bar.refresh()

        if newton_eager and self._use_device_lbfgs():
            from ..fit import _use_graphs
            from ..optimizers import lbfgs_device

            def on_poll(opt):
                ctx.check_health()   # a peer all-reduce timeout inside the L-BFGS graph
                polled = getattr(opt, "polled", None)   # the pipelined poll's host snapshot
                if polled is not None:
                    it, f = polled["n_iter"], polled["f"]
                else:
                    it = opt.n_iter
                    f = float(opt.st[lbfgs_device.F])
                if self.metrics is not None:
                    self.metrics.log("lbfgs", it, f)
                bar.n = min(it, newton_iter)
                bar.set_postfix(loss=f)
                bar.refresh()

            opt = lbfgs_device.minimize(eng.evaluate_fg, flat.data, newton_iter, lr=0.8,
                                        all_reduce=ctx.all_reduce_ if ctx.is_distributed else None,
                                        capture_all_reduce=ctx.capturable(flat.numel() + 1),
                                        use_graph=_use_graphs(self.device),
                                        poll_every=max(1, min(int(self.log_every), 64)), on_poll=on_poll,
                                        stop=stop, images=eng.image_target()
                                        if os.environ.get("TDQ_LBFGS_IMAGES", "1") != "0" else None)
            ctx.check_health()
            with torch.no_grad():
                flat.copy_(opt.best_x)
            self.min_loss["l-bfgs"] = opt.min_loss
            self.best_epoch["l-bfgs"] = opt.best_epoch
            self.lbfgs_state = opt
            info = {"impl": "device", "n_iter": opt.n_iter, "func_evals": opt.func_eval, "reason": opt.reason}
        elif newton_eager:
            from ..optimizers.lbfgs import Struct
            state = Struct()
            x, _, fe, best_w, min_loss, best_epoch = eager_lbfgs(
                eng, flat.detach().clone(), state=state, maxIter=newton_iter, learningRate=0.8, on_eval=on_eval,
                stop=stop)
            ctx.check_health()
            with torch.no_grad():
                flat.copy_(best_w)
            self.min_loss["l-bfgs"] = float(min_loss)
            self.best_epoch["l-bfgs"] = int(best_epoch)
            info = {"impl": "host", "n_iter": int(getattr(state, "nIter", 0)), "func_evals": int(fe),
                    "reason": getattr(state, "reason", "?")}
        else:
            # the reference's graph-mode L-BFGS (tfp lbfgs_minimize, fit.py:107-122): line-search
            # L-BFGS with 10 pairs and tolerance 1e-20, state on the device (optimizers/lbfgs_wolfe.py)
            from ..fit import _use_graphs
            from ..optimizers import lbfgs_wolfe
            prec = getattr(getattr(eng, "program", None), "precision", None)
            prec = prec if getattr(getattr(eng, "program", None), "backend", None) == "hip" else "fp32"
            opt = lbfgs_wolfe.minimize(eng.evaluate_fg, flat.data, newton_iter,
                                       all_reduce=ctx.all_reduce_ if ctx.is_distributed else None,
                                       capture_all_reduce=ctx.capturable(flat.numel() + 1),
                                       use_graph=_use_graphs(self.device), on_iter=on_eval,
                                       hz_eps=lbfgs_wolfe.hz_eps_for(prec))
            ctx.check_health()
            self.min_loss["l-bfgs"] = float(opt.min_loss)
            self.best_epoch["l-bfgs"] = int(opt.n_iter)
            info = {"impl": "strong-wolfe" + (" (device)" if opt.use_graph else ""), "n_iter": int(opt.n_iter),
                    "hz_eps": opt.hz_eps,
                    "func_evals": int(opt.func_eval), "reason": opt.reason, "restarts": int(opt.n_restarts)}
        bar.close()
        self._best_flat["l-bfgs"] = flat.detach().clone()
        self.best_model["l-bfgs"] = _FlatModel(self.u_model, self._best_flat["l-bfgs"])
        info["stop"] = stop
        return info

    def _select_overall(self, start_epoch, tf_iter):
        if self.min_loss["adam"] <= self.min_loss["l-bfgs"]:
            key, off = "adam", 0
        else:
            key, off = "l-bfgs", tf_iter
        self.min_loss["overall"] = self.min_loss[key]
        self.best_epoch["overall"] = self.best_epoch[key] + off if self.best_epoch[key] >= 0 else -1
        if key in self._best_flat:
            self._best_flat["overall"] = self._best_flat[key]
            self.best_model["overall"] = _FlatModel(self.u_model, self._best_flat[key])

    # ================================================================== outputs =========
    @property
    def losses(self):
        """Per-epoch loss history: list of dicts (term name -> value, plus 'Total Loss')."""
        st = self._state
        if st is None or st["hist"] is None:
            return []
        n = int(st["epoch_host"])
        h = st["hist"][:n].detach().cpu().numpy()
        names = [t.name for t in self.program().terms]
        out = []
        for row in h:
            d = {nm: float(v) for nm, v in zip(names, row[1:])}
            d["Total Loss"] = float(row[0])
            out.append(d)
        return out

    def predict(self, X_star, best_model=False, chunk=65536):
        params = None
        if best_model:
            if "overall" not in self._best_flat:
                raise ValueError("no best model recorded yet (call fit first)")
            params = self._best_flat["overall"]
        X = torch.as_tensor(np.asarray(X_star) if not torch.is_tensor(X_star) else X_star,
                            dtype=torch.float32).to(self.device)
        # u is the value stream of the same jet launch that computes the residual's derivatives
        # (HIP kernels on the hip backend), in bf16x3 when the solver trains in bf16 (the
        # L-BFGS phase's program, usually built already): prediction error ~1e-5, not bf16's ~1e-3
        prog = self.program(precision="bf16x3" if self.precision == "bf16" else None)
        vals = []
        f = prog.residual_on(self.f_model, X, params=params, chunk=chunk, values=vals)
        if vals and all(v is not None for v in vals):
            u = torch.cat(vals, dim=0)
        else:
            with torch.no_grad():
                u = torch.cat([self.u_model(X[i:i + chunk], params=params)
                               for i in range(0, X.shape[0], chunk)], dim=0)
        f_np = [x.cpu().numpy() for x in f]
        return u.cpu().numpy(), (f_np[0] if len(f_np) == 1 else tuple(f_np))

    def save(self, path, include_state=True):
        checkpoint.save_solver(self, path, include_state=include_state)

    def load_model(self, path, compile_model=False, restore_state=False):
        checkpoint.load_into_solver(self, path, restore_state=restore_state)

    def resume(self, path):
        """Load weights AND training state (SA weights, Adam moments, epoch, best snapshot)."""
        checkpoint.load_into_solver(self, path, restore_state=True)
