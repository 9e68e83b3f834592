"""The one-launch step tail (csrc/jet_bf3.hip ``tail_one_kernel``: a workgroup owns 256 theta columns
from the gradient-slab rows through to the updated parameters) against the two-launch tail
(``tdq_step_tail_bf3``), bit for bit - at the kernel level on synthetic slabs and optimizer state, and
through the Adam engine (``TDQ_TAIL_ONE=1`` against ``0``)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NETS = [(2, 32, 1), (2, 20, 20, 20, 1), (2, 128, 128, 128, 128, 1)]
ROWS = [1, 5, 8, 9, 228]
N_TERMS, N_SCAL, HIST_ROWS, S_STREAMS, N_PTS = 3, 2, 4, 3, 64


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))   # NaN-proof


def _param_count(net):
    return sum((a + 1) * b for a, b in zip(net[:-1], net[1:]))


class _Case:
    """Synthetic slabs, loss partials and optimizer / bookkeeping state of one step."""

    def __init__(self, net, rows, half, mode, with_gx, with_targets, seed=0):
        """``with_gx``: a second theta gradient; ``with_targets``: snapshot and weight-image targets."""
        from tensordiffeq_amd.ops import _lib
        lib = _lib.load()
        dev = torch.device("cuda", 0)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.net, self.rows, self.half = net, rows, half
        self.widths = (ctypes.c_int * (len(net) - 2))(*net[1:-1])
        self.P = P = _param_count(net)
        self.Pst = Pst = (P + 7) & ~7
        chunks = min(rows, 8)

        def rnd(*shape, scale=1.0):
            return torch.randn(*shape, device=dev, generator=g) * scale

        slab = rnd(rows, Pst, scale=1e-2)
        self.work = torch.zeros((rows + chunks) * Pst, device=dev)
        if half:
            self.slab = slab.to(torch.bfloat16)
            self.work.view(torch.bfloat16)[:rows * Pst] = self.slab.reshape(-1)
        else:
            self.slab = slab
            self.work[:rows * Pst] = slab.reshape(-1)
        self.n_lblocks = 300 if rows == 9 else rows   # 300: more partial rows than reducing threads
        self.lpart = rnd(self.n_lblocks, N_TERMS + N_SCAL).abs().contiguous()
        if mode == "nan":
            self.lpart[self.n_lblocks // 2, 1] = float("nan")
        self.gx = rnd(P, scale=1e-2) if with_gx else None
        n_sc = lib.tdq_jet_bf3_scratch_floats(N_PTS, net[0], self.widths, len(net) - 2, S_STREAMS, 0)
        assert n_sc > 0
        self.with_targets = with_targets
        st = {"scratch": torch.zeros(n_sc, device=dev), "snap": torch.zeros(P, device=dev),
              "grad": torch.zeros(P, device=dev), "losses": torch.zeros(N_TERMS, device=dev),
              "total": torch.zeros((), device=dev), "dscal": torch.zeros(N_SCAL, device=dev),
              "hist": torch.zeros(HIST_ROWS, 1 + N_TERMS, device=dev),
              "epoch": torch.tensor(HIST_ROWS if mode == "hist_full" else 1, dtype=torch.int64, device=dev),
              "best_loss": torch.tensor(-1e30 if mode == "no_improve" else float("inf"), device=dev),
              "best_epoch": torch.tensor(-1, dtype=torch.int64, device=dev),
              "improved": torch.tensor(7, dtype=torch.int32, device=dev),
              "c0": torch.tensor(3.0, dtype=torch.float64, device=dev),
              "c1": torch.tensor(7.0, dtype=torch.float64, device=dev),
              "best_prev": torch.tensor(123.0, device=dev)}
        # groups: theta, 37 (ascent), 513, 2 (gradient = dscal)
        self.sizes = [P, 37, 513, N_SCAL]
        for i, n in enumerate(self.sizes):
            st[f"p{i}"], st[f"m{i}"], st[f"v{i}"] = rnd(n), rnd(n, scale=1e-2), rnd(n, scale=1e-3).abs()
            if i in (1, 2):
                st[f"g{i}"] = rnd(n, scale=1e-2)
        self.base = st

    def state(self):
        return {k: v.clone() for k, v in self.base.items()}

    def step(self, st, one):
        """One step tail on ``st``: the two launches, or the pre-bookkeeping + the one launch."""
        from tensordiffeq_amd.ops import _lib, fused, jet_hip
        lib = _lib.load()
        net = self.net
        gsrc = [st["grad"], st["g1"], st["g2"], st["dscal"]]
        hyp = [(1.0, "c0", 1e-3), (-1.0, "c1", 5e-3), (1.0, "c1", 2e-3), (1.0, "c0", 1e-2)]
        arr = (fused._Group * 4)()
        for i, (sign, cnt, lr) in enumerate(hyp):
            arr[i] = fused._Group(st[f"p{i}"].data_ptr(), gsrc[i].data_ptr(), st[f"m{i}"].data_ptr(),
                                  st[f"v{i}"].data_ptr(), self.sizes[i], sign, lr, 0.9, 0.999, 1e-7, 0.0,
                                  st[cnt].data_ptr())
        counters = [st["c0"], st["c1"]]
        carr = (ctypes.c_void_p * 2)(*[c.data_ptr() for c in counters])
        p = _lib.ptr
        args = [p(self.work), p(st["grad"]), p(st["scratch"]) if self.with_targets else None, N_PTS, net[0],
                self.widths, net[-1], len(net) - 2, S_STREAMS, 0 if self.half else 1, p(self.lpart), self.n_lblocks,
                N_TERMS, N_SCAL, p(st["losses"]), p(st["total"]), p(st["dscal"]), p(st["hist"]), HIST_ROWS,
                p(st["epoch"]), p(st["best_loss"]), p(st["best_epoch"]), p(st["improved"]),
                ctypes.cast(carr, ctypes.c_void_p), 2, ctypes.cast(arr, ctypes.c_void_p), 4,
                p(st["snap"]) if self.with_targets else None, 0, p(self.gx), self.rows]
        stream = _lib.stream_ptr(self.work.device)
        if one:
            pre = jet_hip.prebook_struct(counters, st["best_loss"], st["best_prev"])
            jet_hip.step_prebook(pre)
            rc = lib.tdq_step_tail1_bf3(*args, p(st["best_prev"]), stream)
        else:
            rc = lib.tdq_step_tail_bf3(*args, stream)
        assert rc == 0
        torch.cuda.synchronize()


@pytest.mark.parametrize("half", [True, False], ids=["bf16rows", "fp32rows"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("net", NETS, ids=lambda n: "x".join(map(str, n)))
def test_tail_one_matches_two_launches(net, rows, half):
    """Every output of the step tail, one launch against two, over two consecutive steps (the second
    reads what the first wrote): an improving step, a non-improving one, a NaN loss and an exhausted
    history; with and without gx, with and without snapshot + weight-image targets (all four).  Groups: theta, 37 (ascent),
    513, and 2 elements whose gradient is dscal."""
    for mode in ("improve", "no_improve", "nan", "hist_full"):
        for with_gx, targets in ((True, True), (True, False), (False, True), (False, False)):
            extras = (with_gx, targets)
            case = _Case(net, rows, half, mode, with_gx=with_gx, with_targets=targets)
            a, b = case.state(), case.state()
            for step in range(2):
                case.step(a, one=True)
                case.step(b, one=False)
                for k in a:
                    if k == "best_prev":
                        continue
                    assert _same(a[k], b[k]), (mode, extras, step, k)
            # the run exercised what it claims
            assert float(b["c0"]) == 5.0 and float(b["c1"]) == 9.0
            # two steps on the same loss: the first improves on an infinite best loss, the second never
            assert int(b["improved"]) == 0
            if mode in ("improve", "hist_full"):
                assert int(b["best_epoch"]) == (1 if mode == "improve" else HIST_ROWS)
                assert float(b["best_loss"]) == float(b["total"])
                assert bool((b["hist"][1] != 0).all()) == (mode == "improve")   # row of the first step
            else:
                assert int(b["best_epoch"]) == -1 and _same(b["best_loss"], case.base["best_loss"])
                assert torch.isnan(b["total"]) == (mode == "nan")
            if targets and mode in ("improve", "hist_full"):
                assert torch.equal(b["snap"], case.base["p0"])   # the weights before the first (best) step
            else:
                assert not b["snap"].any()
            assert bool(b["scratch"].any()) == targets


@pytest.mark.parametrize("half", [True, False], ids=["bf16rows", "fp32rows"])
@pytest.mark.parametrize("rows", ROWS)
def test_tail_one_gradient_against_float64(rows, half):
    """Independent of the two-launch tail: the reduced gradient against a float64 sum of the rows.
    Allowed error per column: rows * 2^-24 * sum |row values| - the worst-case bound of an fp32
    summation of ``rows`` values in any order (nothing fitted)."""
    for net in NETS:
        case = _Case(net, rows, half, "improve", with_gx=False, with_targets=False, seed=1)
        st = case.state()
        case.step(st, one=True)
        rows64 = case.slab.double()[:, :case.P]
        ref, bound = rows64.sum(0), rows * 2.0 ** -24 * rows64.abs().sum(0)
        err = (st["grad"].double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"TAIL_ONE_F64 net {net} rows {rows} half {half}: worst err / bound {worst:.3f}")
        assert bool((err <= bound).all()), worst


# ------------------------------------------------------------------------------ engine ------
def _build(problem, n_f):
    import bench
    torch.manual_seed(0)
    return bench.PROBLEMS[problem]["build"](n_f, 1, "hip", torch.device("cuda", 0), False, "bf16",
                                            layers=(2, 128, 128, 128, 128, 1))


def _fit_twice(m):
    m.fit(tf_iter=25)
    with torch.no_grad():
        m.u_model.flat.mul_(0.97)
    m.fit(tf_iter=15)
    return m


@pytest.mark.parametrize("problem,n_f,layout", [("ac-sa", 517, "plain"), ("ac-sa", 3001, "plain"),
                                                ("ac-baseline", 517, "split")])
def test_engine_tail_one_matches_two_launches(problem, n_f, layout, monkeypatch):
    """fit(25), parameters scaled by 0.97, fit(15) on the fused step with the one-launch tail against
    the two-launch tail: parameters, SA weights, the 40 loss rows, best loss / epoch and the
    best-model prediction, bit for bit."""
    monkeypatch.setenv("TDQ_FUSED_STEP", "1")
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("TDQ_TAIL_ONE", flag)
        m = _fit_twice(_build(problem, n_f))
        fs = m.program()._fused_step
        assert fs is not None and fs.layout == layout, m.program().fused_step_reason
        assert m._get_engine(None, 1).tail_launches == (1 if flag == "1" else 2)
        out[flag] = m
    a, b = out["1"], out["0"]
    assert torch.equal(a.u_model.flat, b.u_model.flat)
    assert len(a.lambdas) == len(b.lambdas)
    for x, y in zip(a.lambdas, b.lambdas):
        assert torch.equal(x, y)
    assert len(a.losses) == 40 and a.losses == b.losses
    assert a.min_loss["adam"] == b.min_loss["adam"] and a.best_epoch["adam"] == b.best_epoch["adam"]
    X = torch.rand(300, 2, generator=torch.Generator().manual_seed(3)).numpy()
    u1, _ = a.predict(X, best_model=True)
    u2, _ = b.predict(X, best_model=True)
    assert (u1 == u2).all()


def test_engine_tail_one_discovery(monkeypatch):
    """A small discovery model (PDE coefficients updated through dscal): identical trajectories with
    the one-launch and the two-launch tail when it takes the fused step.  When it does not, the
    recorded reason is asserted and the step keeps the two launches."""
    import numpy as np
    import tensordiffeq_amd as tdq
    from tensordiffeq_amd.models import DiscoveryModel
    monkeypatch.setenv("TDQ_FUSED_STEP", "1")

    def run(flag):
        monkeypatch.setenv("TDQ_TAIL_ONE", flag)
        tdq.set_seed(0)
        rng = np.random.default_rng(0)
        X = rng.uniform(-1, 1, (2000, 2)).astype(np.float32)
        X[:, 1] = (X[:, 1] + 1) / 2
        u = (X[:, :1] ** 2 * np.cos(np.pi * X[:, :1])).astype(np.float32)
        params = [tdq.Variable(0.0), tdq.Variable(0.0)]

        def f_model(u_model, var, x, t):
            uu = u_model(torch.cat([x, t], 1))
            u_xx = tdq.grad(tdq.grad(uu, x), x)
            return tdq.grad(uu, t) - var[0] * u_xx + var[1] * uu * uu * uu - var[1] * uu

        m = DiscoveryModel(verbose=False)
        m.compile([2, 128, 128, 128, 1], f_model, [X[:, :1], X[:, 1:]], u, params,
                  col_weights=torch.rand(2000, 1, generator=torch.Generator().manual_seed(0)),
                  backend="hip", device="cuda", precision="bf16")
        m.fit(tf_iter=30)
        return m

    a, b = run("1"), run("0")
    prog = a.program()
    eng = a._engine   # the engine fit() ran
    assert eng is not None and eng.program is prog
    if getattr(prog, "_fused_step", None) is None:
        print(f"TAIL_ONE_DISCOVERY not on the fused step: {prog.fused_step_reason}")
        assert isinstance(prog.fused_step_reason, str) and prog.fused_step_reason
        assert eng.tail_launches != 1
    else:
        assert eng.tail_launches == 1
    assert torch.equal(a.u_model.flat, b.u_model.flat)
    for x, y in zip(a.vars, b.vars):
        assert torch.equal(x, y)
    assert torch.equal(a.col_weights, b.col_weights)
