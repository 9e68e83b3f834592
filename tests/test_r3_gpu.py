"""R3 resampling on the GPU: the update kernel (``csrc/r3.hip``) against the torch mirror (bit for bit in the
written rows) and against a float64 re-statement of the threshold and the released set, its bounds, its
argument checks and its capture in a graph; then the solver on the ``hip`` backend - the two copies of the
residual points, captured steps against eager ones, the mirror on the GPU against the kernel, the loss on the
moved points against the float64 torch jet and the L-BFGS objective's copies."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOX = [(-1.0, 1.0), (0.0, 1.0), (-3.0, 0.5), (2.0, 10.0), (-0.25, 0.0)]
TAIL = 64
SEED, STEP = 0x9E3779B97F4A7C15, (7 << 32) + 5
# the loss of the step's kernels against the float64 torch jet on the same points (tests/test_fused_kernels.py)
LOSS_BOUND = {"bf16": 1e-2, "bf16x3": 1e-5}


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from tensordiffeq_amd.ops import _lib
    return _lib.load(required=True)


# ------------------------------------------------------------------------------------------
# a. the kernel
# ------------------------------------------------------------------------------------------
def inputs(n):
    """``r2`` as in tests/test_causal_gpu.py: ``rand * 10^randint(-6, 7)``, a fifth zeroed, one entry 1e6."""
    g = torch.Generator().manual_seed(n)
    r2 = torch.rand(n, generator=g) * 10.0 ** torch.randint(-6, 7, (n,), generator=g).float()
    r2[torch.rand(n, generator=g) < 0.2] = 0.0
    r2[int(torch.randint(0, n, (1,), generator=g))] = 1e6
    return r2, g


def restate64(r2, inv_c):
    """``(tau, released)`` in float64 on the CPU: an exactly rounded sum."""
    a = np.sqrt(r2.double().numpy() * inv_c)
    tau = math.fsum(a.tolist()) / a.size
    return a, tau, torch.from_numpy(~(a > tau))


def same_bits(x, y):
    """Equal, the NaN padding included."""
    return torch.equal(torch.nan_to_num(x.double(), nan=-123.0), torch.nan_to_num(y.double(), nan=-123.0))


class Buffers:
    """Every array of one call with ``TAIL`` NaN (or -7) elements behind it; ``X`` has ``TAIL`` NaN rows behind
    its ``n`` rows, ``X2`` (if any) ``first2`` NaN rows in front as well."""

    def __init__(self, n, d_in, ld, second, lib):
        d = dev()
        self.n, self.d_in, self.ld = n, d_in, ld
        r2, g = inputs(n)
        self.r2_host = r2
        self.r2 = torch.full((n + TAIL,), float("nan"), device=d)
        self.r2[:n] = r2.to(d)
        self.X0 = torch.rand(n, ld, generator=g) * 0.5 + 0.125
        self.X = torch.full((n + TAIL, ld), float("nan"), device=d)
        self.first2, self.ld2 = 5, d_in + 1
        self.X2 = torch.full((self.first2 + n + TAIL, self.ld2), float("nan"), device=d) if second else None
        self.box = torch.tensor(BOX[:d_in], dtype=torch.float64, device=d)
        self.state = torch.zeros((), dtype=torch.int64, device=d)
        self.nw, self.nc = lib.tdq_r3_work_doubles(n), lib.tdq_r3_count_ints(n)
        self.work = torch.full((self.nw + TAIL,), float("nan"), dtype=torch.float64, device=d)
        self.stats = torch.full((2 + TAIL,), float("nan"), dtype=torch.float64, device=d)
        self.counts = torch.full((self.nc + TAIL,), -7, dtype=torch.int32, device=d)
        self.reset()

    def reset(self):
        self.X[:self.n] = self.X0.to(self.X.device)
        if self.X2 is not None:
            self.X2[self.first2:self.first2 + self.n] = self.X0[:, :self.ld2].to(self.X.device)
        self.state.fill_(STEP)

    def call(self, inv_c):
        from tensordiffeq_amd.ops import r3
        r3.r3_resample(self.r2[:self.n], inv_c, self.box, self.state, SEED, self.X, 0, self.X2, self.first2, self.n,
                       self.d_in, self.work[:self.nw], self.stats[:2], self.counts[:self.nc])

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.X, self.stats, self.counts, self.state)] + \
               ([self.X2.clone()] if self.X2 is not None else [])


@pytest.mark.parametrize("variant", ["tight", "strided+second"])
@pytest.mark.parametrize("d_in", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000, 70001])
def test_kernel_matches_mirror_and_fp64(n, d_in, variant, lib):
    from tensordiffeq_amd.ops import r3
    second = variant != "tight"
    ld = d_in + 3 if second else d_in
    inv_c = 3.0
    b = Buffers(n, d_in, ld, second, lib)
    a, tau, released = restate64(b.r2_host, inv_c)
    if n > 1:
        gap = float(np.abs(a - tau).min() / tau)
        print(f"R3_KERNEL n={n}: closest |a_i - tau| / tau = {gap:.3e}")
        assert gap > 1e-9                       # the released set is decided, not a matter of the last bit
    if n == 70001:
        assert lib.tdq_r3_count_ints(n) > 256 and lib.tdq_r3_work_doubles(n) == lib.tdq_r3_count_ints(n) + 1
    b.call(inv_c)
    got = b.snapshot()
    X, stats, counts, state = got[:4]
    # the mirror on the CPU, same inputs
    Xm = b.X0.clone()
    st_m = torch.tensor(STEP, dtype=torch.int64)
    stats_m = torch.zeros(2, dtype=torch.float64)
    counts_m = torch.zeros(b.nc, dtype=torch.int32)
    r3.r3_update_torch(b.r2_host, inv_c, b.box.cpu(), st_m, SEED, [Xm[:, :d_in]], stats_m, counts_m)
    Xc = X.cpu()
    changed = (Xc[:n, :d_in] != b.X0[:, :d_in]).any(1)
    assert torch.equal(changed, released)                              # the float64 set, no case left out
    assert torch.equal(Xc[:n], Xm)                                     # written rows: the mirror's bits;
    assert torch.equal(Xc[:n][~released], b.X0[~released])             # retained rows and the columns beside
    assert torch.equal(Xc[:n, d_in:], b.X0[:, d_in:])                  # the coordinates: untouched
    assert bool(torch.isnan(Xc[n:]).all())                             # nothing behind X
    lo = torch.tensor([p[0] for p in BOX[:d_in]])
    hi = torch.tensor([p[1] for p in BOX[:d_in]])
    assert bool(((Xc[:n, :d_in][released] >= lo) & (Xc[:n, :d_in][released] <= hi)).all())
    if second:
        X2 = got[4].cpu()
        f2 = b.first2
        assert bool(torch.isnan(X2[:f2]).all()) and bool(torch.isnan(X2[f2 + n:]).all())
        assert torch.equal(X2[f2:f2 + n, :d_in][released], Xc[:n, :d_in][released])    # the same values
        assert torch.equal(X2[f2:f2 + n][~released], b.X0[:, :b.ld2][~released])
        assert torch.equal(X2[f2:f2 + n, d_in:], b.X0[:, d_in:b.ld2])
    assert abs(float(stats[0]) - tau) <= 1e-12 * tau and float(stats[1]) == float(STEP)
    assert float(stats_m[0]) == pytest.approx(tau, rel=1e-12)
    assert bool(torch.isnan(stats[2:]).all()) and bool(torch.isnan(b.work[b.nw:]).all())
    assert int(counts[:b.nc].sum()) == int(released.sum())             # exact
    assert torch.equal(counts[:b.nc].cpu(), counts_m) and bool((counts[b.nc:] == -7).all())
    assert int(state) == STEP + 1 == int(st_m)
    assert bool(torch.isnan(b.r2[n:]).all())
    # the same inputs again: the same bits
    b.reset()
    b.call(inv_c)
    for x, y in zip(got, b.snapshot()):
        assert same_bits(x, y)


@pytest.mark.parametrize("case", ["tie", "nan"])
def test_kernel_tie_and_nan_release_everything(case, lib):
    n, d_in = 257, 2
    b = Buffers(n, d_in, d_in, False, lib)
    b.r2[:n] = 0.25
    if case == "nan":
        b.r2[:n] = torch.rand(n, device=dev()) + 0.5
        b.r2[n // 2] = float("nan")
    b.call(1.0)
    X, stats, counts, state = b.snapshot()
    assert int(counts[:b.nc].sum()) == n and int(state) == STEP + 1
    assert bool((X[:n].cpu() != b.X0).any(1).all())
    assert float(stats[0]) == 0.5 if case == "tie" else math.isnan(float(stats[0]))


def test_three_replayed_calls_equal_three_eager_calls(lib):
    from tensordiffeq_amd.graphs import capture_graph
    n, d_in = 5000, 5
    b = Buffers(n, d_in, d_in + 3, True, lib)
    for _ in range(3):
        b.call(3.0)
    eager = b.snapshot()
    assert int(eager[3]) == STEP + 3
    b.reset()
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):      # a first call outside the capture, as the engines do
        b.call(3.0)
    torch.cuda.current_stream(dev()).wait_stream(side)
    torch.cuda.synchronize()
    b.reset()
    g = torch.cuda.CUDAGraph()
    with capture_graph(g):
        for _ in range(3):
            b.call(3.0)
    b.reset()
    g.replay()
    for x, y in zip(eager, b.snapshot()):
        assert same_bits(x, y)


def test_kernel_refuses_bad_arguments(lib):
    import ctypes
    from tensordiffeq_amd.ops import _lib
    d = dev()
    n, d_in = 300, 2
    r2 = torch.rand(n, device=d)
    box = torch.tensor(BOX + BOX[:4], dtype=torch.float64, device=d)       # room for the refused d_in = 9
    state = torch.full((), 21, dtype=torch.int64, device=d)
    X = torch.full((n, 9), 7.0, device=d)
    X2 = torch.full((n + 5, 9), 7.0, device=d)
    work = torch.full((8,), 7.0, dtype=torch.float64, device=d)
    stats = torch.full((2,), 7.0, dtype=torch.float64, device=d)
    counts = torch.full((2,), 7, dtype=torch.int32, device=d)
    null = ctypes.c_void_p(0)
    P = _lib.ptr

    def call(n_arg=n, d=d_in, ldx=9, ldx2=9, start2=5, **ptrs):
        a = dict(r2=P(r2), box=P(box), state=P(state), X=P(X), X2=P(X2), work=P(work), stats=P(stats),
                 counts=P(counts))
        a.update(ptrs)
        rc = lib.tdq_r3_resample(a["r2"], 1.0, a["box"], a["state"], 11, a["X"], ldx, a["X2"], ldx2, start2, n_arg, d,
                                 a["work"], a["stats"], a["counts"], _lib.stream_ptr(dev()))
        torch.cuda.synchronize()
        return rc

    bad = [dict(n_arg=0), dict(n_arg=-3), dict(d=0), dict(d=9), dict(ldx=1), dict(ldx2=1), dict(start2=-1)]
    bad += [{k: null} for k in ("r2", "box", "state", "X", "work", "stats", "counts")]
    for kw in bad:
        assert call(**kw) != 0, kw
    for t in (X, X2, work, stats):
        assert bool((t == 7.0).all())
    assert int(state) == 21 and bool((counts == 7).all())
    assert call() == 0                       # the same arguments, well formed; and X2 alone may be null
    assert int(state) == 22 and not bool((stats == 7.0).any()) and int(counts.sum()) > 0
    assert call(X2=null) == 0 and int(state) == 23


# ------------------------------------------------------------------------------------------
# b. the solver
# ------------------------------------------------------------------------------------------
LAYERS = (2, 128, 128, 128, 1)
N_F = 3001


def ac_r3(precision="bf16", backend="hip", resample="r3", n_f=N_F, seed=1234, **kw):
    """Allen-Cahn residual on ``n_f`` points and the IC on 512."""
    import tensordiffeq_amd as tdq
    from tensordiffeq_amd.boundaries import DomainND, IC
    tdq.set_seed(seed)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-1.0, 1.0], 512)
    D.add("t", [0.0, 1.0], 201)
    D.generate_collocation_points(n_f)

    def f_model(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        u_xx = tdq.grad(tdq.grad(u, x), x)
        return tdq.grad(u, t) - 0.0001 * u_xx + 5.0 * u * u * u - 5.0 * u

    init = IC(D, [lambda x: x ** 2 * np.cos(math.pi * x)], var=[["x"]])
    m = tdq.CollocationSolverND(verbose=False)
    m.compile(list(LAYERS), f_model, D, [init], backend=backend, device=dev(), precision=precision,
              resample=resample, resample_seed=kw.pop("resample_seed", 7), **kw)
    return m


def copies(m, prog=None):
    """``(rows of X_all, rows of FusedStepOp.X or None)`` of the residual points of ``prog``."""
    from tensordiffeq_amd.ops import fused_step
    prog = m.program() if prog is None else prog
    si = m._r3_residual_segment(prog)
    rows = prog.segment_rows(si)
    fs = fused_step.for_program(prog)
    if fs is None:
        return rows, None
    start = fs.segment_start(si)
    assert start is not None
    return rows, fs.X[start:start + rows.shape[0]]


def run_1_then_8(env, monkeypatch, check=None, n_f=N_F):
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        m = ac_r3(n_f=n_f)
        X0 = m.collocation_points()
        m.fit(tf_iter=1)
        if check is not None:
            check(m, 1, X0)
        m.fit(tf_iter=8)
        if check is not None:
            check(m, 9, X0)
        torch.cuda.synchronize()
        return m, m.collocation_points(), m.u_model.flat.detach().clone()


@pytest.mark.parametrize("n_f", [N_F, 9001])
def test_both_copies_move_together_under_the_step_graphs(n_f, monkeypatch):
    """After 1 step (the 1-step graph's eager warm-up) and after 8 more (one 8-step graph) the residual rows of
    ``X_all`` and of the one-launch step's own point set are equal bit for bit; the population equals that of
    the same steps without graphs.  3,001 + 512 points are 110 tiles, one per workgroup on an MI355X; 9,001 +
    512 are 298, more than its 256 CUs, so workgroups run two tile rounds; both end in a partial tile."""
    from tensordiffeq_amd.ops import fused_step

    def check(m, steps, X0):
        rows, frows = copies(m)
        assert frows is not None and torch.equal(rows, frows), steps
        assert m.resample_stats()["step"] == steps
        assert not torch.equal(rows.cpu(), X0)

    monkeypatch.setenv("TDQ_STEP_UNROLL", "8")
    m, pop, flat = run_1_then_8({}, monkeypatch, check, n_f)
    eng = m._get_engine(None, 1)
    fs = fused_step.for_program(m.program())
    print(f"R3_SOLVER fused point set N={fs.N} tile={fs.pt} tiles={-(-fs.N // fs.pt)} workgroups={fs.G}")
    if n_f == 9001:
        assert -(-fs.N // fs.pt) > fs.G                        # more than one tile round
    assert eng.graph_k is not None and eng._tail_one() and m._r3_op().hip
    assert fs.N % fs.pt != 0                                   # a partial last tile
    assert len(m._r3_op().dests) == 2
    e, pop_e, flat_e = run_1_then_8({"TDQ_NO_GRAPH": "1"}, monkeypatch, check, n_f)
    assert e._get_engine(None, 1).graph_a is None
    assert torch.equal(pop, pop_e) and torch.equal(flat, flat_e)
    lo, hi = torch.tensor([-1.0, 0.0]), torch.tensor([1.0, 1.0])
    assert bool(((pop >= lo) & (pop <= hi)).all())


@pytest.mark.parametrize("n_f", [N_F, 9001])
def test_point_ranges_path_graphs_equal_eager(n_f, monkeypatch):
    """``TDQ_FUSED_STEP=0``: the step on the point-range launches has one copy of the points (from 8,192 points
    on, two ranges on two streams)."""
    def check(m, steps, X0):
        rows, frows = copies(m)
        assert frows is None and m.resample_stats()["step"] == steps
        assert len(m._r3_op().dests) == 1

    monkeypatch.setenv("TDQ_FUSED_STEP", "0")
    monkeypatch.setenv("TDQ_STEP_UNROLL", "8")
    m, pop, flat = run_1_then_8({}, monkeypatch, check, n_f)
    assert m._get_engine(None, 1).graph_k is not None
    _, pop_e, flat_e = run_1_then_8({"TDQ_NO_GRAPH": "1"}, monkeypatch, check, n_f)
    assert torch.equal(pop, pop_e) and torch.equal(flat, flat_e)


def test_mirror_on_the_gpu_matches_the_kernel(monkeypatch):
    monkeypatch.setenv("TDQ_STEP_UNROLL", "8")
    k, pop_k, flat_k = run_1_then_8({}, monkeypatch)
    t, pop_t, flat_t = run_1_then_8({"TDQ_R3_KERNEL": "0"}, monkeypatch)
    assert k._r3_op().hip and not t._r3_op().hip
    assert t._get_engine(None, 1).graph_k is not None           # the mirror is captured too
    rows, frows = copies(t)
    assert torch.equal(rows, frows)
    assert torch.equal(pop_k, pop_t) and torch.equal(flat_k, flat_t)
    sk, st = k.resample_stats(), t.resample_stats()
    assert sk["step"] == st["step"] == 9 and sk["released"] == st["released"]
    assert sk["threshold"] == pytest.approx(st["threshold"], rel=1e-12)


def loss_error(m, prog):
    """Relative error of the HIP objective of ``prog`` (on its own copies of the points, as they are now)
    against the float64 torch jet on the current population."""
    from tensordiffeq_amd.fit import LossGradEngine
    fg = LossGradEngine(m, prog, m.lambdas).evaluate_fg()
    torch.cuda.synchronize()
    ref = ac_r3(backend="jet", resample=None, precision=None)
    rp = ref.program()
    si = next(t for t in rp.terms if t.kind == "residual").seg
    rp.refresh_points(si, m.collocation_points())
    tot, _ = rp.evaluate(m.u_model.flat.detach().double(), [])
    return abs(float(fg[-1]) - float(tot)) / abs(float(tot))


def test_loss_on_the_moved_points_and_the_lbfgs_copies():
    from tensordiffeq_amd.ops import fused_step
    m = ac_r3(precision="bf16", newton_precision="bf16x3")
    X0 = m.collocation_points()
    m.fit(tf_iter=8)
    assert not torch.equal(m.collocation_points(), X0)
    e16 = loss_error(m, m.program())
    lb = m._get_lbfgs_engine().program
    assert lb is not m.program() and lb.precision == "bf16x3"
    e3 = loss_error(m, lb)
    print(f"R3_LOSS after 8 steps: bf16 step {e16:.3e} (bound {LOSS_BOUND['bf16']:.0e}), "
          f"bf16x3 objective {e3:.3e} (bound {LOSS_BOUND['bf16x3']:.0e})")
    assert e16 < LOSS_BOUND["bf16"] and e3 < LOSS_BOUND["bf16x3"]
    # a whole fit: the objective's two copies hold the population the Adam phase ended with
    m2 = ac_r3(precision="bf16", newton_precision="bf16x3")
    m2.fit(tf_iter=8, newton_iter=3)
    twin = ac_r3(precision="bf16", newton_precision="bf16x3")
    twin.fit(tf_iter=8)
    final = twin.collocation_points()
    lb2 = m2._get_lbfgs_engine().program
    assert fused_step.for_program(lb2) is not None and fused_step.for_program(lb2).lo
    rows, frows = copies(m2, lb2)
    assert torch.equal(rows.cpu(), final) and torch.equal(frows.cpu(), final)
    assert torch.equal(m2.X_f_local.cpu(), final) and torch.equal(m2.collocation_points(), final)
    assert m2.resample_stats()["step"] == 8 and m2.fit_info["lbfgs"]["n_iter"] >= 1
    # once more: the objective's one-launch step exists by now and is refreshed in place
    m2.fit(tf_iter=8, newton_iter=3)
    again = m2.collocation_points()
    rows, frows = copies(m2, lb2)
    assert not torch.equal(again, final) and m2.resample_stats()["step"] == 16
    assert torch.equal(rows.cpu(), again) and torch.equal(frows.cpu(), again)
    assert torch.equal(copies(m2)[0].cpu(), again) and torch.equal(copies(m2)[1].cpu(), again)


def test_refuses_a_high_order_residual():
    """A KdV residual on 4,096 points plans as a mixed program whose residual segment runs on the high-order
    kernels (tests/test_high_order_residual.py): its points cannot be moved."""
    import tensordiffeq_amd as tdq
    from tensordiffeq_amd.boundaries import DomainND, IC, dirichletBC
    tdq.set_seed(0)
    D = DomainND(["x", "t"], time_var="t")
    D.add("x", [-5.0, 5.0], 128)
    D.add("t", [0.0, 1.0], 64)
    D.generate_collocation_points(4096)

    def kdv(u_model, x, t):
        u = u_model(torch.cat([x, t], 1))
        u_x = tdq.grad(u, x)
        return tdq.grad(u, t) + 6.0 * u * u_x + tdq.grad(tdq.grad(u_x, x), x)

    bcs = [IC(D, [lambda x: 0.5 / np.cosh(0.5 * x) ** 2], var=[["x"]]),
           dirichletBC(D, val=0.0, var="x", target="upper"), dirichletBC(D, val=0.0, var="x", target="lower")]
    plain = tdq.CollocationSolverND(verbose=False)
    plain.compile([2, 64, 64, 64, 1], kdv, D, bcs, backend="auto", device=dev(), precision="bf16x3")
    p = plain.program()
    assert p.mixed and p.segments[next(t for t in p.terms if t.kind == "residual").seg].hi
    m = tdq.CollocationSolverND(verbose=False)
    with pytest.raises(ValueError, match="order 3 or 4"):
        m.compile([2, 64, 64, 64, 1], kdv, D, bcs, backend="auto", device=dev(), precision="bf16x3", resample="r3")
