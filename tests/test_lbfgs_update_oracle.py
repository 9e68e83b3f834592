"""Every native L-BFGS update against an fp64 oracle of ITS OWN state (csrc/lbfgs.hip,
optimizers/lbfgs_device.py).

Principle: one step from the same state.  After every ``update(fg)`` the test synchronises, reads
the optimizer's buffers and recomputes in float64, from those buffers and from clones taken before
the step, what the step had to produce.  Nothing depends on two trajectories staying together, so
the bounds sit at rounding level and the runs may be long.

Oracle (``check_step``), per step:
  * direction: ``d_ref = -H g`` by the two-loop recursion in fp64 over the chronological pairs (a
    different formulation from the kernels' compact form), ``d_cmp`` by the mirror's from-scratch
    triangular solves, ``delta_ref = |d_cmp - d_ref| / |d_ref|``; bound
    ``|d - d_ref| / |d_ref| <= 2^-22 + 10 delta_ref`` (4x the one fp32 rounding of ``d`` + the
    conditioning noise the two references show between themselves);
  * ring: the pushed rows of S / Y bitwise (fp32 ops), every other row bitwise unchanged, K / HEAD /
    SLOT by the push rule, HDIAG = y.s / y.y;
  * stored matrices (native): S^T Y, Y^T Y at ``p 2^-52 sum|terms|``; the packed R^{-1} at
    ``C cond_2(R) 2^-53 |R^{-1}|_F`` with ``C`` measured below;
  * scalars: G1, DT1 (relative ``p 2^-52``), GTD (``p 2^-52 sum|g_i d_i|``); F, FOLD, T, NITER,
    FEVAL, MINLOSS, BESTEP exact; coef of invalid slots 0;
  * iterate: x within 1 ulp of ``float32(x_prev + float32(T) d)`` evaluated in fp64; ``best_x``
    bitwise the x at which MINLOSS was evaluated.

Driver: a drifting-target quadratic ``g_t(x) = a (x - c_t)``, ``a = logspace(0, 3, p)``,
``c_{t+1} = c_t + DRIFT N(0, I)`` - it never converges and pushes a pair almost every step.

Measured values (MI355X for the native cases; both update paths give the same figures)
  * delta_ref (two-loop vs from-scratch compact form, fp64), worst: CPU runs 5.3e-15 (p=37 m=4,
    120 steps) and 4.3e-15 (p=120 m=50, 130 steps); over the native cases 5.5e-15 (p=50049).
  * the bordering recurrence of R^{-1} in fp64 torch (``Bordered``; it never calls a kernel)
    against a from-scratch triangular solve of the blocked-sum S^T Y (``gram``), worst ratio
    ``|dR^{-1}|_F / (cond_2(R) 2^-53 |R^{-1}|_F)``: CPU runs 0.62 (p=37 m=4), 0.015 (p=120 m=50);
    the mirror over every native case's shape <= 1.39 (p=266251 m=3); along the native
    trajectories <= 3.8 (p=4097 m=5)  ->  RINV_C = 8 x 3.8 ~ 30.  The kernels' own worst ratio:
    0.21 (p=50049), 0.15 (1), 0.010 (65), 2.33 (2113), 2.92 (4097), 1.21 (266251), 0.22 (3001,
    2000 steps).  (With a plain ``S @ Y.T`` as reference both figures rose with p - 71 for the
    kernels at p=266251 - : that was the reference's summation, hence ``gram``.)
  * push share of the driver: 1.000 in every run (asserted >= 0.9); p = 1 only with the seed of
    ``SEEDS``, see there.
  * worst native direction error ``|d - d_ref| / |d_ref|`` per case (bound 2.4e-7): 2.61e-8
    (p=50049 m=50), 4.85e-8 (1, 3), 3.74e-8 (63, 1), 4.02e-8 (65, 64), 2.69e-8 (2113, 7), 2.64e-8
    (4097, 5), 2.55e-8 (266251, 3), 2.80e-8 (3001, 50, 2000 steps).
"""
import math

import pytest
import torch

from tensordiffeq_amd.optimizers import lbfgs_device as LD

U53 = 2.0 ** -53
U52 = 2.0 ** -52
DRIFT = 1e-3
RINV_C = 30.0           # 8 x 3.8, the worst ratio of the fp64 bordering recurrence (docstring)
DIR_ABS = 2.0 ** -22    # 4 x the one fp32 rounding d receives


# ------------------------------------------------------------------ driver ------------------
class Drift:
    """Drifting-target quadratic: f = 1/2 sum a (x - c_t)^2, c_{t+1} = c_t + DRIFT N(0, I)."""

    def __init__(self, p, device, seed=0, drift=DRIFT):
        self.gen = torch.Generator().manual_seed(seed)
        self.a = torch.logspace(0, 3, p, dtype=torch.float64).to(device)
        self.c = torch.randn(p, generator=self.gen, dtype=torch.float64).to(device)
        self.drift = drift
        self.device = device

    def evaluate(self, x, f=None, gscale=1.0):
        """``[g | f]`` in fp32 at x (``f``: loss override, ``gscale``: gradient scale), then drift"""
        e = x.double() - self.c
        g = self.a * e * gscale
        loss = 0.5 * (self.a * e * e).sum() if f is None else torch.tensor(float(f), dtype=torch.float64)
        fg = torch.cat([g, loss.reshape(1).to(g.device)]).float().contiguous()
        self.c += self.drift * torch.randn(self.c.numel(), generator=self.gen, dtype=torch.float64).to(self.device)
        return fg


# ------------------------------------------------------------------ oracle ------------------
FIELDS = ("d", "g_old", "x", "best_x", "S", "Y", "SY", "YY", "coef", "st")


def snap(opt):
    return {k: getattr(opt, k).clone() for k in FIELDS}


def chron(k, head, m):
    return [(head + i) % m for i in range(k)]


def gram(A, B, blk=2048):
    """``A @ B.T`` in fp64 with the long sums blocked (sums of ``blk`` terms, then torch's cascade
    sum over the blocks): the reference's own error stays near ``blk 2^-53 sum|terms|`` at any p,
    whatever order the BLAS underneath sums in"""
    k, p = A.shape
    n = p // blk
    out = A[:, n * blk:] @ B[:, n * blk:].T
    if n:
        a = A[:, :n * blk].reshape(k, n, blk).transpose(0, 1)
        b = B[:, :n * blk].reshape(B.shape[0], n, blk).transpose(0, 1)
        out = out + torch.bmm(a, b.transpose(1, 2)).sum(0)
    return out


def two_loop(Sk, Yk, g, h0):
    """-H g by the two-loop recursion (Nocedal 1980), fp64, pairs oldest first"""
    k = Sk.shape[0]
    q = g.clone()
    rho = 1.0 / (Yk * Sk).sum(1)
    al = [None] * k
    for i in reversed(range(k)):
        al[i] = rho[i] * (Sk[i] @ q)
        q -= al[i] * Yk[i]
    r = h0 * q
    for i in range(k):
        r += (al[i] - rho[i] * (Yk[i] @ r)) * Sk[i]
    return -r


def compact(Sk, Yk, g, gam, SY, YY):
    """-H g by the compact representation with from-scratch triangular solves (the mirror's form);
    SY = S^T Y, YY = Y^T Y of the pairs"""
    R = torch.triu(SY)
    u = torch.linalg.solve_triangular(R, (Sk @ g).unsqueeze(1), upper=True).squeeze(1)
    rhs = torch.diagonal(SY) * u + gam * (YY @ u) - gam * (Yk @ g)
    p1 = torch.linalg.solve_triangular(R.T, rhs.unsqueeze(1), upper=False).squeeze(1)
    return -gam * g - Sk.T @ p1 + gam * (Yk.T @ u)


def rinv_scratch(SY):
    R = torch.triu(SY)
    eye = torch.eye(R.shape[0], dtype=torch.float64, device=R.device)
    return R, torch.linalg.solve_triangular(R, eye, upper=True)


def rinv_scale(R, Rinv):
    """cond_2(R) 2^-53 |R^{-1}|_F: the unit of the inverse's bound"""
    return float(torch.linalg.cond(R.cpu(), 2)) * U53 * float(Rinv.norm())


class Bordered:
    """Reference implementation of the kernels' R^{-1} recurrence in fp64 torch: dropping the
    oldest pair keeps the lower-right block, a push borders with the column -R^{-1} c / d and the
    diagonal 1 / d (c_i = s_i . y_new, d = s_new . y_new, plain matrix-vector products: sums in
    another order than :func:`gram`'s, as the kernels' are).  Chronological order, never re-solved."""

    def __init__(self):
        self.Ri = None

    def push(self, Sk, Yk, dropped):
        """Sk / Yk: the chronological pairs AFTER the push (the new pair last)"""
        k = Sk.shape[0]
        old = self.Ri
        if old is not None and dropped:
            old = old[1:, 1:]
        d = Sk[-1] @ Yk[-1]
        Ri = torch.zeros(k, k, dtype=torch.float64, device=Sk.device)
        if k > 1:
            c = Sk[:-1] @ Yk[-1]
            Ri[:-1, :-1] = old
            Ri[:-1, -1] = -(old @ c) / d
        Ri[-1, -1] = 1.0 / d
        self.Ri = Ri


def ulp32(v):
    """spacing of float32 at |v| (v: fp64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 23.0)


def check_step(opt, fg, pre, direction=True, matrices=True, iterate=True, stats=None):
    """One update from ``pre`` (clones before ``update(fg)``; afterwards the step has been taken:
    fused path, or ``axpy()`` on the other paths) - the run is expected to go on (no stop)."""
    stats = stats if stats is not None else {}
    p, m, dev = opt.p, opt.m, opt.x.device
    st, ps = opt.st.tolist(), pre["st"].tolist()
    assert ps[LD.ACTIVE] == 1.0 and st[LD.ACTIVE] == 1.0 and st[LD.REASON] == 0.0, (st[LD.ACTIVE], st[LD.REASON])
    g32 = fg[:-1]
    g = g32.double()
    f = float(fg[-1])
    n0 = int(ps[LD.NITER])
    # ---- exact scalars
    improved = math.isfinite(f) if n0 == 0 else f < ps[LD.MINLOSS]
    assert st[LD.F] == f and st[LD.FOLD] == f
    assert st[LD.NITER] == n0 + 1
    assert st[LD.FEVAL] == ps[LD.FEVAL] + (1 if n0 > 0 else 0)
    assert st[LD.MINLOSS] == (f if improved else ps[LD.MINLOSS])
    assert st[LD.BESTEP] == (float(n0 - 1) if improved else ps[LD.BESTEP])
    assert st[LD.T] == (min(1.0, 1.0 / st[LD.G1]) if n0 == 0 else opt.lr)
    # ---- ring
    t32 = torch.tensor(ps[LD.T], dtype=torch.float32, device=dev)
    s32, y32 = t32 * pre["d"], g32 - pre["g_old"]
    sd, yd = s32.double(), y32.double()
    ys, yy = float(sd @ yd), float(yd @ yd)
    push = n0 >= 1 and ys > 1e-10
    k, head, slot = int(ps[LD.K]), int(ps[LD.HEAD]), -1
    dropped = False
    if push:
        if k == m:
            slot, head, dropped = head, (head + 1) % m, True
        else:
            slot, k = (head + k) % m, k + 1
    assert (st[LD.K], st[LD.HEAD], st[LD.PUSHED], st[LD.SLOT]) == (k, head, float(push), slot)
    keep = torch.ones(m, dtype=torch.bool, device=dev)
    if push:
        keep[slot] = False
        assert torch.equal(opt.S[slot], s32), "pushed s row"
        assert torch.equal(opt.Y[slot], y32), "pushed y row"
        e_ys = p * U52 * float(sd.abs() @ yd.abs())
        rel = e_ys / abs(ys) + p * U52 + U52   # both sums + the quotient's rounding, relative
        assert abs(st[LD.HDIAG] - ys / yy) <= rel * abs(ys / yy), (st[LD.HDIAG], ys / yy)
    else:
        assert st[LD.HDIAG] == ps[LD.HDIAG]
    assert torch.equal(opt.S[keep], pre["S"][keep]) and torch.equal(opt.Y[keep], pre["Y"][keep]), "ring rows"
    assert torch.equal(opt.g_old, g32)
    # ---- scalars with sums
    dd = opt.d.double()
    g1 = float(g.abs().sum())
    assert abs(st[LD.G1] - g1) <= p * U52 * g1
    dt1 = float(dd.abs().sum()) * st[LD.T]
    assert abs(st[LD.DT1] - dt1) <= p * U52 * dt1
    assert abs(st[LD.GTD] - float(g @ dd)) <= p * U52 * float(g.abs() @ dd.abs())
    idx = chron(k, head, m)
    valid = torch.zeros(m, dtype=torch.bool, device=dev)
    valid[idx] = True
    if opt.native:
        assert not opt.coef[:m][~valid].any() and not opt.coef[m:2 * m][~valid].any(), "coef of invalid slots"
    # ---- direction
    out = {"push": push, "dropped": dropped, "idx": idx}
    mats = matrices and opt.native and k > 0
    if (direction and k > 0 and n0 > 0) or mats:
        Sk, Yk = opt.S[idx].double(), opt.Y[idx].double()
        SYr, YYr = gram(Sk, Yk), gram(Yk, Yk)
    if direction:
        h0 = 1.0 if n0 == 0 else st[LD.HDIAG]
        if k == 0 or n0 == 0:
            d_ref = d_cmp = -h0 * g
        else:
            d_ref, d_cmp = two_loop(Sk, Yk, g, h0), compact(Sk, Yk, g, h0, SYr, YYr)
        nr = float(d_ref.norm())
        delta = float((d_cmp - d_ref).norm()) / nr
        err = float((dd - d_ref).norm()) / nr
        stats["delta_ref"] = max(stats.get("delta_ref", 0.0), delta)
        stats["dir_err"] = max(stats.get("dir_err", 0.0), err)
        assert err <= DIR_ABS + 10 * delta, (err, delta, n0, k)
    # ---- stored matrices
    if mats:
        ii = torch.tensor(idx, device=dev)
        SYs, YYs = opt.SY[ii][:, ii], opt.YY[ii][:, ii]
        Ya = Yk.abs()
        bad = (SYs - SYr).abs() > p * U52 * (Sk.abs() @ Ya.T)
        assert not bad.any(), ("S^T Y", n0, bad.nonzero().tolist()[:4])
        bad = torch.triu((YYs - YYr).abs() - p * U52 * (Ya @ Ya.T)) > 0
        assert not bad.any(), ("Y^T Y", n0, bad.nonzero().tolist()[:4])
        if k > 1:
            R, Rinv = rinv_scratch(SYr)
            out["unit"] = unit = rinv_scale(R, Rinv)
            out["Rinv"] = Rinv
            ratio = float((torch.triu(YYs.T, 1) - torch.triu(Rinv, 1)).norm()) / unit
            stats["rinv_ratio"] = max(stats.get("rinv_ratio", 0.0), ratio)
            assert ratio <= RINV_C, ("R^-1", ratio, n0, k)
    # ---- iterate
    if iterate:
        ref = pre["x"].double() + float(torch.tensor(st[LD.T], dtype=torch.float32)) * dd
        bad = (opt.x.double() - ref).abs() > ulp32(ref)
        assert not bad.any(), ("x", n0, bad.nonzero().tolist()[:4])
    assert torch.equal(opt.best_x, pre["x"] if improved else pre["best_x"]), "best_x"
    stats["steps"] = stats.get("steps", 0) + 1
    stats["pushes"] = stats.get("pushes", 0) + int(push)
    return out


class Runner:
    """optimizer + driver: ``step()`` = evaluate at x, update, take the step, check"""

    def __init__(self, p, m, device, native, seed=0, x0=None, **kw):
        self.x = torch.zeros(p, device=device) if x0 is None else x0
        self.opt = LD.DeviceLBFGS(self.x, m=m, max_iter=kw.pop("max_iter", 10 ** 6), **kw)
        if not native:
            self.opt.native = self.opt.fused = False
        self.drv = Drift(p, device, seed)
        self.stats = {}
        self.rec = Bordered()

    def sync(self):
        if self.x.is_cuda:
            torch.cuda.synchronize()

    def step(self, fg=None, recurrence=False, **checks):
        opt = self.opt
        if fg is None:
            fg = self.drv.evaluate(self.x)
        pre = snap(opt)
        opt.update(fg)
        opt.axpy()
        self.sync()
        out = check_step(opt, fg, pre, stats=self.stats, **checks)
        if recurrence and out["push"]:
            Sk, Yk = opt.S[out["idx"]].double(), opt.Y[out["idx"]].double()
            self.rec.push(Sk, Yk, out["dropped"])
            if Sk.shape[0] > 1:
                if "Rinv" in out:
                    Rinv, unit = out["Rinv"], out["unit"]
                else:
                    R, Rinv = rinv_scratch(gram(Sk, Yk))
                    unit = rinv_scale(R, Rinv)
                ratio = float((self.rec.Ri - Rinv).norm()) / unit
                self.stats["rec_ratio"] = max(self.stats.get("rec_ratio", 0.0), ratio)
        return pre

    def share(self):
        # the first update cannot push (no step behind it)
        return self.stats["pushes"] / max(1, self.stats["steps"] - 1)


def report(tag, r):
    s = r.stats
    print(f"LBFGS_ORACLE {tag}: steps {s['steps']} push share {r.share():.3f} delta_ref {s.get('delta_ref', 0):.2e} "
          f"dir_err {s.get('dir_err', 0):.2e} rinv_ratio {s.get('rinv_ratio', 0):.3g} rec_ratio {s.get('rec_ratio', 0):.3g}")


# ------------------------------------------------------------------ CPU: the mirror ---------
@pytest.mark.parametrize("p,m,steps", [(37, 4, 120), (120, 50, 130)])
def test_mirror_update_matches_oracle(p, m, steps):
    """The torch mirror against the oracle at every step, across the ring's wrap-around (the
    mirror keeps no S^T Y / Y^T Y: no matrix checks), and the fp64 bordering recurrence against a
    from-scratch solve (the ratio behind RINV_C)."""
    r = Runner(p, m, "cpu", native=False)
    for _ in range(steps):
        r.step(recurrence=True, matrices=False, iterate=False)   # (x.add_ rounds twice: no 1-ulp claim)
    report(f"mirror p={p} m={m}", r)
    assert int(r.opt.st[LD.K]) == m
    assert r.share() >= 0.9
    assert 8 * r.stats["rec_ratio"] <= RINV_C


# ------------------------------------------------------------------ GPU ---------------------
CASES = [
    (50049, 50, 130),   # production vector (odd p), ring wraps, R^{-1} shift at k = 50
    (1, 3, 20),         # one element, one block everywhere
    (63, 1, 20),        # m = 1: every push replaces the only pair
    (65, 64, 80),       # m = LB_MAXM, wraps at 64, 2 direction blocks
    (2113, 7, 40),      # 34 direction blocks: tree groups of size 2 and 1; 8 dots blocks (< 32)
    (4097, 5, 30),      # 2 dots chunks of 2048 / 2049
    (266251, 3, 12),    # nchunks capped at 64, nblk capped at 2048: 2-3 tiles per block
]


# In one dimension the secant step is exact, the iterate lands on the target of the evaluation
# before, and y.s = a s (s - drift) then has the sign of a ratio of two independent normal
# draws: 53-74 % of the steps push at ANY drift scale (measured at 1e-3 ... 10, seeds 0-2).
# The p = 1 case therefore runs the seed below, one of the ~0.1 % of seeds (11 of the first 12000)
# whose 20 draws push at every step; the oracle checks themselves do not depend on it.
SEEDS = {1: 2630}


def _native(monkeypatch, fused):
    from tensordiffeq_amd.ops import _lib
    _lib.load(required=True)
    monkeypatch.setenv("TDQ_LBFGS_FUSED", fused)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("p,m,steps", CASES)
def test_native_update_matches_oracle(p, m, steps, fused, monkeypatch):
    _native(monkeypatch, fused)
    r = Runner(p, m, "cuda", native=True, seed=SEEDS.get(p, 0))
    assert r.opt.native and r.opt.fused == (fused == "1")
    for _ in range(steps):
        r.step(recurrence=True)
    report(f"native p={p} m={m} fused={fused}", r)
    assert r.share() >= 0.9
    assert int(r.opt.st[LD.K]) == min(m, r.stats["pushes"])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
def test_native_update_long_run(fused, monkeypatch):
    """2000 steps at m = 50 (1950 drop-oldest shifts of R^{-1}): scalar and ring checks every
    step, direction and matrix checks every 10th step and on each of the last 60."""
    _native(monkeypatch, fused)
    p, m, steps = 3001, 50, 2000
    r = Runner(p, m, "cuda", native=True)
    for i in range(steps):
        full = i % 10 == 0 or i >= steps - 60
        r.step(direction=full, matrices=full)
    report(f"native long p={p} m={m} fused={fused}", r)
    assert r.share() >= 0.9


def _same(a, b, skip_best=True):
    for k in FIELDS:
        u, v = a[k], b[k]
        if k == "st" and skip_best:
            u, v = u.clone(), v.clone()
            u[LD.BEST] = v[LD.BEST] = 0.0
        if k == "best_x":
            continue
        # bitwise (NaN-proof): compare the bytes
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("warm", [3, 12], ids=["k<m", "wrapped"])
def test_native_skipped_push(warm, fused, monkeypatch):
    """y = 0, then y.s < 0: no push, ring / H0 / S^T Y / Y^T Y + R^{-1} bitwise unchanged, the
    direction still the oracle's on the old history; then a normal step passes every check."""
    _native(monkeypatch, fused)
    p, m = 777, 4
    r = Runner(p, m, "cuda", native=True)
    for _ in range(warm):
        r.step()
    opt = r.opt
    assert int(opt.st[LD.K]) == (m if warm > m + 1 else warm - 1)
    f = float(opt.st[LD.F])
    for j in range(2):
        if j == 0:
            g = opt.g_old.clone()                                        # y = 0
        else:
            s = torch.tensor(float(opt.st[LD.T]), dtype=torch.float32, device="cuda") * opt.d
            g = opt.g_old - 0.1 * s                                      # y.s = -0.1 s.s < 0
        fg = torch.cat([g, torch.tensor([f - 1.0 - j], device="cuda")]).contiguous()
        pre = r.step(fg=fg)
        assert float(opt.st[LD.PUSHED]) == 0.0 and float(opt.st[LD.SLOT]) == -1.0
        for k in ("S", "Y", "SY", "YY"):
            assert torch.equal(getattr(opt, k), pre[k]), k
        for k in (LD.K, LD.HEAD, LD.HDIAG):
            assert float(opt.st[k]) == float(pre["st"][k])
    n = r.stats["pushes"]
    for j in range(3):   # (the first gradient after the made-up ones need not satisfy y.s > 0)
        r.step(fg=r.drv.evaluate(r.x, f=f - 5.0 - j))
    assert r.stats["pushes"] > n


# ---- native stop paths: one step from the same state, against the mirror ----
EXACT = (LD.ACTIVE, LD.NITER, LD.FEVAL, LD.K, LD.HEAD, LD.PUSHED, LD.SLOT, LD.F, LD.FOLD, LD.MINLOSS,
         LD.BESTEP, LD.REASON)
# sums in another order (G1, T = 1 / G1), a quotient of two (HDIAG); DT1 and GTD are sums over the
# fp32 d, whose rounding may fall differently in single elements
CLOSE = {LD.G1: 1e-12, LD.T: 1e-12, LD.HDIAG: 1e-9, LD.DT1: 1e-5, LD.GTD: 1e-5}


class Lockstep:
    """A native optimizer and a mirror that is reset to the native one's state before every step"""

    def __init__(self, p, m, **kw):
        self.xn = torch.zeros(p, device="cuda")
        self.xm = self.xn.clone()
        self.on = LD.DeviceLBFGS(self.xn, m=m, **kw)
        self.om = LD.DeviceLBFGS(self.xm, m=m, **kw)
        assert self.on.native
        self.om.native = self.om.fused = False
        self.drv = Drift(p, "cuda", seed=3)
        self.p = p

    def step(self, fg):
        on, om = self.on, self.om
        for k in ("x", "g_old", "d", "S", "Y", "best_x", "st", "fhist"):
            getattr(om, k).copy_(getattr(on, k))
        om.tol_x = on.tol_x
        pre_x = self.xn.clone()
        on.update(fg)
        on.axpy()
        om.update(fg)
        om.axpy()
        torch.cuda.synchronize()
        sn, sm = on.st.tolist(), om.st.tolist()
        for k in EXACT:
            assert sn[k] == sm[k] or (math.isnan(sn[k]) and math.isnan(sm[k])), (k, sn[k], sm[k])
        if sm[LD.ACTIVE] or sm[LD.REASON] == 5.0:
            for k, rel in CLOSE.items():
                assert sn[k] == pytest.approx(sm[k], rel=rel, abs=1e-300), (k, sn[k], sm[k])
        assert torch.equal(on.best_x, om.best_x)
        if sm[LD.ACTIVE]:
            td = (float(torch.tensor(sm[LD.T], dtype=torch.float32)) * om.d.double()).abs()
            assert not ((self.xn.double() - self.xm.double()).abs() > 2.0 ** -22 * (pre_x.double().abs() + td)).any()
        else:
            assert torch.equal(self.xn, pre_x) and torch.equal(self.xm, pre_x)   # a stop takes no step

    def after_stop(self):
        """three more update / axpy calls change nothing (BEST -> 0 apart)"""
        on = self.on
        before = snap(on)
        for _ in range(3):
            on.update(self.drv.evaluate(self.xn))
            on.axpy()
        torch.cuda.synchronize()
        _same(before, snap(on))
        assert torch.equal(before["best_x"], on.best_x)
        assert float(on.st[LD.BEST]) == 0.0


def _scenario(name, warm):
    """(optimizer kwargs, number of scripted evaluations -> fg, expected (reason, checks))"""
    W = warm
    if name == "zeros_at_start":
        return dict(max_iter=10), [lambda L, i: torch.zeros(L.p + 1, device="cuda")], 1
    if name == "nan_loss":
        fs = [10.0 - i for i in range(W + 2)] + [float("nan")]
        return dict(max_iter=100), [lambda L, i, f=f: L.drv.evaluate(L.xn, f=f) for f in fs], 2
    if name == "inf_at_eval0":
        fs = [float("inf"), 7.0, 8.0, 6.0]
        return dict(max_iter=3), [lambda L, i, f=f: L.drv.evaluate(L.xn, f=f) for f in fs], 3
    if name == "max_eval":
        return (dict(max_iter=W + 10, max_eval=W + 4),
                [lambda L, i: L.drv.evaluate(L.xn, f=50.0 + (i % 3)) for _ in range(W + 4)], 3)
    if name == "max_iter_last_best":
        return dict(max_iter=W + 5), [lambda L, i: L.drv.evaluate(L.xn, f=1000.0 - i) for _ in range(W + 6)], 3
    if name == "dt1_first":
        # g = 100: d = -g, t = 1 / |g|_1, DT1 = 1 <= tolX = 2 <= -g.d = 1e4 p
        g = lambda L, i: torch.cat([torch.full((L.p,), 100.0, device="cuda"), torch.tensor([50.0 - 10 * i], device="cuda")])
        return dict(max_iter=10, tol_x=2.0), [g, g], 4
    if name == "dt1":
        return dict(max_iter=W + 10), [lambda L, i: L.drv.evaluate(L.xn, f=1000.0 - 10 * i) for _ in range(W + 2)], 4
    if name == "fchange_fixed":
        fs = [9.0 - i for i in range(W + 1)] + [9.0 - W]
        return dict(max_iter=100, stop="fixed"), [lambda L, i, f=f: L.drv.evaluate(L.xn, f=f) for f in fs], 4
    if name == "fchange_legacy":
        # |f - f_old| = 0 does not stop the legacy test; |f| = 0 < tolX does
        fs = [9.0 - i for i in range(W + 1)] + [9.0 - W, 0.0]
        return dict(max_iter=100, stop="legacy"), [lambda L, i, f=f: L.drv.evaluate(L.xn, f=f) for f in fs], 4
    if name == "no_descent":
        ev = [lambda L, i: L.drv.evaluate(L.xn, f=1000.0 - i) for _ in range(W + 1)]
        return dict(max_iter=100), ev + [lambda L, i: L.drv.evaluate(L.xn, f=1.0, gscale=1e-12)], 5
    raise KeyError(name)


SCENARIOS = [("zeros_at_start", 0), ("nan_loss", 0), ("nan_loss", 8), ("inf_at_eval0", 0), ("max_eval", 0),
             ("max_eval", 8), ("max_iter_last_best", 0), ("max_iter_last_best", 8), ("dt1_first", 0), ("dt1", 1),
             ("dt1", 8), ("fchange_fixed", 1), ("fchange_fixed", 8), ("fchange_legacy", 1), ("fchange_legacy", 8),
             ("no_descent", 0), ("no_descent", 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("name,warm", SCENARIOS, ids=[f"{n}-{w}" for n, w in SCENARIOS])
def test_native_stop_paths(name, warm, fused, monkeypatch):
    """Every native stop against the mirror stepped from the native state, at k < m (warm 0 / 1)
    and after the ring (m = 3) has wrapped (warm 8); then nothing changes after the stop."""
    _native(monkeypatch, fused)
    kw, script, reason = _scenario(name, warm)
    L = Lockstep(70, 3, **kw)
    for i, ev in enumerate(script):
        assert L.on.active(), (name, i)
        if name == "dt1" and i == len(script) - 1:
            # DT1 <= tolX < -g.d of the state just reached: the next update stops on DT1 alone
            dt1, gtd = float(L.on.st[LD.DT1]), float(L.on.st[LD.GTD])
            assert dt1 < -gtd
            L.on.tol_x = math.sqrt(dt1 * -gtd)
        L.step(ev(L, i))
    on = L.on
    assert not on.active() and int(on.st[LD.REASON]) == reason, (on.reason, on.n_iter)
    if warm >= 8:
        assert int(on.st[LD.K]) == 3
    if name == "zeros_at_start":
        assert on.n_iter == 0 and torch.equal(L.xn, torch.zeros(70, device="cuda"))
    if name == "nan_loss":
        assert on.n_iter == warm + 2 and on.min_loss == 10.0 - (warm + 1)
    if name == "inf_at_eval0":
        assert on.min_loss == 6.0 and on.best_epoch == 2 and torch.equal(on.best_x, L.xn)
    if name == "max_eval":
        assert on.func_eval == warm + 4 and on.n_iter == warm + 3
    if name == "max_iter_last_best":
        assert on.n_iter == warm + 5 and torch.equal(on.best_x, L.xn) and on.best_epoch == warm + 4
    L.after_stop()


# ---- weight images (fused path) ----
def _image_setup(sizes, monkeypatch):
    from tensordiffeq_amd.jet import JetPlan
    from tensordiffeq_amd.models.networks import TanhMLP
    from tensordiffeq_amd.ops import jet_hip
    _native(monkeypatch, "1")
    torch.manual_seed(0)
    net = TanhMLP(sizes, device="cuda")
    P = net.flat.detach().clone().contiguous()
    X = (torch.rand(512, 2, device="cuda") * 2 - 1).contiguous()
    plan = JetPlan([(0,), (1,), (0, 0)], 2)
    _, saved = jet_hip.alloc_forward(X, P, net, plan, "bf16x3")
    saved[2].zero_()
    jet_hip.pack_images(saved)
    return P, saved, jet_hip


def _images_match_pack(saved, jet_hip):
    torch.cuda.synchronize()
    have = saved[2].clone()
    jet_hip.pack_images(saved)
    torch.cuda.synchronize()
    return torch.equal(have.view(torch.int32), saved[2].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[2, 128, 128, 128, 128, 1], [2, 128, 128, 128, 1]], ids=["128x4", "128x3"])
def test_update_scatters_exactly_what_pack_writes(sizes, monkeypatch):
    """The fused update's scatter of the new x into the objective's weight images against a pack
    from x, bitwise, after each of 60 steps (m = 8: the ring wraps).  A "no descent direction" stop
    undoes the step in x only: the images are flagged stale, and a run restarted behind a pack
    scatters exactly again."""
    P, saved, jet_hip = _image_setup(sizes, monkeypatch)
    r = Runner(P.numel(), 8, "cuda", native=True, x0=P, img_target=jet_hip.img_target(saved))
    assert r.opt.fused and r.opt.img_target is not None
    for i in range(60):
        r.step(direction=False, matrices=False)
        assert _images_match_pack(saved, jet_hip), i
        assert not r.opt.images_stale
    x_before = P.clone()
    # |g|_1 > tolFun but g.d > -tolX (the evaluation of test_fused_update_descent_stop_restores_x)
    r.opt.update(torch.cat([torch.full((P.numel(),), 1e-9, device="cuda"), torch.ones(1, device="cuda")]).contiguous())
    torch.cuda.synchronize()
    assert r.opt.reason == LD.REASONS[5]
    assert torch.equal(P, x_before)
    assert r.opt.images_stale
    jet_hip.pack_images(saved)         # what the next run's first evaluation does
    r.opt.reset()
    assert not r.opt.images_stale
    for i in range(3):
        r.step(direction=False, matrices=False)
        assert _images_match_pack(saved, jet_hip), i
