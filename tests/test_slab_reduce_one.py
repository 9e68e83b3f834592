"""``tdq_dp_tail_a_bf3`` (the gradient + loss reduction of the L-BFGS objective and of the DP step):
the one-launch column-block reduction (csrc/jet_bf3.hip ``tail_one_reduce_kernel``) against the two
passes, bit for bit.  bf16 slab rows take the one launch by default (``TDQ_TAIL_ONE=0``: the two
passes); fp32 rows keep the two passes (no gain measured) and reach the one launch only through the
test value 2 of the ``half_ovr`` argument."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NET = (2, 128, 128, 128, 128, 1)
SMALL = (2, 32, 1)            # P = 129: a partial last column block
N_TERMS, N_SCAL, S_STREAMS = 3, 2, 3


def _setup(net, rows, half, n_lblocks, seed=0):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    P = sum((a + 1) * b for a, b in zip(net[:-1], net[1:]))
    Pst = (P + 7) & ~7
    chunks = min(rows, 8)
    slab = torch.randn(rows, Pst, device=dev, generator=g) * 1e-2
    work = torch.zeros((rows + chunks) * Pst, device=dev)
    if half:
        work.view(torch.bfloat16)[:rows * Pst] = slab.to(torch.bfloat16).reshape(-1)
    else:
        work[:rows * Pst] = slab.reshape(-1)
    lpart = torch.randn(n_lblocks, N_TERMS + N_SCAL, device=dev, generator=g).contiguous()
    gx = torch.randn(P, device=dev, generator=g) * 1e-2
    return P, Pst, work, lpart, gx


def _reduce(net, rows, half, work, lpart, gx, P, c_first=0, one=True):
    from tensordiffeq_amd.ops import _lib
    lib = _lib.load()
    dev = work.device
    out = {"grad": torch.zeros(P, device=dev), "losses": torch.zeros(N_TERMS, device=dev),
           "dscal": torch.zeros(N_SCAL, device=dev), "total": torch.zeros(1, device=dev)}
    widths = (ctypes.c_int * (len(net) - 2))(*net[1:-1])
    p = _lib.ptr
    rc = lib.tdq_dp_tail_a_bf3(p(work), p(out["grad"]), 64, net[0], widths, net[-1], len(net) - 2, S_STREAMS, 0,
                               p(lpart), lpart.shape[0], N_TERMS, N_SCAL, p(out["losses"]), p(out["dscal"]),
                               p(out["total"]), c_first, p(gx), rows, 1 if half else (2 if one else 0),
                               _lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("half", [True, False], ids=["bf16rows", "fp32rows"])
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 245])
@pytest.mark.parametrize("net", [SMALL, NET], ids=["P129", "P50049"])
def test_reduce_one_launch_matches_two_passes(net, rows, half, monkeypatch):
    for with_gx in (True, False):
        P, Pst, work, lpart, gx = _setup(net, rows, half, n_lblocks=300 if rows == 9 else rows)
        gx = gx if with_gx else None
        monkeypatch.delenv("TDQ_TAIL_ONE", raising=False)   # the shipped default
        one = _reduce(net, rows, half, work, lpart, gx, P, one=True)
        # the one launch keeps its partials in LDS: the partial rows in memory stay untouched
        assert not work[rows * Pst:].any()
        monkeypatch.setenv("TDQ_TAIL_ONE", "0")
        two = _reduce(net, rows, half, work, lpart, gx, P, one=False)
        assert work[rows * Pst:].any()
        for k in one:
            assert torch.equal(one[k], two[k]), (k, with_gx)
        assert one["grad"].abs().sum() > 0 and one["losses"].abs().sum() > 0


@pytest.mark.parametrize("half", [True, False], ids=["bf16rows", "fp32rows"])
def test_reduce_with_prereduced_chunks_keeps_two_passes(half, monkeypatch):
    """c_first > 0: chunks below it come from the partial rows in memory, which only the two passes
    read - so the rows of chunk 0 may be destroyed after a first full reduction without changing the
    result, and the switch makes no difference."""
    rows = 19
    P, Pst, work, lpart, gx = _setup(SMALL, rows, half, n_lblocks=rows, seed=2)
    monkeypatch.setenv("TDQ_TAIL_ONE", "0")
    ref = _reduce(SMALL, rows, half, work, lpart, gx, P, one=False)   # leaves every chunk's partial row
    n0 = rows * 1 // 8                                            # rows of chunk 0: [0, floor(rows / 8))
    if half:
        work.view(torch.bfloat16)[:n0 * Pst] = 0
    else:
        work[:n0 * Pst] = 0
    for flag in ("1", "0"):
        monkeypatch.setenv("TDQ_TAIL_ONE", flag)
        out = _reduce(SMALL, rows, half, work, lpart, gx, P, c_first=1, one=flag == "1")
        for k in ref:
            assert torch.equal(out[k], ref[k]), (flag, k)
    monkeypatch.setenv("TDQ_TAIL_ONE", "1")                       # and the rows did matter
    assert not torch.equal(_reduce(SMALL, rows, half, work, lpart, gx, P, one=True)["grad"], ref["grad"])


def test_fp32_rows_keep_two_passes_by_default(monkeypatch):
    """fp32 slab rows (the bf16x3 L-BFGS objective) showed no gain from the one launch: whatever the
    switch says they take the two passes, which leave their partial rows in memory."""
    for flag in (None, "1"):
        if flag is None:
            monkeypatch.delenv("TDQ_TAIL_ONE", raising=False)
        else:
            monkeypatch.setenv("TDQ_TAIL_ONE", flag)
        P, Pst, work, lpart, gx = _setup(SMALL, 9, False, n_lblocks=9, seed=3)
        _reduce(SMALL, 9, False, work, lpart, gx, P, one=False)
        assert work[9 * Pst:].any()
