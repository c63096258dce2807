"""GPU: zedo_prune_rank and zedo_prune_gather - the piece between two stages of a pruned OIL loop.  The table of kept slots against the
numpy reference of tests/_prune_ref.py (pinned on its own in tests/test_prune_ref.py), the gather against torch indexing; every
comparison is exact.  Tile tails, one lane, tile boundaries, every tile size of the rank kernel on both sides of the H at which it changes
(64 poses per tile up to H = 256, 32 up to 512, 16 up to 1024), planted duplicates, signed zeros, infinities, NaNs; every number of 64-word
trips along a row of the gather and a second trip of its grid over the rows; chained stages; out-of-range table entries; guard bands; the refusals of the raw ABI; one
capture of both calls replayed on new input.
Whether pruning by reprojection error costs accuracy is not measured here or anywhere: these tests hold the arithmetic.  The pruning
does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import BADARG, all_same, bits, cur_stream, ptr as P, same, sentinels
from _prune_ref import GATHER_J, RANK_CASES, case, gather_ref, keep_ref, rank_ks
from _shared import dev, one_arithmetic_mode, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def rows(H, N, J, seed=0):
    g = np.random.Generator(np.random.Philox(key=[78, 100000 * J + 100 * H + N + seed]))
    return g.standard_normal((H * N, J, 3)).astype(np.float32), g.standard_normal((H * N, 3)).astype(np.float32)


# ---- 1. the table --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,N", RANK_CASES, ids=lambda v: str(v))
def test_the_table_is_the_reference_table(zh, H, N):
    e = case(H, N)
    ed = dev(e, torch.float64)
    for K in rank_ks(H):
        keep = zh.prune_rank(ed, N, K)
        assert keep.shape == (K, N) and keep.dtype == torch.int32
        got, ref = keep.cpu().numpy(), keep_ref(e, N, K)
        print(f"prune_rank H={H} N={N} K={K}: {int((got != ref).sum())} of {K * N} entries differ")
        assert np.array_equal(got, ref), K
        if K == H:
            assert np.array_equal(got, np.broadcast_to(np.arange(H, dtype=np.int32)[:, None], (H, N)))       # the identity table


def test_the_planted_poses_hold_what_the_case_says():
    """On the reference alone: the inputs above do contain the cases the comparison is about."""
    H, N = 50, 65
    e = case(H, N).reshape(H, N)
    assert np.isnan(e[:, 0]).all() and np.isposinf(e[:, 1]).all() and np.isfinite(e[:, 2]).sum() == 1
    assert np.isnan(e[:, 3:]).any() and np.isposinf(e[:, 3:]).any()
    assert any(((e[:, n] == 0) & np.signbit(e[:, n])).any() and ((e[:, n] == 0) & ~np.signbit(e[:, n])).any() for n in range(3, N))
    assert any(len(np.unique(e[np.isfinite(e[:, n]), n])) < np.isfinite(e[:, n]).sum() - 1 for n in range(3, N))   # duplicates besides the zeros
    k = keep_ref(e.reshape(-1), N, 2)
    assert k[:, 0].tolist() == [0, 1] and k[:, 1].tolist() == [0, 1] and k[:, 2].tolist() == [1, H // 2]         # two NaNs; two +inf; 3.25 and the first +inf


# ---- 2. the gather -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("J", GATHER_J)
def test_the_gather_is_torch_indexing_and_stages_chain(zh, J):
    H, N, K1, K2 = 7, 130, 5, 2
    x, T = rows(H, N, J)
    xd, Td = dev(x), dev(T)
    e1 = case(H, N)
    k1 = zh.prune_rank(dev(e1, torch.float64), N, K1)
    for hyp in (None, (100 + np.arange(H * N, dtype=np.int32)).reshape(H, N)):
        hd = None if hyp is None else dev(hyp, torch.int32)
        xo, To, ho = zh.prune_gather(k1, xd, Td, hd)
        assert xo.shape == (K1 * N, J, 3) and To.shape == (K1 * N, 3) and ho.shape == (K1, N) and ho.dtype == torch.int32
        g = (k1.long() * N + torch.arange(N, device="cuda")[None, :]).reshape(-1)
        assert same(xo, xd[g]) and same(To, Td[g])
        assert same(ho, k1 if hyp is None else hd.reshape(-1)[g].reshape(K1, N))
        rx, rT, rh = gather_ref(k1.cpu().numpy(), x, T, hyp)
        assert np.array_equal(xo.cpu().numpy().view(np.int32), rx.view(np.int32)) and np.array_equal(ho.cpu().numpy(), rh)
        assert np.array_equal(To.cpu().numpy().view(np.int32), rT.view(np.int32))
    # a second stage on the survivors: the ids are the composed table
    x1, T1, h1 = zh.prune_gather(k1, xd, Td)
    e2 = case(K1, N, seed=1)
    k2 = zh.prune_rank(dev(e2, torch.float64), N, K2)
    x2, T2, h2 = zh.prune_gather(k2, x1, T1, h1)
    composed = torch.gather(k1, 0, k2.long())                                  # k1[k2[r, n], n]
    assert same(h2, composed) and np.array_equal(composed.cpu().numpy(), np.take_along_axis(keep_ref(e1, N, K1), keep_ref(e2, N, K2), 0))
    g2 = (composed.long() * N + torch.arange(N, device="cuda")[None, :]).reshape(-1)
    assert same(x2, xd[g2]) and same(T2, Td[g2])
    # the identity table returns the inputs bit for bit
    ident = zh.prune_rank(dev(e1, torch.float64), N, H)
    xi, Ti, hi = zh.prune_gather(ident, xd, Td)
    assert same(xi, xd) and same(Ti, Td) and same(hi, ident)


@pytest.mark.parametrize("J", [J for J in GATHER_J if J != 5])
def test_an_entry_outside_the_slots_is_never_an_address(zh, J):
    """-1 and H planted in the table: those rows are NaN with id -1, every other row is intact, and the guard bands around the three
    outputs (raw ABI, outputs carved from larger buffers) keep their bytes."""
    H, N, K = 6, 65, 4
    x, T = rows(H, N, J)
    xd, Td = dev(x), dev(T)
    keep = keep_ref(case(H, N), N, K).copy()
    bad = [(0, 0), (1, 64), (3, 33), (2, 7)]
    for i, (r, n) in enumerate(bad):
        keep[r, n] = -1 if i % 2 == 0 else H
    keep[3, 64] = 2 ** 31 - 1
    keep[0, 63] = -2 ** 31
    kd = dev(keep, torch.int32)
    hyp = dev((7 * np.arange(H * N, dtype=np.int32)).reshape(H, N), torch.int32)
    G = 64                                                                    # guard words on either side
    for hd in (None, hyp):
        bx = torch.full((K * N * J * 3 + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
        bT = torch.full((K * N * 3 + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
        bh = torch.full((K * N + 2 * G,), -7, dtype=torch.int32, device="cuda")
        xo, To, ho = bx[G:-G], bT[G:-G], bh[G:-G]
        assert zh._lib.zedo_prune_gather(P(kd), H, K, N, J, P(xd), P(Td), P(hd), P(xo), P(To), P(ho), cur_stream()) == 0
        torch.cuda.synchronize()
        for b in (bx, bT, bh):
            assert bool((b[:G] == -7).all()) and bool((b[-G:] == -7).all())
        rx, rT, rh = gather_ref(keep, x, T, None if hd is None else hd.cpu().numpy())
        gx, gT, gh = xo.cpu().numpy().reshape(K * N, J, 3), To.cpu().numpy().reshape(K * N, 3), ho.cpu().numpy().reshape(K, N)
        outside = ((keep < 0) | (keep >= H)).reshape(-1)
        assert outside.sum() == 6
        assert np.isnan(gx[outside]).all() and np.isnan(gT[outside]).all() and (gh.reshape(-1)[outside] == -1).all()
        assert np.array_equal(gx[~outside].view(np.int32), rx[~outside].view(np.int32))
        assert np.array_equal(gT[~outside].view(np.int32), rT[~outside].view(np.int32)) and np.array_equal(gh, rh)


def test_the_gather_walks_the_rows_behind_the_grids_first_trip(zh):
    """The gather's grid is capped at 2^20 workgroups of four rows: from 4 194 304 output rows up a wavefront takes a second row.  J = 1,
    H = K = 2, N = 2 097 157: 4 194 314 rows, ten of them behind the first trip.  Outputs pre-filled with a sentinel, compared with torch
    indexing on the device: all rows, and on their own the rows from 4 194 304 up and the last one."""
    J, H, K, N = 1, 2, 2, 2097157
    rows, first_trip = K * N, 4 * (1 << 20)
    assert rows == first_trip + 10
    gen = torch.Generator(device="cuda").manual_seed(78)
    xd = torch.randn((H * N, J, 3), generator=gen, device="cuda")
    Td = torch.randn((H * N, 3), generator=gen, device="cuda")
    hd = torch.arange(100, 100 + H * N, dtype=torch.int32, device="cuda").reshape(H, N)
    # row 0 of the table: slot n % 2, row 1: the other one (not the ascending table of prune_rank: the gather takes any table)
    first = (torch.arange(N, device="cuda") % 2).to(torch.int32)
    keep = torch.stack([first, 1 - first]).contiguous()
    xo, To, ho = sentinels((((rows, J, 3), torch.float32), ((rows, 3), torch.float32), ((K, N), torch.int32)))
    assert zh._lib.zedo_prune_gather(P(keep), H, K, N, J, P(xd), P(Td), P(hd), P(xo), P(To), P(ho), cur_stream()) == 0
    torch.cuda.synchronize()
    g = (keep.long() * N + torch.arange(N, device="cuda")[None, :]).reshape(-1)
    tail = slice(first_trip, rows)
    for name, out, want in (("x", xo, xd[g]), ("T", To, Td[g]), ("hyp", ho.reshape(-1), hd.reshape(-1)[g])):
        print(f"gather {rows} rows, {name}: {int((bits(out) != bits(want)).reshape(rows, -1).any(1).sum())} rows differ, "
              f"{int((out[tail] == -7).reshape(10, -1).all(1).sum())} of the last 10 untouched")
        assert same(out[tail], want[tail]) and same(out[-1], want[-1]), name
        assert same(out, want), name


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(zh):
    H, N, K, J = 5, 9, 3, 17
    lib = zh._lib
    e = dev(case(H, N), torch.float64)
    big = torch.zeros((1025 * N,), dtype=torch.float64, device="cuda")
    keep = torch.full((1025, N), -7, dtype=torch.int32, device="cuda")
    rank = lambda err, h, n, k, out: lib.zedo_prune_rank(P(err), h, n, k, P(out), None)
    assert rank(e, H, N, 0, keep) == BADARG and rank(e, H, N, H + 1, keep) == BADARG and rank(e, H, N, -1, keep) == BADARG
    assert rank(big, 1025, N, 3, keep) == BADARG and rank(big, 1025, N, 1025, keep) == BADARG
    assert rank(e, H, 0, K, keep) == BADARG and rank(e, 0, N, 0, keep) == BADARG
    assert rank(None, H, N, K, keep) == BADARG and rank(e, H, N, K, None) == BADARG
    assert rank(e, 1024, 2 ** 31 // 1024 + 1, K, keep) == BADARG                                   # H*N above INT_MAX (refused before any access)
    torch.cuda.synchronize()
    assert bool((keep == -7).all())
    assert rank(big, 1024, N, 3, keep) == 0                                                         # the largest H is accepted
    torch.cuda.synchronize()
    assert bool((keep[:3] == torch.arange(3, device="cuda", dtype=torch.int32)[:, None]).all()) and bool((keep[3:] == -7).all())

    x, T = (dev(a) for a in rows(H, N, J))
    hyp = torch.zeros((H, N), dtype=torch.int32, device="cuda")
    kd = dev(keep_ref(case(H, N), N, K), torch.int32)
    xo, To, ho = sentinels((((K * N, J, 3), torch.float32), ((K * N, 3), torch.float32), ((K, N), torch.int32)))
    ok = dict(keep=kd, H=H, K=K, N=N, J=J, x=x, T=T, hyp=hyp, xo=xo, To=To, ho=ho)

    def gather(**kw):
        a = dict(ok, **kw)
        return lib.zedo_prune_gather(P(a["keep"]), a["H"], a["K"], a["N"], a["J"], P(a["x"]), P(a["T"]), P(a["hyp"]), P(a["xo"]), P(a["To"]),
                                     P(a["ho"]), None)
    for kw in (dict(K=0), dict(K=H + 1), dict(N=0), dict(J=0), dict(H=0, K=0), dict(keep=None), dict(x=None), dict(T=None), dict(xo=None),
               dict(To=None), dict(ho=None), dict(xo=x), dict(To=T), dict(ho=hyp), dict(ho=kd)):
        assert gather(**kw) == BADARG, kw
    torch.cuda.synchronize()
    assert bool((xo == -7).all()) and bool((To == -7).all()) and bool((ho == -7).all())
    assert bool((x == dev(rows(H, N, J)[0])).all()) and bool((hyp == 0).all())                       # the aliased inputs too
    assert gather() == 0 and gather(hyp=None) == 0
    with pytest.raises(ValueError):
        zh.prune_rank(e, N, 0)
    with pytest.raises(ValueError):
        zh.prune_rank(e, N, H + 1)
    with pytest.raises(ValueError):
        zh.prune_gather(kd, x[:-1], T[:-1])


# ---- 4. capture ----------------------------------------------------------------------------------------------------------------------

def test_one_capture_of_both_calls_replays_on_new_input(zh):
    """prune_rank + prune_gather captured once on a single stream (one branch); the static inputs are overwritten and the replay equals
    the eager calls on the new input bit for bit: neither call allocates or synchronises on its own."""
    H, N, K, J = 50, 130, 10, 17
    x, T = rows(H, N, J)
    e_s, x_s, T_s = dev(case(H, N), torch.float64), dev(x), dev(T)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        zh.prune_gather(zh.prune_rank(e_s, N, K), x_s, T_s)                    # warms the allocator for the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        keep = zh.prune_rank(e_s, N, K)
        out = zh.prune_gather(keep, x_s, T_s)
    for seed in (1, 2):
        e2 = case(H, N, seed)
        x2, T2 = rows(H, N, J, seed)
        e_s.copy_(dev(e2, torch.float64)); x_s.copy_(dev(x2)); T_s.copy_(dev(T2))
        for t in (keep,) + tuple(out):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        k_e = zh.prune_rank(dev(e2, torch.float64), N, K)
        o_e = zh.prune_gather(k_e, dev(x2), dev(T2))
        assert same(keep, k_e) and np.array_equal(k_e.cpu().numpy(), keep_ref(e2, N, K))
        assert all_same(out, o_e)
        assert not np.array_equal(keep_ref(e2, N, K), keep_ref(case(H, N), N, K))                  # the input did change the table
