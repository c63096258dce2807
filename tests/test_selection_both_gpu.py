"""GPU: zedo_min_mpjpe_both - both protocols' row errors, per-pose minima and first arg-mins from ONE pass over the rows
(the reference scores every batch twice from the same preds: run/opt_main.py:227-228).  Slot 0 must be what
zedo_min_mpjpe(procrustes = 0) writes and slot 1 what procrustes = 1 writes, BIT FOR BIT, through each of the three row-error
kernels (generic, row-major staged, pose-major), both arg-min kernels, every joint count, shards, NaN and ties.

"equal" is torch.equal on _invariance.bits (NaN payloads included).
The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import bits, misaligned, ptr as P, refusal_sweep, replays_to, sentinels
from _shared import dev, one_arithmetic_mode, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


NAMES = ("err", "best", "best_h")


def pair(zh, x, gt, N, off=0):
    """The two-call form: (P1 outputs, P2 outputs) of zedo_min_mpjpe."""
    return zh.min_mpjpe(x, gt, N, procrustes=False, row_offset=off), zh.min_mpjpe(x, gt, N, procrustes=True, row_offset=off)


def assert_is_the_pair(both, two, what=""):
    B, N = two[0][0].shape[0], two[0][1].shape[0]
    assert both[0].shape == (2, B) and both[1].shape == (2, N) and both[2].shape == (2, N)
    assert both[0].dtype == torch.float64 and both[1].dtype == torch.float64 and both[2].dtype == torch.int32
    for slot in (0, 1):
        for name, tb, tt in zip(NAMES, both, two[slot]):
            assert tb[slot].is_contiguous()
            assert torch.equal(bits(tb[slot]), bits(tt)), (what, "slot", slot, name, int((bits(tb[slot]) != bits(tt)).sum()))


def assert_same(a, b, what=""):
    for name, ta, tb in zip(NAMES, a, b):
        assert torch.equal(bits(ta), bits(tb)), (what, name, int((bits(ta) != bits(tb)).sum()))


# ---- 1. the reference's own values -------------------------------------------------------------------------------------------

def test_both_golden(zh, golden):
    """tests/golden/eval_multi.npz, prepared as test_min_mpjpe_golden prepares it: slot 0 within 1e-12 of err_p1, slot 1 within
    3e-7 of err_p2 (the project's bounds for these quantities), minima and arg-mins those of the golden arrays; the row shard
    [N+5, 3N+2) against the same per-pose reference; the rank-2 fixtures (deg_planar_*) in slot 1 within 3e-7."""
    g = golden("eval_multi")
    preds = g["preds"]
    N, H = preds.shape[:2]
    rows = np.ascontiguousarray(np.swapaxes(preds, 0, 1).reshape(H * N, 17, 3))
    gt = (g["gt_mm_h36m"] - g["gt_mm_h36m"][:, 0:1]) / 1000.0
    err, best, best_h = zh.min_mpjpe_both(dev(rows), dev(gt, torch.float64), N)
    assert err.shape == (2, H * N) and best.shape == (2, N) and best_h.shape == (2, N)
    for slot, key, tol in ((0, "err_p1", 1e-12), (1, "err_p2", 3e-7)):
        e = err[slot].cpu().numpy().reshape(H, N).T
        print(f"both_golden {key}: max |d| {np.abs(e - g[key]).max():.3e} (bound {tol:g})")
        np.testing.assert_allclose(e, g[key], atol=tol, rtol=0)
        np.testing.assert_allclose(best[slot].cpu().numpy(), g[key].min(1), atol=tol, rtol=0)
        assert np.array_equal(best_h[slot].cpu().numpy(), g[key].argmin(1))
    lo, hi = N + 5, 3 * N + 2
    err, best, best_h = zh.min_mpjpe_both(dev(rows[lo:hi]), dev(gt, torch.float64), N, row_offset=lo)
    for slot, key, tol in ((0, "err_p1", 1e-12), (1, "err_p2", 3e-7)):
        full = g[key]
        for n in range(N):
            hs = [h for h in range(H) if lo <= h * N + n < hi]
            ref = min(full[n, h] for h in hs)
            assert abs(best[slot, n].item() - ref) <= tol and best_h[slot, n].item() == min(hs, key=lambda h: full[n, h])
    for tag in ("planar_pred", "planar_gt"):
        G, P, ref = g[f"deg_{tag}_gt"], g[f"deg_{tag}_pred"], g[f"deg_{tag}_err_p2"]
        err, _, _ = zh.min_mpjpe_both(dev(P.astype(np.float32)), dev(G - 0.0, torch.float64), len(G))
        print(f"both_golden rank2 {tag}: max |d| {np.abs(err[1].cpu().numpy() - ref).max():.3e} (bound 3e-7)")
        np.testing.assert_allclose(err[1].cpu().numpy(), ref, atol=3e-7, rtol=0)
        assert bool(torch.isfinite(err[0]).all())


# ---- 2. + 3. row-major staged kernel and generic kernel ---------------------------------------------------------------------------

def _row_major_case(N, H, off, cut, seed):
    rng = np.random.default_rng(seed)
    B = N * H - off - cut
    x = (0.3 * rng.standard_normal((B, 17, 3))).astype(np.float32)
    x[5, 3, 1] = np.nan
    x[B // 2:B // 2 + 3] = np.nan
    return dev(x), dev(0.3 * rng.standard_normal((N, 17, 3)), torch.float64), B


@pytest.mark.parametrize("N,H,off,cut", [(23, 211, 17, 5), (7, 5, 0, 0)], ids=["23x211-shard", "7x5"])
def test_both_row_major_staged_kernel_is_bitwise_the_two_calls(zh, N, H, off, cut):
    """J = 17, aligned rows, N < 8192: row_error17_kernel.  23 x 211 on the shard [17, N H - 5): the tiles wrap round the poses several
    times and the last tile is ragged; 7 x 5: N < 64, several wraps inside one tile.  One NaN coordinate and three all-NaN rows."""
    x, gt, B = _row_major_case(N, H, off, cut, 166)
    both = zh.min_mpjpe_both(x, gt, N, row_offset=off)
    assert_is_the_pair(both, pair(zh, x, gt, N, off), (N, H))
    assert int(torch.isnan(both[0][0]).sum()) == 4 and int(torch.isnan(both[0][1]).sum()) == 4


@pytest.mark.parametrize("N,H,off,cut", [(23, 211, 17, 5), (7, 5, 0, 0)], ids=["23x211-shard", "7x5"])
def test_both_generic_kernel_is_bitwise_the_aligned_run_and_the_two_calls(zh, N, H, off, cut):
    """The same inputs with the row pointer 4 bytes off a 16-byte boundary (row_error_kernel): equal to the aligned run of the one
    call and to the two calls on the unaligned pointer."""
    x, gt, B = _row_major_case(N, H, off, cut, 166)
    xb = misaligned(x, floats=1)                                 # 4 bytes off a 16-byte boundary: the generic one-lane-per-row kernel
    both_b = zh.min_mpjpe_both(xb, gt, N, row_offset=off)
    assert_same(both_b, zh.min_mpjpe_both(x, gt, N, row_offset=off), "generic vs staged")
    assert_is_the_pair(both_b, pair(zh, xb, gt, N, off), "generic")


# ---- 4. pose-major kernel, lane-per-pose arg-min --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pose_major_gt():
    rng = np.random.default_rng(168)
    return 8219, 5, dev(0.3 * rng.standard_normal((8219, 17, 3)), torch.float64)


@pytest.mark.parametrize("shard", ["whole", "inside", "partial"])
def test_both_pose_major_kernel_is_bitwise_the_two_calls(zh, pose_major_gt, shard):
    """J = 17, N = 8219 >= 8192 (odd: every hypothesis' tile starts at another 4-byte alignment), H = 5: row_error17_pose_major_kernel
    and the lane-per-pose arg-min, NaN rows as in test_selection_pose_major_kernel_is_bitwise_the_row_major_pair.  Equal to the two
    calls and to the unaligned (generic, row-major) run of the one call.  `partial`: rows [2N+100, 2N+100 + N//2) - the poses
    outside 100 .. 100 + N//2 hold no local row and read +inf / -1 in BOTH slots."""
    N, H, gt = pose_major_gt
    off, B = {"whole": (0, N * H), "inside": (N + 777, 3 * N + 5), "partial": (2 * N + 100, N // 2)}[shard]
    rng = np.random.default_rng(1680 + B % 97)
    x = (0.3 * rng.standard_normal((B, 17, 3))).astype(np.float32)
    x[11, 2, 0] = np.nan
    x[B - 3] = np.nan
    xa = dev(x)
    both = zh.min_mpjpe_both(xa, gt, N, row_offset=off)
    assert_is_the_pair(both, pair(zh, xa, gt, N, off), shard)
    assert_same(both, zh.min_mpjpe_both(misaligned(xa, floats=1), gt, N, row_offset=off), shard + ": pose-major vs generic")
    assert int(torch.isnan(both[0][0]).sum()) == 2 and int(torch.isnan(both[0][1]).sum()) == 2
    held = torch.zeros(N, dtype=torch.bool, device="cuda")
    if shard == "partial":
        held[100:100 + B] = True
    else:
        held[:] = True
    for slot in (0, 1):
        assert torch.equal(both[2][slot] >= 0, held)
        assert bool((both[2][slot][~held] == -1).all()) and bool(torch.isposinf(both[1][slot][~held]).all())
        assert not bool(torch.isinf(both[1][slot][held]).any())


# ---- 5. other joint counts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("J", [1, 2, 3, 5, 16, 21])
def test_both_at_other_joint_counts(zh, J):
    """N = 37, H = 6: equal to the two calls.  J = 1: slot 1 is all NaN with best_h 0 (the alignment of one joint is 0 / 0), slot 0
    finite - the NaN of one protocol does not reach the other."""
    g = np.random.Generator(np.random.Philox(key=[138, J]))
    N, H = 37, 6
    gt = 0.3 * g.standard_normal((N, J, 3))
    gt = gt - gt[:, 0:1]
    x = dev((np.tile(gt, (H, 1, 1)) + 0.05 * g.standard_normal((H * N, J, 3))).astype(np.float32))
    gtd = dev(gt, torch.float64)
    both = zh.min_mpjpe_both(x, gtd, N)
    assert_is_the_pair(both, pair(zh, x, gtd, N), J)
    assert bool(torch.isfinite(both[0][0]).all()) and bool(torch.isfinite(both[1][0]).all())
    if J == 1:
        assert bool(torch.isnan(both[0][1]).all()) and bool(torch.isnan(both[1][1]).all()) and bool((both[2][1] == 0).all())
    else:
        assert bool(torch.isfinite(both[0][1]).all())


def test_both_rank1_alignment_of_seventeen_collinear_joints(zh):
    """Seventeen predicted joints on one line (a rank-1 alignment, like J = 2 above): equal to the two calls."""
    g = np.random.Generator(np.random.Philox(key=[138, 170]))
    N, H = 37, 6
    gt = 0.3 * g.standard_normal((N, 17, 3))
    d = g.standard_normal((H * N, 1, 3))
    x = dev((g.standard_normal((H * N, 17, 1)) * d / np.linalg.norm(d, axis=2, keepdims=True)).astype(np.float32))
    gtd = dev(gt, torch.float64)
    both = zh.min_mpjpe_both(x, gtd, N)
    assert_is_the_pair(both, pair(zh, x, gtd, N), "collinear")
    assert bool(torch.isfinite(both[0]).all())


# ---- 6. ties and NaN order ------------------------------------------------------------------------------------------------------

def test_both_ties_and_nan_order(zh):
    """Hypotheses 1 and 3 of pose 2 are the same row, the closest to its ground truth: both slots report 1 (np.argmin).  Pose 4: NaN
    in hypotheses 4 and 2 -> index 2 and a NaN minimum in both slots (np.amin / np.argmin)."""
    g = np.random.Generator(np.random.Philox(key=[138, 6]))
    N, H = 9, 6
    gt = 0.3 * g.standard_normal((N, 17, 3))
    x = (np.tile(gt, (H, 1, 1)) + 0.1 * g.standard_normal((H * N, 17, 3))).astype(np.float32).reshape(H, N, 17, 3)
    x[1, 2] = (gt[2] + 0.001 * g.standard_normal((17, 3))).astype(np.float32)
    x[3, 2] = x[1, 2]
    x[4, 4, 7, 0] = np.nan
    x[2, 4] = np.nan
    xd, gtd = dev(x.reshape(H * N, 17, 3)), dev(gt, torch.float64)
    err, best, best_h = zh.min_mpjpe_both(xd, gtd, N)
    assert_is_the_pair((err, best, best_h), pair(zh, xd, gtd, N), "ties")
    for slot in (0, 1):
        e = err[slot].reshape(H, N)
        assert torch.equal(bits(e[1, 2]), bits(e[3, 2])) and best_h[slot, 2].item() == 1 and torch.equal(bits(best[slot, 2]), bits(e[1, 2]))
        assert bool(torch.isnan(e[2, 4])) and bool(torch.isnan(e[4, 4])) and int(torch.isnan(e).sum()) == 2
        assert best_h[slot, 4].item() == 2 and bool(torch.isnan(best[slot, 4]))


# ---- 7. each half of err is an input of zedo_pose_min ---------------------------------------------------------------------------

def test_both_halves_feed_pose_min(zh):
    x, gt, B = _row_major_case(23, 11, 17, 5, 167)
    err, best, best_h = zh.min_mpjpe_both(x, gt, 23, row_offset=17)
    for slot in (0, 1):
        assert err[slot].is_contiguous()
        b, i = zh.pose_min(err[slot], 23, 17)
        assert torch.equal(bits(b), bits(best[slot])) and torch.equal(i, best_h[slot])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------

def test_both_refusals_at_the_raw_abi(zh):
    """A NULL pointer for each of the five pointers in turn, B = 0, N = 0, J = 0 and row_offset = -1: ZEDO_E_BADARG, nothing written."""
    lib = zh._lib
    B, N, J = 12, 4, 17
    x = torch.full((B, J, 3), 0.25, device="cuda")
    gt = torch.zeros((N, J, 3), dtype=torch.float64, device="cuda")
    err, best, bh = sentinels((((2, B), torch.float64), ((2, N), torch.float64), ((2, N), torch.int32)))
    ptrs = [P(x), P(gt), P(err), P(best), P(bh)]
    call = lambda p=ptrs, b=B, n=N, j=J, off=0: lib.zedo_min_mpjpe_both(p[0], p[1], b, n, j, off, p[2], p[3], p[4], None)
    refusal_sweep(call, ptrs, range(5), sizes=[dict(b=0), dict(n=0), dict(j=0), dict(off=-1)],
                  untouched=((err, -7.0), (best, -7.0), (bh, -7)))              # ... and the control: the same call is accepted
    assert bool((err != -7.0).all()) and bool((best != -7.0).all()) and bool((bh >= 0).all())


# ---- 9. the pipeline ------------------------------------------------------------------------------------------------------------

def test_pipeline_select_is_bitwise_the_two_calls(zh, weights0):
    """Pipeline.select on a 64 x 5 problem and on a row shard of it: the dict built from two min_mpjpe calls, on bits; contiguous.
    The one call on the same rows agrees with both."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    g = np.random.Generator(np.random.Philox(key=[138, 9]))
    N, H = 64, 5
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10))
    pipe.H, pipe.N = H, N                                       # what load() sets; select reads the pose count only
    gt = 0.3 * g.standard_normal((N, 17, 3))
    x = dev((np.tile(gt, (H, 1, 1)) + 0.05 * g.standard_normal((H * N, 17, 3))).astype(np.float32))
    gtd = dev(gt, torch.float64)
    for lo, hi in ((0, H * N), (N + 9, 4 * N - 3)):
        xs = x[lo:hi].contiguous()
        sel = pipe.select(xs, gt, row_offset=lo)
        two = pair(zh, xs, gtd, N, lo)
        (_, b1, i1), (_, b2, i2) = two
        assert_is_the_pair(zh.min_mpjpe_both(xs, gtd, N, row_offset=lo), two, (lo, hi))
        assert sorted(sel) == ["p1", "p2"]
        for key, (b, i) in (("p1", (b1, i1)), ("p2", (b2, i2))):
            sb, si = sel[key]
            assert sb.is_contiguous() and si.is_contiguous() and sb.shape == (N,) and si.shape == (N,)
            assert sb.dtype == torch.float64 and si.dtype == torch.int32
            assert torch.equal(bits(sb), bits(b)) and torch.equal(si, i), (lo, hi, key)


# ---- 10. stream capture ---------------------------------------------------------------------------------------------------------

def test_both_is_capturable(zh):
    """The call captured into a graph on a side stream and replayed twice reproduces the eager outputs: it allocates nothing and
    synchronises nothing of its own."""
    x, gt, B = _row_major_case(23, 11, 17, 5, 169)
    eager = zh.min_mpjpe_both(x, gt, 23, row_offset=17)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        zh.min_mpjpe_both(x, gt, 23, row_offset=17)             # warm the allocator on the capture stream
    torch.cuda.synchronize()
    replays_to(eager, lambda: zh.min_mpjpe_both(x, gt, 23, row_offset=17), s)
