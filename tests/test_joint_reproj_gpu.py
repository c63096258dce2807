"""GPU: zedo_joint_reproj / zedo_joint_compose - joint-wise aggregation WITHOUT ground truth: per (pose, joint) the hypothesis whose joint
of x + T reprojects closest to its detection (fp64 on the fp32 inputs, zedo_pose_min's rules on the flattened [B,J] distances), and the
pose assembled from those joints.  Held to the float64 reference of tests/_joint_ref.py (pinned on its own in
tests/test_joint_reproj_ref.py) on general intrinsics, through both routes (the walking kernel without d_jerr, the row kernel +
zedo_pose_min with it), on shards, ties, NaN, joints behind the camera, at the raw ABI's refusals and under stream capture.

Distance bound 1e-9 px, the bound and derivation of tests/test_select_reproj_gpu.py: pixel coordinates are below 2^14, where an fp64 ulp is
1.8e-12; a joint's chain has fewer than 20 roundings, and a single joint's chain is shorter than the row's weighted mean: about 4e-11.
"bitwise" is torch.equal on _invariance.bits, the integer view of a floating tensor.
Whether the assembled pose is closer to ground truth than the pose-level selection is not measured here or anywhere: these tests hold the
arithmetic, not the criterion's accuracy.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import misaligned, ptr as P, replays_to, same, sentinels
from _joint_ref import CASES, IDS, case, check_inputs, compose_ref, joint_reproj_ref, joint_select_ref
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-9


def run(zh, x, T, uv, K, off=0, rows=True):
    return zh.joint_reproj(dev(x), dev(T), dev(uv), dev(K), row_offset=off, return_rows=rows)


def test_the_inputs_are_what_the_bounds_assume():
    check_inputs()


@pytest.mark.parametrize("J,N,H", CASES, ids=IDS)
def test_row_distances_and_selection_match_the_float64_reference(zh, J, N, H):
    x, T, uv, K, _ = case(J, N, H)
    best, idx, jerr = run(zh, x, T, uv, K)
    assert jerr.shape == (H * N, J) and best.shape == (N, J) and idx.shape == (N, J)
    assert jerr.dtype == torch.float64 and best.dtype == torch.float64 and idx.dtype == torch.int32
    d_ref = joint_reproj_ref(x, T, uv, K)
    d = np.abs(jerr.cpu().numpy() - d_ref).max()
    print(f"joint reproj J={J} N={N} H={H}: max |jerr - ref| = {d:.3e} px (bound {TOL:g})")
    assert d <= TOL
    rbest, ridx = joint_select_ref(d_ref, N)
    assert np.array_equal(idx.cpu().numpy(), ridx)                                          # every (pose, joint), none excluded
    n = torch.arange(N, device="cuda")[:, None]
    j = torch.arange(J, device="cuda")[None, :]
    pick = jerr[idx.to(torch.int64) * N + n, j]
    assert same(best, pick)
    assert np.abs(best.cpu().numpy() - rbest).max() <= TOL
    b2, i2 = run(zh, x, T, uv, K, rows=False)                                               # the walking kernel: the same answer
    assert b2.shape == (N, J) and i2.shape == (N, J) and b2.dtype == torch.float64 and i2.dtype == torch.int32
    assert np.array_equal(i2.cpu().numpy(), ridx) and same(b2, pick)


@pytest.mark.parametrize("J,N,H", CASES, ids=IDS)
def test_the_routes_agree(zh, J, N, H):
    """best / idx with and without d_jerr are bitwise equal and bitwise zedo_pose_min on the flattened distances; x as a view 51 floats
    into a larger buffer (not 16-byte aligned) gives the same bits in all three outputs."""
    x, T, uv, K, _ = case(J, N, H)
    B = H * N
    xd, Td, uvd, Kd = dev(x), dev(T), dev(uv), dev(K)
    best, idx, jerr = zh.joint_reproj(xd, Td, uvd, Kd, return_rows=True)
    wb, wi = zh.joint_reproj(xd, Td, uvd, Kd)
    assert same(wb, best) and same(wi, idx)
    pb, pi = zh.pose_min(jerr.reshape(-1), N * J, 0)
    assert same(pb.reshape(N, J), best) and same(pi.reshape(N, J), idx)
    xb = misaligned(xd, floats=51)
    ub, ui, uj = zh.joint_reproj(xb, Td, uvd, Kd, return_rows=True)
    assert same(ub, best) and same(ui, idx) and same(uj, jerr)
    ub, ui = zh.joint_reproj(xb, Td, uvd, Kd)
    assert same(ub, best) and same(ui, idx)


@pytest.mark.parametrize("N", [64, 70])
def test_the_row_sum_is_the_existing_calls_row_error(zh, N):
    """No joint is behind the camera in these cases: the sum of jerr[b,:] in ascending j (np.cumsum: sequential, not pairwise), divided
    by J, is zedo_min_reproj(conf=None)'s err[b] - the same per-joint statements, the row's num += 1.0 * d and den += 1.0 being the same
    sequential sum and an exact count.  Asserted BITWISE (which is within the 1 fp64 ulp the contract asks for)."""
    J, H = 17, 5
    x, T, uv, K, _ = case(J, N, H)
    _, _, jerr = run(zh, x, T, uv, K)
    err = zh.min_reproj(dev(x), dev(T), dev(uv), dev(K), None)[0].cpu().numpy()
    mean = np.cumsum(jerr.cpu().numpy(), axis=1)[:, -1] / J
    ulps = np.abs(mean - err) / np.spacing(err)
    print(f"N={N}: max |cumsum(jerr)/J - err| = {ulps.max():.2f} ulp")
    assert ulps.max() <= 1.0
    assert np.array_equal(mean.view(np.int64), err.view(np.int64))


@pytest.mark.parametrize("J,N,H", CASES, ids=IDS)
def test_the_assembled_pose_is_at_least_as_close_as_the_pose_level_winner(zh, J, N, H):
    """For every pose: zedo_min_reproj of the camera-frame composed pose (T = 0, one hypothesis, the case's confidences) <= the pose-level
    best + 1e-3 px.  The slack covers the fp32 rounding of the composed coordinates: about 6e-8 m at these depths and focal lengths, well
    under 1e-4 px."""
    x, T, uv, K, conf = case(J, N, H)
    xd, Td, uvd, Kd, cd = dev(x), dev(T), dev(uv), dev(K), dev(conf)
    _, pose_best, _ = zh.min_reproj(xd, Td, uvd, Kd, cd)
    _, idx = zh.joint_reproj(xd, Td, uvd, Kd)
    cam = zh.joint_compose(xd, Td, idx)
    _, agg, ai = zh.min_reproj(cam, torch.zeros((N, 3), device="cuda"), uvd, Kd, cd)
    assert bool((ai == 0).all())
    slack = (agg - pose_best).max().item()
    print(f"J={J} N={N} H={H}: max (aggregated - pose-level) = {slack:.3e} px (bound 1e-3), mean {agg.mean().item():.3f} vs {pose_best.mean().item():.3f} px")
    assert bool((agg <= pose_best + 1e-3).all())


def _combine(parts):
    """(best, idx) of several shards -> one, on the host: NaN first, then the value, then the hypothesis index."""
    key = lambda c: (0 if np.isnan(c[0]) else 1, 0.0 if np.isnan(c[0]) else c[0], c[1])
    M = len(parts[0][0])
    best, idx = np.full(M, np.inf), np.full(M, -1, np.int32)
    for m in range(M):
        cand = [(b[m], i[m]) for b, i in parts if i[m] >= 0]
        if cand:
            best[m], idx[m] = min(cand, key=key)
    return best, idx


@pytest.mark.parametrize("shape,cuts,rows", [((17, 70, 5), [0, 93, 211, 350], True), ((17, 70, 5), [0, 93, 211, 350], False),
                                             ((17, 483, 3), [0, 93, 700, 1449], True), ((17, 483, 3), [0, 93, 700, 1449], False)],
                         ids=["with_jerr", "walking", "J17-N483-H3-with_jerr", "J17-N483-H3-walking"])
def test_shards_are_slices_of_the_whole(zh, shape, cuts, rows):
    """(17, 70, 5) cut at rows 0 / 93 / 211 / 350 and (17, 483, 3) at 0 / 93 / 700 / 1449 (N J = 8211: the row route's arg-min runs one lane
    per (pose, joint), with flattened offsets 93 J and 700 J that are no multiple of 64 J), on both routes: each shard's jerr is bitwise
    the slice, the shards' selections combined on the host are bitwise the unsharded selection, and a pose with no row in a shard reports
    (+inf, -1) for all its joints there."""
    J, N, H = shape
    x, T, uv, K, _ = case(J, N, H)
    best, idx, jerr = run(zh, x, T, uv, K)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out = run(zh, x[lo:hi], T[lo:hi], uv, K, off=lo, rows=rows)
        if rows:
            assert same(out[2], jerr[lo:hi]), (lo, hi)
        b, i = out[0].cpu().numpy(), out[1].cpu().numpy()
        held = np.zeros(N, bool)
        held[np.arange(lo, hi) % N] = True
        assert np.array_equal(i >= 0, np.repeat(held[:, None], J, 1)) and (i[~held] == -1).all() and np.isposinf(b[~held]).all()
        parts.append((b.reshape(-1), i.reshape(-1)))
    cb, ci = _combine(parts)
    assert np.array_equal(cb.view(np.int64), best.cpu().numpy().reshape(-1).view(np.int64))
    assert np.array_equal(ci, idx.cpu().numpy().reshape(-1))
    # rows [93, 120): 27 poses of one hypothesis only (N = 70: poses 23 .. 49 of hypothesis 1), the others report (+inf, -1) for all joints
    out = run(zh, x[93:120], T[93:120], uv, K, off=93, rows=rows)
    if rows:
        assert same(out[2], jerr[93:120])
    b, i = out[0], out[1].cpu().numpy()
    p0 = 93 % N
    held = (np.arange(N) >= p0) & (np.arange(N) < p0 + 27)
    assert (i[held] == 93 // N).all() and (i[~held] == -1).all() and int((~held).sum()) == N - 27
    assert np.isposinf(b.cpu().numpy()[~held]).all() and same(b[p0:p0 + 27], jerr[93:120])


def test_ties_nan_and_joints_behind_the_camera(zh):
    J, N, H = 17, 70, 5
    x, T, uv, K, _ = (a.copy() for a in case(J, N, H))
    x, T = x.reshape(H, N, J, 3), T.reshape(H, N, 3)
    # pose 2: its detections become the projection of hypothesis 1 (by far the best then, every joint), hypothesis 3 a bitwise copy -> 1
    X = x[1, 2].astype(np.float64) + T[1, 2].astype(np.float64)
    q = X @ K[2].astype(np.float64).T
    uv[2] = (q[:, :2] / q[:, 2:]).astype(np.float32)
    x[3, 2], T[3, 2] = x[1, 2], T[1, 2]
    # pose 4: a NaN coordinate in joint 7 of hypotheses 4 and 2 -> NaN, index 2, for that joint only
    x[4, 4, 7, 0] = np.nan
    x[2, 4, 7, 1] = np.nan
    # pose 6: hypothesis 0 has joint 5 at depth -1 -> +inf for that joint of that row only; pose 8: joint 3 so in every hypothesis
    x[0, 6, 5, 2] = -1.0 - T[0, 6, 2]
    x[:, 8, 3, 2] = -1.0 - T[:, 8, 2]
    xr, Tr = x.reshape(H * N, J, 3), T.reshape(H * N, 3)
    d_ref = joint_reproj_ref(xr, Tr, uv, K)
    rb, ri = joint_select_ref(d_ref, N)
    for rows in (True, False):
        out = run(zh, xr, Tr, uv, K, rows=rows)
        best, idx = out[0], out[1]
        assert np.array_equal(idx.cpu().numpy(), ri), rows
        assert bool((idx[2] == 1).all()) and float(best[2].max()) < 1e-2
        assert int(torch.isnan(best).sum()) == 1 and bool(torch.isnan(best[4, 7])) and idx[4, 7].item() == 2
        assert bool(torch.isfinite(best[4, torch.arange(J, device="cuda") != 7]).all())
        assert idx[6, 5].item() != 0 and bool(torch.isfinite(best[6]).all())
        assert int(torch.isposinf(best).sum()) == 1 and bool(torch.isposinf(best[8, 3])) and idx[8, 3].item() == 0
        if rows:
            e = out[2].reshape(H, N, J)
            assert same(e[1, 2], e[3, 2]) and same(best[2], e[1, 2])
            assert int(torch.isnan(e).sum()) == 2 and bool(torch.isnan(e[2, 4, 7])) and bool(torch.isnan(e[4, 4, 7]))
            assert int(torch.isposinf(e).sum()) == 1 + H and bool(torch.isposinf(e[0, 6, 5])) and bool(torch.isposinf(e[:, 8, 3]).all())
            assert np.isposinf(d_ref.reshape(H, N, J)[0, 6, 5]) and np.isposinf(d_ref.reshape(H, N, J)[:, 8, 3]).all()
            ok = np.isfinite(d_ref)
            assert np.abs(out[2].cpu().numpy()[ok] - d_ref[ok]).max() <= TOL
            first = (best, idx)
        else:
            assert same(best, first[0]) and same(idx, first[1])
    # the same joint behind the camera in every hypothesis of a SHARD: +inf and the first LOCAL hypothesis (rows [93, 350): pose 8 from h 2)
    b, i = run(zh, xr[93:], Tr[93:], uv, K, off=93, rows=False)
    assert bool(torch.isposinf(b[8, 3])) and i[8, 3].item() == 2
    b2, i2, _ = run(zh, xr[93:], Tr[93:], uv, K, off=93, rows=True)
    assert same(b, b2) and same(i, i2)


@pytest.mark.parametrize("J,N,H", CASES, ids=IDS)
def test_compose_is_the_float64_formula_in_both_frames(zh, J, N, H):
    """Every case of the table, J up to 65: the camera frame and the frame of the pose-level winner, bitwise compose_ref."""
    x, T, uv, K, conf = case(J, N, H)
    xd, Td = dev(x), dev(T)
    _, idx = zh.joint_reproj(xd, Td, dev(uv), dev(K))
    _, _, ref = zh.min_reproj(xd, Td, dev(uv), dev(K), dev(conf))
    jh, rh = idx.cpu().numpy(), ref.cpu().numpy()
    cam, rel = zh.joint_compose(xd, Td, idx), zh.joint_compose(xd, Td, idx, ref)
    assert cam.shape == (N, J, 3) and rel.shape == (N, J, 3) and cam.dtype == torch.float32 and rel.dtype == torch.float32
    assert np.array_equal(cam.cpu().numpy().view(np.int32), compose_ref(x, T, jh).view(np.int32))
    assert np.array_equal(rel.cpu().numpy().view(np.int32), compose_ref(x, T, jh, rh).view(np.int32))


def test_compose(zh):
    """Bitwise the float64 formula, without and with ref_idx; joints whose hypothesis is the reference come back as x exactly; -1 or H at
    the raw ABI give NaN for those joints and leave the rest untouched; the binding raises ValueError."""
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = case(J, N, H)
    xd, Td = dev(x), dev(T)
    _, idx = zh.joint_reproj(xd, Td, dev(uv), dev(K))
    _, _, ref = zh.min_reproj(xd, Td, dev(uv), dev(K), dev(conf))
    jh, rh = idx.cpu().numpy(), ref.cpu().numpy()
    cam, rel = zh.joint_compose(xd, Td, idx), zh.joint_compose(xd, Td, idx, ref)
    assert cam.shape == (N, J, 3) and cam.dtype == torch.float32 and rel.shape == (N, J, 3)
    x4, T3 = x.reshape(H, N, J, 3).astype(np.float64), T.reshape(H, N, 3).astype(np.float64)
    n, j = np.arange(N)[:, None], np.arange(J)[None, :]
    want = x4[jh, n, j] + T3[jh, n]
    assert np.array_equal(cam.cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32))
    assert np.array_equal(cam.cpu().numpy().view(np.int32), compose_ref(x, T, jh).view(np.int32))
    want_rel = (want - T3[rh, np.arange(N)][:, None, :]).astype(np.float32)
    assert np.array_equal(rel.cpu().numpy().view(np.int32), want_rel.view(np.int32))
    assert np.array_equal(rel.cpu().numpy().view(np.int32), compose_ref(x, T, jh, rh).view(np.int32))
    own = jh == rh[:, None]
    assert own.any() and not own.all()
    assert np.array_equal(rel.cpu().numpy()[own].view(np.int32), x.reshape(H, N, J, 3)[rh, np.arange(N)][own].view(np.int32))
    # raw ABI: indices outside 0 .. H-1
    lib = zh._lib
    bad = idx.clone()
    bad[3, 4], bad[5, 0] = -1, H
    out = torch.full((N, J, 3), -7.0, device="cuda")
    assert lib.zedo_joint_compose(P(xd), P(Td), P(bad), P(ref), H, N, J, P(out), None) == 0
    torch.cuda.synchronize()
    hit = torch.zeros((N, J), dtype=torch.bool, device="cuda")
    hit[3, 4] = hit[5, 0] = True
    assert bool(torch.isnan(out[hit]).all()) and torch.equal(out[~hit], rel[~hit])
    badref = ref.clone()
    badref[9], badref[11] = H, -1
    assert lib.zedo_joint_compose(P(xd), P(Td), P(idx), P(badref), H, N, J, P(out), None) == 0
    torch.cuda.synchronize()
    rows = torch.zeros(N, dtype=torch.bool, device="cuda")
    rows[9] = rows[11] = True
    assert bool(torch.isnan(out[rows]).all()) and torch.equal(out[~rows], rel[~rows])
    for ji, ri in ((bad, ref), (idx, badref), (bad, None)):
        with pytest.raises(ValueError):
            zh.joint_compose(xd, Td, ji, ri)
    # refusals
    out.fill_(-7.0)
    args = [P(xd), P(Td), P(idx), P(ref)]
    for k in (0, 1, 2):
        assert lib.zedo_joint_compose(*[None if i == k else a for i, a in enumerate(args)], H, N, J, P(out), None) == -1
    assert lib.zedo_joint_compose(*args, H, N, J, None, None) == -1
    assert lib.zedo_joint_compose(*args, 0, N, J, P(out), None) == -1 and lib.zedo_joint_compose(*args, H, 0, J, P(out), None) == -1
    assert lib.zedo_joint_compose(*args, H, N, 0, P(out), None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_refusals_at_the_raw_abi(zh):
    """Each required NULL, B = 0, N = 0, J = 0 and row_offset = -1: ZEDO_E_BADARG, nothing written; B*J above INT_MAX as well (refused before
    any pointer is used); a NULL d_jerr is accepted."""
    lib = zh._lib
    J, N, H = 17, 3, 4
    B = N * H
    x = torch.full((B, J, 3), 0.25, device="cuda")
    T = torch.tensor([[0.0, 0.0, 5.0]], device="cuda").repeat(B, 1).contiguous()
    uv = torch.full((N, J, 2), 500.0, device="cuda")
    K = torch.tensor([[1100.0, 0, 500], [0, 1100, 500], [0, 0, 1]], device="cuda").repeat(N, 1, 1).contiguous()
    jerr, best, bh = sentinels((((B, J), torch.float64), ((N, J), torch.float64), ((N, J), torch.int32)))
    ptrs = [P(x), P(T), P(uv), P(K), P(jerr), P(best), P(bh)]
    call = lambda p, b=B, n=N, j=J, off=0: lib.zedo_joint_reproj(p[0], p[1], p[2], p[3], b, n, j, off, p[4], p[5], p[6], None)
    for k in (0, 1, 2, 3, 5, 6):
        assert call([None if i == k else p for i, p in enumerate(ptrs)]) == -1, k
    assert call(ptrs, b=0) == -1 and call(ptrs, n=0) == -1 and call(ptrs, j=0) == -1 and call(ptrs, off=-1) == -1
    assert call(ptrs, b=2 ** 31 - 1, j=2) == -1 and call(ptrs, n=2 ** 31 - 1, j=2) == -1
    torch.cuda.synchronize()
    assert bool((jerr == -7.0).all()) and bool((best == -7.0).all()) and bool((bh == -7).all())
    assert call([None if i == 4 else p for i, p in enumerate(ptrs)]) == 0                  # the control: no d_jerr is legal
    torch.cuda.synchronize()
    assert bool((jerr == -7.0).all()) and bool((best >= 0).all()) and bool((bh == 0).all())
    assert call(ptrs) == 0
    torch.cuda.synchronize()
    assert bool((jerr >= 0).all())
    with pytest.raises(zh.ZedoError):
        zh.joint_reproj(x, T[:-1].contiguous(), uv, K)


@pytest.mark.parametrize("rows", [True, False], ids=["with_jerr", "walking"])
def test_the_call_is_capturable(zh, rows):
    """One call per route captured into a graph on a side stream (a single branch) and replayed twice reproduces the eager bits: it
    allocates nothing and synchronises nothing of its own."""
    x, T, uv, K, _ = (dev(a) for a in case(17, 70, 5))
    eager = zh.joint_reproj(x, T, uv, K, return_rows=rows)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        zh.joint_reproj(x, T, uv, K, return_rows=rows)            # warm the allocator on the capture stream
    torch.cuda.synchronize()
    replays_to(eager, lambda: zh.joint_reproj(x, T, uv, K, return_rows=rows), s)


def test_pipeline_aggregate_reproj_and_compose(zh, weights0):
    """Pipeline.aggregate_reproj on the problem of load() is joint_reproj on its detections and intrinsics (whole and a shard; an empty
    shard is empty_selection shaped [N,J]); Pipeline.compose is joint_compose."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    best, idx = zh.joint_reproj(xd, Td, dev(uv), dev(K))
    sb, si = pipe.aggregate_reproj(xd, Td)
    assert same(sb, best) and same(si, idx)
    lo, hi = 93, 211
    sb, si = pipe.aggregate_reproj(xd[lo:hi].contiguous(), Td[lo:hi].contiguous(), row_offset=lo)
    b2, i2 = zh.joint_reproj(xd[lo:hi].contiguous(), Td[lo:hi].contiguous(), dev(uv), dev(K), row_offset=lo)
    assert same(sb, b2) and same(si, i2)
    eb, ei = pipe.aggregate_reproj(xd[:0], Td[:0])
    assert eb.shape == (N, J) and ei.shape == (N, J) and eb.dtype == torch.float64 and ei.dtype == torch.int32
    assert bool(torch.isposinf(eb).all()) and bool((ei == -1).all())
    _, ref = pipe.select_reproj(xd, Td)
    assert torch.equal(pipe.compose(xd, Td, idx, ref), zh.joint_compose(xd, Td, idx, ref))
    assert torch.equal(pipe.compose(xd, Td, idx), zh.joint_compose(xd, Td, idx))
    with pytest.raises(ValueError):
        pipe.compose(xd, Td, ei, ref)
