"""GPU: zedo_min_reproj - selection of a hypothesis WITHOUT ground truth: per row the confidence-weighted mean reprojection distance
of x + T in pixels (fp64 on the fp32 inputs), per pose the minimum over the hypotheses and its index (zedo_pose_min's rules).
Held to the float64 reference of tests/_select_ref.py (pinned on its own in tests/test_select_reproj_ref.py) on general intrinsics,
through both row kernels (J = 17 staged through the LDS, generic one lane per row), on shards, ties, NaN, points behind the camera,
at the raw ABI's refusals and under stream capture.

Row-error bound 1e-9 px: pixel coordinates are below 2^14, where an fp64 ulp is 1.8e-12; a joint's chain has fewer than 20 roundings and
the weighted mean does not amplify: about 4e-11, so 1e-9 leaves a 25x margin.
"bitwise" is torch.equal on _invariance.bits, the integer view of a floating tensor.
The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import functools

import numpy as np
import pytest

from _invariance import bits, misaligned, ptr as P, replays_to, sentinels
from _select_ref import reproj_ref, select_ref
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = [(1, 1, 1), (1, 3, 2), (5, 3, 5), (17, 1, 5), (17, 64, 5), (17, 70, 5), (21, 70, 3)]
# what the table above stays below (csrc/zedo_metric.hip): a 64-row tile of row_reproj17_kernel that wraps round N = 7 poses nine times
# and one that wraps once, a row short of the tile (N = 63); J above 21, up to the ABI's 64; and N >= POSE_MIN_LANE_N = 8192, where
# launch_pose_min takes the lane-per-pose arg-min behind both row kernels (J = 17, odd N: every hypothesis starts at another alignment; J = 5)
BOUNDARY_CASES = [(17, 7, 30), (17, 63, 3), (33, 5, 4), (64, 3, 3), (17, 8219, 2), (5, 8200, 2)]
CASES = CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}" for J, N, H in CASES]
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def case(J, N, H):
    """-> (x [H N,J,3], T [H N,3], uv [N,J,2], K [N,3,3] general, conf [N,J] in (-0.2, 1.3)), float32 numpy; rows (h, n).  Read-only."""
    cl, uv, K = problem(J, N, H, general=True)
    g = np.random.Generator(np.random.Philox(key=[77, 1000 * J + N]))
    B = H * N
    x = (np.repeat(cl, N, axis=0) + 0.05 * g.standard_normal((B, J, 3))).astype(np.float32)
    T = np.stack([0.4 * g.standard_normal(B), 0.4 * g.standard_normal(B), 5 + 0.5 * g.standard_normal(B)], -1).astype(np.float32)
    conf = g.uniform(-0.2, 1.3, (N, J)).astype(np.float32)
    out = (x, T, np.ascontiguousarray(uv, dtype=np.float32), np.ascontiguousarray(K, dtype=np.float32), conf)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref(J, N, H, with_conf):
    x, T, uv, K, conf = case(J, N, H)
    e = reproj_ref(x, T, uv, K, conf if with_conf else None)
    e.setflags(write=False)
    return e


def run(zh, x, T, uv, K, conf=None, off=0):
    return zh.min_reproj(dev(x), dev(T), dev(uv), dev(K), None if conf is None else dev(conf), row_offset=off)


def test_the_inputs_are_what_the_bounds_assume():
    """On the reference alone: every joint in front of the camera, row errors of tens to hundreds of pixels, and no pose whose best
    and second-best hypotheses are closer than 1e-6 px - the arg-min comparison below cannot hide a failure behind a near tie."""
    gaps = []
    for J, N, H in CASES:
        x, T, uv, K, conf = case(J, N, H)
        q = np.einsum("bik,bjk->bji", K.astype(np.float64)[np.arange(H * N) % N], x.astype(np.float64) + T.astype(np.float64)[:, None])
        assert q[..., 2].min() > 1.0
        for with_conf in (False, True):
            e = ref(J, N, H, with_conf)
            assert np.isfinite(e).all() and 10 < e.min() and e.max() < 1000
            if H > 1:
                s = np.sort(e.reshape(H, N), axis=0)
                gaps.append((s[1] - s[0]).min())
    print(f"smallest best-to-second gap: {min(gaps):.3g} px")
    assert min(gaps) > 1e-6


@pytest.mark.parametrize("with_conf", [False, True], ids=["noconf", "conf"])
@pytest.mark.parametrize("J,N,H", CASES, ids=IDS)
def test_row_errors_and_selection_match_the_float64_reference(zh, J, N, H, with_conf):
    x, T, uv, K, conf = case(J, N, H)
    err, best, idx = run(zh, x, T, uv, K, conf if with_conf else None)
    assert err.shape == (H * N,) and best.shape == (N,) and idx.shape == (N,)
    assert err.dtype == torch.float64 and best.dtype == torch.float64 and idx.dtype == torch.int32
    e = ref(J, N, H, with_conf)
    d = np.abs(err.cpu().numpy() - e).max()
    print(f"reproj J={J} N={N} H={H} conf={with_conf}: max |err - ref| = {d:.3e} px (bound {TOL:g})")
    assert d <= TOL
    rbest, ridx = select_ref(e, N)
    assert np.array_equal(idx.cpu().numpy(), ridx)                                          # every pose, none excluded
    pick = err[idx.to(torch.int64) * N + torch.arange(N, device="cuda")]
    assert torch.equal(bits(best), bits(pick))
    assert np.abs(best.cpu().numpy() - rbest).max() <= TOL


@pytest.mark.parametrize("J,N,H", [(17, 64, 5), (17, 70, 5), (17, 8219, 2), (5, 8200, 2)], ids=["64", "70", "J17-N8219-H2", "J5-N8200-H2"])
def test_every_path_returns_the_same_bits(zh, J, N, H):
    """J = 17: a view of x one row (204 bytes) into a larger buffer is not 16-byte aligned and takes the generic kernel - the bits of
    the staged kernel, also where the lane-per-pose arg-min follows (N = 8219; J = 5 takes the generic kernel either way).
    No confidences = confidences of one; 5.0 acts as 1.0 and 0.0 as 1e-4, bitwise."""
    x, T, uv, K, conf = case(J, N, H)
    B = H * N
    xd, Td, uvd, Kd, cd = dev(x), dev(T), dev(uv), dev(K), dev(conf)
    xb = misaligned(xd, floats=J * 3)                               # one row in: 204 or 60 bytes, 12 past a 16-byte boundary
    for c in (None, cd):
        a, b = zh.min_reproj(xd, Td, uvd, Kd, c), zh.min_reproj(xb, Td, uvd, Kd, c)
        for ta, tb in zip(a, b):
            assert torch.equal(bits(ta), bits(tb))
    full = lambda v: torch.full((N, J), v, dtype=torch.float32, device="cuda")
    for x_ in (xd, xb):
        e_none = zh.min_reproj(x_, Td, uvd, Kd, None)[0]
        e_one = zh.min_reproj(x_, Td, uvd, Kd, full(1.0))[0]
        assert torch.equal(bits(e_none), bits(e_one))
        assert torch.equal(bits(zh.min_reproj(x_, Td, uvd, Kd, full(5.0))[0]), bits(e_one))
        assert torch.equal(bits(zh.min_reproj(x_, Td, uvd, Kd, full(0.0))[0]), bits(zh.min_reproj(x_, Td, uvd, Kd, full(1e-4))[0]))


def _combine(parts):
    """(best, idx) of several shards -> one, on the host: NaN first, then the value, then the hypothesis index."""
    key = lambda c: (0 if np.isnan(c[0]) else 1, 0.0 if np.isnan(c[0]) else c[0], c[1])
    N = len(parts[0][0])
    best, idx = np.full(N, np.inf), np.full(N, -1, np.int32)
    for n in range(N):
        cand = [(b[n], i[n]) for b, i in parts if i[n] >= 0]
        if cand:
            best[n], idx[n] = min(cand, key=key)
    return best, idx


def test_shards_are_slices_of_the_whole(zh):
    """(17, 70, 5) cut at rows 0 / 93 / 211 / 350: each shard's err is bitwise the slice, the shards' selections combined on the host are
    bitwise the unsharded selection, and a pose with no row in a shard reports (+inf, -1) there."""
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = case(J, N, H)
    err, best, idx = run(zh, x, T, uv, K, conf)
    cuts, parts = [0, 93, 211, 350], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        e, b, i = run(zh, x[lo:hi], T[lo:hi], uv, K, conf, off=lo)
        assert torch.equal(bits(e), bits(err[lo:hi])), (lo, hi)
        b, i = b.cpu().numpy(), i.cpu().numpy()
        held = np.zeros(N, bool)
        held[np.arange(lo, hi) % N] = True
        assert np.array_equal(i >= 0, held) and (i[~held] == -1).all() and np.isposinf(b[~held]).all()
        parts.append((b, i))
    cb, ci = _combine(parts)
    assert np.array_equal(cb.view(np.int64), best.cpu().numpy().view(np.int64)) and np.array_equal(ci, idx.cpu().numpy())
    # (the three shards above hold every pose at least once) rows [93, 120): poses 23 .. 49 only, the other 43 report (+inf, -1)
    e, b, i = run(zh, x[93:120], T[93:120], uv, K, conf, off=93)
    assert torch.equal(bits(e), bits(err[93:120]))
    held = (np.arange(N) >= 23) & (np.arange(N) < 50)
    assert np.array_equal(i.cpu().numpy() >= 0, held) and (i.cpu().numpy()[held] == 1).all() and (i.cpu().numpy()[~held] == -1).all()
    assert np.isposinf(b.cpu().numpy()[~held]).all() and torch.equal(bits(b[23:50]), bits(err[93:120]))


@pytest.mark.parametrize("J,N,H", [(17, 7, 30), (17, 8219, 2)], ids=["J17-N7-H30", "J17-N8219-H2"])
@pytest.mark.parametrize("with_conf", [False, True], ids=["noconf", "conf"])
def test_a_shard_that_starts_inside_the_poses_is_a_slice_of_the_whole(zh, J, N, H, with_conf):
    """Rows [17, N H - 5), the shard of tests/test_selection_both_gpu.py: the first tile starts at pose 17 % N, not 0 (N = 7: and wraps
    nine times; N = 8219: the lane-per-pose arg-min counts the hypotheses of poses 0 .. 16 from 1 and loses the last five of h = 1).
    err is bitwise the slice of the whole; best / idx are select_ref's on the float64 reference of the slice, best bitwise the row it names."""
    x, T, uv, K, conf = case(J, N, H)
    c = conf if with_conf else None
    lo, hi = 17, N * H - 5
    err = run(zh, x, T, uv, K, c)[0]
    e, b, i = run(zh, x[lo:hi], T[lo:hi], uv, K, c, off=lo)
    assert torch.equal(bits(e), bits(err[lo:hi]))
    rbest, ridx = select_ref(ref(J, N, H, with_conf)[lo:hi], N, lo)
    local = np.full(H * N, np.inf)
    local[lo:hi] = ref(J, N, H, with_conf)[lo:hi]
    s = np.sort(local.reshape(H, N), axis=0)
    assert np.isfinite(s[0]).all() and (s[1] - s[0]).min() > 1e-6                           # every pose is held, and by no near tie
    assert np.array_equal(i.cpu().numpy(), ridx) and (ridx >= 0).all()
    pick = err[i.to(torch.int64) * N + torch.arange(N, device="cuda")]
    assert torch.equal(bits(b), bits(pick)) and np.abs(b.cpu().numpy() - rbest).max() <= TOL
    if H == 2:                                                                              # the poses that the cut leaves one hypothesis
        assert (ridx[:lo] == 1).all() and (ridx[N - 5:] == 0).all()


def test_ties_nan_and_points_behind_the_camera(zh):
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = (a.copy() for a in case(J, N, H))
    x, T = x.reshape(H, N, J, 3), T.reshape(H, N, 3)
    # pose 2: its detections become the projection of hypothesis 1 (by far the best then), hypothesis 3 a bitwise copy of it -> index 1
    X = x[1, 2].astype(np.float64) + T[1, 2].astype(np.float64)
    q = X @ K[2].astype(np.float64).T
    uv[2] = (q[:, :2] / q[:, 2:]).astype(np.float32)
    x[3, 2], T[3, 2] = x[1, 2], T[1, 2]
    # pose 4: NaN coordinates in hypotheses 4 and 2 -> NaN, index 2
    x[4, 4, 7, 0] = np.nan
    x[2, 4, 0, 1] = np.nan
    # pose 6: hypothesis 0 has a joint at depth -1 -> +inf for that row; pose 8: every row so
    x[0, 6, 5, 2] = -1.0 - T[0, 6, 2]
    x[:, 8, 3, 2] = -1.0 - T[:, 8, 2]
    xr, Tr = x.reshape(H * N, J, 3), T.reshape(H * N, 3)
    e_ref = reproj_ref(xr, Tr, uv, K, conf)
    err, best, idx = run(zh, xr, Tr, uv, K, conf)
    e = err.reshape(H, N)
    assert torch.equal(bits(e[1, 2]), bits(e[3, 2])) and float(e[1, 2]) < 1e-2 and float(e[:, 2].min()) == float(e[1, 2])
    assert idx[2].item() == 1 and torch.equal(bits(best[2]), bits(e[1, 2]))
    assert bool(torch.isnan(e[2, 4])) and bool(torch.isnan(e[4, 4])) and int(torch.isnan(err).sum()) == 2
    assert idx[4].item() == 2 and bool(torch.isnan(best[4]))
    assert np.isposinf(e_ref.reshape(H, N)[0, 6]) and bool(torch.isposinf(e[0, 6])) and idx[6].item() != 0 and bool(torch.isfinite(best[6]))
    assert np.isposinf(e_ref.reshape(H, N)[:, 8]).all() and bool(torch.isposinf(e[:, 8]).all())
    assert int(torch.isposinf(err).sum()) == 1 + H
    pb, pi = zh.pose_min(err, N)                                                            # d_err is a valid input of zedo_pose_min
    assert torch.equal(bits(pb), bits(best)) and torch.equal(pi, idx)
    assert bool(torch.isposinf(best[8])) and idx[8].item() == pi[8].item()
    ok = np.isfinite(e_ref)
    assert np.abs(err.cpu().numpy()[ok] - e_ref[ok]).max() <= TOL
    rb, ri = select_ref(e_ref, N)
    assert np.array_equal(idx.cpu().numpy(), ri)


def test_refusals_at_the_raw_abi(zh):
    """A NULL d_err (and every other required pointer), B = 0, N = 0, J = 0 and row_offset = -1: ZEDO_E_BADARG, nothing written; a NULL
    d_conf is accepted."""
    lib = zh._lib
    J, N, H = 17, 3, 4
    B = N * H
    x = torch.full((B, J, 3), 0.25, device="cuda")
    T = torch.tensor([[0.0, 0.0, 5.0]], device="cuda").repeat(B, 1).contiguous()
    uv = torch.full((N, J, 2), 500.0, device="cuda")
    K = torch.tensor([[1100.0, 0, 500], [0, 1100, 500], [0, 0, 1]], device="cuda").repeat(N, 1, 1).contiguous()
    conf = torch.full((N, J), 0.5, device="cuda")
    err, best, bh = sentinels((((B,), torch.float64), ((N,), torch.float64), ((N,), torch.int32)))
    ptrs = [P(x), P(T), P(uv), P(K), P(conf), P(err), P(best), P(bh)]
    call = lambda p, b=B, n=N, j=J, off=0: lib.zedo_min_reproj(p[0], p[1], p[2], p[3], p[4], b, n, j, off, p[5], p[6], p[7], None)
    for k in (5, 0, 1, 2, 3, 6, 7):
        assert call([None if i == k else p for i, p in enumerate(ptrs)]) == -1, k
    assert call(ptrs, b=0) == -1 and call(ptrs, n=0) == -1 and call(ptrs, j=0) == -1 and call(ptrs, off=-1) == -1
    torch.cuda.synchronize()
    assert bool((err == -7.0).all()) and bool((best == -7.0).all()) and bool((bh == -7).all())
    assert call([None if i == 4 else p for i, p in enumerate(ptrs)]) == 0                  # the control: no confidences is legal
    torch.cuda.synchronize()
    assert bool((err >= 0).all()) and bool((best >= 0).all()) and bool((bh >= 0).all())
    with pytest.raises(zh.ZedoError):
        zh.min_reproj(x, T[:-1].contiguous(), uv, K, conf)


def test_the_call_is_capturable(zh):
    """One call captured into a graph on a side stream (a single branch) and replayed reproduces the eager bits: it allocates nothing
    and synchronises nothing of its own."""
    x, T, uv, K, conf = (dev(a) for a in case(17, 70, 5))
    eager = zh.min_reproj(x, T, uv, K, conf)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        zh.min_reproj(x, T, uv, K, conf)                          # warm the allocator on the capture stream
    torch.cuda.synchronize()
    replays_to(eager, lambda: zh.min_reproj(x, T, uv, K, conf), s)


def test_pipeline_select_reproj_and_take(zh, weights0):
    """Pipeline.select_reproj on the problem of load() is min_reproj on its detections, intrinsics and confidences (whole and a shard, an
    empty shard is empty_selection); Pipeline.take picks row idx[n] * N + n of every pose and refuses an index of -1."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    _, best, idx = zh.min_reproj(xd, Td, dev(uv), dev(K), dev(conf))
    sb, si = pipe.select_reproj(xd, Td)
    assert torch.equal(bits(sb), bits(best)) and torch.equal(si, idx)
    lo, hi = 93, 211
    sb, si = pipe.select_reproj(xd[lo:hi].contiguous(), Td[lo:hi].contiguous(), row_offset=lo)
    _, b2, i2 = zh.min_reproj(xd[lo:hi].contiguous(), Td[lo:hi].contiguous(), dev(uv), dev(K), dev(conf), row_offset=lo)
    assert torch.equal(bits(sb), bits(b2)) and torch.equal(si, i2)
    eb, ei = pipe.select_reproj(xd[:0], Td[:0])
    assert bool(torch.isposinf(eb).all()) and bool((ei == -1).all())
    won = pipe.take(xd, idx)
    assert won.shape == (N, J, 3) and np.array_equal(won.cpu().numpy(), x.reshape(H, N, J, 3)[idx.cpu().numpy(), np.arange(N)])
    assert np.array_equal(pipe.take(Td, idx).cpu().numpy(), T.reshape(H, N, 3)[idx.cpu().numpy(), np.arange(N)])
    with pytest.raises(ValueError):
        pipe.take(xd, ei)
