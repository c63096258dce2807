"""GPU: zedo_temporal_select - the hypothesis sequence along the clips of a video that minimises a per-row cost plus lambda times the
mean joint displacement between consecutive choices (Viterbi in fp64: transition, scan and backtrack kernels).  Held to the float64
reference of tests/_temporal_ref.py (pinned on its own in tests/test_temporal_ref.py): the PATH exactly, the cost within
4 L (J + 4) 2^-53 relative.  That bound is under 1e-8 at the largest case, and check_inputs() asserts on the reference alone that no
minimum the recurrence takes has a runner-up closer than 1e-6: an exact comparison of paths cannot hide behind a near tie.
Bit identity across chunk sizes, a dirty workspace, stream capture, a side stream and the alignment of d_x; unaries from
zedo_min_reproj; the limits (lambda = 0, clips of one frame); excluded rows and dead frames; the refusals of the raw ABI.
Whether the temporal path is closer to ground truth than the per-frame arg-min is not measured here or anywhere: these tests hold the
arithmetic, not the criterion's accuracy.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import clamped_offsets, dirty, launch_invariant, misaligned, ptr as P, refusal_sweep, same, sentinels
from _joint_ref import case as reproj_case
from _select_ref import reproj_ref, select_ref
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_ref import (ALL_CASES, IDS, LAMBDAS, case, check_inputs, clips, cost_bound, dead_frame_case, reference,
                           temporal_ref)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OUT_SPECS = lambda N: (((N,), torch.int32), ((N,), torch.float64))


def run(zh, x, u, seq, lam, chunk=0):
    return zh.temporal_select(dev(u, torch.float64), dev(x), seq, lam=lam, chunk_frames=chunk)


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs()


@pytest.mark.parametrize("J,N,H,L", ALL_CASES, ids=IDS)
def test_path_and_cost_match_the_float64_reference(zh, J, N, H, L):
    x, u = case(J, N, H)
    worst = 0.0
    for lam in LAMBDAS:
        path, cost = run(zh, x, u, clips(N, L), lam)
        assert path.shape == (N,) and path.dtype == torch.int32 and cost.shape == (N,) and cost.dtype == torch.float64
        r = reference(J, N, H, L, lam)
        err = np.abs(cost.cpu().numpy() - r["cost"])
        worst = max(worst, float((err / r["cost"]).max()))
        print(f"temporal J={J} N={N} H={H} L={L} lambda={lam:g}: max |cost - ref| = {err.max():.3e} ({(err / r['cost']).max():.3e} relative, "
              f"bound {4.0 * L * (J + 4) * 2.0 ** -53:.3e}); path differs on {int((path.cpu().numpy() != r['path']).sum())} of {N} frames")
        assert np.array_equal(path.cpu().numpy(), r["path"]), lam
        assert (err <= cost_bound(J, L, r["cost"])).all(), lam
    print(f"worst relative cost error over the three lambdas: {worst:.3e}")


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (17, 130, 130, 50), (21, 40, 65, 40), (17, 300, 7, 300), (33, 9, 5, 9), (17, 40, 300, 13)],
                         ids=lambda v: str(v))
def test_the_bits_do_not_depend_on_the_chunk_the_workspace_or_the_stream(zh, J, N, H, L):
    """Chunks of 1, 2 and 7 frames (forced through the workspace size) against the default (all N frames); a workspace pre-filled with
    NaN bytes at the raw ABI; a side stream; one call captured into a graph and replayed twice.  (33, 9, 5, 9): the accumulators of the
    transition kernel carried over a second joint piece; (17, 40, 300, 13): two h per lane of the resident scan, whose first frame of
    every chunk fetches D[n-1,.] from the table."""
    x, u = case(J, N, H)
    xd, ud, seq = dev(x), dev(u, torch.float64), clips(N, L)
    lam = 100.0
    path, cost = zh.temporal_select(ud, xd, seq, lam=lam)
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, lam)["path"])
    for c in (1, 2, 7):
        assert zh._lib.zedo_temporal_workspace_bytes(N, H, c) < zh._lib.zedo_temporal_workspace_bytes(N, H, 0)
        p, k = zh.temporal_select(ud, xd, seq, lam=lam, chunk_frames=c)
        assert same(p, path) and same(k, cost), c
    nbytes = zh._lib.zedo_temporal_workspace_bytes(N, H, 3)         # the raw call: a workspace sized for chunks of 3 frames
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")

    def raw(ws, o, st):
        return zh._lib.zedo_temporal_select(P(ud), P(xd), P(sd), len(seq) - 1, H, N, J, lam, P(ws), nbytes, P(o[0]), P(o[1]), st)

    def via_binding(x=xd, seq_on_device=False):
        # under capture N is given: reading it off the device tensor would synchronise
        return zh.temporal_select(ud, x, sd if seq_on_device else seq, N=N if torch.cuda.is_current_stream_capturing() else None, lam=lam,
                                  chunk_frames=7)

    launch_invariant((path, cost), via_binding, xd, raw, OUT_SPECS(N), nbytes)


def test_an_unaligned_pose_tensor_gives_the_same_bits(zh):
    J, N, H, L = 17, 70, 50, 35
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    path, cost = zh.temporal_select(ud, xd, clips(N, L), lam=100.0)
    xb = misaligned(xd, floats=51)
    p, k = zh.temporal_select(ud, xb, clips(N, L), lam=100.0)
    assert same(p, path) and same(k, cost)


def test_unaries_from_min_reproj(zh):
    """The intended use: the unaries are zedo_min_reproj's per-row errors.  The reference is fed reproj_ref's float64 errors, which the
    kernel's differ from by at most 1e-9 px (tests/test_select_reproj_gpu.py): the reference's smallest gap must stay above 1e-6 for
    the exact comparison of paths, and a cost may differ by L times 1e-9 more than the bound of the recurrence."""
    J, N, H, L = 17, 70, 5, 35
    x, T, uv, K, conf = reproj_case(J, N, H)
    xd = dev(x)
    err, best, idx = zh.min_reproj(xd, dev(T), dev(uv), dev(K), dev(conf))
    u_ref = reproj_ref(x, T, uv, K, conf)
    assert np.abs(err.cpu().numpy() - u_ref).max() <= 1e-9
    for lam in LAMBDAS:
        r = temporal_ref(u_ref, x, clips(N, L), lam)
        assert r["gap"] > 1e-6
        path, cost = zh.temporal_select(err, xd, clips(N, L), lam=lam)
        d = np.abs(cost.cpu().numpy() - r["cost"])
        print(f"unaries of zedo_min_reproj, lambda={lam:g}: max |cost - ref| = {d.max():.3e}; gap {r['gap']:.3e}")
        assert np.array_equal(path.cpu().numpy(), r["path"])
        assert (d <= cost_bound(J, L, r["cost"]) + L * 1e-9).all()
    # lambda = 0: the per-frame selection of the same call
    path, cost = zh.temporal_select(err, xd, clips(N, L), lam=0.0)
    assert torch.equal(path, idx)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (5, 12, 3, 4), (17, 130, 130, 50)], ids=lambda v: str(v))
def test_the_limits(zh, J, N, H, L):
    """lambda = 0: the per-frame arg-min (ties to the lower hypothesis).  Clips of one frame: the per-frame arg-min and its unary,
    bit for bit, at any lambda."""
    x, u = case(J, N, H)
    best, idx = select_ref(u, N)
    path, _ = run(zh, x, u, clips(N, L), 0.0)
    assert np.array_equal(path.cpu().numpy(), idx)
    for lam in (0.0, 100.0, 1e6):
        path, cost = run(zh, x, u, clips(N, 1), lam)
        assert np.array_equal(path.cpu().numpy(), idx) and np.array_equal(cost.cpu().numpy().view(np.int64), best.view(np.int64))


def test_excluded_rows_and_dead_frames(zh):
    """The hand-built case of tests/test_temporal_ref.py (NaN, +inf and -inf unaries; frame 4 without a finite one): the reference's
    path and cost; the dead frame reports hypothesis 0 and +inf and splits the chain; and a larger case with a dead frame in the
    middle of a clip that spans two chunks."""
    x, u = dead_frame_case()
    for lam in (0.0, 100.0):
        r = temporal_ref(u, x, [0, 9], lam)
        for chunk in (0, 1, 2):
            path, cost = run(zh, x, u, [0, 9], lam, chunk)
            assert np.array_equal(path.cpu().numpy(), r["path"]) and path[4].item() == 0
            c = cost.cpu().numpy()
            assert np.isposinf(c[4]) and np.isposinf(r["cost"][4])
            ok = np.arange(9) != 4
            assert (np.abs(c[ok] - r["cost"][ok]) <= cost_bound(5, 9, r["cost"][ok])).all()
    J, N, H, L = 17, 70, 50, 35
    x, u = case(J, N, H)
    u = u.reshape(H, N).copy()
    u[:, 20] = np.nan
    u[:, 34] = np.inf                                                # the last frame of the first clip
    u[:, 35] = -np.inf                                               # the first frame of the second
    u[7, 50] = np.nan
    u = u.reshape(-1)
    r = temporal_ref(u, x, clips(N, L), 100.0)
    assert r["gap"] > 1e-6
    for chunk in (0, 3):
        path, cost = run(zh, x, u, clips(N, L), 100.0, chunk)
        assert np.array_equal(path.cpu().numpy(), r["path"])
        c, dead = cost.cpu().numpy(), np.isin(np.arange(N), (20, 34, 35))
        assert np.isposinf(c[dead]).all() and (path.cpu().numpy()[dead] == 0).all()
        assert (np.abs(c[~dead] - r["cost"][~dead]) <= cost_bound(J, L, r["cost"][~dead])).all()


def test_clip_offsets_that_break_the_rules_are_clamped(zh):
    """The call cannot validate a device array: offsets outside 0 .. N are clamped and never become addresses.  [0, N + 1000] and
    [-5, N] are then the one clip [0, N]; the result of other broken arrays is unspecified and not looked at here."""
    J, N, H = 17, 70, 50
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    clamped_offsets(lambda seq: zh.temporal_select(ud, xd, seq, N=N, lam=100.0), N)


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer, non-positive size, n_seq > N, a negative / NaN / infinite lambda, a misaligned workspace and H*N or H*H above
    INT_MAX: ZEDO_E_BADARG; a workspace one byte short of one frame of transitions: ZEDO_E_WORKSPACE; nothing written either way.  The
    same call with valid arguments is accepted."""
    lib = zh._lib
    J, N, H, L = 5, 12, 3, 4
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    seq = clips(N, L)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")
    one = lib.zedo_temporal_workspace_bytes(N, H, 1)
    assert one == N * H * 8 + (N * H + 2 * N) * 4 + H * H * 8
    assert lib.zedo_temporal_workspace_bytes(N, H, 5) == one + 4 * H * H * 8
    assert lib.zedo_temporal_workspace_bytes(N, H, 0) == lib.zedo_temporal_workspace_bytes(N, H, N) == lib.zedo_temporal_workspace_bytes(N, H, N + 9)
    assert lib.zedo_temporal_workspace_bytes(70880, 50, 0) - lib.zedo_temporal_workspace_bytes(70880, 50, 1) + 50 * 50 * 8 <= 256 << 20
    assert lib.zedo_temporal_workspace_bytes(0, H, 0) == 0 and lib.zedo_temporal_workspace_bytes(N, 2 ** 16, 0) == 0
    ws = dirty(one + 8, 0x5A)
    path, cost = sentinels(OUT_SPECS(N))
    ptrs = [P(ud), P(xd), P(sd), P(ws), P(path), P(cost)]

    def call(p=ptrs, n_seq=len(seq) - 1, h=H, n=N, j=J, lam=100.0, nbytes=one):
        return lib.zedo_temporal_select(p[0], p[1], p[2], n_seq, h, n, j, lam, p[3], nbytes, p[4], p[5], None)

    sizes = [dict(n_seq=0), dict(n_seq=N + 1), dict(h=0), dict(n=0), dict(j=0), dict(h=2 ** 16, n=2 ** 16), dict(h=46341, n=1, n_seq=1)]
    refusal_sweep(call, ptrs, range(6), sizes=sizes, weights=("lam",), workspace_slot=3, need=one,
                  untouched=((path, -7), (cost, -7.0), (ws, 0x5A)))
    r = reference(J, N, H, L, 100.0)
    assert np.array_equal(path.cpu().numpy(), r["path"]) and bool((ws[one:] == 0x5A).all())
    with pytest.raises(ValueError):
        zh.temporal_select(ud[:-1], xd, seq)


def test_pipeline_select_temporal(zh, weights0):
    """Pipeline.select_temporal on the problem of load() is min_reproj's per-row errors fed to temporal_select; take() gathers the rows."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    err = zh.min_reproj(xd, Td, dev(uv), dev(K), dev(conf))[0]
    for lam, seq in ((100.0, [0, 35, N]), (30.0, [0, N])):
        path, cost = zh.temporal_select(err, xd, seq, lam=lam)
        p, k, e = pipe.select_temporal(xd, Td, seq, lam=lam)
        assert same(p, path) and same(k, cost) and same(e, err)
    assert torch.equal(pipe.take(xd, p), xd.view(H, N, J, 3)[p.long(), torch.arange(N, device="cuda")])
    with pytest.raises(ValueError):
        pipe.select_temporal(xd[:N], Td[:N], [0, N])
