"""GPU: zedo_joint_accel_select - for every joint of every clip the hypothesis path that minimises that joint's cost plus lambda_v times its
displacement plus lambda_a times its second difference X[n] - 2 X[n-1] + X[n-2] in the camera frame: J independent chains over PAIRS of
hypotheses per clip in fp64 (dead, scan, backtrack and cost kernels of csrc/zedo_joint_accel.hip).  Held to the float64 reference of
tests/_joint_accel_ref.py (pinned on its own in tests/test_joint_accel_ref.py): the PATHS exactly, the re-accumulated costs within
8 L 2^-53 relative (asserted; the difference each case shows is printed - the reference replays the same order, so equal bits are the
expectation); check_inputs() asserts on the reference alone that no minimum taken has a runner-up closer than 1e-8.  At lambda_a = 0 the
paths are those of zedo_joint_temporal_select on the GPU.  Bit identity across a dirty workspace, a side stream, stream capture, the
alignment of d_x and seq_start on the device; clips of one and two frames; excluded entries and a dead (frame, joint); the refusals of
the raw ABI; the pipeline's method.
Whether second-order paths are closer to ground truth than the first-order ones is not measured here or anywhere: these tests hold the
arithmetic.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import clamped_offsets, dirty, launch_invariant, ptr as P, refusal_sweep, same, sentinels
from _joint_accel_ref import ALL_CASES, IDS, WEIGHTS, check_inputs, cost_bound, joint_accel_ref, reference
from _joint_ref import case as reproj_case
from _joint_temporal_ref import case, dead_joint_case, per_frame_argmin
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OUT_SPECS = lambda N, J: (((N, J), torch.int32), ((N, J), torch.float64))


def run(zh, x, T, u, seq, lam_v, lam_a):
    return zh.joint_accel_select(dev(u, torch.float64), dev(x), None if T is None else dev(T), seq, lam=lam_v, accel=lam_a)


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs(verbose=False)


@pytest.mark.parametrize("J,N,H,L", ALL_CASES, ids=IDS)
def test_paths_and_costs_match_the_float64_reference(zh, J, N, H, L):
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lam_v, lam_a in WEIGHTS:
        path, cost = zh.joint_accel_select(ud, xd, Td, clips(N, L), lam=lam_v, accel=lam_a)
        assert path.shape == (N, J) and path.dtype == torch.int32 and cost.shape == (N, J) and cost.dtype == torch.float64
        r = reference(J, N, H, L, lam_v, lam_a)
        err = np.abs(cost.cpu().numpy() - r["cost"])
        print(f"joint-accel J={J} N={N} H={H} L={L} lambda_v={lam_v:g} lambda_a={lam_a:g}: max |cost - ref| = {err.max():.3e}, relative "
              f"{(err / r['cost']).max():.3e} (bound {8.0 * L * 2.0 ** -53:.3e}); path differs on "
              f"{int((path.cpu().numpy() != r['path']).sum())} of {N * J}; gap {r['gap']:.3e}")
        assert np.array_equal(path.cpu().numpy(), r["path"]), (lam_v, lam_a)
        assert (err <= cost_bound(L, r["cost"])).all(), (lam_v, lam_a)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (3, 40, 64, 9), (3, 130, 7, 130), (5, 12, 3, 4)], ids=lambda v: str(v))
def test_without_the_second_order_term_the_paths_are_the_first_order_call(zh, J, N, H, L):
    """lambda_a = 0: the chain over pairs minimises what zedo_joint_temporal_select minimises - the same paths on the GPU, with and
    without T; the costs are the same terms associated differently: within 8 L 2^-53 relative."""
    x, T, u = case(J, N, H)
    xd, Td, ud, seq = dev(x), dev(T), dev(u, torch.float64), clips(N, L)
    for Tq, lam in ((Td, 100.0), (None, 30.0)):
        p1, c1 = zh.joint_temporal_select(ud, xd, Tq, seq, lam=lam)
        p2, c2 = zh.joint_accel_select(ud, xd, Tq, seq, lam=lam, accel=0.0)
        assert same(p1, p2)
        c1, c2 = c1.cpu().numpy(), c2.cpu().numpy()
        assert (np.abs(c1 - c2) <= cost_bound(L, c1)).all()


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (3, 40, 64, 9), (1, 20, 17, 20), (2, 300, 3, 300)], ids=lambda v: str(v))
def test_the_bits_do_not_depend_on_the_workspace_the_stream_or_the_alignment(zh, J, N, H, L):
    """A workspace pre-filled with 0xFF bytes at the raw ABI; a side stream with seq_start as a device tensor; one call captured into a
    graph and replayed twice; d_x at a 12-byte offset."""
    x, T, u = case(J, N, H)
    xd, Td, ud, seq = dev(x), dev(T), dev(u, torch.float64), clips(N, L)
    lam_v, lam_a = 30.0, 100.0
    path, cost = zh.joint_accel_select(ud, xd, Td, seq, lam=lam_v, accel=lam_a)
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, lam_v, lam_a)["path"])
    nbytes = zh._lib.zedo_joint_accel_workspace_bytes(N, H, J)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")

    def raw(ws, o, st):
        return zh._lib.zedo_joint_accel_select(P(ud), P(xd), P(Td), P(sd), len(seq) - 1, H, N, J, lam_v, lam_a, P(ws), nbytes, P(o[0]), P(o[1]), st)

    def via_binding(x=xd, seq_on_device=False):
        # under capture N is given: reading it off the device tensor would synchronise
        return zh.joint_accel_select(ud, x, Td, sd if seq_on_device else seq, N=N if torch.cuda.is_current_stream_capturing() else None,
                                     lam=lam_v, accel=lam_a)

    launch_invariant((path, cost), via_binding, xd, raw, OUT_SPECS(N, J), nbytes)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (5, 12, 3, 4), (3, 40, 64, 9)], ids=lambda v: str(v))
def test_the_limits(zh, J, N, H, L):
    """Clips of one frame: the per-frame joint arg-min (ties to the lower hypothesis) and its unary, bit for bit, at any weights.  Clips
    of two frames have no second difference: the path of the first-order call, whatever lambda_a; at lambda_v = 0 that is the per-frame
    joint arg-min again.  lambda_v = lambda_a = 0 at the case's own clips: the per-frame joint arg-min."""
    x, T, u = case(J, N, H)
    idx = per_frame_argmin(u, N)
    best = u.reshape(H, N, J).min(0)
    for lam_v, lam_a in ((0.0, 0.0), (30.0, 100.0), (0.0, 1e6)):
        path, cost = run(zh, x, T, u, clips(N, 1), lam_v, lam_a)
        assert np.array_equal(path.cpu().numpy(), idx) and np.array_equal(cost.cpu().numpy().view(np.int64), best.view(np.int64))
    path, _ = run(zh, x, T, u, clips(N, 2), 0.0, 1e6)
    assert np.array_equal(path.cpu().numpy(), idx)
    path, _ = run(zh, x, T, u, clips(N, 2), 30.0, 1e6)
    first, _ = zh.joint_temporal_select(dev(u, torch.float64), dev(x), dev(T), clips(N, 2), lam=30.0)
    assert same(path, first)
    path, _ = run(zh, x, T, u, clips(N, L), 0.0, 0.0)
    assert np.array_equal(path.cpu().numpy(), idx)


def test_excluded_entries_and_a_dead_frame_joint(zh):
    """The hand-built case of tests/test_joint_accel_ref.py (NaN, +inf and -inf unaries of ONE joint; (frame 4, joint 2) without a finite
    one): the reference's paths and costs, the dead entry reports hypothesis 0 and +inf and splits that joint's chain only - the other
    joints return the bits of the untouched unaries; with (frame 1, joint 2) dead as well that joint has chains of one and of two frames;
    and a larger case with dead entries at a clip boundary."""
    x, T, u, j = dead_joint_case()
    clean = case(5, 9, 3)[2]
    u3 = u.reshape(3, 9, 5)
    for lam_v, lam_a in ((0.0, 100.0), (30.0, 100.0)):
        r = joint_accel_ref(u, x, T, [0, 9], lam_v, lam_a)
        path, cost = run(zh, x, T, u, [0, 9], lam_v, lam_a)
        p0, c0 = run(zh, x, T, clean, [0, 9], lam_v, lam_a)
        others = [i for i in range(5) if i != j]
        assert same(path[:, others], p0[:, others]) and same(cost[:, others], c0[:, others])
        assert np.array_equal(path.cpu().numpy(), r["path"]) and path[4, j].item() == 0
        c = cost.cpu().numpy()
        assert np.isposinf(c[4, j]) and np.isposinf(r["cost"][4, j])
        ok = np.isfinite(r["cost"])
        assert ok.sum() == 44 and (np.abs(c[ok] - r["cost"][ok]) <= cost_bound(9, r["cost"][ok])).all()
        live = np.arange(9) != 4
        assert np.isfinite(u3[path.cpu().numpy()[live, j], np.arange(9)[live], j]).all()      # an excluded entry is never on the path
        v = u3.copy()
        v[:, 1, j] = np.nan                                          # joint j: chains [0, 1), [2, 4) and [5, 9)
        v = v.reshape(27, 5)
        r = joint_accel_ref(v, x, T, [0, 9], lam_v, lam_a)
        path, cost = run(zh, x, T, v, [0, 9], lam_v, lam_a)
        c, ok = cost.cpu().numpy(), np.isfinite(r["cost"])
        assert np.array_equal(path.cpu().numpy(), r["path"]) and ok.sum() == 43 and np.isposinf(c[~ok]).all()
        assert (np.abs(c[ok] - r["cost"][ok]) <= cost_bound(9, r["cost"][ok])).all()
        assert same(path[:, others], p0[:, others]) and same(cost[:, others], c0[:, others])
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    u = u.reshape(H, N, J).copy()
    u[:, 20, 3] = np.nan
    u[:, 34, 5] = np.inf                                             # the last frame of the first clip
    u[:, 35, 5] = -np.inf                                            # the first frame of the second
    u[:, 0, 16] = np.nan                                             # the first frame of all
    u[:, 69, 0] = np.inf                                             # the last
    u[:, 22, 3] = np.nan                                             # (21, 3) is a chain of one frame
    u[:, 67, 0] = np.inf                                             # (68, 0) as well, at the end of the clip
    u[7, 50, :] = np.nan
    u = u.reshape(H * N, J)
    r = joint_accel_ref(u, x, T, clips(N, L), 30.0, 100.0)
    assert r["gap"] > 1e-8
    path, cost = run(zh, x, T, u, clips(N, L), 30.0, 100.0)
    assert np.array_equal(path.cpu().numpy(), r["path"])
    c, dead = cost.cpu().numpy(), np.zeros((N, J), bool)
    for n, jj in ((20, 3), (34, 5), (35, 5), (0, 16), (69, 0), (22, 3), (67, 0)):
        dead[n, jj] = True
    assert np.isposinf(c[dead]).all() and (path.cpu().numpy()[dead] == 0).all() and np.isfinite(c[~dead]).all()
    assert (np.abs(c[~dead] - r["cost"][~dead]) <= cost_bound(L, r["cost"][~dead])).all()


def test_clip_offsets_that_break_the_rules_are_clamped(zh):
    """Offsets outside 0 .. N are clamped and never become addresses: [0, N + 1000] and [-5, N] are the one clip [0, N]."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    clamped_offsets(lambda seq: zh.joint_accel_select(ud, xd, Td, seq, N=N, lam=30.0, accel=100.0), N)


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer other than d_T, non-positive size, H > 64, n_seq > N, N J H above INT_MAX, a negative / NaN / infinite lambda_v
    or lambda_a and a misaligned workspace: ZEDO_E_BADARG; a workspace one byte short: ZEDO_E_WORKSPACE; nothing written either way.
    The same call with valid arguments is accepted, with and without d_T, and H = 64 is."""
    lib = zh._lib
    J, N, H, L = 5, 12, 3, 4
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    seq = clips(N, L)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")
    need = lib.zedo_joint_accel_workspace_bytes(N, H, J)
    assert need == N * J * H * H + N * J * 8                         # back2 (540 bytes: a multiple of 4) and two int32 flags
    assert lib.zedo_joint_accel_workspace_bytes(3, 3, 1) == 28 + 3 * 8                                           # 27 rounded up to 4
    assert lib.zedo_joint_accel_workspace_bytes(1015, 50, 17) == 1015 * 17 * 2500 + 1015 * 17 * 8              # 43 MB
    assert lib.zedo_joint_accel_workspace_bytes(70880, 50, 17) == 70880 * 17 * 2500 + 70880 * 17 * 8           # 3.0 GB: past 2^31
    assert lib.zedo_joint_accel_workspace_bytes(1, 64, 1) > 0
    for n, h, j in ((0, H, J), (N, 0, J), (N, H, 0), (-1, H, J), (N, 65, J), (N, 1024, J), (2 ** 20, 2 ** 6, 2 ** 5), (2 ** 30, 1, 2)):
        assert lib.zedo_joint_accel_workspace_bytes(n, h, j) == 0, (n, h, j)
    ws = dirty(need + 8, 0x5A)
    path, cost = sentinels(OUT_SPECS(N, J))
    ptrs = [P(ud), P(xd), P(Td), P(sd), P(ws), P(path), P(cost)]

    def call(p=ptrs, n_seq=len(seq) - 1, h=H, n=N, j=J, lam_v=30.0, lam_a=100.0, nbytes=need):
        return lib.zedo_joint_accel_select(p[0], p[1], p[2], p[3], n_seq, h, n, j, lam_v, lam_a, p[4], nbytes, p[5], p[6], None)

    sizes = [dict(n_seq=0), dict(n_seq=N + 1), dict(h=0), dict(n=0), dict(j=0), dict(h=-1), dict(n=-3), dict(j=-1), dict(h=65, nbytes=2 ** 40),
             dict(h=2 ** 6, n=2 ** 20, j=2 ** 5, nbytes=2 ** 40), dict(h=1, n=2 ** 30, j=2, nbytes=2 ** 40)]
    refusal_sweep(call, ptrs, (0, 1, 3, 4, 5, 6), sizes=sizes, weights=("lam_a", "lam_v"), workspace_slot=4, need=need,
                  untouched=((path, -7), (cost, -7.0), (ws, 0x5A)))
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, 30.0, 100.0)["path"]) and bool((ws[need:] == 0x5A).all())
    assert call([None if i == 2 else p for i, p in enumerate(ptrs)]) == 0          # d_T may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, 30.0, 100.0, False)["path"])
    with pytest.raises(ValueError):
        zh.joint_accel_select(ud[:-1], xd, Td, seq)
    with pytest.raises(ValueError):
        zh.joint_accel_select(ud, xd, Td[:-1], seq)
    with pytest.raises(zh.ZedoError):
        zh.joint_accel_select(torch.zeros((65, 1), dtype=torch.float64, device="cuda"), torch.zeros((65, 1, 3), device="cuda"), None, [0, 1])


def test_pipeline_select_joints_accel(zh, weights0):
    """Pipeline.select_joints_accel on the problem of load() is joint_reproj's per-(row, joint) distances fed to joint_accel_select;
    compose() assembles the pose from the paths."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)[2]
    for lam, accel, seq in ((100.0, 100.0, [0, 35, N]), (0.0, 300.0, [0, N])):
        path, cost = zh.joint_accel_select(jerr, xd, Td, seq, lam=lam, accel=accel)
        p, k, e = pipe.select_joints_accel(xd, Td, seq, lam=lam, accel=accel)
        assert same(p, path) and same(k, cost) and same(e, jerr)
    assert same(pipe.compose(xd, Td, p), zh.joint_compose(xd, Td, path))
    with pytest.raises(ValueError):
        pipe.select_joints_accel(xd[:N], Td[:N], [0, N])
