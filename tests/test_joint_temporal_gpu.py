"""GPU: zedo_joint_temporal_select - for every joint of every clip the hypothesis path that minimises that joint's cost plus lambda times
that joint's displacement in the camera frame (x + T) between consecutive choices: J independent Viterbi chains per clip in fp64, the
transition costs computed inside the recurrence (dead, scan and backtrack kernels of csrc/zedo_joint_temporal.hip).  Held to the float64
reference of tests/_joint_temporal_ref.py (pinned on its own in tests/test_joint_temporal_ref.py): the PATHS exactly, the costs within
_temporal_ref.cost_bound(1, L, .) = 20 L 2^-53 relative (asserted; the difference each case shows is printed); check_inputs() asserts
on the reference alone that no minimum the recurrence takes has a runner-up closer than 1e-6.  Without T the call is held, bit for bit, to J calls of zedo_temporal_select on one-joint
slices.  Bit identity across a dirty workspace, a side stream, stream capture, the alignment of d_x and seq_start on the device; unaries
from zedo_joint_reproj; the limits (lambda = 0, clips of one frame); excluded entries and a dead (frame, joint); the refusals of the raw
ABI.
Whether joint-wise temporal paths are closer to ground truth than the per-frame joint-wise arg-min is not measured here or anywhere:
these tests hold the arithmetic.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import clamped_offsets, dirty, launch_invariant, ptr as P, refusal_sweep, same, sentinels
from _joint_ref import case as reproj_case
from _joint_ref import joint_reproj_ref
from _joint_temporal_ref import (ALL_CASES, IDS, LAMBDAS, case, check_inputs, dead_joint_case, joint_temporal_ref, per_frame_argmin,
                                 reference)
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_ref import clips, cost_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OUT_SPECS = lambda N, J: (((N, J), torch.int32), ((N, J), torch.float64))


def run(zh, x, T, u, seq, lam):
    return zh.joint_temporal_select(dev(u, torch.float64), dev(x), None if T is None else dev(T), seq, lam=lam)


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs()


@pytest.mark.parametrize("J,N,H,L", ALL_CASES, ids=IDS)
def test_paths_and_costs_match_the_float64_reference(zh, J, N, H, L):
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lam in LAMBDAS:
        path, cost = zh.joint_temporal_select(ud, xd, Td, clips(N, L), lam=lam)
        assert path.shape == (N, J) and path.dtype == torch.int32 and cost.shape == (N, J) and cost.dtype == torch.float64
        r = reference(J, N, H, L, lam)
        err = np.abs(cost.cpu().numpy() - r["cost"])
        print(f"joint-temporal J={J} N={N} H={H} L={L} lambda={lam:g}: max |cost - ref| = {err.max():.3e} (largest bound "
              f"{cost_bound(1, L, r['cost']).max():.3e}), relative {(err / r['cost']).max():.3e} (relative bound {4.0 * L * 5 * 2.0 ** -53:.3e}); "
              f"path differs on {int((path.cpu().numpy() != r['path']).sum())} of {N * J}")
        assert np.array_equal(path.cpu().numpy(), r["path"]), lam
        assert (err <= cost_bound(1, L, r["cost"])).all(), lam


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (21, 20, 65, 20), (2, 30, 130, 13)], ids=lambda v: str(v))
def test_without_T_every_joint_is_the_pose_level_call_on_its_slice(zh, J, N, H, L):
    """d_T = NULL: path and cost are, bit for bit, those of J calls of zedo_temporal_select on unary = junary[:, j] and
    x = x[:, j:j+1, :] - the same statements on the same operands, and the division by J = 1 is exact."""
    x, T, u = case(J, N, H)
    xd, ud, seq = dev(x), dev(u, torch.float64), clips(N, L)
    for lam in (30.0, 100.0):
        path, cost = zh.joint_temporal_select(ud, xd, None, seq, lam=lam)
        assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, lam, False)["path"])
        for j in range(J):
            p, k = zh.temporal_select(ud[:, j].contiguous(), xd[:, j:j + 1, :].contiguous(), seq, lam=lam)
            assert same(p, path[:, j].contiguous()) and same(k, cost[:, j].contiguous()), (lam, j)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (2, 30, 130, 13), (1, 6, 300, 3), (2, 300, 3, 300)], ids=lambda v: str(v))
def test_the_bits_do_not_depend_on_the_workspace_the_stream_or_the_alignment(zh, J, N, H, L):
    """A workspace pre-filled with 0xFF bytes at the raw ABI; a side stream with seq_start as a device tensor; one call captured into a
    graph and replayed twice; d_x at a 12-byte offset."""
    x, T, u = case(J, N, H)
    xd, Td, ud, seq = dev(x), dev(T), dev(u, torch.float64), clips(N, L)
    lam = 100.0
    path, cost = zh.joint_temporal_select(ud, xd, Td, seq, lam=lam)
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, lam)["path"])
    nbytes = zh._lib.zedo_joint_temporal_workspace_bytes(N, H, J)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")

    def raw(ws, o, st):
        return zh._lib.zedo_joint_temporal_select(P(ud), P(xd), P(Td), P(sd), len(seq) - 1, H, N, J, lam, P(ws), nbytes, P(o[0]), P(o[1]), st)

    def via_binding(x=xd, seq_on_device=False):
        # under capture N is given: reading it off the device tensor would synchronise
        return zh.joint_temporal_select(ud, x, Td, sd if seq_on_device else seq, N=N if torch.cuda.is_current_stream_capturing() else None, lam=lam)

    launch_invariant((path, cost), via_binding, xd, raw, OUT_SPECS(N, J), nbytes)


def test_unaries_from_joint_reproj(zh):
    """The intended use: the unaries are zedo_joint_reproj's per-(row, joint) distances.  The reference is fed joint_reproj_ref's float64
    distances, which the kernel's differ from by at most 1e-9 px (asserted here): the reference's smallest gap must stay above 1e-6 for
    the exact comparison of paths, and a cost may differ by L times 1e-9 more than the bound of the recurrence."""
    J, N, H, L = 17, 70, 5, 35
    x, T, uv, K, _ = reproj_case(J, N, H)
    xd, Td = dev(x), dev(T)
    best, idx, jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)
    u_ref = joint_reproj_ref(x, T, uv, K)
    assert np.abs(jerr.cpu().numpy() - u_ref).max() <= 1e-9
    for lam in LAMBDAS:
        r = joint_temporal_ref(u_ref, x, T, clips(N, L), lam)
        assert r["gap"] > 1e-6
        path, cost = zh.joint_temporal_select(jerr, xd, Td, clips(N, L), lam=lam)
        d = np.abs(cost.cpu().numpy() - r["cost"])
        print(f"unaries of zedo_joint_reproj, lambda={lam:g}: max |cost - ref| = {d.max():.3e}; gap {r['gap']:.3e}")
        assert np.array_equal(path.cpu().numpy(), r["path"])
        assert (d <= cost_bound(1, L, r["cost"]) + L * 1e-9).all()
    # lambda = 0: the per-frame joint-wise selection of the same call
    path, _ = zh.joint_temporal_select(jerr, xd, Td, clips(N, L), lam=0.0)
    assert torch.equal(path, idx)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (5, 12, 3, 4), (2, 30, 130, 13), (1, 6, 300, 3)], ids=lambda v: str(v))
def test_the_limits(zh, J, N, H, L):
    """lambda = 0: the per-frame joint-wise arg-min (ties to the lower hypothesis).  Clips of one frame: the lowest finite arg-min and its
    unary, bit for bit, at any lambda."""
    x, T, u = case(J, N, H)
    idx = per_frame_argmin(u, N)
    best = u.reshape(H, N, J).min(0)
    path, _ = run(zh, x, T, u, clips(N, L), 0.0)
    assert np.array_equal(path.cpu().numpy(), idx)
    for lam in (0.0, 100.0, 1e6):
        path, cost = run(zh, x, T, u, clips(N, 1), lam)
        assert np.array_equal(path.cpu().numpy(), idx) and np.array_equal(cost.cpu().numpy().view(np.int64), best.view(np.int64))


def test_excluded_entries_and_a_dead_frame_joint(zh):
    """The hand-built case of tests/test_joint_temporal_ref.py (NaN, +inf and -inf unaries of ONE joint; (frame 4, joint 2) without a
    finite one): the reference's paths and costs, the dead entry reports hypothesis 0 and +inf and splits that joint's chain only - the
    other joints return the bits of the untouched unaries; and a larger case with dead entries at a clip boundary."""
    x, T, u, j = dead_joint_case()
    clean = case(5, 9, 3)[2]
    for lam in (0.0, 100.0):
        r = joint_temporal_ref(u, x, T, [0, 9], lam)
        path, cost = run(zh, x, T, u, [0, 9], lam)
        p0, c0 = run(zh, x, T, clean, [0, 9], lam)
        others = [i for i in range(5) if i != j]
        assert same(path[:, others], p0[:, others]) and same(cost[:, others], c0[:, others])
        assert np.array_equal(path.cpu().numpy(), r["path"]) and path[4, j].item() == 0
        c = cost.cpu().numpy()
        assert np.isposinf(c[4, j]) and np.isposinf(r["cost"][4, j])
        ok = np.isfinite(r["cost"])
        assert ok.sum() == 44 and (np.abs(c[ok] - r["cost"][ok]) <= cost_bound(1, 9, r["cost"][ok])).all()
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    u = u.reshape(H, N, J).copy()
    u[:, 20, 3] = np.nan
    u[:, 34, 5] = np.inf                                             # the last frame of the first clip
    u[:, 35, 5] = -np.inf                                            # the first frame of the second
    u[:, 0, 16] = np.nan                                             # the first frame of all
    u[:, 69, 0] = np.inf                                             # the last
    u[7, 50, :] = np.nan
    u = u.reshape(H * N, J)
    r = joint_temporal_ref(u, x, T, clips(N, L), 100.0)
    assert r["gap"] > 1e-6
    path, cost = run(zh, x, T, u, clips(N, L), 100.0)
    assert np.array_equal(path.cpu().numpy(), r["path"])
    c, dead = cost.cpu().numpy(), np.zeros((N, J), bool)
    for n, jj in ((20, 3), (34, 5), (35, 5), (0, 16), (69, 0)):
        dead[n, jj] = True
    assert np.isposinf(c[dead]).all() and (path.cpu().numpy()[dead] == 0).all() and np.isfinite(c[~dead]).all()
    assert (np.abs(c[~dead] - r["cost"][~dead]) <= cost_bound(1, L, r["cost"][~dead])).all()


def test_clip_offsets_that_break_the_rules_are_clamped(zh):
    """Offsets outside 0 .. N are clamped and never become addresses: [0, N + 1000] and [-5, N] are the one clip [0, N]."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    clamped_offsets(lambda seq: zh.joint_temporal_select(ud, xd, Td, seq, N=N, lam=100.0), N)


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer other than d_T, non-positive size, H > 1024, n_seq > N, N J H above INT_MAX, a negative / NaN / infinite lambda
    and a misaligned workspace: ZEDO_E_BADARG; a workspace one byte short: ZEDO_E_WORKSPACE; nothing written either way.  The same call
    with valid arguments is accepted, with and without d_T."""
    lib = zh._lib
    J, N, H, L = 5, 12, 3, 4
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    seq = clips(N, L)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")
    need = lib.zedo_joint_temporal_workspace_bytes(N, H, J)
    assert need == N * J * H * 8 + (N * J * H + 2 * N * J) * 4
    assert lib.zedo_joint_temporal_workspace_bytes(3, 3, 1) == 3 * 3 * 8 + ((3 * 3 + 6) * 4 + 7) // 8 * 8       # padded to 8 bytes
    assert lib.zedo_joint_temporal_workspace_bytes(1, 1024, 1) > 0
    for n, h, j in ((0, H, J), (N, 0, J), (N, H, 0), (-1, H, J), (N, 1025, J), (2 ** 16, 2 ** 10, 2 ** 5), (2 ** 30, 1, 2)):
        assert lib.zedo_joint_temporal_workspace_bytes(n, h, j) == 0, (n, h, j)
    ws = dirty(need + 8, 0x5A)
    path, cost = sentinels(OUT_SPECS(N, J))
    ptrs = [P(ud), P(xd), P(Td), P(sd), P(ws), P(path), P(cost)]

    def call(p=ptrs, n_seq=len(seq) - 1, h=H, n=N, j=J, lam=100.0, nbytes=need):
        return lib.zedo_joint_temporal_select(p[0], p[1], p[2], p[3], n_seq, h, n, j, lam, p[4], nbytes, p[5], p[6], None)

    sizes = [dict(n_seq=0), dict(n_seq=N + 1), dict(h=0), dict(n=0), dict(j=0), dict(h=-1), dict(n=-3), dict(j=-1), dict(h=1025, nbytes=2 ** 40),
             dict(h=2 ** 10, n=2 ** 16, j=2 ** 5, nbytes=2 ** 40), dict(h=1, n=2 ** 30, j=2, nbytes=2 ** 40)]
    refusal_sweep(call, ptrs, (0, 1, 3, 4, 5, 6), sizes=sizes, weights=("lam",), workspace_slot=4, need=need,
                  untouched=((path, -7), (cost, -7.0), (ws, 0x5A)))
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, 100.0)["path"]) and bool((ws[need:] == 0x5A).all())
    assert call([None if i == 2 else p for i, p in enumerate(ptrs)]) == 0          # d_T may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, 100.0, False)["path"])
    with pytest.raises(ValueError):
        zh.joint_temporal_select(ud[:-1], xd, Td, seq)
    with pytest.raises(ValueError):
        zh.joint_temporal_select(ud, xd, Td[:-1], seq)
    with pytest.raises(zh.ZedoError):
        zh.joint_temporal_select(torch.zeros((1025, 1), dtype=torch.float64, device="cuda"), torch.zeros((1025, 1, 3), device="cuda"), None, [0, 1])


def test_pipeline_select_joints_temporal(zh, weights0):
    """Pipeline.select_joints_temporal on the problem of load() is joint_reproj's per-(row, joint) distances fed to joint_temporal_select;
    compose() assembles the pose from the paths."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)[2]
    for lam, seq in ((100.0, [0, 35, N]), (30.0, [0, N])):
        path, cost = zh.joint_temporal_select(jerr, xd, Td, seq, lam=lam)
        p, k, e = pipe.select_joints_temporal(xd, Td, seq, lam=lam)
        assert same(p, path) and same(k, cost) and same(e, jerr)
    assert same(pipe.compose(xd, Td, p), zh.joint_compose(xd, Td, path))
    with pytest.raises(ValueError):
        pipe.select_joints_temporal(xd[:N], Td[:N], [0, N])
