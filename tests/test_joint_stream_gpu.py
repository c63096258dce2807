"""GPU: zedo_joint_stream_push - the first-order joint-wise chain of zedo_joint_temporal_select on live streams: frames pushed in chunks,
the tables in caller-owned state, every frame decided `lag` frames after it went in (dead, scan, emit and advance kernels of
csrc/zedo_joint_stream.hip).  Held to
  - the GPU offline call, bit for bit, where the lag covers the clip (torch.equal on the int64 view), and on truncated clips at a
    finite lag;
  - the float64 reference of tests/_joint_stream_ref.py (pinned on its own in tests/test_joint_stream_ref.py): the PATHS exactly, the
    costs within _temporal_ref.cost_bound(1, L, .) (asserted; the difference each case shows is printed); check_inputs() asserts on the
    reference alone that the two best entries of D[n,j,.] are more than 1e-6 apart at every live (n, j), so every arg-min is compared
    exactly;
  - itself across chunkings, streams, a dirty state, a side stream, the alignment of d_x and stream capture, bit for bit.
Every push of the comparisons goes through Streams: the raw ABI on a state pre-filled with 0xFF bytes and then reset, outputs pre-filled with a
sentinel; d_emit is held to the header's formula after every push and the rows past the count to the sentinel.
Whether a fixed-lag path is closer to ground truth than the per-frame choice is not measured here or anywhere: these tests hold the
arithmetic.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, launch_invariant, misaligned, ptr as P, refusal_sweep, same
from _joint_ref import case as reproj_case
from _joint_stream_ref import LAGS, check_inputs, chunkings, fixed_lag
from _joint_temporal_ref import ALL_CASES, IDS, LAMBDAS, case, dead_joint_case, joint_temporal_ref, reference
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _stream_harness import (Streams, StreamCall, each_alone, frames_of, gather, groups, raw_push, replay_frame_by_frame, reset_refusals,
                             run_clips, sizes, state_in_use, whole_push)
from _temporal_ref import clips, cost_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CALL = StreamCall("zedo_joint_stream", ("lam",), lambda S, rows, J, H: (((S, rows, J), torch.int32), ((S, rows, J), torch.float64)), index=0,
                  max_h=1024)


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs()


@pytest.mark.parametrize("J,N,H,L", ALL_CASES, ids=IDS)
def test_a_lag_that_covers_the_clip_gives_the_bits_of_the_offline_call(zh, J, N, H, L):
    """lag = L - 1 and a flush at the end, pushed whole, frame by frame and in growing chunks, with T and without: path and cost are those
    of zedo_joint_temporal_select on the GPU, bit for bit; the paths are the float64 reference's."""
    x, T, u = case(J, N, H)
    xd, ud, lam = dev(x), dev(u, torch.float64), 100.0
    for with_T in (True, False):
        Td = dev(T) if with_T else None
        path, cost = zh.joint_temporal_select(ud, xd, Td, clips(N, L), lam=lam)
        assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, lam, with_T)["path"])
        for starts, Lc in groups(N, L):
            rows = torch.as_tensor(frames_of(starts, Lc), device="cuda")
            for name, cut in chunkings(Lc).items():
                p, c = run_clips(zh, CALL, xd, Td, ud, N, starts, Lc, L - 1, cut, (lam,))
                assert same(p, path[rows]) and same(c, cost[rows]), (with_T, name, Lc)


FINITE = [(17, 70, 50, 35), (3, 130, 7, 130), (2, 30, 130, 13), (1, 9, 1024, 9), (1, 6, 300, 3)]


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("J,N,H,L", FINITE, ids=lambda v: str(v))
def test_a_finite_lag_is_the_reference_and_the_offline_call_on_the_truncated_clip(zh, J, N, H, L, lag):
    """Paths equal fixed_lag exactly, costs within cost_bound(1, L, .); the three chunkings agree bit for bit; for three frames of the
    first clip the row equals the GPU offline call on the clip cut after min(n + lag, last)."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    seq = clips(N, L)
    for lam in LAMBDAS:
        rp, rc = fixed_lag(reference(J, N, H, L, lam), seq, lag)
        for starts, Lc in groups(N, L):
            rows = frames_of(starts, Lc)
            first = None
            for name, cut in chunkings(Lc).items():
                p, c = run_clips(zh, CALL, xd, Td, ud, N, starts, Lc, lag, cut, (lam,))
                if first is None:
                    first = (p, c)
                    err = np.abs(c.cpu().numpy() - rc[rows])
                    print(f"joint-stream J={J} N={N} H={H} L={Lc} lag={lag} lambda={lam:g}: max |cost - ref| = {err.max():.3e} (largest "
                          f"bound {cost_bound(1, L, rc[rows]).max():.3e}); path differs on {int((p.cpu().numpy() != rp[rows]).sum())} of "
                          f"{rows.size * J}")
                    assert np.array_equal(p.cpu().numpy(), rp[rows]), (lam, name)
                    assert (err <= cost_bound(1, L, rc[rows])).all(), lam
                else:
                    assert same(p, first[0]) and same(c, first[1]), (lam, name)
        if lam == 100.0:
            a, Lc = seq[0], seq[1] - seq[0]
            for n in sorted({0, Lc // 2, max(0, Lc - 1 - lag)}):
                e = min(n + lag, Lc - 1)
                ut, xt, Tt = gather(xd, Td, ud, N, [list(range(a, a + e + 1))])
                op, oc = zh.joint_temporal_select(ut, xt, Tt, [0, e + 1], lam=lam)
                p, c = run_clips(zh, CALL, xd, Td, ud, N, [a], Lc, lag, [Lc], (lam,))
                assert same(p[0, n], op[n]) and same(c[0, n], oc[n]), (n, e)


def test_streams_are_independent(zh):
    """Three streams carry different clips of (5, 12, 3), one frame per push at lag 2: stream 1 is flushed mid-way and goes on with
    another clip, stream 2 is reset through d_which after two frames - those are dropped - and starts over.  Each stream emits, bit for
    bit and push by push, what it emits alone; and what the reference says of its clips."""
    J, N, H, lag, lam = 5, 12, 3, 2, 100.0
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    frames = [[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11], [8, 9, 0, 1, 2, 3, 4, 5]]
    flush_at = [{7}, {3, 7}, {7}]
    reset_after = [set(), set(), {1}]
    all3 = each_alone(zh, CALL, xd, Td, ud, N, frames, flush_at, reset_after, lag, (lam,))
    # the clips each stream carried, in the order it emitted them: (frames of the case, ...)
    carried = [[list(range(0, 8))], [list(range(4, 8)), list(range(8, 12))], [list(range(0, 6))]]
    for s in range(3):
        fr, (p, c) = all3.collected(s)
        assert fr == [f for cl in carried[s] for f in range(len(cl))]
        at = 0
        for cl in carried[s]:
            ut, xt, Tt = gather(xd, Td, ud, N, [cl])
            r = joint_temporal_ref(ut.cpu().numpy(), xt.cpu().numpy(), Tt.cpu().numpy(), [0, len(cl)], lam)
            rp, rc = fixed_lag(r, [0, len(cl)], lag)
            assert np.array_equal(p[at:at + len(cl)].cpu().numpy(), rp)
            assert (np.abs(c[at:at + len(cl)].cpu().numpy() - rc) <= cost_bound(1, len(cl), rc)).all()
            at += len(cl)


@pytest.mark.parametrize("lag", (0, 1, 2, 8))
def test_excluded_entries_and_a_dead_frame_joint_inside_the_lag_window(zh, lag):
    """dead_joint_case: (frame 4, joint 2) has no finite unary - a dead entry inside the lag window and a chain end before the horizon -
    and frames 2 and 6 carry a NaN and a +inf.  The reference's paths and costs under every chunking; the dead entry reports 0 and +inf;
    the other joints return the bits of the untouched unaries; joint 2's path is the pinned one at lag 0 and at lag 8."""
    x, T, u, j = dead_joint_case()
    xd, Td, ud, cd = dev(x), dev(T), dev(u, torch.float64), dev(case(5, 9, 3)[2], torch.float64)
    others = [i for i in range(5) if i != j]
    for lam in (0.0, 100.0):
        rp, rc = fixed_lag(joint_temporal_ref(u, x, T, [0, 9], lam), [0, 9], lag)
        for name, cut in chunkings(9).items():
            p, c = run_clips(zh, CALL, xd, Td, ud, 9, [0], 9, lag, cut, (lam,))
            p0, c0 = run_clips(zh, CALL, xd, Td, cd, 9, [0], 9, lag, cut, (lam,))
            assert same(p[0][:, others], p0[0][:, others]) and same(c[0][:, others], c0[0][:, others])
            pn, cn = p[0].cpu().numpy(), c[0].cpu().numpy()
            assert np.array_equal(pn, rp) and pn[4, j] == 0 and np.isposinf(cn[4, j])
            ok = np.isfinite(rc)
            assert ok.sum() == 44 and np.isfinite(cn[ok]).all() and (np.abs(cn[ok] - rc[ok]) <= cost_bound(1, 9, rc[ok])).all()
            if lam == 100.0 and lag in (0, 8):
                assert pn[:, j].tolist() == ([0, 0, 0, 1, 0, 2, 0, 0, 0] if lag == 0 else [1, 1, 1, 1, 0, 0, 0, 0, 0])


def test_the_bits_do_not_depend_on_the_state_the_stream_or_the_alignment(zh):
    """A state pre-filled with 0x00 instead of 0xFF; a side stream, the call captured and replayed twice and d_x at a 12-byte offset
    (launch_invariant, on reset + push + flush as one call); a flush with F = 0; and one F = 1 push captured into a graph on a single
    branch and replayed L times with the inputs copied into its static tensors - a replay advances the state - whose concatenated
    emission, with that of a final flush of no frames, is the offline call."""
    J, N, H, L, lam = 17, 70, 50, 35, 100.0
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    offline = [t.view(2, L, J) for t in zh.joint_temporal_select(ud, xd, Td, clips(N, L), lam=lam)]
    for lag in (3, L - 1):
        cut = chunkings(L)["growing"]
        want = run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, cut, (lam,))
        if lag == L - 1:
            assert all_same(want, offline)
        assert all_same(run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, cut, (lam,), fill=0x00), want)
        uu, xx, TT = gather(xd, Td, ud, N, [list(range(0, L)), list(range(L, 2 * L))])
        whole = whole_push(zh, CALL, (uu, xx, TT), 2, L, H, J, lag, (lam,))
        ref = whole()
        torch.cuda.synchronize()
        assert all_same(ref[:-1], want) and ref[-1].tolist() == [[0, L]] * 2
        launch_invariant(ref, whole, xx)
        # d_x at the offset again, without a flush: L - lag frames come out; F = 0: the pending min(lag, L) frames
        st = Streams(zh, CALL, 2, H, J, lag, L, (lam,))
        st.push(uu, misaligned(xx), TT, L)
        st.push(None, None, None, 0, [1, 1])
        for k in range(2):
            fr, o = st.collected(k)
            assert fr == list(range(L)) and all_same(o, [t[k] for t in want])
    # captured: one frame per replay on static tensors, lag = L - 1
    assert all_same(replay_frame_by_frame(zh, CALL, xd, Td, ud, N, [0, L], L, L - 1, (lam,)), offline)


def test_the_binding_owns_the_state(zh):
    """zh.JointStream: push, flush and reset with flags given as lists or tensors; the same bits as the raw ABI; the refusals of the
    binding itself."""
    J, N, H, L, lag, lam = 5, 12, 3, 4, 2, 30.0
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    starts = [0, 4, 8]
    want = run_clips(zh, CALL, xd, Td, ud, N, starts, L, lag, [3, 1], (lam,))
    js = zh.JointStream(3, H, J, lag, 3, lam=lam)
    assert js.state_bytes == zh.joint_stream_state_bytes(3, H, J, lag, 3) == js.state.numel()
    js.push(*gather(xd, Td, ud, N, [[a] for a in starts]))           # to be dropped
    js.reset()
    chunk = gather(xd, Td, ud, N, [[a, a + 1, a + 2] for a in starts])
    f1, n1, p1, c1 = js.push(*chunk)
    assert f1.tolist() == [0] * 3 and n1.tolist() == [1] * 3 and p1.shape == (3, 3 + lag, J) and c1.dtype == torch.float64
    f2, n2, p2, c2 = js.push(*gather(xd, Td, ud, N, [[a + 3] for a in starts]), flush=torch.tensor([1, 0, 1]))
    assert f2.tolist() == [1] * 3 and n2.tolist() == [3, 1, 3]
    f3, n3, p3, c3 = js.flush([0, 1, 0])
    assert f3.tolist() == [0, 2, 0] and n3.tolist() == [0, 2, 0] and p3.shape == (3, lag, J)
    for k, (pp, cc) in enumerate(((p2, c2), (torch.cat([p2[:, :1], p3], 1), torch.cat([c2[:, :1], c3], 1)), (p2, c2))):
        assert same(torch.cat([p1[k, :1], pp[k, :3]]), want[0][k]) and same(torch.cat([c1[k, :1], cc[k, :3]]), want[1][k])
    f4, n4, _, _ = js.flush()
    assert n4.tolist() == [0, 0, 0] and f4.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        js.push(chunk[0][:-1], chunk[1], chunk[2])
    with pytest.raises(ValueError):
        js.push(chunk[0], chunk[1], chunk[2], flush=[1, 0])
    with pytest.raises(ValueError):
        js.push(None, None, None)
    with pytest.raises(zh.ZedoError):
        js.push(*gather(xd, Td, ud, N, [[a, a + 1, a + 2, a + 3] for a in starts]))      # F > max_frames
    with pytest.raises(zh.ZedoError):
        zh.JointStream(1, 1025, 1, 0, 1)
    assert zh.joint_stream_state_bytes(1, 1025, 1, 0, 1) == 0


def test_refusals_at_the_raw_abi(zh):
    """refusal_sweep: a NULL pointer other than d_T / d_flush / d_which, every size out of range - H = 1025 included - F > max_frames,
    F = 0 without d_flush, a negative lag, lambda < 0, NaN or inf, a misaligned state: ZEDO_E_BADARG; a state one byte short or of no
    bytes: ZEDO_E_WORKSPACE; outputs and the bytes of a state in use unchanged either way, by the refusals of the reset as well.  The
    same call as it stands is accepted."""
    lib = zh._lib
    J, N, H, lag, mf, w = 5, 12, 3, 2, 4, (100.0,)
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    S, F, starts = 3, 4, (0, 4, 8)
    uu, xx, TT = gather(xd, Td, ud, N, [list(range(a, a + F)) for a in starts])
    use = state_in_use(zh, CALL, xd, Td, ud, N, starts, lag, mf, w)  # two frames per stream
    state, need = use.state, use.need
    out, emit = CALL.blank(S, F + lag, J, H), torch.full((S, 2), -1, dtype=torch.int64, device="cuda")
    fl = torch.ones(S, dtype=torch.int32, device="cuda")
    ptrs = [P(uu), P(xx), P(TT), P(fl), P(state)] + [P(t) for t in out] + [P(emit)]
    call = raw_push(lib, CALL, ptrs, S, F, H, J, lag, mf, w, need)
    reset_refusals(lib, CALL, use, S, H, J, lag, mf)
    refusal_sweep(call, ptrs, CALL.required(), sizes=sizes(CALL, mf), weights=CALL.weights, workspace_slot=4, need=need,
                  untouched=[(t, CALL.sentinel) for t in out] + [(emit, -1), (state, use.before)])
    # the control of the sweep pushed four frames onto the two and flushed: six come out
    assert emit.tolist() == [[0, 6]] * S and bool((state[need:] == 0x5A).all()) and not torch.equal(state, use.before)
    # without T and without flush; then a flush of no frames
    assert call([P(t) for t in use.chunk2[:2]] + [None] + ptrs[3:], f=2, no_flush=True) == 0
    assert call([None, None, None] + ptrs[3:], f=0) == 0
    torch.cuda.synchronize()
    assert emit.tolist() == [[0, 2]] * S and bool((state[need:] == 0x5A).all())


def test_pipeline_push_joints_temporal(zh, weights0):
    """Pipeline.push_joints_temporal on the problem of load(), with a lag that covers the clips and a flush, is
    Pipeline.select_joints_temporal, bit for bit: joint_reproj's distances fed to the streaming call."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    p, k, e = pipe.select_joints_temporal(xd, Td, [0, 35, N], lam=30.0)
    js = pipe.open_joint_stream(2, 34, 35, lam=30.0)
    assert (js.S, js.H, js.J, js.lag, js.max_frames) == (2, H, J, 34, 35)
    first, count, sp, sc, jerr = pipe.push_joints_temporal(js, xd, Td, flush=[1, 1])
    assert first.tolist() == [0, 0] and count.tolist() == [35, 35] and same(jerr, e)
    assert same(sp[:, :35].reshape(N, J), p) and same(sc[:, :35].reshape(N, J), k)
    with pytest.raises(ValueError):
        pipe.push_joints_temporal(js, xd[:N], Td[:N])
    with pytest.raises(ValueError):
        pipe.push_joints_temporal(pipe.open_joint_stream(3, 1, 35), xd, Td)
