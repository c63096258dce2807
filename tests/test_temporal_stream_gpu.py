"""GPU: zedo_temporal_stream_push - the pose-level chain of zedo_temporal_select on live streams: frames pushed in chunks, the tables in
caller-owned state, every frame decided `lag` frames after it went in (the transition and scan kernels of csrc/zedo_temporal_stream.hip,
the dead, emit and advance kernels of csrc/zedo_joint_stream.hip with J = 1) - and what Pipeline builds on it (push_temporal,
push_live_joints).  Held to
  - the GPU offline call, bit for bit, where the lag covers the clip (torch.equal on the int64 view), and on truncated clips at a
    finite lag;
  - the float64 reference of tests/_temporal_stream_ref.py (pinned on its own in tests/test_temporal_stream_ref.py): the PATHS exactly,
    the costs within _temporal_ref.cost_bound(J, L, .) (asserted; the difference each case shows is printed); check_inputs() asserts on
    the reference alone that the two best entries of D[n,.] and the two best candidates of every minimum are more than 1e-8 apart, so
    every arg-min is compared exactly;
  - zedo_joint_stream_push with d_T = NULL, bit for bit, at J = 1;
  - itself across chunkings, streams, ring sizes, a dirty state, a side stream, the alignment of d_x and stream capture, bit for bit.
Every push of the comparisons goes through tests/_stream_harness.py::Streams: the raw ABI on a state pre-filled with 0xFF bytes and then
reset, outputs pre-filled with a sentinel; d_emit is held to the header's formula after every push and the rows past the count to the
sentinel.  The call has no d_T: POSE leaves that slot of the harness's pointer list out, and the harness's T is None throughout.
Whether a fixed-lag path is closer to ground truth than the per-frame choice is not measured here or anywhere: these tests hold the
arithmetic.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, cur_stream, launch_invariant, misaligned, ptr as P, refusal_sweep, same
from _joint_ref import case as reproj_case
from _joint_stream_ref import chunkings, fixed_lag as joint_fixed_lag
from _joint_temporal_ref import joint_temporal_ref
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _joint_stream_ref import emitted
from _stream_harness import (Streams, StreamCall, each_alone, emit_blank, frames_of, gather, groups, raw_push, reset_refusals, run_clips, sizes,
                             stacked, state_in_use, whole_push)
from _temporal_ref import LAMBDAS, case, clips, cost_bound, dead_frame_case, reference, temporal_ref
from _temporal_stream_ref import LAGS, REFUSED, STREAM_CASES, STREAM_IDS, check_inputs, fixed_lag

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class PoseStreamCall(StreamCall):
    """A streaming push without d_T: slot 2 of the harness's pointer list is not passed on."""

    def push(self, lib, p, S, F, H, J, lag, mf, weights, nbytes, stream):
        assert p[2] is None
        return self.fn(lib, "push")(p[0], p[1], S, F, H, J, lag, mf, *weights, p[3], p[4], nbytes, *p[5:], stream)


POSE = PoseStreamCall("zedo_temporal_stream", ("lam",), lambda S, rows, J, H: (((S, rows), torch.int32), ((S, rows), torch.float64)),
                      index=0, max_h=1024)
JOINT = StreamCall("zedo_joint_stream", ("lam",), lambda S, rows, J, H: (((S, rows, J), torch.int32), ((S, rows, J), torch.float64)),
                   index=0, max_h=1024)


def replay_frame_by_frame(zh, xd, ud, N, starts, L, lag, weights):
    """_stream_harness.replay_frame_by_frame for a call without T (the helper clones all three static inputs): one F = 1 push without flush
    captured into a graph on a side stream (a single branch) over static input tensors, and replayed L times with frame f of every clip
    copied into them - a replay advances the state; d_emit is held to the header's formula after every replay.  With the emission of a
    final flush of no frames -> the outputs [S, L, ..]."""
    S, H, J = len(starts), xd.shape[0] // N, xd.shape[1]
    st = Streams(zh, POSE, S, H, J, lag, 1, weights)
    static = [t.clone() for t in gather(xd, None, ud, N, [[a] for a in starts])[:2]]
    o, emit = POSE.blank(S, 1 + lag, J, H), emit_blank(S)
    ptrs = [P(t) for t in static] + [None, None, P(st.state)] + [P(t) for t in o] + [P(emit)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = POSE.push(st.lib, ptrs, S, 1, H, J, lag, 1, st.w, st.nbytes, cur_stream())
    assert rc == 0
    for f in range(L):
        for dst, src in zip(static, gather(xd, None, ud, N, [[a + f] for a in starts])[:2]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        first, count = emitted(f, 1, lag, False)
        assert emit.cpu().tolist() == [[first, count]] * S
        for s in range(S):
            st.out[s].append((first, [t[s, :count].clone() for t in o]))
    st.t = [L] * S
    st.push(None, None, None, 0, [1] * S)
    return stacked(st, L)


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs()


COVERED = [(c, 100.0) for c in STREAM_CASES] + [((17, 70, 50, 35), lam) for lam in LAMBDAS if lam != 100.0]


@pytest.mark.parametrize("shape,lam", COVERED, ids=STREAM_IDS + ["J17-N70-H50-L35-lam30", "J17-N70-H50-L35-lam300"])
def test_a_lag_that_covers_the_clip_gives_the_bits_of_the_offline_call(zh, shape, lam):
    """lag = L - 1 and a flush at the end, pushed whole, frame by frame - every transition takes its predecessor from the state, at
    J = 33, 64 and 65 too - and in growing chunks: path and cost are those of zedo_temporal_select on the GPU, bit for bit; the paths
    are the float64 reference's."""
    J, N, H, L = shape
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    path, cost = zh.temporal_select(ud, xd, clips(N, L), lam=lam)
    assert np.array_equal(path.cpu().numpy(), reference(J, N, H, L, lam)["path"])
    for starts, Lc in groups(N, L):
        rows = torch.as_tensor(frames_of(starts, Lc), device="cuda")
        for name, cut in chunkings(Lc).items():
            p, c = run_clips(zh, POSE, xd, None, ud, N, starts, Lc, L - 1, cut, (lam,))
            assert same(p, path[rows]) and same(c, cost[rows]), (name, Lc)


FINITE = [(17, 70, 50, 35), (33, 9, 5, 9), (21, 40, 65, 40), (17, 40, 300, 13)]


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("J,N,H,L", FINITE, ids=lambda v: str(v))
def test_a_finite_lag_is_the_reference_and_the_offline_call_on_the_truncated_clip(zh, J, N, H, L, lag):
    """Paths equal fixed_lag exactly, costs within cost_bound(J, L, .) (whether they were bit-equal is printed); the three chunkings agree
    bit for bit; for three frames of the first clip the row equals the GPU offline call on the clip cut after min(n + lag, last)."""
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    seq = clips(N, L)
    for lam in LAMBDAS:
        rp, rc = fixed_lag(reference(J, N, H, L, lam), seq, lag)
        for starts, Lc in groups(N, L):
            rows = frames_of(starts, Lc)
            first = None
            for name, cut in chunkings(Lc).items():
                p, c = run_clips(zh, POSE, xd, None, ud, N, starts, Lc, lag, cut, (lam,))
                if first is None:
                    first = (p, c)
                    cn = c.cpu().numpy()
                    err = np.abs(cn - rc[rows])
                    print(f"temporal-stream J={J} N={N} H={H} L={Lc} lag={lag} lambda={lam:g}: max |cost - ref| = {err.max():.3e} (largest "
                          f"bound {cost_bound(J, L, rc[rows]).max():.3e}, bit-equal: {np.array_equal(cn.view(np.int64), rc[rows].view(np.int64))}); "
                          f"path differs on {int((p.cpu().numpy() != rp[rows]).sum())} of {rows.size}")
                    assert np.array_equal(p.cpu().numpy(), rp[rows]), (lam, name)
                    assert (err <= cost_bound(J, L, rc[rows])).all(), lam
                else:
                    assert same(p, first[0]) and same(c, first[1]), (lam, name)
        if lam == 100.0:
            a, Lc = seq[0], seq[1] - seq[0]
            p, c = run_clips(zh, POSE, xd, None, ud, N, [a], Lc, lag, [Lc], (lam,))
            for n in sorted({0, Lc // 2, max(0, Lc - 1 - lag)}):
                e = min(n + lag, Lc - 1)
                ut, xt, _ = gather(xd, None, ud, N, [list(range(a, a + e + 1))])
                op, oc = zh.temporal_select(ut, xt, [0, e + 1], lam=lam)
                assert same(p[0, n], op[n]) and same(c[0, n], oc[n]), (n, e)


@pytest.mark.parametrize("N,H,L", [(7, 2, 7), (30, 130, 13), (9, 300, 9), (4, 1024, 4)], ids=lambda v: str(v))
def test_one_joint_is_the_joint_stream_without_T(zh, N, H, L):
    """J = 1: path and cost are the bits of zedo_joint_stream_push with d_T = NULL on the same tensors, at lags 0, 3 and L - 1, in
    growing chunks."""
    x, u = case(1, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    for lag in (0, 3, L - 1):
        for starts, Lc in groups(N, L):
            cut = chunkings(Lc)["growing"]
            p, c = run_clips(zh, POSE, xd, None, ud, N, starts, Lc, lag, cut, (100.0,))
            jp, jc = run_clips(zh, JOINT, xd, None, ud.view(-1, 1), N, starts, Lc, lag, cut, (100.0,))
            assert same(p, jp[:, :, 0]) and same(c, jc[:, :, 0]), (lag, Lc)


def test_the_rings(zh):
    """R = 4 wrapped 32 times (lag 3, one frame per push, 128 frames of (17, 300, 7)); lag 0 with every push of max_frames frames (the
    dead kernel reuses the row of the frame before: the scan takes that flag from the state); R = 1.  Each is the reference's path and,
    bit for bit, the same clip pushed whole into a ring that never wraps."""
    J, N, H, lam, Lc = 17, 300, 7, 100.0, 128
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    tables = reference(J, N, H, 300, lam)                            # D and back of the frames 0 .. 127 are prefix quantities
    for lag, cut in ((3, [1] * Lc), (0, [8] * 16), (0, [1] * Lc)):
        rp, rc = fixed_lag(tables, [0, Lc], lag)
        p, c = run_clips(zh, POSE, xd, None, ud, N, [0], Lc, lag, cut, (lam,))
        assert zh.temporal_stream_state_bytes(1, H, J, lag, max(cut)) < zh.temporal_stream_state_bytes(1, H, J, lag, Lc)
        pw, cw = run_clips(zh, POSE, xd, None, ud, N, [0], Lc, lag, [Lc], (lam,))
        assert same(p, pw) and same(c, cw), (lag, cut[0])
        assert np.array_equal(p[0].cpu().numpy(), rp[:Lc]) and (np.abs(c[0].cpu().numpy() - rc[:Lc]) <= cost_bound(J, Lc, rc[:Lc])).all()


@pytest.mark.parametrize("lag", (0, 1, 2, 8))
def test_excluded_entries_and_a_dead_frame_inside_the_lag_window(zh, lag):
    """dead_frame_case: frame 4 has no finite unary - a dead frame inside the lag window and a chain end before the horizon - and
    frames 2 and 6 carry a NaN and a +inf.  The reference's paths and costs under every chunking; the dead frame reports 0 and +inf; the
    path is [0,0,0,1,0,1,0,0,0] at lag 0 and the offline [0,0,0,1,0,0,0,0,0] from lag 1 on."""
    x, u = dead_frame_case()
    xd, ud = dev(x), dev(u, torch.float64)
    for lam in (0.0, 100.0):
        rp, rc = fixed_lag(temporal_ref(u, x, [0, 9], lam), [0, 9], lag)
        for name, cut in chunkings(9).items():
            p, c = run_clips(zh, POSE, xd, None, ud, 9, [0], 9, lag, cut, (lam,))
            pn, cn = p[0].cpu().numpy(), c[0].cpu().numpy()
            assert np.array_equal(pn, rp) and pn[4] == 0 and np.isposinf(cn[4]), (lam, name)
            ok = np.isfinite(rc)
            assert ok.sum() == 8 and np.isfinite(cn[ok]).all() and (np.abs(cn[ok] - rc[ok]) <= cost_bound(5, 9, rc[ok])).all()
            if lam == 100.0:
                assert pn.tolist() == ([0, 0, 0, 1, 0, 1, 0, 0, 0] if lag == 0 else [0, 0, 0, 1, 0, 0, 0, 0, 0])
    if lag == 8:
        op, oc = zh.temporal_select(ud, xd, [0, 9], lam=100.0)
        assert same(p[0], op) and same(c[0], oc)


def test_streams_are_independent(zh):
    """Three streams carry different clips of (5, 12, 3), one frame per push at lag 2: stream 0's first clip is one frame long, stream 1
    is flushed mid-way and goes on with another clip, stream 2 is reset through d_which after two frames - those are dropped - and
    starts over: the streams' clips hold different numbers of frames at every push.  Each stream emits, bit for bit and push by push,
    what it emits alone; and what the reference says of its clips."""
    J, N, H, lag, lam = 5, 12, 3, 2, 100.0
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    frames = [[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11], [8, 9, 0, 1, 2, 3, 4, 5]]
    flush_at = [{0, 7}, {3, 7}, {7}]
    reset_after = [set(), set(), {1}]
    all3 = each_alone(zh, POSE, xd, None, ud, N, frames, flush_at, reset_after, lag, (lam,))
    carried = [[[0], list(range(1, 8))], [list(range(4, 8)), list(range(8, 12))], [list(range(0, 6))]]
    for s in range(3):
        fr, (p, c) = all3.collected(s)
        assert fr == [f for cl in carried[s] for f in range(len(cl))]
        at = 0
        for cl in carried[s]:
            ut, xt, _ = gather(xd, None, ud, N, [cl])
            rp, rc = fixed_lag(temporal_ref(ut.cpu().numpy(), xt.cpu().numpy(), [0, len(cl)], lam), [0, len(cl)], lag)
            assert np.array_equal(p[at:at + len(cl)].cpu().numpy(), rp)
            assert (np.abs(c[at:at + len(cl)].cpu().numpy() - rc) <= cost_bound(J, len(cl), rc)).all()
            at += len(cl)


def test_the_bits_do_not_depend_on_the_state_the_stream_or_the_alignment(zh):
    """A state pre-filled with 0x00 instead of 0xFF; the stream index (clip 1 as stream 0 of one); a side stream, the call captured and
    replayed twice and d_x at a 12-byte offset (launch_invariant, on reset + push + flush as one call); a flush with F = 0; and one F = 1
    push captured into a graph on a single branch and replayed L times with the inputs copied into its static tensors - a replay
    advances the state - whose concatenated emission, with that of a final flush of no frames, is the offline call."""
    J, N, H, L, lam = 17, 70, 50, 35, 100.0
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    offline = [t.view(2, L) for t in zh.temporal_select(ud, xd, clips(N, L), lam=lam)]
    for lag in (3, L - 1):
        cut = chunkings(L)["growing"]
        want = run_clips(zh, POSE, xd, None, ud, N, [0, L], L, lag, cut, (lam,))
        if lag == L - 1:
            assert all_same(want, offline)
        assert all_same(run_clips(zh, POSE, xd, None, ud, N, [0, L], L, lag, cut, (lam,), fill=0x00), want)
        assert all_same(run_clips(zh, POSE, xd, None, ud, N, [L], L, lag, cut, (lam,)), [t[1:] for t in want])
        uu, xx, _ = gather(xd, None, ud, N, [list(range(0, L)), list(range(L, 2 * L))])
        whole = whole_push(zh, POSE, (uu, xx, None), 2, L, H, J, lag, (lam,))
        ref = whole()
        torch.cuda.synchronize()
        assert all_same(ref[:-1], want) and ref[-1].tolist() == [[0, L]] * 2
        launch_invariant(ref, whole, xx)
        # d_x at the offset again, without a flush: L - lag frames come out; F = 0: the pending min(lag, L) frames
        st = Streams(zh, POSE, 2, H, J, lag, L, (lam,))
        st.push(uu, misaligned(xx), None, L)
        st.push(None, None, None, 0, [1, 1])
        for k in range(2):
            fr, o = st.collected(k)
            assert fr == list(range(L)) and all_same(o, [t[k] for t in want])
    # captured: one frame per replay on static tensors, lag = L - 1 and lag = 3
    assert all_same(replay_frame_by_frame(zh, xd, ud, N, [0, L], L, L - 1, (lam,)), offline)
    assert all_same(replay_frame_by_frame(zh, xd, ud, N, [0, L], L, 3, (lam,)),
                    run_clips(zh, POSE, xd, None, ud, N, [0, L], L, 3, [L], (lam,)))


def test_the_binding_owns_the_state(zh):
    """zh.TemporalStream: push, flush and reset with flags given as lists or tensors; the same bits as the raw ABI; the refusals of the
    binding itself."""
    J, N, H, L, lag, lam = 5, 12, 3, 4, 2, 30.0
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    starts = [0, 4, 8]
    want = run_clips(zh, POSE, xd, None, ud, N, starts, L, lag, [3, 1], (lam,))
    ts = zh.TemporalStream(3, H, J, lag, 3, lam=lam)
    assert ts.state_bytes == zh.temporal_stream_state_bytes(3, H, J, lag, 3) == ts.state.numel()
    ts.push(*gather(xd, None, ud, N, [[a] for a in starts])[:2])     # to be dropped
    ts.reset()
    chunk = gather(xd, None, ud, N, [[a, a + 1, a + 2] for a in starts])[:2]
    f1, n1, p1, c1 = ts.push(*chunk)
    assert f1.tolist() == [0] * 3 and n1.tolist() == [1] * 3 and p1.shape == (3, 3 + lag) and c1.dtype == torch.float64
    f2, n2, p2, c2 = ts.push(*gather(xd, None, ud, N, [[a + 3] for a in starts])[:2], flush=torch.tensor([1, 0, 1]))
    assert f2.tolist() == [1] * 3 and n2.tolist() == [3, 1, 3]
    f3, n3, p3, c3 = ts.flush([0, 1, 0])
    assert f3.tolist() == [0, 2, 0] and n3.tolist() == [0, 2, 0] and p3.shape == (3, lag)
    for k, (pp, cc) in enumerate(((p2, c2), (torch.cat([p2[:, :1], p3], 1), torch.cat([c2[:, :1], c3], 1)), (p2, c2))):
        assert same(torch.cat([p1[k, :1], pp[k, :3]]), want[0][k]) and same(torch.cat([c1[k, :1], cc[k, :3]]), want[1][k])
    f4, n4, _, _ = ts.flush()
    assert n4.tolist() == [0, 0, 0] and f4.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        ts.push(chunk[0][:-1], chunk[1])
    with pytest.raises(ValueError):
        ts.push(chunk[0], chunk[1], flush=[1, 0])
    with pytest.raises(ValueError):
        ts.push(None, None)
    with pytest.raises(zh.ZedoError):
        ts.push(*gather(xd, None, ud, N, [[a, a + 1, a + 2, a + 3] for a in starts])[:2])    # F > max_frames
    with pytest.raises(zh.ZedoError):
        zh.TemporalStream(1, 1025, 1, 0, 1)
    J, N, H, L = REFUSED
    assert zh.temporal_stream_state_bytes(1, H, J, L - 1, L) == 0 and zh.temporal_stream_state_bytes(1, 1024, J, L - 1, L) > 0


def test_refusals_at_the_raw_abi(zh):
    """refusal_sweep: a NULL pointer other than d_flush / d_which, every size out of range - H = 1025 included - F > max_frames, F = 0
    without d_flush, a negative lag, lambda < 0, NaN or inf, a misaligned state: ZEDO_E_BADARG; a state one byte short or of no bytes:
    ZEDO_E_WORKSPACE; outputs and the bytes of a state in use unchanged either way, by the refusals of the reset as well.  The same call
    as it stands is accepted."""
    lib = zh._lib
    J, N, H, lag, mf, w = 5, 12, 3, 2, 4, (100.0,)
    x, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    S, F, starts = 3, 4, (0, 4, 8)
    uu, xx, _ = gather(xd, None, ud, N, [list(range(a, a + F)) for a in starts])
    use = state_in_use(zh, POSE, xd, None, ud, N, starts, lag, mf, w)  # two frames per stream
    state, need = use.state, use.need
    out, emit = POSE.blank(S, F + lag, J, H), torch.full((S, 2), -1, dtype=torch.int64, device="cuda")
    fl = torch.ones(S, dtype=torch.int32, device="cuda")
    ptrs = [P(uu), P(xx), None, P(fl), P(state)] + [P(t) for t in out] + [P(emit)]
    call = raw_push(lib, POSE, ptrs, S, F, H, J, lag, mf, w, need)
    reset_refusals(lib, POSE, use, S, H, J, lag, mf)
    refusal_sweep(call, ptrs, POSE.required(), sizes=sizes(POSE, mf), weights=POSE.weights, workspace_slot=4, need=need,
                  untouched=[(t, POSE.sentinel) for t in out] + [(emit, -1), (state, use.before)])
    # the control of the sweep pushed four frames onto the two and flushed: six come out
    assert emit.tolist() == [[0, 6]] * S and bool((state[need:] == 0x5A).all()) and not torch.equal(state, use.before)
    # without flush; then a flush of no frames
    assert call([P(t) for t in use.chunk2[:2]] + [None] + ptrs[3:], f=2, no_flush=True) == 0
    assert call([None, None, None] + ptrs[3:], f=0) == 0
    torch.cuda.synchronize()
    assert emit.tolist() == [[0, 2]] * S and bool((state[need:] == 0x5A).all())


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------

def loaded(weights0, J, N, H, frames=None):
    """A Pipeline on the detections of _joint_ref.case(J, N, H) - of its poses `frames` if given."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    _, _, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    d2 = np.concatenate([uv, conf[:, :, None]], -1)
    fr = slice(None) if frames is None else np.asarray(frames).reshape(-1)      # [S][F] -> pose n = s F + f
    return Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, d2[fr], K[fr])


def rows_of(H, N, frames):
    """The rows (h, n) of the poses `frames` [S][F], h-major with n = s F + f."""
    fr = np.asarray(frames).reshape(-1)
    return torch.as_tensor((np.arange(H)[:, None] * N + fr[None, :]).reshape(-1), device="cuda")


def test_pipeline_push_temporal(zh, weights0):
    """Pipeline.push_temporal on the problem of load(), with a lag that covers the clips and a flush, is Pipeline.select_temporal, bit
    for bit, and the raw call on min_reproj's errors."""
    J, N, H = 17, 70, 5
    x, T = reproj_case(J, N, H)[:2]
    pipe = loaded(weights0, J, N, H)
    xd, Td = dev(x), dev(T)
    p, k, e = pipe.select_temporal(xd, Td, [0, 35, N], lam=30.0)
    ps = pipe.open_pose_stream(2, 34, 35, lam=30.0)
    assert (ps.S, ps.H, ps.J, ps.lag, ps.max_frames) == (2, H, J, 34, 35)
    first, count, sp, sc, err = pipe.push_temporal(ps, xd, Td, flush=[1, 1])
    assert first.tolist() == [0, 0] and count.tolist() == [35, 35] and same(err, e)
    assert same(sp[:, :35].reshape(N), p) and same(sc[:, :35].reshape(N), k)
    rp, rc = run_clips(zh, POSE, xd, None, e, N, [0, 35], 35, 34, [35], (30.0,))
    assert same(sp[:, :35], rp) and same(sc[:, :35], rc)
    with pytest.raises(ValueError):
        pipe.push_temporal(ps, xd[:N], Td[:N])
    with pytest.raises(ValueError):
        pipe.push_temporal(pipe.open_pose_stream(3, 1, 35), xd, Td)


def test_push_live_joints_where_the_lag_covers_the_clip(zh, weights0):
    """One push of both clips at lag 34 with a flush: pose is joint_compose(x, T, joint path, pose path) of the two GPU offline calls -
    the pose --select joints-temporal writes - bit for bit; T_sel is T of the pose path; the paths are the offline calls'."""
    J, N, H, L = 17, 70, 5, 35
    x, T = reproj_case(J, N, H)[:2]
    pipe = loaded(weights0, J, N, H)
    xd, Td = dev(x), dev(T)
    idx = pipe.select_temporal(xd, Td, [0, L, N], lam=30.0)[0]
    jpath = pipe.select_joints_temporal(xd, Td, [0, L, N], lam=30.0)[0]
    want = zh.joint_compose(xd, Td, jpath, idx, N)
    lj = pipe.open_live_joints(2, L - 1, L, lam=30.0)
    first, count, pose, jp, pp, T_sel = pipe.push_live_joints(lj, xd, Td, flush=[1, 1])
    assert first.tolist() == [0, 0] and count.tolist() == [L, L] and pose.shape == (2, 2 * L - 1, J, 3) and pose.dtype == torch.float32
    assert same(pose[:, :L].reshape(N, J, 3), want) and same(jp[:, :L].reshape(N, J), jpath) and same(pp[:, :L].reshape(N), idx)
    assert same(T_sel[:, :L].reshape(N, 3), Td[idx.long() * N + torch.arange(N, device="cuda")])
    assert bool(torch.isnan(pose[:, L:]).all()) and bool(torch.isnan(T_sel[:, L:]).all())
    assert bool((jp[:, L:] == -1).all()) and bool((pp[:, L:] == -1).all()) and lj.t == [0, 0]


def test_push_live_joints_at_lag_3(zh, weights0):
    """Two streams at lag 3: pushed frame by frame and in chunks of 5 (a flush with the last), every emitted row bit-equal between the
    two, rows past the count NaN and -1; the concatenated emission is joint_compose on the two REFERENCE paths (the numpy fixed-lag
    decisions on the unaries the pipeline formed)."""
    J, N, H, L, lag, lam = 17, 70, 5, 35, 3, 30.0
    x, T = reproj_case(J, N, H)[:2]
    xd, Td = dev(x), dev(T)
    whole = loaded(weights0, J, N, H)
    err = whole.select_temporal(xd, Td, [0, L, N], lam=lam)[2].cpu().numpy()
    jerr = whole.select_joints_temporal(xd, Td, [0, L, N], lam=lam)[2].cpu().numpy()
    rp = fixed_lag(temporal_ref(err, x, [0, L, N], lam), [0, L, N], lag)[0]
    rjp = joint_fixed_lag(joint_temporal_ref(jerr, x, T, [0, L, N], lam), [0, L, N], lag)[0]
    want = zh.joint_compose(xd, Td, dev(rjp, torch.int32), dev(rp, torch.int32), N).view(2, L, J, 3)
    got = {}
    for F in (1, 5):
        lj = whole.open_live_joints(2, lag, F, lam=lam)
        outs = [[] for _ in range(4)]
        for f0 in range(0, L, F):
            frames = [[a + f0 + f for f in range(F)] for a in (0, L)]
            pipe = loaded(weights0, J, N, H, frames)
            rows = rows_of(H, N, frames)
            last = f0 + F == L
            first, count, *o = pipe.push_live_joints(lj, xd[rows].contiguous(), Td[rows].contiguous(), flush=[1, 1] if last else None)
            held = min(lag, f0) + F
            assert first.tolist() == [max(0, f0 - lag)] * 2 and count.tolist() == [held if last else max(0, held - lag)] * 2
            k = int(count[0])
            assert o[0].shape == (2, F + lag, J, 3) and bool(torch.isnan(o[0][:, k:]).all()) and bool(torch.isnan(o[3][:, k:]).all())
            assert bool((o[1][:, k:] == -1).all()) and bool((o[2][:, k:] == -1).all())
            for dst, t in zip(outs, o):
                dst.append(t[:, :k])
        got[F] = [torch.cat(k, 1) for k in outs]
        assert got[F][0].shape == (2, L, J, 3)
    assert all_same(got[1], got[5])
    pose, jp, pp, T_sel = got[1]
    assert np.array_equal(pp.cpu().numpy(), rp.reshape(2, L)) and np.array_equal(jp.cpu().numpy(), rjp.reshape(2, L, J))
    assert same(pose, want)
    assert same(T_sel.reshape(N, 3), Td[dev(rp, torch.int64) * N + torch.arange(N, device="cuda")])
