"""GPU: zedo_joint_accel_stream_push - the second-order joint-wise chain of zedo_joint_accel_select on live streams: frames pushed in
chunks, the tables in caller-owned state, every frame decided `lag` frames after it went in (scan and emit kernels of
csrc/zedo_joint_accel_stream.hip between the dead and advance kernels of csrc/zedo_joint_stream.hip).  Held to
  - the GPU offline call where the lag covers the clip: the PATHS bit for bit; the cost at every frame of a chain against that call's
    cost at the chain's last frame, within the sum of the two cost_bounds (min E there against the same additions re-accumulated);
  - the float64 reference of tests/_joint_accel_stream_ref.py (pinned on its own in tests/test_joint_accel_stream_ref.py, which also
    asserts that the two best entries at every horizon are more than 1e-8 apart on every case used here): the paths exactly at every
    lag of LAGS, the costs within _joint_accel_ref.cost_bound(L, .) = 8 L 2^-53 relative (asserted; the largest share is printed);
  - itself across chunkings, streams, a dirty state, a side stream, the alignment of d_x and stream capture, bit for bit;
  - zedo_joint_stream_push at lambda_a = 0, and the arg-min pair of the reference at lag 0.
Every push of the comparisons goes through Streams: the raw ABI on a state pre-filled with 0xFF bytes and then reset, outputs pre-filled
with a sentinel; d_emit is held to the header's formula after every push and the rows past the count to the sentinel.
Recorded on the MI355X: 97 passed in 5.6 s; pytest's --durations: the slowest case 0.77 s ((17, 70, 50, 35) at the five lags, its numpy
reference included), every other below 0.5 s.
Whether a fixed-lag second-order path is closer to ground truth than any other is not measured here or anywhere: these tests hold the
arithmetic.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, launch_invariant, misaligned, ptr as P, refusal_sweep, same
from _joint_accel_ref import cost_bound
from _joint_accel_stream_ref import (BIG, BIG_WEIGHTS, GPU_CASES, LAGS, WEIGHTS, case, chunkings, clips, dead_joint_case, fixed_lag,
                                     forward, tables)
from _joint_ref import case as reproj_case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _stream_harness import (Streams, StreamCall, each_alone, frames_of, gather, groups, raw_push, replay_frame_by_frame, reset_refusals,
                             run_clips, sizes, state_in_use, whole_push)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CALL = StreamCall("zedo_joint_accel_stream", ("lam_v", "lam_a"), lambda S, rows, J, H: (((S, rows, J), torch.int32), ((S, rows, J), torch.float64)),
                  index=0, max_h=64)
CELLS = [(c, w) for c in GPU_CASES for w in WEIGHTS] + [(BIG, BIG_WEIGHTS)]
CELL_IDS = [f"J{c[0]}-N{c[1]}-H{c[2]}-L{c[3]}-v{w[0]:g}-a{w[1]:g}" for c, w in CELLS]


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_a_lag_that_covers_the_clip_gives_the_paths_of_the_offline_call(zh, cell):
    """lag = L - 1 and a flush at the end, pushed whole, frame by frame and in growing chunks, with T and without: the paths are those of
    zedo_joint_accel_select on the GPU, bit for bit; the cost at every frame of a chain is that call's cost at the chain's last frame
    within the sum of the two cost_bounds."""
    (J, N, H, L), w = cell
    x, T, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    for with_T in (True, False):
        Td = dev(T) if with_T else None
        path, cost = zh.joint_accel_select(ud, xd, Td, clips(N, L), lam=w[0], accel=w[1])
        cn = cost.cpu().numpy()
        for starts, Lc in groups(N, L):
            rows = frames_of(starts, Lc)
            end = np.repeat(cn[rows][:, -1:], Lc, axis=1)            # (no dead frame in these cases: a clip is one chain per joint)
            assert np.isfinite(end).all()
            for name, cut in chunkings(Lc).items():
                p, c = run_clips(zh, CALL, xd, Td, ud, N, starts, Lc, L - 1, cut, w)
                assert same(p, path[torch.as_tensor(rows, device="cuda")]), (with_T, name, Lc)
                c = c.cpu().numpy()
                assert (np.abs(c - end) <= cost_bound(Lc, c) + cost_bound(Lc, end)).all(), (with_T, name, Lc)


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_a_finite_lag_is_the_reference(zh, cell):
    """At every lag of LAGS the paths equal fixed_lag exactly and the costs lie within cost_bound(L, .); the chunkings agree bit for bit
    (a long clip: whole and growing)."""
    (J, N, H, L), w = cell
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    tab, seq, worst = tables(J, N, H, L, *w), clips(N, L), 0.0
    for lag in LAGS:
        rp, rc = fixed_lag(tab, seq, lag)
        for starts, Lc in groups(N, L):
            rows, first = frames_of(starts, Lc), None
            for name, cut in chunkings(Lc).items():
                if Lc > 40 and name == "single":
                    continue
                p, c = run_clips(zh, CALL, xd, Td, ud, N, starts, Lc, lag, cut, w)
                if first is None:
                    first = (p, c)
                    err, bound = np.abs(c.cpu().numpy() - rc[rows]), cost_bound(L, rc[rows])
                    worst = max(worst, float((err / bound).max()) if bound.min() > 0 else 0.0)
                    assert np.array_equal(p.cpu().numpy(), rp[rows]), (lag, name)
                    assert (err <= bound).all(), lag
                else:
                    assert same(p, first[0]) and same(c, first[1]), (lag, name)
    print(f"joint-accel-stream J={J} N={N} H={H} L={L} ({w[0]:g}, {w[1]:g}): largest |cost - ref| / bound = {worst:.3f}")


def test_the_ring_wraps(zh):
    """(3, 130, 7, 130): one frame per push at lag 3 - a ring of 4 rows, wrapped 32 times - and lag 0 with F = max_frames = 4, a ring of
    exactly the chunk: the rows of the two frames before the chunk are reused before the scan wants their flags."""
    J, N, H, L = 3, 130, 7, 130
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for w in WEIGHTS:
        tab = tables(J, N, H, L, *w)
        for lag, cut in ((3, [1] * L), (0, [4] * 32 + [2]), (1, [4] * 32 + [2])):
            rp, rc = fixed_lag(tab, [0, L], lag)
            p, c = run_clips(zh, CALL, xd, Td, ud, N, [0], L, lag, cut, w)
            assert np.array_equal(p[0].cpu().numpy(), rp), (w, lag)
            assert (np.abs(c[0].cpu().numpy() - rc) <= cost_bound(L, rc)).all(), (w, lag)


@pytest.mark.parametrize("lag", LAGS)
def test_excluded_entries_and_a_dead_frame_joint_inside_the_lag_window(zh, lag):
    """dead_joint_case: (frame 4, joint 2) has no finite unary - a dead entry inside the lag window and a chain end before the horizon -
    and frames 2 and 6 carry a NaN and a +inf.  The reference's paths and costs under every chunking; the dead entry reports 0 and +inf;
    the other joints return the bits of the untouched unaries."""
    x, T, u, j = dead_joint_case()
    xd, Td, ud, cd = dev(x), dev(T), dev(u, torch.float64), dev(case(5, 9, 3)[2], torch.float64)
    others = [i for i in range(5) if i != j]
    for w in WEIGHTS:
        rp, rc = fixed_lag(forward(u, x, T, [0, 9], *w), [0, 9], lag)
        for name, cut in chunkings(9).items():
            p, c = run_clips(zh, CALL, xd, Td, ud, 9, [0], 9, lag, cut, w)
            p0, c0 = run_clips(zh, CALL, xd, Td, cd, 9, [0], 9, lag, cut, w)
            assert same(p[0][:, others], p0[0][:, others]) and same(c[0][:, others], c0[0][:, others])
            pn, cn = p[0].cpu().numpy(), c[0].cpu().numpy()
            assert np.array_equal(pn, rp) and pn[4, j] == 0 and np.isposinf(cn[4, j])
            ok = np.isfinite(rc)
            assert ok.sum() == 44 and np.isfinite(cn[ok]).all() and (np.abs(cn[ok] - rc[ok]) <= cost_bound(9, rc[ok])).all()


@pytest.mark.parametrize("lag", (2, 3))                             # (at least 2: nothing comes out of stream 2 before its reset)
def test_streams_are_independent_and_chains_of_one_and_two_frames(zh, lag):
    """Three streams carry different clips of dead_joint_case, one frame per push: stream 1 carries frames 3 .. 5 - joint 2's chains there
    have ONE frame each - is flushed and goes on with frames 2 .. 6 - chains of TWO frames; stream 2 is reset through d_which after two
    frames - those are dropped - and starts over; the three are flushed at different pushes, so their frame counts differ.  Each stream
    emits, bit for bit and push by push, what it emits alone; and what the reference says of its clips."""
    x, T, u, _ = dead_joint_case()
    xd, Td, ud, N, H, J, w = dev(x), dev(T), dev(u, torch.float64), 9, 3, 5, (30.0, 100.0)
    frames = [[0, 1, 2, 3, 4, 5, 6, 7], [3, 4, 5, 2, 3, 4, 5, 6], [8, 7, 0, 1, 2, 3, 4, 5]]
    flush_at = [{5, 7}, {2, 7}, {7}]
    reset_after = [set(), set(), {1}]
    all3 = each_alone(zh, CALL, xd, Td, ud, N, frames, flush_at, reset_after, lag, w)
    carried = [[[0, 1, 2, 3, 4, 5], [6, 7]], [[3, 4, 5], [2, 3, 4, 5, 6]], [[0, 1, 2, 3, 4, 5]]]
    for s in range(3):
        fr, (p, c) = all3.collected(s)
        assert fr == [f for cl in carried[s] for f in range(len(cl))]
        at = 0
        for cl in carried[s]:
            ut, xt, Tt = gather(xd, Td, ud, N, [cl])
            rp, rc = fixed_lag(forward(ut.cpu().numpy(), xt.cpu().numpy(), Tt.cpu().numpy(), [0, len(cl)], *w), [0, len(cl)], lag)
            got_p, got_c = p[at:at + len(cl)].cpu().numpy(), c[at:at + len(cl)].cpu().numpy()
            ok = np.isfinite(rc)
            assert np.array_equal(got_p, rp) and np.array_equal(np.isfinite(got_c), ok)
            assert (np.abs(got_c[ok] - rc[ok]) <= cost_bound(len(cl), rc[ok])).all()
            at += len(cl)


def test_the_bits_do_not_depend_on_the_state_the_stream_or_the_alignment(zh):
    """On BIG, two clips as two streams: a state pre-filled with 0x00 instead of 0xFF; each stream alone (the stream index); a side
    stream, the call captured and replayed twice and d_x at a 12-byte offset (launch_invariant, on reset + push + flush as one call); a
    flush with F = 0; and one F = 1 push captured into a graph and replayed L times with the inputs copied into its static tensors - a
    replay advances the state - whose concatenated emission, with that of a final flush of no frames, is the clip pushed whole."""
    (J, N, H, L), w = BIG, BIG_WEIGHTS
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lag in (3, L - 1):
        want = run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, chunkings(L)["growing"], w)
        assert all_same(run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, [L], w, fill=0x00), want)
        for k, a in enumerate((0, L)):
            got = run_clips(zh, CALL, xd, Td, ud, N, [a], L, lag, [L], w)
            assert all_same([t[0] for t in got], [t[k] for t in want])
        uu, xx, TT = gather(xd, Td, ud, N, [list(range(0, L)), list(range(L, 2 * L))])
        whole = whole_push(zh, CALL, (uu, xx, TT), 2, L, H, J, lag, w)
        ref = whole()
        torch.cuda.synchronize()
        assert all_same(ref[:-1], want) and ref[-1].tolist() == [[0, L]] * 2
        launch_invariant(ref, whole, xx)
        # d_x at the offset again, without a flush: L - lag frames come out; F = 0: the pending min(lag, L) frames
        st = Streams(zh, CALL, 2, H, J, lag, L, w)
        st.push(uu, misaligned(xx), TT, L)
        st.push(None, None, None, 0, [1, 1])
        for k in range(2):
            fr, o = st.collected(k)
            assert fr == list(range(L)) and all_same(o, [t[k] for t in want])
    # captured: one frame per replay on static tensors, lag = 3
    want = run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, 3, [L], w)
    assert all_same(replay_frame_by_frame(zh, CALL, xd, Td, ud, N, [0, L], L, 3, w), want)


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (3, 130, 7, 130), (3, 40, 64, 9)], ids=lambda v: str(v))
def test_the_degenerate_weights(zh, J, N, H, L):
    """lambda_a = 0 at a lag that covers the clip: the chain over pairs minimises what the first-order chain minimises - the paths of
    zedo_joint_stream_push at the same lambda_v.  lag = 0: every emitted h is the h of the arg-min pair of E[n] (of u at a chain's first
    frame), read from the reference."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for starts, Lc in groups(N, L):
        S = len(starts)
        chunk = gather(xd, Td, ud, N, [[a + f for f in range(Lc)] for a in starts])
        for lam in (30.0, 100.0):
            hard = zh.JointStream(S, H, J, Lc - 1, Lc, lam=lam).push(*chunk, flush=[1] * S)
            mine = zh.JointAccelStream(S, H, J, Lc - 1, Lc, lam=lam, accel=0.0).push(*chunk, flush=[1] * S)
            assert hard[1].tolist() == mine[1].tolist() == [Lc] * S and same(hard[2][:, :Lc], mine[2][:, :Lc])
        for w in WEIGHTS:
            tab = tables(J, N, H, L, *w)
            p, _ = run_clips(zh, CALL, xd, Td, ud, N, starts, Lc, 0, chunkings(Lc)["growing"], w)
            rows = frames_of(starts, Lc)
            assert np.array_equal(p.cpu().numpy(), np.where(tab["start"], tab["argq"], tab["argq"] % H)[rows])


def test_the_binding_owns_the_state(zh):
    """zh.JointAccelStream: push, flush and reset with flags given as lists or tensors; the same bits as the raw ABI; the refusals of the
    binding itself."""
    J, N, H, L, lag, w = 5, 12, 3, 4, 2, (30.0, 100.0)
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    starts = [0, 4, 8]
    want = run_clips(zh, CALL, xd, Td, ud, N, starts, L, lag, [3, 1], w)
    js = zh.JointAccelStream(3, H, J, lag, 3, lam=w[0], accel=w[1])
    assert js.state_bytes == zh.joint_accel_stream_state_bytes(3, H, J, lag, 3) == js.state.numel()
    js.push(*gather(xd, Td, ud, N, [[a] for a in starts]))           # to be dropped
    js.reset()
    chunk = gather(xd, Td, ud, N, [[a, a + 1, a + 2] for a in starts])
    f1, n1, p1, c1 = js.push(*chunk)
    assert f1.tolist() == [0] * 3 and n1.tolist() == [1] * 3 and p1.shape == (3, 3 + lag, J) and c1.dtype == torch.float64
    f2, n2, p2, c2 = js.push(*gather(xd, Td, ud, N, [[a + 3] for a in starts]), flush=torch.tensor([1, 0, 1]))
    assert f2.tolist() == [1] * 3 and n2.tolist() == [3, 1, 3]
    f3, n3, p3, c3 = js.flush([0, 1, 0])
    assert f3.tolist() == [0, 2, 0] and n3.tolist() == [0, 2, 0] and p3.shape == (3, lag, J)
    # streams 0 and 2: frame 0 at lag 2 on three frames, the rest at the flush; stream 1: frames 0 and 1 at lag 2, the rest at its flush
    for k in (0, 2):
        assert same(torch.cat([p1[k, :1], p2[k, :3]]), want[0][k]) and same(torch.cat([c1[k, :1], c2[k, :3]]), want[1][k])
    assert same(torch.cat([p1[1, :1], p2[1, :1], p3[1, :2]]), want[0][1]) and same(torch.cat([c1[1, :1], c2[1, :1], c3[1, :2]]), want[1][1])
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
        zh.JointAccelStream(1, 65, 1, 0, 1)
    assert zh.joint_accel_stream_state_bytes(1, 65, 1, 0, 1) == 0 and zh.joint_accel_stream_state_bytes(1, 64, 1, 0, 1) > 0


def test_refusals_at_the_raw_abi(zh):
    """refusal_sweep: a NULL pointer other than d_T / d_flush / d_which, every size out of range - H = 65 included - F > max_frames,
    F = 0 without d_flush, a negative lag, the index bound, a weight < 0, NaN or inf, a misaligned state: ZEDO_E_BADARG; a state one byte
    short or of no bytes: ZEDO_E_WORKSPACE; outputs and the bytes of a state in use unchanged either way, by the refusals of the reset as
    well.  The same call as it stands is accepted."""
    lib = zh._lib
    J, N, H, lag, mf, w = 5, 12, 3, 2, 4, (30.0, 100.0)
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
    more = [dict(h=1024, nbytes=2 ** 40), dict(h=64, s=2 ** 10, j=2 ** 5, lg=8, m=8, nbytes=2 ** 40)]
    refusal_sweep(call, ptrs, CALL.required(), sizes=sizes(CALL, mf) + more, weights=CALL.weights, workspace_slot=4, need=need,
                  untouched=[(t, CALL.sentinel) for t in out] + [(emit, -1), (state, use.before)])
    # the control of the sweep pushed four frames onto the two and flushed: six come out
    assert emit.tolist() == [[0, 6]] * S and bool((state[need:] == 0x5A).all()) and not torch.equal(state, use.before)
    # without T and without flush; then a flush of no frames
    assert call([P(t) for t in use.chunk2[:2]] + [None] + ptrs[3:], f=2, no_flush=True) == 0
    assert call([None, None, None] + ptrs[3:], f=0) == 0
    torch.cuda.synchronize()
    assert emit.tolist() == [[0, 2]] * S and bool((state[need:] == 0x5A).all())


def test_pipeline_push_joints_accel(zh, weights0):
    """Pipeline.push_joints_accel on the problem of load(), with a lag that covers the clips and a flush, gives the paths of
    Pipeline.select_joints_accel, bit for bit: joint_reproj's distances fed to the streaming call."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    p, k, e = pipe.select_joints_accel(xd, Td, [0, 35, N], lam=30.0, accel=100.0)
    js = pipe.open_joint_accel_stream(2, 34, 35, lam=30.0, accel=100.0)
    assert (js.S, js.H, js.J, js.lag, js.max_frames, js.lam, js.accel) == (2, H, J, 34, 35, 30.0, 100.0)
    first, count, sp, sc, jerr = pipe.push_joints_accel(js, xd, Td, flush=[1, 1])
    assert first.tolist() == [0, 0] and count.tolist() == [35, 35] and same(jerr, e)
    assert same(sp[:, :35].reshape(N, J), p)
    end = k.view(2, 35, J)[:, -1:].cpu().numpy()
    got = sc[:, :35].cpu().numpy()
    assert (np.abs(got - end) <= cost_bound(35, got) + cost_bound(35, np.broadcast_to(end, got.shape))).all()
    with pytest.raises(ValueError):
        pipe.push_joints_accel(js, xd[:N], Td[:N])
