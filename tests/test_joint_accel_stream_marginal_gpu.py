"""GPU: zedo_joint_accel_stream_marginal_push - the sum-product chain over pairs of zedo_joint_accel_marginal on live streams: frames
pushed in chunks, A2, X and l of the last lag + max_frames + 2 frames in caller-owned state, every frame's marginals formed `lag` frames
after it went in (forward and emit kernels of csrc/zedo_joint_accel_stream_marginal.hip, the dead and advance kernels of
csrc/zedo_joint_stream.hip).  Held to
  - the GPU offline call, bit for bit, where the lag covers the clip (torch.equal on the int64 view), and on truncated clips at a
    finite lag;
  - the float64 reference of tests/_joint_accel_stream_marginal_ref.py (pinned on its own in
    tests/test_joint_accel_stream_marginal_ref.py) within accel_marg_bound and the mean and covariance bounds that follow from it
    (asserted, and the difference each case shows is printed); its check_inputs() - asserted in the CPU file - leaves no arg-max in
    doubt, so hmax is compared on every live (n, j);
  - zedo_joint_accel_stream_push at a small temperature, zedo_joint_stream_marginal_push at lambda_a = 0, and itself across chunkings,
    streams, a dirty state, a side stream, the alignment of d_x, d_w given or not, and stream capture, bit for bit.
Every push of the comparisons goes through Streams: the raw ABI on a state pre-filled with 0xFF bytes and then reset, outputs pre-filled
with a sentinel; d_emit is held to the header's formula after every push and the rows past the count to the sentinel.
Whether the fused pose is closer to ground truth than any other is not measured here or anywhere: these tests hold the arithmetic.
The fusion does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, launch_invariant, misaligned, ptr as P, refusal_sweep, same
from _joint_accel_marginal_ref import COLD_CASES, COLD_TAU, WEIGHTS, accel_marg_bound
from _joint_accel_stream_marginal_ref import LAGS, SMALL, fixed_lag_accel_marginal, hold_to, reference
from _joint_accel_stream_ref import GPU_CASES
from _joint_marginal_ref import cov_bound, marg_bound, mean_bound, spread_of
from _joint_ref import case as reproj_case
from _joint_stream_marginal_ref import reference as first_order_reference
from _joint_stream_ref import chunkings
from _joint_temporal_ref import case, dead_joint_case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _stream_harness import (Streams, StreamCall, by_frame, each_alone, frames_of, gather, groups, raw_push, replay_frame_by_frame,
                             reset_refusals, run_clips, sizes, state_in_use, whole_push)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VAT = WEIGHTS[1]                                                     # (lambda_v, lambda_a, tau) = (30, 100, 1)
NAMES = ("mean", "cov", "hmax", "wmax", "logz", "w")
BIG = (17, 70, 50, 35)


def outputs(S, rows, J, H):
    f64 = lambda *tail: ((S, rows, J) + tail, torch.float64)
    return f64(3), f64(6), ((S, rows, J), torch.int32), f64(), f64(), f64(H)


CALL = StreamCall("zedo_joint_accel_stream_marginal", ("lam_v", "lam_a", "tau"), outputs, index=2, max_h=64, optional=dict(with_w=5))
FIRST_ORDER = StreamCall("zedo_joint_stream_marginal", ("lam", "tau"), outputs, index=2, max_h=1024, optional=dict(with_w=5))
COVER_CASES = GPU_CASES + [(2, 11, 4, 3)]


def offline(zh, ud, xd, Td, seq, w):
    return zh.joint_accel_marginal(ud, xd, Td, seq, lam=w[0], accel=w[1], tau=w[2], return_weights=True)


def cut_rows_match(zh, first, xd, Td, ud, N, L, lag, w):
    """For three frames of the first clip the streamed row equals the GPU offline call on the clip cut after min(n + lag, last), bit for
    bit."""
    seq = clips(N, L)
    a, Lc = seq[0], seq[1] - seq[0]
    for n in sorted({0, Lc // 2, max(0, Lc - 1 - lag)}):
        e = min(n + lag, Lc - 1)
        ut, xt, Tt = gather(xd, Td, ud, N, [list(range(a, a + e + 1))])
        for k, s, o in zip(NAMES, first, offline(zh, ut, xt, Tt, [0, e + 1], w)):
            assert same(s[a + n], o[n]), (n, e, k)


@pytest.mark.parametrize("J,N,H,L", COVER_CASES, ids=lambda v: str(v))
def test_a_lag_that_covers_the_clip_gives_the_bits_of_the_offline_call(zh, J, N, H, L):
    """lag = L - 1 and a flush at the end, pushed whole, frame by frame and in growing chunks, with T and without: all six outputs are
    those of zedo_joint_accel_marginal on the GPU, bit for bit."""
    x, T, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    for with_T in (True, False):
        Td = dev(T) if with_T else None
        ref = offline(zh, ud, xd, Td, clips(N, L), VAT)
        for name in ("whole", "single", "growing"):
            out = by_frame(zh, CALL, xd, Td, ud, N, L, L - 1, name, VAT)
            for k, a, b in zip(NAMES, out, ref):
                assert same(a, b), (with_T, name, k)


@pytest.mark.parametrize("w", WEIGHTS, ids=lambda v: str(v))
@pytest.mark.parametrize("J,N,H,L", SMALL, ids=lambda v: str(v))
def test_a_finite_lag_is_the_reference_and_the_offline_call_on_the_truncated_clip(zh, J, N, H, L, w):
    """At every lag of LAGS: hold_to against fixed_lag_accel_marginal (the derived bounds, hmax on every live entry); the three chunkings
    agree bit for bit; three rows of the first clip against the GPU offline call on the truncated clip, bit for bit."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lag in LAGS:
        first = by_frame(zh, CALL, xd, Td, ud, N, L, lag, "whole", w)
        hold_to([t.cpu().numpy() for t in first], reference(J, N, H, L, *w, lag), x, T, N, L,
                f"J={J} N={N} H={H} L={L} lag={lag} lambda_v={w[0]:g} lambda_a={w[1]:g} tau={w[2]:g}")
        for name in ("single", "growing"):
            assert all_same(by_frame(zh, CALL, xd, Td, ud, N, L, lag, name, w), first), (lag, name)
        cut_rows_match(zh, first, xd, Td, ud, N, L, lag, w)


@pytest.mark.parametrize("lag", (0, 3))
def test_the_shape_of_the_timings_is_the_offline_call_on_the_truncated_clip(zh, lag):
    """(17, 70, 50, 35) at (30, 100, 1): the numpy reference is too slow, the offline call on the truncated clip is the yardstick - three
    rows, bit for bit; the chunkings agree bit for bit."""
    J, N, H, L = BIG
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    first = by_frame(zh, CALL, xd, Td, ud, N, L, lag, "whole", VAT)
    for name in ("single", "growing"):
        assert all_same(by_frame(zh, CALL, xd, Td, ud, N, L, lag, name, VAT), first), name
    cut_rows_match(zh, first, xd, Td, ud, N, L, lag, VAT)


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (1, 20, 17, 20), (1, 6, 33, 6)], ids=lambda v: str(v))
def test_lag_zero_is_the_column_sums_of_the_softmax_of_A2(zh, J, N, H, L):
    """lag = 0: for every frame with a table, w[n,.] is the column sums of the softmax over the pairs of A2[n] - A2 read from the state's
    ring as the header lays it out (a whole clip per push, R = L + 2: frame m in row m) and held to the reference's A2, log w to the log
    of the column sums, both within accel_marg_bound."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    starts, Lc = groups(N, L)[0]
    S, R = len(starts), Lc + 2
    st = Streams(zh, CALL, S, H, J, 0, Lc, VAT)
    o, _ = st.push(*gather(xd, Td, ud, N, [[a + f for f in range(Lc)] for a in starts]), Lc)
    torch.cuda.synchronize()
    A2 = st.state[:S * J * R * H * H * 8].view(torch.float64).view(S, J, R, H, H)[:, :, 1:Lc].permute(0, 2, 1, 3, 4).cpu().numpy()   # [S, Lc-1, J, H, H]
    r = reference(J, N, H, L, *VAT, 0)
    rows = frames_of(starts, Lc)[:, 1:]
    beta = accel_marg_bound(Lc, H, r["G"])
    e_A = float(np.abs(A2 - r["A2"][rows]).max())
    flat = A2.reshape(S, Lc - 1, J, H * H).astype(np.longdouble)
    top = flat.max(-1, keepdims=True)
    cols = np.exp(flat - top).reshape(S, Lc - 1, J, H, H).sum(3)
    want = np.log(cols) - np.log(cols.sum(-1, keepdims=True))
    e_w = float(np.abs(np.log(o[5][:, 1:Lc].cpu().numpy().astype(np.longdouble)) - want).max())
    print(f"lag 0, J={J} N={N} H={H} L={Lc}: max |A2(state) - ref| = {e_A:.3e}, max |log w - log colsum softmax A2| = {e_w:.3e} (bound {beta:.3e})")
    assert e_A <= beta and e_w <= beta


@pytest.mark.parametrize("J,N,H,L", COLD_CASES, ids=lambda v: str(v))
def test_a_cold_stream_is_the_hard_stream(zh, J, N, H, L):
    """tau = 1e-9: hmax is the path of zedo_joint_accel_stream_push at the same lag and chunking, exactly, and the largest marginal stays
    at 0.99 or above: no term of a log-sum-exp has underflowed on the way (the two best entries at every horizon of these cases lie
    5.3e-4 or more apart, README.md: far above 1000 tau)."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lag in LAGS:
        for starts, Lc in groups(N, L):
            cut = chunkings(Lc)["growing"]
            o = run_clips(zh, CALL, xd, Td, ud, N, starts, Lc, lag, cut, (30.0, 100.0, COLD_TAU))
            js = zh.JointAccelStream(len(starts), H, J, lag, max(cut), lam=30.0, accel=100.0)
            path, f0 = [], 0
            for i, F in enumerate(cut):
                chunk = gather(xd, Td, ud, N, [[a + f0 + f for f in range(F)] for a in starts])
                first, count, p, _ = js.push(*chunk, flush=[1] * len(starts) if i == len(cut) - 1 else None)
                path.append(p[:, :int(count[0])])
                f0 += F
            assert same(o[2], torch.cat(path, 1)), lag
            assert float(o[3].min()) >= 0.99 and bool(torch.isfinite(o[0]).all()) and bool(torch.isfinite(o[4]).all())


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (3, 130, 7, 130)], ids=lambda v: str(v))
def test_without_the_second_order_term_it_is_the_first_order_stream(zh, J, N, H, L):
    """lambda_a = 0 at lags 0, 3 and L - 1: the outputs of zedo_joint_stream_marginal_push on the GPU - log-marginals and logZ within the
    sum of the two bounds, the mean and the covariance within what follows from that sum."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    lam, tau = 100.0, 1.0
    spread, xmax = spread_of(x, T, N)
    for lag in (0, 3, L - 1):
        one = [t.cpu().numpy() for t in by_frame(zh, FIRST_ORDER, xd, Td, ud, N, L, lag, "growing", (lam, tau))]
        two = [t.cpu().numpy() for t in by_frame(zh, CALL, xd, Td, ud, N, L, lag, "growing", (lam, 0.0, tau))]
        beta = (marg_bound(min(L, N), H, first_order_reference(J, N, H, L, lam, tau, lag)["G"])
                + accel_marg_bound(min(L, N), H, reference(J, N, H, L, lam, 0.0, tau, lag)["G"]))
        assert (one[5] > 0).all() and (two[5] > 0).all()
        e_lw = float(np.abs(np.log(two[5].astype(np.longdouble)) - np.log(one[5].astype(np.longdouble))).max())
        e_lz = float(np.abs(two[4] - one[4]).max())
        print(f"lambda_a = 0, J={J} N={N} H={H} L={L} lag={lag}: max |log w - first order| = {e_lw:.3e}, |logz| {e_lz:.3e} (sum of the bounds {beta:.3e})")
        assert e_lw <= beta and e_lz <= beta
        assert np.abs(two[0] - one[0]).max() <= mean_bound(beta, xmax)
        assert (np.abs(two[1] - one[1]) <= cov_bound(beta, spread, xmax)[:, :, None]).all()


def test_the_ring_wraps(zh):
    """(3, 130, 7, 130): one frame per push at lag 2 - a ring of 5 rows, wrapped 26 times - and at lag 1: the chain's first frame comes
    out under an open horizon, from the row sums of the pair marginals of the second; lag 0 with F = max_frames = 4, where the rows of
    the two frames before a chunk are the ring's two extra rows."""
    J, N, H, L = 3, 130, 7, 130
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lag, cut in ((2, [1] * L), (1, [1] * L), (0, [4] * 32 + [2]), (1, [4] * 32 + [2])):
        o = run_clips(zh, CALL, xd, Td, ud, N, [0], L, lag, cut, VAT)
        hold_to([t[0].cpu().numpy() for t in o], reference(J, N, H, L, *VAT, lag), x, T, N, L, f"ring: lag {lag}, {cut[0]} frame(s) per push")


@pytest.mark.parametrize("lag", (0, 1, 2, 8))
def test_excluded_entries_and_a_dead_frame_joint_inside_the_lag_window(zh, lag):
    """dead_joint_case: (frame 4, joint 2) has no finite unary - a dead entry inside the lag window, a chain end before the horizon and a
    chain start behind it - and frames 2 and 6 carry a NaN and a +inf.  The reference under every chunking; w exactly 0 where excluded;
    the dead row NaN / 0 / -inf; the chain split for that joint only; the other joints return the bits of the untouched unaries; at a
    lag that covers the clip the bits of the offline call."""
    x, T, u, j = dead_joint_case()
    xd, Td, ud, cd = dev(x), dev(T), dev(u, torch.float64), dev(case(5, 9, 3)[2], torch.float64)
    others = [i for i in range(5) if i != j]
    r = fixed_lag_accel_marginal(u, x, T, [0, 9], *VAT, lag)
    first = None
    for name, cut in chunkings(9).items():
        o = [t[0] for t in run_clips(zh, CALL, xd, Td, ud, 9, [0], 9, lag, cut, VAT)]
        o0 = [t[0] for t in run_clips(zh, CALL, xd, Td, cd, 9, [0], 9, lag, cut, VAT)]
        assert all(same(a[:, others], b[:, others]) for a, b in zip(o, o0))
        if first is None:
            first = o
            hold_to([t.cpu().numpy() for t in o], r, x, T, 9, 9, f"dead (frame 4, joint 2), lag {lag}")
        else:
            assert all_same(o, first), name
    mean, cov, hmax, wmax, logz, w = (t.cpu().numpy() for t in first)
    dead = np.zeros((9, 5), bool)
    dead[4, j] = True
    assert np.array_equal(np.isnan(mean).any(2), dead) and np.array_equal(np.isnan(cov).any(2), dead) and np.array_equal(np.isneginf(logz), dead)
    assert hmax[4, j] == 0 and wmax[4, j] == 0.0 and (w[4, j] == 0.0).all()
    excluded = ~np.isfinite(u.reshape(3, 9, 5).transpose(1, 2, 0))
    assert excluded.sum() == 5 and (w[excluded] == 0.0).all() and (w[~excluded & ~dead[:, :, None]] > 0.0).all()
    if lag == 8:                                                     # covers the clip: one log Z per chain
        assert len(set(logz[:4, j].tolist())) == 1 and len(set(logz[5:, j].tolist())) == 1 and logz[3, j] != logz[5, j]
        assert len(set(logz[:, others[0]].tolist())) == 1
        assert all_same(first, list(offline(zh, ud, xd, Td, [0, 9], VAT)))


@pytest.mark.parametrize("lag", (2, 3))                             # (at least 2: nothing comes out of stream 2 before its reset)
def test_streams_are_independent_and_chains_of_one_and_two_frames(zh, lag):
    """Three streams carry different clips of dead_joint_case, one frame per push: stream 1 carries frames 3 .. 5 - joint 2's chains there
    have ONE frame each - is flushed in mid-clip and goes on with frames 2 .. 6 - chains of TWO frames; stream 2 is reset through d_which
    after two frames - those are dropped - and starts over; the three are flushed at different pushes, so their frame counts differ.  Each
    stream emits, bit for bit and push by push, what it emits alone; and what the reference says of its clips."""
    x, T, u, _ = dead_joint_case()
    xd, Td, ud, N = dev(x), dev(T), dev(u, torch.float64), 9
    frames = [[0, 1, 2, 3, 4, 5, 6, 7], [3, 4, 5, 2, 3, 4, 5, 6], [8, 7, 0, 1, 2, 3, 4, 5]]
    flush_at = [{5, 7}, {2, 7}, {7}]
    reset_after = [set(), set(), {1}]
    all3 = each_alone(zh, CALL, xd, Td, ud, N, frames, flush_at, reset_after, lag, VAT)
    carried = [[[0, 1, 2, 3, 4, 5], [6, 7]], [[3, 4, 5], [2, 3, 4, 5, 6]], [[0, 1, 2, 3, 4, 5]]]
    for s in range(3):
        fr, o = all3.collected(s)
        assert fr == [f for cl in carried[s] for f in range(len(cl))]
        at = 0
        for cl in carried[s]:
            ut, xt, Tt = (t.cpu().numpy() for t in gather(xd, Td, ud, N, [cl]))
            r = fixed_lag_accel_marginal(ut, xt, Tt, [0, len(cl)], *VAT, lag)
            hold_to([t[at:at + len(cl)].cpu().numpy() for t in o], r, xt, Tt, len(cl), len(cl), f"stream {s}, frames {cl[0]} .. {cl[-1]}")
            at += len(cl)


def test_the_bits_do_not_depend_on_the_state_the_stream_the_alignment_or_d_w(zh):
    """On (17, 70, 50, 35), two clips as two streams: a state pre-filled with 0x00 instead of 0xFF; d_w NULL; each stream alone (the
    stream index); a side stream, the call captured and replayed twice and d_x at a 12-byte offset (launch_invariant, on reset + push +
    flush as one call); a flush with F = 0; and one F = 1 push captured into a graph on a single branch and replayed L times with the
    inputs copied into its static tensors - a replay advances the state - whose concatenated emission, with that of a final flush of no
    frames, is the clip pushed whole."""
    J, N, H, L = BIG
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    ref = [t.view(2, L, *t.shape[1:]) for t in offline(zh, ud, xd, Td, clips(N, L), VAT)]
    for lag in (3, L - 1):
        cut = chunkings(L)["growing"]
        want = run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, cut, VAT)
        if lag == L - 1:
            assert all_same(want, ref)
        assert all_same(run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, [L], VAT, fill=0x00), want)
        assert all_same(run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, cut, VAT, with_w=False)[:5], want[:5])
        for k, a in enumerate((0, L)):
            got = run_clips(zh, CALL, xd, Td, ud, N, [a], L, lag, [L], VAT)
            assert all_same([t[0] for t in got], [t[k] for t in want])
        uu, xx, TT = gather(xd, Td, ud, N, [list(range(0, L)), list(range(L, 2 * L))])
        whole = whole_push(zh, CALL, (uu, xx, TT), 2, L, H, J, lag, VAT)
        one = whole()
        torch.cuda.synchronize()
        assert all_same(one[:-1], want) and one[-1].tolist() == [[0, L]] * 2
        launch_invariant(one, whole, xx)
        # d_x at the offset again, without a flush: L - lag frames come out; F = 0: the pending min(lag, L) frames
        st = Streams(zh, CALL, 2, H, J, lag, L, VAT)
        st.push(uu, misaligned(xx), TT, L)
        st.push(None, None, None, 0, [1, 1])
        for k in range(2):
            fr, o = st.collected(k)
            assert fr == list(range(L)) and all_same(o, [t[k] for t in want])
    # captured: one frame per replay on static tensors, lag = 3
    want = run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, 3, [L], VAT)
    assert all_same(replay_frame_by_frame(zh, CALL, xd, Td, ud, N, [0, L], L, 3, VAT), want)


def test_the_binding_owns_the_state(zh):
    """zh.JointAccelMarginalStream: push, flush and reset with flags given as lists or tensors; the same bits as the raw ABI, with the
    weights and without; the refusals of the binding itself."""
    J, N, H, L, lag, w = 5, 12, 3, 4, 2, (30.0, 100.0, 0.5)
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    starts = [0, 4, 8]
    want = run_clips(zh, CALL, xd, Td, ud, N, starts, L, lag, [3, 1], w)
    js = zh.JointAccelMarginalStream(3, H, J, lag, 3, lam=w[0], accel=w[1], tau=w[2])
    assert isinstance(js, zh.JointStream) and (js.lam, js.accel, js.tau) == w
    assert js.state_bytes == zh.joint_accel_stream_marginal_state_bytes(3, H, J, lag, 3) == js.state.numel()
    js.push(*gather(xd, Td, ud, N, [[a] for a in starts]))           # to be dropped
    js.reset()
    chunk = gather(xd, Td, ud, N, [[a, a + 1, a + 2] for a in starts])
    f1, n1, *o1 = js.push(*chunk, return_weights=True)
    assert f1.tolist() == [0] * 3 and n1.tolist() == [1] * 3 and len(o1) == 6
    assert o1[0].shape == (3, 3 + lag, J, 3) and o1[1].shape == (3, 3 + lag, J, 6) and o1[2].dtype == torch.int32 and o1[5].shape == (3, 3 + lag, J, H)
    f2, n2, *o2 = js.push(*gather(xd, Td, ud, N, [[a + 3] for a in starts]), flush=torch.tensor([1, 0, 1]), return_weights=True)
    assert f2.tolist() == [1] * 3 and n2.tolist() == [3, 1, 3]
    f3, n3, *o3 = js.flush([0, 1, 0], return_weights=True)
    assert f3.tolist() == [0, 2, 0] and n3.tolist() == [0, 2, 0] and o3[0].shape == (3, lag, J, 3)
    for k in range(3):
        for i in range(6):
            rest = torch.cat([o2[i][k, :1], o3[i][k]]) if k == 1 else o2[i][k, :3]
            assert same(torch.cat([o1[i][k, :1], rest]), want[i][k]), (k, NAMES[i])
    f4, n4, *o4 = js.flush()
    assert n4.tolist() == [0, 0, 0] and f4.tolist() == [0, 0, 0] and len(o4) == 5
    with pytest.raises(ValueError):
        js.push(chunk[0][:-1], chunk[1], chunk[2])
    with pytest.raises(ValueError):
        js.push(chunk[0], chunk[1], chunk[2], flush=[1, 0])
    with pytest.raises(ValueError):
        js.push(None, None, None)
    with pytest.raises(zh.ZedoError):
        js.push(*gather(xd, Td, ud, N, [[a, a + 1, a + 2, a + 3] for a in starts]))      # F > max_frames
    with pytest.raises(zh.ZedoError, match="H <= 64"):
        zh.JointAccelMarginalStream(1, 65, 1, 0, 1)
    with pytest.raises(zh.ZedoError):
        zh.JointAccelMarginalStream(3, H, J, lag, 3, tau=0.0).push(*chunk)
    assert zh.joint_accel_stream_marginal_state_bytes(1, 65, 1, 0, 1) == 0 and zh.joint_accel_stream_marginal_state_bytes(1, 64, 1, 0, 1) > 0
    # lag = 0 and a push of no frames has no output rows: flush() still ends the clip, and the next frame is frame 0 of a new one
    js0 = zh.JointAccelMarginalStream(2, H, J, 0, 1)
    one = lambda f: gather(xd, Td, ud, N, [[f], [f + 4]])
    first, count, *o = js0.push(*one(0))
    js0.push(*one(1))
    f5, n5, *o5 = js0.flush([1, 0])
    assert n5.tolist() == [0, 0] and all(t.shape[1] == 0 for t in o5)
    f6, n6, *o6 = js0.push(*one(0))
    assert f6.tolist() == [0, 2] and n6.tolist() == [1, 1] and all(same(a[0], b[0]) for a, b in zip(o6, o))


def test_refusals_at_the_raw_abi(zh):
    """refusal_sweep: a NULL pointer other than d_T / d_w / d_flush / d_which, every size out of range - H = 65 included - F >
    max_frames, F = 0 without d_flush, a negative lag, the index bound, a weight < 0, NaN or inf, tau of 0, negative, NaN and inf, a
    misaligned state: ZEDO_E_BADARG; a state one byte short or of no bytes: ZEDO_E_WORKSPACE; outputs and the bytes of a state in use
    unchanged either way, by the refusals of the reset as well.  The same call as it stands is accepted."""
    lib = zh._lib
    J, N, H, lag, mf, w = 5, 12, 3, 2, 4, (30.0, 100.0, 0.5)
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
    more = [dict(h=1024, nbytes=2 ** 40), dict(h=64, s=2 ** 10, j=2 ** 5, lg=8, m=6, nbytes=2 ** 40)]
    refusal_sweep(call, ptrs, CALL.required(), sizes=sizes(CALL, mf) + more, weights=("lam_v", "lam_a"), taus=("tau",), workspace_slot=4,
                  need=need, untouched=[(t, CALL.sentinel) for t in out] + [(emit, -1), (state, use.before)])
    # the control of the sweep pushed four frames onto the two and flushed: six come out
    assert emit.tolist() == [[0, 6]] * S and bool((state[need:] == 0x5A).all()) and not torch.equal(state, use.before)
    # without T, without d_w and without flush; then a flush of no frames
    assert call([P(t) for t in use.chunk2[:2]] + [None] + ptrs[3:10] + [None, ptrs[11]], f=2, no_flush=True) == 0
    assert call([None, None, None] + ptrs[3:], f=0) == 0
    torch.cuda.synchronize()
    assert emit.tolist() == [[0, 2]] * S and bool((state[need:] == 0x5A).all())


def test_pipeline_push_fuse_joints_accel(zh, weights0):
    """Pipeline.push_fuse_joints_accel on the problem of load(), with a lag that covers the clips and a flush, is
    Pipeline.fuse_joints_accel, bit for bit: joint_reproj's distances fed to the streaming call."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    ref = pipe.fuse_joints_accel(xd, Td, [0, 35, N], lam=30.0, accel=100.0, tau=0.5)
    js = pipe.open_joint_accel_fuse_stream(2, 34, 35, lam=30.0, accel=100.0, tau=0.5)
    assert (js.S, js.H, js.J, js.lag, js.max_frames, js.lam, js.accel, js.tau) == (2, H, J, 34, 35, 30.0, 100.0, 0.5)
    first, count, *out = pipe.push_fuse_joints_accel(js, xd, Td, flush=[1, 1])
    assert first.tolist() == [0, 0] and count.tolist() == [35, 35] and len(out) == 6 and same(out[5], ref[5])
    for a, b in zip(out[:5], ref[:5]):
        assert same(a[:, :35].reshape(b.shape), b)
    with pytest.raises(ValueError):
        pipe.push_fuse_joints_accel(js, xd[:N], Td[:N])
    with pytest.raises(ValueError):
        pipe.push_fuse_joints_accel(pipe.open_joint_accel_fuse_stream(3, 1, 35), xd, Td)
