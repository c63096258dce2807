"""GPU: zedo_joint_stream_marginal_push - the sum-product chain of zedo_joint_marginal on live streams: frames pushed in chunks, A, X and
l of the last lag + max_frames frames in caller-owned state, every frame's marginals formed `lag` frames after it went in (forward and
emit kernels of csrc/zedo_joint_stream_marginal.hip, the dead and advance kernels of csrc/zedo_joint_stream.hip).  Held to
  - the GPU offline call, bit for bit, where the lag covers the clip (torch.equal on the int64 view), and on truncated clips at a
    finite lag;
  - the float64 reference of tests/_joint_stream_marginal_ref.py (pinned on its own in tests/test_joint_stream_marginal_ref.py) within
    the derived bounds of _joint_marginal_ref (marg_bound, mean_bound, cov_bound; asserted, and the difference each case shows is
    printed); its check_inputs() - asserted in the CPU file - leaves no arg-max in doubt, so hmax is compared on every live (n, j);
  - zedo_joint_stream_push at a small temperature, and itself across chunkings, streams, a dirty state, a side stream, the alignment of
    d_x, d_w given or not, and stream capture, bit for bit.
Every push of the comparisons goes through Streams: the raw ABI on a state pre-filled with 0xFF bytes and then reset, outputs pre-filled
with a sentinel; d_emit is held to the header's formula after every push and the rows past the count to the sentinel.
Whether the fused pose is closer to ground truth than a selected one is not measured here or anywhere: these tests hold the arithmetic.
The fusion does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, launch_invariant, misaligned, ptr as P, refusal_sweep, same
from _joint_marginal_ref import IDS, MARGINAL_CASES, joint_marginal_ref, marg_bound, softmax_bound, softmax_ref
from _joint_ref import case as reproj_case
from _joint_stream_marginal_ref import FINITE_CASES, LAGS, fixed_lag_marginal, hold_to, reference
from _joint_stream_ref import chunkings
from _joint_temporal_ref import case, dead_joint_case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _stream_harness import (Streams, StreamCall, by_frame, each_alone, frames_of, gather, groups, raw_push, replay_frame_by_frame,
                             reset_refusals, run_clips, sizes, state_in_use, whole_push)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAM, TAU = 100.0, 1.0
LT = (LAM, TAU)
NAMES = ("mean", "cov", "hmax", "wmax", "logz", "w")


def outputs(S, rows, J, H):
    f64 = lambda *tail: ((S, rows, J) + tail, torch.float64)
    return f64(3), f64(6), ((S, rows, J), torch.int32), f64(), f64(), f64(H)


CALL = StreamCall("zedo_joint_stream_marginal", ("lam", "tau"), outputs, index=2, max_h=1024, optional=dict(with_w=5))


@pytest.mark.parametrize("J,N,H,L", MARGINAL_CASES, ids=IDS)
def test_a_lag_that_covers_the_clip_gives_the_bits_of_the_offline_call(zh, J, N, H, L):
    """lag = L - 1 and a flush at the end, pushed whole, frame by frame and in growing chunks, with T and without: all six outputs are
    those of zedo_joint_marginal on the GPU, bit for bit."""
    x, T, u = case(J, N, H)
    xd, ud = dev(x), dev(u, torch.float64)
    for with_T in (True, False):
        Td = dev(T) if with_T else None
        ref = zh.joint_marginal(ud, xd, Td, clips(N, L), lam=LAM, tau=TAU, return_weights=True)
        for name in ("whole", "single", "growing"):
            out = by_frame(zh, CALL, xd, Td, ud, N, L, L - 1, name, LT)
            for k, a, b in zip(NAMES, out, ref):
                assert same(a, b), (with_T, name, k)


FINITE = [c + (LAM, TAU) for c in FINITE_CASES] + [(17, 70, 50, 35, 30.0, 0.25), (2, 30, 130, 13, 30.0, 0.25)]


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("J,N,H,L,lam,tau", FINITE, ids=lambda v: str(v))
def test_a_finite_lag_is_the_reference_and_the_offline_call_on_the_truncated_clip(zh, J, N, H, L, lam, tau, lag):
    """hold_to against fixed_lag_marginal (the derived bounds, hmax on every live entry); the three chunkings agree bit for bit; for
    three frames of the first clip the row equals the GPU offline call on the clip cut after min(n + lag, last), bit for bit."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    first = by_frame(zh, CALL, xd, Td, ud, N, L, lag, "whole", (lam, tau))
    hold_to([t.cpu().numpy() for t in first], reference(J, N, H, L, lam, tau, lag), x, T, N, L,
            f"J={J} N={N} H={H} L={L} lag={lag} lambda={lam:g} tau={tau:g}")
    for name in ("single", "growing"):
        assert all_same(by_frame(zh, CALL, xd, Td, ud, N, L, lag, name, (lam, tau)), first), name
    seq = clips(N, L)
    a, Lc = seq[0], seq[1] - seq[0]
    for n in sorted({0, Lc // 2, max(0, Lc - 1 - lag)}):
        e = min(n + lag, Lc - 1)
        ut, xt, Tt = gather(xd, Td, ud, N, [list(range(a, a + e + 1))])
        off = zh.joint_marginal(ut, xt, Tt, [0, e + 1], lam=lam, tau=tau, return_weights=True)
        for k, s, o in zip(NAMES, first, off):
            assert same(s[a + n], o[n]), (n, e, k)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (2, 30, 130, 13), (1, 6, 300, 3)], ids=lambda v: str(v))
def test_lag_zero_is_a_softmax_of_A_and_lambda_zero_a_softmax_of_the_unaries(zh, J, N, H, L):
    """lag = 0: the marginals are the softmax of A[n,j,.] - A read from the state's ring as the header lays it out (a whole clip per
    push: frame m in row m) and held to the reference's A, log w to A - LSE A, both within marg_bound.  lambda = 0 at any lag: the
    per-(frame, joint) softmax of -u / tau in closed form, within softmax_bound."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    starts, Lc = groups(N, L)[0]
    S = len(starts)
    st = Streams(zh, CALL, S, H, J, 0, Lc, LT)
    uu, xx, TT = gather(xd, Td, ud, N, [[a + f for f in range(Lc)] for a in starts])
    o, _ = st.push(uu, xx, TT, Lc)
    torch.cuda.synchronize()
    A = st.state[:S * J * Lc * H * 8].view(torch.float64).view(S, J, Lc, H).permute(0, 2, 1, 3).cpu().numpy()      # [S, Lc, J, H]
    r = reference(J, N, H, L, LAM, TAU, 0)
    rows = frames_of(starts, Lc)
    beta = marg_bound(Lc, H, r["G"])
    e_A = float(np.abs(A - r["A"][rows]).max())
    w, logz = o[5].cpu().numpy(), o[4].cpu().numpy()
    e_w = float(np.abs(np.log(w.astype(np.longdouble)) - (A - logz[..., None])).max())
    print(f"lag 0, J={J} N={N} H={H} L={Lc}: max |A(state) - ref| = {e_A:.3e}, max |log w - (A - logZ)| = {e_w:.3e} (bound {beta:.3e})")
    assert e_A <= beta and e_w <= beta
    sm = softmax_ref(u, N, TAU)
    sb = softmax_bound(L, H, joint_marginal_ref(u, x, T, clips(N, L), 0.0, TAU)["G"], np.log(sm))
    for lag in (0, 3):
        w0 = by_frame(zh, CALL, xd, Td, ud, N, L, lag, "growing", (0.0, TAU))[5].cpu().numpy()
        e = float(np.abs(np.log(w0.astype(np.longdouble)) - np.log(sm)).max())
        print(f"lambda 0, lag {lag}, J={J} N={N} H={H}: max |log w - log softmax| = {e:.3e} (bound {sb:.3e})")
        assert e <= sb


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (2, 30, 130, 13), (3, 130, 7, 130)], ids=lambda v: str(v))
def test_a_cold_stream_is_the_hard_stream(zh, J, N, H, L):
    """tau = 1e-9: the gaps of _joint_stream_ref.check_inputs (1e-6 between the two best entries of D at every live (n, j)) are
    >= 1000 tau, so hmax is the path of zedo_joint_stream_push at the same lag and chunking, exactly, and the largest marginal stays
    above 0.999: no term of a log-sum-exp has underflowed on the way."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lag in LAGS:
        for starts, Lc in groups(N, L):
            cut = chunkings(Lc)["growing"]
            o = run_clips(zh, CALL, xd, Td, ud, N, starts, Lc, lag, cut, (LAM, 1e-9))
            js = zh.JointStream(len(starts), H, J, lag, max(cut), lam=LAM)
            path, f0 = [], 0
            for i, F in enumerate(cut):
                chunk = gather(xd, Td, ud, N, [[a + f0 + f for f in range(F)] for a in starts])
                first, count, p, _ = js.push(*chunk, flush=[1] * len(starts) if i == len(cut) - 1 else None)
                path.append(p[:, :int(count[0])])
                f0 += F
            assert same(o[2], torch.cat(path, 1)), lag
            assert float(o[3].min()) > 0.999 and bool(torch.isfinite(o[0]).all()) and bool(torch.isfinite(o[4]).all())


def test_streams_are_independent(zh):
    """Three streams carry different clips of (5, 12, 3), one frame per push at lag 2: stream 1 is flushed mid-way and goes on with
    another clip, stream 2 is reset through d_which after two frames - those are dropped - and starts over.  Each stream emits, bit for
    bit and push by push, what it emits alone; and what the reference says of its clips."""
    J, N, H, lag = 5, 12, 3, 2
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    frames = [[0, 1, 2, 3, 4, 5, 6, 7], [4, 5, 6, 7, 8, 9, 10, 11], [8, 9, 0, 1, 2, 3, 4, 5]]
    flush_at = [{7}, {3, 7}, {7}]
    reset_after = [set(), set(), {1}]
    all3 = each_alone(zh, CALL, xd, Td, ud, N, frames, flush_at, reset_after, lag, LT)
    carried = [[list(range(0, 8))], [list(range(4, 8)), list(range(8, 12))], [list(range(0, 6))]]
    for s in range(3):
        fr, o = all3.collected(s)
        assert fr == [f for cl in carried[s] for f in range(len(cl))]
        at = 0
        for cl in carried[s]:
            ut, xt, Tt = (t.cpu().numpy() for t in gather(xd, Td, ud, N, [cl]))
            r = fixed_lag_marginal(ut, xt, Tt, [0, len(cl)], LAM, TAU, lag)
            hold_to([t[at:at + len(cl)].cpu().numpy() for t in o], r, xt, Tt, len(cl), len(cl), f"stream {s}, frames {cl[0]} .. {cl[-1]}")
            at += len(cl)


@pytest.mark.parametrize("lag", (0, 1, 2, 8))
def test_excluded_entries_and_a_dead_frame_joint_inside_the_lag_window(zh, lag):
    """dead_joint_case: (frame 4, joint 2) has no finite unary - a dead entry inside the lag window and a chain end before the horizon -
    and frames 2 and 6 carry a NaN and a +inf.  The reference under every chunking; w exactly 0 where excluded; the dead row NaN / 0 /
    -inf; the chain split for that joint only (two values of logz at lag 8); the other joints return the bits of the untouched unaries."""
    x, T, u, j = dead_joint_case()
    xd, Td, ud, cd = dev(x), dev(T), dev(u, torch.float64), dev(case(5, 9, 3)[2], torch.float64)
    others = [i for i in range(5) if i != j]
    r = fixed_lag_marginal(u, x, T, [0, 9], LAM, TAU, lag)
    first = None
    for name, cut in chunkings(9).items():
        o = [t[0] for t in run_clips(zh, CALL, xd, Td, ud, 9, [0], 9, lag, cut, LT)]
        o0 = [t[0] for t in run_clips(zh, CALL, xd, Td, cd, 9, [0], 9, lag, cut, LT)]
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
        off = zh.joint_marginal(ud, xd, Td, [0, 9], lam=LAM, tau=TAU, return_weights=True)
        assert all_same(first, list(off))


def test_the_bits_do_not_depend_on_the_state_the_stream_the_alignment_or_d_w(zh):
    """A state pre-filled with 0x00 instead of 0xFF; d_w NULL; a side stream, the call captured and replayed twice and d_x at a 12-byte
    offset (launch_invariant, on reset + push + flush as one call); a flush with F = 0; and one F = 1 push captured into a graph on a
    single branch and replayed L times with the inputs copied into its static tensors - a replay advances the state - whose concatenated
    emission, with that of a final flush of no frames, is the offline call."""
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    ref = [t.view(2, L, *t.shape[1:]) for t in zh.joint_marginal(ud, xd, Td, clips(N, L), lam=LAM, tau=TAU, return_weights=True)]
    for lag in (3, L - 1):
        cut = chunkings(L)["growing"]
        want = run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, cut, LT)
        if lag == L - 1:
            assert all_same(want, ref)
        assert all_same(run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, cut, LT, fill=0x00), want)
        assert all_same(run_clips(zh, CALL, xd, Td, ud, N, [0, L], L, lag, cut, LT, with_w=False)[:5], want[:5])
        uu, xx, TT = gather(xd, Td, ud, N, [list(range(0, L)), list(range(L, 2 * L))])
        whole = whole_push(zh, CALL, (uu, xx, TT), 2, L, H, J, lag, LT)
        one = whole()
        torch.cuda.synchronize()
        assert all_same(one[:-1], want) and one[-1].tolist() == [[0, L]] * 2
        launch_invariant(one, whole, xx)
        # d_x at the offset again, without a flush: L - lag frames come out; F = 0: the pending min(lag, L) frames
        st = Streams(zh, CALL, 2, H, J, lag, L, LT)
        st.push(uu, misaligned(xx), TT, L)
        st.push(None, None, None, 0, [1, 1])
        for k in range(2):
            fr, o = st.collected(k)
            assert fr == list(range(L)) and all_same(o, [t[k] for t in want])
    # captured: one frame per replay on static tensors, lag = L - 1
    assert all_same(replay_frame_by_frame(zh, CALL, xd, Td, ud, N, [0, L], L, L - 1, LT), ref)


def test_the_binding_owns_the_state(zh):
    """zh.JointMarginalStream: push, flush and reset with flags given as lists or tensors; the same bits as the raw ABI, with the
    weights and without; the refusals of the binding itself."""
    J, N, H, L, lag, lam, tau = 5, 12, 3, 4, 2, 30.0, 0.5
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    starts = [0, 4, 8]
    want = run_clips(zh, CALL, xd, Td, ud, N, starts, L, lag, [3, 1], (lam, tau))
    js = zh.JointMarginalStream(3, H, J, lag, 3, lam=lam, tau=tau)
    assert js.state_bytes == zh.joint_stream_marginal_state_bytes(3, H, J, lag, 3) == js.state.numel()
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
    with pytest.raises(zh.ZedoError):
        zh.JointMarginalStream(1, 1025, 1, 0, 1)
    with pytest.raises(zh.ZedoError):
        zh.JointMarginalStream(3, H, J, lag, 3, tau=0.0).push(*chunk)
    assert zh.joint_stream_marginal_state_bytes(1, 1025, 1, 0, 1) == 0


def test_the_binding_ends_a_clip_without_frames_at_lag_zero(zh):
    """lag = 0 and a push of no frames has no output rows: the binding still hands the entry point pointers that are not NULL, so
    flush() ends the clip - nothing comes out, and the next frame is frame 0 of a new clip.  The hard stream's binding as well."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    one = lambda f: gather(xd, Td, ud, N, [[f], [f + 4]])
    for js in (zh.JointMarginalStream(2, H, J, 0, 1), zh.JointStream(2, H, J, 0, 1)):
        first, count, *o = js.push(*one(0))
        assert first.tolist() == [0, 0] and count.tolist() == [1, 1]
        f1, n1, *o1 = js.push(*one(1))
        assert f1.tolist() == [1, 1]
        f2, n2, *o2 = js.flush([1, 0])
        assert n2.tolist() == [0, 0] and all(t.shape[1] == 0 for t in o2)
        f3, n3, *o3 = js.push(*one(0))
        assert f3.tolist() == [0, 2] and n3.tolist() == [1, 1]
        assert all(same(a[0], b[0]) for a, b in zip(o3, o))          # stream 0 started over: frame 0 of the same clip again


def test_refusals_at_the_raw_abi(zh):
    """refusal_sweep: a NULL pointer other than d_T / d_w / d_flush / d_which, every size out of range - H = 1025 included - F >
    max_frames, F = 0 without d_flush, a negative lag, lambda < 0, NaN or inf, tau of 0, negative, NaN and inf, a misaligned state:
    ZEDO_E_BADARG; a state one byte short or of no bytes: ZEDO_E_WORKSPACE; outputs and the bytes of a state in use unchanged either way,
    by the refusals of the reset as well.  The same call as it stands is accepted."""
    lib = zh._lib
    J, N, H, lag, mf = 5, 12, 3, 2, 4
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    S, F, starts = 3, 4, (0, 4, 8)
    uu, xx, TT = gather(xd, Td, ud, N, [list(range(a, a + F)) for a in starts])
    use = state_in_use(zh, CALL, xd, Td, ud, N, starts, lag, mf, LT)  # two frames per stream
    state, need = use.state, use.need
    out, emit = CALL.blank(S, F + lag, J, H), torch.full((S, 2), -1, dtype=torch.int64, device="cuda")
    fl = torch.ones(S, dtype=torch.int32, device="cuda")
    ptrs = [P(uu), P(xx), P(TT), P(fl), P(state)] + [P(t) for t in out] + [P(emit)]
    call = raw_push(lib, CALL, ptrs, S, F, H, J, lag, mf, LT, need)
    reset_refusals(lib, CALL, use, S, H, J, lag, mf)
    refusal_sweep(call, ptrs, CALL.required(), sizes=sizes(CALL, mf), weights=("lam",), taus=("tau",), workspace_slot=4, need=need,
                  untouched=[(t, CALL.sentinel) for t in out] + [(emit, -1), (state, use.before)])
    # the control of the sweep pushed four frames onto the two and flushed: six come out
    assert emit.tolist() == [[0, 6]] * S and bool((state[need:] == 0x5A).all()) and not torch.equal(state, use.before)
    # without T, without d_w and without flush; then a flush of no frames
    assert call([P(t) for t in use.chunk2[:2]] + [None] + ptrs[3:10] + [None, ptrs[11]], f=2, no_flush=True) == 0
    assert call([None, None, None] + ptrs[3:], f=0) == 0
    torch.cuda.synchronize()
    assert emit.tolist() == [[0, 2]] * S and bool((state[need:] == 0x5A).all())


def test_pipeline_push_fuse_joints_temporal(zh, weights0):
    """Pipeline.push_fuse_joints_temporal on the problem of load(), with a lag that covers the clips and a flush, is
    Pipeline.fuse_joints_temporal, bit for bit: joint_reproj's distances fed to the streaming call."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    ref = pipe.fuse_joints_temporal(xd, Td, [0, 35, N], lam=30.0, tau=0.5)
    js = pipe.open_joint_fuse_stream(2, 34, 35, lam=30.0, tau=0.5)
    assert (js.S, js.H, js.J, js.lag, js.max_frames, js.lam, js.tau) == (2, H, J, 34, 35, 30.0, 0.5)
    first, count, *out = pipe.push_fuse_joints_temporal(js, xd, Td, flush=[1, 1])
    assert first.tolist() == [0, 0] and count.tolist() == [35, 35] and len(out) == 6 and same(out[5], ref[5])
    for a, b in zip(out[:5], ref[:5]):
        assert same(a[:, :35].reshape(b.shape), b)
    with pytest.raises(ValueError):
        pipe.push_fuse_joints_temporal(js, xd[:N], Td[:N])
    with pytest.raises(ValueError):
        pipe.push_fuse_joints_temporal(pipe.open_joint_fuse_stream(3, 1, 35), xd, Td)
