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
import ctypes

import numpy as np
import pytest

from _invariance import cur_stream, dirty, misaligned, ptr as P, same, sentinels
from _joint_ref import case as reproj_case
from _joint_stream_ref import LAGS, check_inputs, chunkings, emitted, fixed_lag
from _joint_temporal_ref import ALL_CASES, IDS, LAMBDAS, case, dead_joint_case, joint_temporal_ref, reference
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_ref import clips, cost_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT_P, SENT_C = -7, -7.0


def gather(xd, Td, ud, N, frames):
    """frames [S][F]: the frame of the case every stream pushes -> the chunk's (u, x, T), rows (h, n) h-major with n = s F + f."""
    H = xd.shape[0] // N
    fr = torch.tensor(frames, dtype=torch.int64, device="cuda")
    rows = (torch.arange(H, device="cuda")[:, None, None] * N + fr[None]).reshape(-1)
    return ud[rows].contiguous(), xd[rows].contiguous(), None if Td is None else Td[rows].contiguous()


class Streams:
    """S streams at the raw ABI: the state pre-filled with `fill` bytes and then reset; every push checks its return code, and - after
    one synchronisation - d_emit against the header's formula and the rows past the count against the sentinel.  out[s]: the (clip-local
    frame, path row [J], cost row [J]) this stream has emitted, in order, on the device."""

    def __init__(self, zh, S, H, J, lag, max_frames, lam, fill=0xFF):
        self.lib, self.S, self.H, self.J, self.lag, self.mf, self.lam = zh._lib, S, H, J, lag, max_frames, lam
        self.nbytes = self.lib.zedo_joint_stream_state_bytes(S, H, J, lag, max_frames)
        assert self.nbytes > 0
        self.state = dirty(self.nbytes, fill)
        self.t = [0] * S
        self.out = [[] for _ in range(S)]
        self.reset()

    def reset(self, which=None):
        w = None if which is None else torch.tensor(which, dtype=torch.int32, device="cuda")
        assert self.lib.zedo_joint_stream_reset(P(self.state), self.nbytes, self.S, self.H, self.J, self.lag, self.mf, P(w), cur_stream()) == 0
        for s in range(self.S):
            if which is None or which[s]:
                self.t[s] = 0

    def push(self, u, x, T, F, flush=None):
        S, J, lag = self.S, self.J, self.lag
        fl = None if flush is None else torch.tensor(flush, dtype=torch.int32, device="cuda")
        path, cost = sentinels((((S, F + lag, J), torch.int32), ((S, F + lag, J), torch.float64)), SENT_P)
        emit = torch.full((S, 2), -1, dtype=torch.int64, device="cuda")
        rc = self.lib.zedo_joint_stream_push(P(u), P(x), P(T), S, F, self.H, J, lag, self.mf, self.lam, P(fl), P(self.state), self.nbytes,
                                             P(path), P(cost), P(emit), cur_stream())
        assert rc == 0, rc
        want = [emitted(self.t[s], F, lag, bool(flush and flush[s])) for s in range(S)]
        assert emit.cpu().tolist() == [list(w) for w in want], (emit.cpu().tolist(), want)
        for s, (first, count) in enumerate(want):
            assert bool((path[s, count:] == SENT_P).all()) and bool((cost[s, count:] == SENT_C).all())
            assert bool((path[s, :count] >= 0).all()) and bool((path[s, :count] < self.H).all())
            self.out[s] += [(first + r, path[s, r], cost[s, r]) for r in range(count)]
            self.t[s] = 0 if flush and flush[s] else self.t[s] + F
        return path, cost, emit

    def collected(self, s):
        """(frames [n], path [n,J], cost [n,J]) of everything stream s has emitted."""
        o = self.out[s]
        return [f for f, _, _ in o], torch.stack([p for _, p, _ in o]), torch.stack([c for _, _, c in o])


def run_clips(zh, xd, Td, ud, N, starts, L, lag, cut, lam, **kw):
    """The clips [a, a + L) for a in starts as len(starts) streams, pushed in chunks of cut[i] frames with a flush at the end ->
    (path [S,L,J] i32, cost [S,L,J] f64) on the device."""
    S, H, J = len(starts), xd.shape[0] // N, xd.shape[1]
    st = Streams(zh, S, H, J, lag, max(cut), lam, **kw)
    f0 = 0
    for i, F in enumerate(cut):
        u, x, T = gather(xd, Td, ud, N, [[a + f0 + f for f in range(F)] for a in starts])
        st.push(u, x, T, F, [1] * S if i == len(cut) - 1 else None)
        f0 += F
    outs = [st.collected(s) for s in range(S)]
    assert all(o[0] == list(range(L)) for o in outs)                 # every frame once, in order
    return torch.stack([o[1] for o in outs]), torch.stack([o[2] for o in outs])


def groups(N, L):
    """The clips of clips(N, L) as groups of equal length: [(starts, length)] - the equal ones as streams of one call, a shorter last one
    on its own."""
    seq = clips(N, L)
    full = [a for a, b in zip(seq[:-1], seq[1:]) if b - a == L]
    out = [(full, L)] if full else []
    if seq[-1] - seq[-2] != L:
        out.append(([seq[-2]], seq[-1] - seq[-2]))
    return out


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
            rows = torch.tensor([[a + f for f in range(Lc)] for a in starts], device="cuda")
            for name, cut in chunkings(Lc).items():
                p, c = run_clips(zh, xd, Td, ud, N, starts, Lc, L - 1, cut, lam)
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
            rows = np.array([[a + f for f in range(Lc)] for a in starts])
            first = None
            for name, cut in chunkings(Lc).items():
                p, c = run_clips(zh, xd, Td, ud, N, starts, Lc, lag, cut, lam)
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
                p, c = run_clips(zh, xd, Td, ud, N, [a], Lc, lag, [Lc], lam)
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

    def run(members):
        st = Streams(zh, len(members), H, J, lag, 1, lam)
        per_push = []
        for i in range(8):
            uu, xx, TT = gather(xd, Td, ud, N, [[frames[s][i]] for s in members])
            fl = [1 if i in flush_at[s] else 0 for s in members]
            p, c, e = st.push(uu, xx, TT, 1, fl if any(fl) else None)
            per_push.append((p, c, e))
            rs = [1 if i in reset_after[s] else 0 for s in members]
            if any(rs):
                st.reset(rs)
        return st, per_push

    all3, pushes3 = run([0, 1, 2])
    for s in range(3):
        alone, pushes1 = run([s])
        for (p3, c3, e3), (p1, c1, e1) in zip(pushes3, pushes1):
            assert same(p3[s:s + 1], p1) and same(c3[s:s + 1], c1) and same(e3[s:s + 1], e1)
    # the clips each stream carried, in the order it emitted them: (frames of the case, ...)
    carried = [[list(range(0, 8))], [list(range(4, 8)), list(range(8, 12))], [list(range(0, 6))]]
    for s in range(3):
        fr, p, c = all3.collected(s)
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
            p, c = run_clips(zh, xd, Td, ud, 9, [0], 9, lag, cut, lam)
            p0, c0 = run_clips(zh, xd, Td, cd, 9, [0], 9, lag, cut, lam)
            assert same(p[0][:, others], p0[0][:, others]) and same(c[0][:, others], c0[0][:, others])
            pn, cn = p[0].cpu().numpy(), c[0].cpu().numpy()
            assert np.array_equal(pn, rp) and pn[4, j] == 0 and np.isposinf(cn[4, j])
            ok = np.isfinite(rc)
            assert ok.sum() == 44 and np.isfinite(cn[ok]).all() and (np.abs(cn[ok] - rc[ok]) <= cost_bound(1, 9, rc[ok])).all()
            if lam == 100.0 and lag in (0, 8):
                assert pn[:, j].tolist() == ([0, 0, 0, 1, 0, 2, 0, 0, 0] if lag == 0 else [1, 1, 1, 1, 0, 0, 0, 0, 0])


def test_the_bits_do_not_depend_on_the_state_the_stream_or_the_alignment(zh):
    """A state pre-filled with 0x00 instead of 0xFF; a side stream; d_x at a 12-byte offset; a flush with F = 0; and one F = 1 push
    captured into a graph on a single branch and replayed L times with the inputs copied into its static tensors - a replay advances the
    state - whose concatenated emission, with that of a final flush of no frames, is the offline call."""
    J, N, H, L, lam = 17, 70, 50, 35, 100.0
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    path, cost = zh.joint_temporal_select(ud, xd, Td, clips(N, L), lam=lam)
    for lag in (3, L - 1):
        cut = chunkings(L)["growing"]
        want = run_clips(zh, xd, Td, ud, N, [0, L], L, lag, cut, lam)
        if lag == L - 1:
            assert same(want[0], path.view(2, L, J)) and same(want[1], cost.view(2, L, J))
        got = run_clips(zh, xd, Td, ud, N, [0, L], L, lag, cut, lam, fill=0x00)
        assert same(got[0], want[0]) and same(got[1], want[1])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = run_clips(zh, xd, Td, ud, N, [0, L], L, lag, cut, lam)
        torch.cuda.synchronize()
        assert same(got[0], want[0]) and same(got[1], want[1])
        # d_x 12 bytes past a 16-byte boundary, pushed whole
        st = Streams(zh, 2, H, J, lag, L, lam)
        uu, xx, TT = gather(xd, Td, ud, N, [list(range(0, L)), list(range(L, 2 * L))])
        st.push(uu, misaligned(xx), TT, L)                                        # no flush: L - lag frames come out
        st.push(None, None, None, 0, [1, 1])                          # F = 0: the pending min(lag, L) frames
        for k in range(2):
            fr, p, c = st.collected(k)
            assert fr == list(range(L)) and same(p, want[0][k]) and same(c, want[1][k])
    # captured: one frame per replay on static tensors, lag = L - 1
    lag = L - 1
    st = Streams(zh, 2, H, J, lag, 1, lam)
    su, sx, sT = (t.clone() for t in gather(xd, Td, ud, N, [[0], [L]]))
    op, oc = sentinels((((2, 1 + lag, J), torch.int32), ((2, 1 + lag, J), torch.float64)), SENT_P)
    oe = torch.full((2, 2), -1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = st.lib.zedo_joint_stream_push(P(su), P(sx), P(sT), 2, 1, H, J, lag, 1, lam, None, P(st.state), st.nbytes, P(op), P(oc), P(oe),
                                           cur_stream())
    assert rc == 0
    got_p, got_c = [[], []], [[], []]
    for f in range(L):
        for dst, src in zip((su, sx, sT), gather(xd, Td, ud, N, [[f], [L + f]])):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert oe.cpu().tolist() == [list(emitted(f, 1, lag, False))] * 2
        for k in range(2):
            n = int(oe[k, 1])
            got_p[k] += [op[k, r].clone() for r in range(n)]
            got_c[k] += [oc[k, r].clone() for r in range(n)]
    st.t = [L, L]
    fp, fc, _ = st.push(None, None, None, 0, [1, 1])
    for k in range(2):
        p = torch.stack(got_p[k] + [fp[k, r] for r in range(lag)])
        c = torch.stack(got_c[k] + [fc[k, r] for r in range(lag)])
        assert same(p, path.view(2, L, J)[k]) and same(c, cost.view(2, L, J)[k])


def test_the_binding_owns_the_state(zh):
    """zh.JointStream: push, flush and reset with flags given as lists or tensors; the same bits as the raw ABI; the refusals of the
    binding itself."""
    J, N, H, L, lag, lam = 5, 12, 3, 4, 2, 30.0
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    starts = [0, 4, 8]
    want = run_clips(zh, xd, Td, ud, N, starts, L, lag, [3, 1], lam)
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
    """A NULL pointer other than d_T / d_flush / d_which, H = 1025, F > max_frames, F = 0 without d_flush, a negative lag, lambda < 0
    or NaN, a misaligned state: ZEDO_E_BADARG; a state one byte short: ZEDO_E_WORKSPACE; outputs and the state's bytes unchanged either
    way.  The same call with valid arguments is accepted."""
    lib = zh._lib
    J, N, H, L, lag, mf, lam = 5, 12, 3, 4, 2, 4, 100.0
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    S, F = 3, 4
    uu, xx, TT = gather(xd, Td, ud, N, [list(range(a, a + F)) for a in (0, 4, 8)])
    need = lib.zedo_joint_stream_state_bytes(S, H, J, lag, mf)
    state = dirty(need + 8, 0x5A)
    assert lib.zedo_joint_stream_reset(P(state), need, S, H, J, lag, mf, None, None) == 0
    u2, x2, T2 = gather(xd, Td, ud, N, [[a, a + 1] for a in (0, 4, 8)])
    tmp = (torch.empty((S, 2 + lag, J), dtype=torch.int32, device="cuda"), torch.empty((S, 2 + lag, J), dtype=torch.float64, device="cuda"),
           torch.empty((S, 2), dtype=torch.int64, device="cuda"))
    assert lib.zedo_joint_stream_push(P(u2), P(x2), P(T2), S, 2, H, J, lag, mf, lam, None, P(state), need, P(tmp[0]), P(tmp[1]), P(tmp[2]),
                                      None) == 0
    torch.cuda.synchronize()
    before = state.clone()                                           # a state in use: two frames per stream
    path, cost = sentinels((((S, F + lag, J), torch.int32), ((S, F + lag, J), torch.float64)), SENT_P)
    emit = torch.full((S, 2), -1, dtype=torch.int64, device="cuda")
    fl = torch.ones(S, dtype=torch.int32, device="cuda")
    ptrs = dict(u=P(uu), x=P(xx), T=P(TT), fl=P(fl), st=P(state), p=P(path), c=P(cost), e=P(emit))

    def call(f=F, h=H, j=J, s=S, lg=lag, m=mf, lm=lam, nbytes=need, **over):
        q = dict(ptrs, **over)
        return lib.zedo_joint_stream_push(q["u"], q["x"], q["T"], s, f, h, j, lg, m, lm, q["fl"], q["st"], nbytes, q["p"], q["c"], q["e"], None)

    for k in ("u", "x", "st", "p", "c", "e"):
        assert call(**{k: None}) == -1, k
    assert call(h=1025, nbytes=2 ** 40) == -1 and call(h=0) == -1 and call(j=0) == -1 and call(s=0) == -1 and call(m=0) == -1
    assert call(f=mf + 1) == -1 and call(f=-1) == -1
    assert call(f=0, fl=None) == -1                                  # a push of no frames that flushes nothing
    assert call(lg=-1) == -1 and call(lg=2 ** 31 - 1, nbytes=2 ** 40) == -1
    assert call(lm=-1.0) == -1 and call(lm=float("nan")) == -1 and call(lm=float("inf")) == -1
    assert call(st=ctypes.c_void_p(state.data_ptr() + 4)) == -1
    assert call(nbytes=need - 1) == -3 and call(nbytes=0) == -3
    for bad in (dict(h=1025), dict(lg=-1), dict(m=0)):
        kw = dict(zip(("h", "lg", "m"), (H, lag, mf)))
        kw.update(bad)
        assert lib.zedo_joint_stream_reset(P(state), 2 ** 40, S, kw["h"], J, kw["lg"], kw["m"], None, None) == -1
    assert lib.zedo_joint_stream_reset(None, need, S, H, J, lag, mf, None, None) == -1
    assert lib.zedo_joint_stream_reset(ctypes.c_void_p(state.data_ptr() + 4), need, S, H, J, lag, mf, None, None) == -1
    assert lib.zedo_joint_stream_reset(P(state), need - 1, S, H, J, lag, mf, None, None) == -3
    torch.cuda.synchronize()
    assert bool((path == SENT_P).all()) and bool((cost == SENT_C).all()) and bool((emit == -1).all()) and torch.equal(state, before)
    # the controls: without T and without flush; then a flush of no frames
    assert call(f=2, T=None, fl=None, u=P(u2), x=P(x2)) == 0
    assert call(f=0, u=None, x=None, T=None) == 0
    torch.cuda.synchronize()
    assert emit.tolist() == [[2, 2]] * S and bool((state[need:] == 0x5A).all()) and not torch.equal(state, before)


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
