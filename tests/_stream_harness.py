"""What the GPU tests of the three fixed-lag streaming calls share, defined once, on top of tests/_invariance.py: a call described by a
StreamCall (one instance at the top of each test file), S streams at the raw ABI with every push checked (Streams), the drivers that
push clips through them (run_clips, by_frame, replay_frame_by_frame, interleaved, each_alone, whole_push) and the two ends of a refusal
test (state_in_use, raw_push, sizes, reset_refusals).  The pure parts are pinned by tests/test_stream_harness_cpu.py.

A list of raw pointers `ptrs` is always [d_junary, d_x, d_T, d_flush, d_state, the outputs in ABI order .., d_emit]."""
import ctypes
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np
import torch

from _invariance import BADARG, WORKSPACE, all_same, cur_stream, dirty, ptr as P, sentinels
from _joint_stream_ref import chunkings, emitted
from _temporal_ref import clips

HUGE = 2 ** 40                                                       # a state size no shape needs: the refusal is the shape's


@dataclass(frozen=True)
class StreamCall:
    """One streaming entry point: <prefix>_state_bytes, <prefix>_reset and <prefix>_push of include/zedo_hip.h."""
    prefix: str
    weights: tuple                                                   # the names of the doubles between max_frames and d_flush, in ABI order
    outputs: object                                                  # (S, rows, J, H) -> ((shape, dtype), ..) in ABI order
    index: int                                                       # the output that holds a hypothesis: 0 .. H-1 on every emitted row
    max_h: int                                                       # the largest H the call accepts
    optional: dict = field(default_factory=dict)                     # keyword of Streams -> the output that may be NULL
    sentinel: int = -7

    def fn(self, lib, what):
        return getattr(lib, f"{self.prefix}_{what}")

    def blank(self, S, rows, J, H):
        """The outputs [S, rows, ..] pre-filled with the sentinel."""
        return sentinels(self.outputs(S, rows, J, H), self.sentinel)

    def required(self):
        """The slots of `ptrs` that must not be NULL."""
        n = len(self.outputs(1, 1, 1, 1))
        return (0, 1, 4) + tuple(5 + i for i in range(n) if i not in self.optional.values()) + (5 + n,)

    def push(self, lib, p, S, F, H, J, lag, mf, weights, nbytes, stream):
        return self.fn(lib, "push")(p[0], p[1], p[2], S, F, H, J, lag, mf, *weights, p[3], p[4], nbytes, *p[5:], stream)


def gather(xd, Td, ud, N, frames):
    """frames [S][F]: the frame of the case every stream pushes -> the chunk's (u, x, T), rows (h, n) h-major with n = s F + f."""
    H = xd.shape[0] // N
    fr = torch.tensor(frames, dtype=torch.int64, device="cuda")
    rows = (torch.arange(H, device="cuda")[:, None, None] * N + fr[None]).reshape(-1)
    return ud[rows].contiguous(), xd[rows].contiguous(), None if Td is None else Td[rows].contiguous()


def groups(N, L):
    """The clips of clips(N, L) as groups of equal length: [(starts, length)] - the equal ones as streams of one call, a shorter last one
    on its own."""
    seq = clips(N, L)
    full = [a for a, b in zip(seq[:-1], seq[1:]) if b - a == L]
    out = [(full, L)] if full else []
    if seq[-1] - seq[-2] != L:
        out.append(([seq[-2]], seq[-1] - seq[-2]))
    return out


def frames_of(starts, Lc):
    return np.array([[a + f for f in range(Lc)] for a in starts])


def emit_blank(S):
    return torch.full((S, 2), -1, dtype=torch.int64, device="cuda")


class Streams:
    """S streams at the raw ABI: the state pre-filled with `fill` bytes and then reset; every push checks its return code, and - after
    one synchronisation - d_emit against the header's formula, the rows past the count against the sentinel and the index output
    against 0 .. H-1.  out[s]: the (clip-local first frame, [the emitted rows of every output]) of every push of this stream, in order,
    on the device.  An optional output switched off (with_w=False) is passed as NULL: all of it stays at the sentinel."""

    def __init__(self, zh, call, S, H, J, lag, max_frames, weights, fill=0xFF, **optional):
        self.lib, self.call, self.S, self.H, self.J, self.lag, self.mf, self.w = zh._lib, call, S, H, J, lag, max_frames, tuple(weights)
        self.null = {call.optional[k] for k, on in optional.items() if not on}
        self.nbytes = call.fn(self.lib, "state_bytes")(S, H, J, lag, max_frames)
        assert self.nbytes > 0 and len(self.w) == len(call.weights)
        self.state = dirty(self.nbytes, fill)
        self.t = [0] * S
        self.out = [[] for _ in range(S)]
        self.reset()

    def reset(self, which=None):
        w = None if which is None else torch.tensor(which, dtype=torch.int32, device="cuda")
        assert self.call.fn(self.lib, "reset")(P(self.state), self.nbytes, self.S, self.H, self.J, self.lag, self.mf, P(w), cur_stream()) == 0
        for s in range(self.S):
            if which is None or which[s]:
                self.t[s] = 0

    def push(self, u, x, T, F, flush=None):
        """-> (the outputs [S, F + lag, ..], d_emit [S,2])"""
        S, call = self.S, self.call
        fl = None if flush is None else torch.tensor(flush, dtype=torch.int32, device="cuda")
        o, emit = call.blank(S, F + self.lag, self.J, self.H), emit_blank(S)
        ptrs = [P(u), P(x), P(T), P(fl), P(self.state)] + [None if i in self.null else P(t) for i, t in enumerate(o)] + [P(emit)]
        rc = call.push(self.lib, ptrs, S, F, self.H, self.J, self.lag, self.mf, self.w, self.nbytes, cur_stream())
        assert rc == 0, rc
        want = [emitted(self.t[s], F, self.lag, bool(flush and flush[s])) for s in range(S)]
        assert emit.cpu().tolist() == [list(w) for w in want], (emit.cpu().tolist(), want)
        assert all(bool((o[i] == call.sentinel).all()) for i in self.null)
        for s, (first, count) in enumerate(want):
            assert all(bool((t[s, count:] == call.sentinel).all()) for t in o)
            assert bool((o[call.index][s, :count] >= 0).all()) and bool((o[call.index][s, :count] < self.H).all())
            self.out[s].append((first, [t[s, :count] for t in o]))
            self.t[s] = 0 if flush and flush[s] else self.t[s] + F
        return o, emit

    def collected(self, s):
        """(frames [n], the outputs [n, ..]) of everything stream s has emitted."""
        o = self.out[s]
        return [f + r for f, rows in o for r in range(rows[0].shape[0])], [torch.cat(k) for k in zip(*(rows for _, rows in o))]


def stacked(st, L):
    """Every stream of st has emitted the frames 0 .. L-1 once each, in order -> the outputs [S, L, ..]."""
    outs = [st.collected(s) for s in range(st.S)]
    assert all(o[0] == list(range(L)) for o in outs)
    return [torch.stack(k) for k in zip(*(o[1] for o in outs))]


def run_clips(zh, call, xd, Td, ud, N, starts, L, lag, cut, weights, **kw):
    """The clips [a, a + L) for a in starts as len(starts) streams, pushed in chunks of cut[i] frames with a flush at the end -> the
    outputs [S, L, ..] on the device."""
    S, H, J = len(starts), xd.shape[0] // N, xd.shape[1]
    st = Streams(zh, call, S, H, J, lag, max(cut), weights, **kw)
    f0 = 0
    for i, F in enumerate(cut):
        u, x, T = gather(xd, Td, ud, N, [[a + f0 + f for f in range(F)] for a in starts])
        st.push(u, x, T, F, [1] * S if i == len(cut) - 1 else None)
        f0 += F
    return stacked(st, L)


def by_frame(zh, call, xd, Td, ud, N, L, lag, name, weights, **kw):
    """All clips of clips(N, L) streamed under the chunking `name` -> the outputs [N, ..] on the device, in the case's frame order."""
    out = None
    for starts, Lc in groups(N, L):
        o = run_clips(zh, call, xd, Td, ud, N, starts, Lc, lag, chunkings(Lc)[name], weights, **kw)
        if out is None:
            out = [torch.empty((N,) + tuple(t.shape[2:]), dtype=t.dtype, device="cuda") for t in o]
        rows = torch.as_tensor(frames_of(starts, Lc), device="cuda")
        for dst, src in zip(out, o):
            dst[rows] = src
    return out


def replay_frame_by_frame(zh, call, xd, Td, ud, N, starts, L, lag, weights):
    """One F = 1 push without flush captured into a graph on a side stream (a single branch) over static input tensors, and replayed L
    times with frame f of every clip copied into them - a replay advances the state; d_emit is held to the header's formula after
    every replay.  With the emission of a final flush of no frames -> the outputs [S, L, ..]."""
    S, H, J = len(starts), xd.shape[0] // N, xd.shape[1]
    st = Streams(zh, call, S, H, J, lag, 1, weights)
    static = [t.clone() for t in gather(xd, Td, ud, N, [[a] for a in starts])]
    o, emit = call.blank(S, 1 + lag, J, H), emit_blank(S)
    ptrs = [P(t) for t in static] + [None, P(st.state)] + [P(t) for t in o] + [P(emit)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = call.push(st.lib, ptrs, S, 1, H, J, lag, 1, st.w, st.nbytes, cur_stream())
    assert rc == 0
    for f in range(L):
        for dst, src in zip(static, gather(xd, Td, ud, N, [[a + f] for a in starts])):
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


def interleaved(zh, call, xd, Td, ud, N, frames, flush_at, reset_after, members, lag, weights):
    """The streams `members` of frames [s][i], one frame per push: stream s is flushed at the pushes of flush_at[s] and reset through
    d_which after those of reset_after[s] -> (the Streams, [the outputs and d_emit of every push])."""
    st = Streams(zh, call, len(members), xd.shape[0] // N, xd.shape[1], lag, 1, weights)
    per_push = []
    for i in range(len(frames[0])):
        uu, xx, TT = gather(xd, Td, ud, N, [[frames[s][i]] for s in members])
        fl = [1 if i in flush_at[s] else 0 for s in members]
        o, e = st.push(uu, xx, TT, 1, fl if any(fl) else None)
        per_push.append(o + [e])
        rs = [1 if i in reset_after[s] else 0 for s in members]
        if any(rs):
            st.reset(rs)
    return st, per_push


def each_alone(zh, call, xd, Td, ud, N, frames, flush_at, reset_after, lag, weights):
    """interleaved with every stream, and with each alone: a stream emits, bit for bit and push by push, what it emits alone.  -> the
    Streams of the run with all of them."""
    args = (zh, call, xd, Td, ud, N, frames, flush_at, reset_after)
    together, pushes = interleaved(*args, list(range(len(frames))), lag, weights)
    for s in range(len(frames)):
        _, alone = interleaved(*args, [s], lag, weights)
        for o3, o1 in zip(pushes, alone):
            assert all_same([t[s:s + 1] for t in o3], o1), s
    return together


def whole_push(zh, call, chunk, S, L, H, J, lag, weights):
    """-> whole(x=None, seq_on_device=False), for launch_invariant: reset + the S clips of chunk = (u, x, T) pushed whole and flushed,
    on a fresh 0xFF state with sentinel outputs, nothing synchronised -> [the L emitted rows of every output .., d_emit]."""
    lib = zh._lib
    nbytes = call.fn(lib, "state_bytes")(S, H, J, lag, L)
    fl = torch.ones(S, dtype=torch.int32, device="cuda")

    def whole(x=None, seq_on_device=False):
        state, o, emit = dirty(nbytes, 0xFF), call.blank(S, L + lag, J, H), emit_blank(S)
        assert call.fn(lib, "reset")(P(state), nbytes, S, H, J, lag, L, None, cur_stream()) == 0
        ptrs = [P(chunk[0]), P(chunk[1] if x is None else x), P(chunk[2]), P(fl), P(state)] + [P(t) for t in o] + [P(emit)]
        assert call.push(lib, ptrs, S, L, H, J, lag, L, weights, nbytes, cur_stream()) == 0
        return [t[:, :L] for t in o] + [emit]

    return whole


# ---- the refusals ------------------------------------------------------------------------------------------------------------

def state_in_use(zh, call, xd, Td, ud, N, starts, lag, mf, weights):
    """A state of need + 8 bytes of 0x5A, reset, with two frames of every stream pushed into sentinel scratch outputs -> .state,
    .need, .before (its bytes, guard included, after one synchronisation) and .chunk2, the (u, x, T) of those two frames."""
    lib, S, H, J = zh._lib, len(starts), xd.shape[0] // N, xd.shape[1]
    need = call.fn(lib, "state_bytes")(S, H, J, lag, mf)
    state = dirty(need + 8, 0x5A)
    assert call.fn(lib, "reset")(P(state), need, S, H, J, lag, mf, None, None) == 0
    chunk2 = gather(xd, Td, ud, N, [[a, a + 1] for a in starts])
    scratch = call.blank(S, 2 + lag, J, H) + sentinels((((S, 2), torch.int64),))
    ptrs = [P(t) for t in chunk2] + [None, P(state)] + [P(t) for t in scratch]
    assert call.push(lib, ptrs, S, 2, H, J, lag, mf, weights, need, None) == 0
    torch.cuda.synchronize()
    return SimpleNamespace(state=state, need=need, before=state.clone(), chunk2=chunk2)


def raw_push(lib, call, ptrs, S, F, H, J, lag, mf, weights, need):
    """-> push(p=ptrs, f=, h=, j=, s=, lg=, m=, nbytes=, no_flush=False, <a weight by its name>=): the return code of the push on the
    default stream with these overrides - the `call` of refusal_sweep."""
    def push(p=ptrs, f=F, h=H, j=J, s=S, lg=lag, m=mf, nbytes=need, no_flush=False, **over):
        assert set(over) <= set(call.weights), over
        w = [over.get(name, v) for name, v in zip(call.weights, weights)]
        return call.push(lib, p[:3] + [None if no_flush else p[3]] + p[4:], s, f, h, j, lg, m, w, nbytes, None)
    return push


def sizes(call, mf):
    """The size arguments every streaming push refuses: H past the call's cap and below 1, no joints, no streams, no frames per push,
    F past max_frames or negative, F = 0 without d_flush (a push of no frames that flushes nothing), a negative lag and one that
    overflows lag + max_frames."""
    return [dict(h=call.max_h + 1, nbytes=HUGE), dict(h=0), dict(h=-1), dict(j=0), dict(s=0), dict(m=0), dict(f=mf + 1), dict(f=-1),
            dict(f=0, no_flush=True), dict(lg=-1), dict(lg=2 ** 31 - 1, nbytes=HUGE)]


def reset_refusals(lib, call, use, S, H, J, lag, mf):
    """<prefix>_reset on the state in use: H past the cap, a negative lag, max_frames = 0, NULL and a state 4 bytes off its alignment:
    ZEDO_E_BADARG; one byte short: ZEDO_E_WORKSPACE; the state's bytes unchanged and the 8 guard bytes still 0x5A."""
    reset, state, need = call.fn(lib, "reset"), use.state, use.need
    for h, lg, m in ((call.max_h + 1, lag, mf), (H, -1, mf), (H, lag, 0)):
        assert reset(P(state), HUGE, S, h, J, lg, m, None, None) == BADARG, (h, lg, m)
    assert reset(None, need, S, H, J, lag, mf, None, None) == BADARG
    assert reset(ctypes.c_void_p(state.data_ptr() + 4), need, S, H, J, lag, mf, None, None) == BADARG
    assert reset(P(state), need - 1, S, H, J, lag, mf, None, None) == WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(state, use.before) and bool((state[need:] == 0x5A).all())
