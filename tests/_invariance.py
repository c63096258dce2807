"""What the GPU tests of the label-free selection / fusion family share, defined once: the bitwise comparison, the plumbing of a call at the
raw ABI, the launch forms a call's bits must not depend on, the refusals every entry point owes and the clamping of clip offsets.  Plain
functions, imported by the test files the way tests/_shared.py is; pinned on their own by tests/test_invariance_helpers_cpu.py.

bits(t) is the integer view of EVERY floating dtype at its own width, so same() tells +0.0 from -0.0 and one NaN payload from another in
float32 as in float64, and shape and dtype are part of equality."""
import ctypes

import numpy as np
import torch

_INT_OF = {2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---- 1. comparison ---------------------------------------------------------------------------------------------------------

def bits(t):
    """A torch tensor or a numpy array of a floating dtype as integers of the same width (a view); anything else unchanged."""
    if isinstance(t, np.ndarray):
        return t.view(f"i{t.dtype.itemsize}") if t.dtype.kind == "f" else t
    return t.view(_INT_OF[t.element_size()]) if t.is_floating_point() else t


def same(a, b):
    """Equal shape, equal dtype, equal bits (two tensors or two arrays)."""
    if isinstance(a, np.ndarray) != isinstance(b, np.ndarray) or a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(bits(a), bits(b)) if isinstance(a, np.ndarray) else torch.equal(bits(a), bits(b))


def all_same(out, ref):
    return len(out) == len(ref) and all(same(a, b) for a, b in zip(out, ref))


# ---- 2. the plumbing of a call at the raw ABI -------------------------------------------------------------------------------

def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def cur_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sentinels(specs, value=-7):
    """One device tensor per (shape, dtype), filled with `value`: outputs a call is to overwrite, or to leave alone."""
    return [torch.full(tuple(shape), value, dtype=dt, device="cuda") for shape, dt in specs]


def dirty(nbytes, byte):
    return torch.full((nbytes,), byte, dtype=torch.uint8, device="cuda")


def misaligned(t, floats=3):
    """A contiguous copy of t that starts `floats` elements behind a fresh allocation: 12 bytes past a 16-byte boundary for fp32 at the
    default (and at any floats = 3 mod 4), 4 bytes past it at floats = 1."""
    buf = torch.empty(t.numel() + floats, dtype=t.dtype, device=t.device)
    tb = buf[floats:].view(t.shape)
    tb.copy_(t)
    assert t.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == floats * t.element_size() % 16 and tb.is_contiguous()
    return tb


# ---- 3. the launch forms the bits must not depend on ------------------------------------------------------------------------

def replays_to(ref, fn, stream, n=2):
    """fn() captured into a graph on `stream` (a single branch: the call allocates nothing and synchronises nothing of its own) and
    replayed n times, its outputs zeroed before every replay: the bits of ref each time.  -> the captured outputs."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        out = fn()
    for _ in range(n):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all_same(out, ref)
    return out


def launch_invariant(ref, via_binding, x, raw=None, out_specs=None, nbytes=0):
    """The bits of ref from: raw(ws, outs, stream) - the call at the raw ABI on a workspace of nbytes 0xFF bytes (all NaN as float64)
    with sentinel outputs of out_specs, for the calls that take a workspace; via_binding(seq_on_device=True) on a side stream (which
    also warms the allocator for the capture); the same call captured and replayed twice; and via_binding(x=...) on the copy of x that
    starts 12 bytes past a 16-byte boundary."""
    if raw is not None:
        ws = dirty(nbytes, 0xFF)
        assert bool(torch.isnan(ws[:nbytes // 8 * 8].view(torch.float64)).all())
        outs = sentinels(out_specs)
        assert raw(ws, outs, cur_stream()) == 0
        torch.cuda.synchronize()
        assert all_same(outs, ref)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = via_binding(seq_on_device=True)
    torch.cuda.synchronize()
    assert all_same(out, ref)
    replays_to(ref, lambda: via_binding(seq_on_device=True), s)
    assert all_same(via_binding(x=misaligned(x)), ref)


# ---- 4. the refusals ---------------------------------------------------------------------------------------------------------

BADARG, WORKSPACE = -1, -3                                           # ZEDO_E_BADARG, ZEDO_E_WORKSPACE of include/zedo_hip.h


def refusal_sweep(call, ptrs, required, *, sizes, weights=(), taus=(), workspace_slot=None, need=None, untouched=()):
    """call(p=ptrs, **overrides) -> the entry point's return code.  ZEDO_E_BADARG for: a NULL in every slot of `required`; every dict
    of overrides in `sizes`; -1, NaN and inf in every keyword of `weights`; 0, -0, -1, NaN, inf and -inf in every keyword of `taus`;
    the workspace (slot workspace_slot) 4 bytes off its alignment.  ZEDO_E_WORKSPACE for a workspace of need - 1 bytes and of none.
    Then nothing was written: every (tensor, value) of `untouched` still holds its value everywhere.  Last the control: the call as it
    stands is accepted (and synchronised: the caller looks at its outputs)."""
    for k in required:
        assert call([None if i == k else p for i, p in enumerate(ptrs)]) == BADARG, k
    for over in sizes:
        assert call(**over) == BADARG, over
    for name in weights:
        for v in (-1.0, float("nan"), float("inf")):
            assert call(**{name: v}) == BADARG, (name, v)
    for name in taus:
        for v in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            assert call(**{name: v}) == BADARG, (name, v)
    if workspace_slot is not None:
        off = ctypes.c_void_p(ptrs[workspace_slot].value + 4)
        assert call([off if i == workspace_slot else p for i, p in enumerate(ptrs)]) == BADARG
        assert call(nbytes=need - 1) == WORKSPACE and call(nbytes=0) == WORKSPACE
    on_device = any(t.is_cuda for t, _ in untouched)
    if on_device:
        torch.cuda.synchronize()
    for i, (t, v) in enumerate(untouched):
        assert bool((t == v).all()), i
    assert call() == 0                                               # the control
    if on_device:
        torch.cuda.synchronize()


# ---- 5. clip offsets -----------------------------------------------------------------------------------------------------------

def clamped_offsets(call_with_seq, N):
    """Offsets outside 0 .. N are clamped and never become addresses: [0, N + 1000] and [-5, N] are the one clip [0, N], bit for bit."""
    ref = call_with_seq([0, N])
    for seq in ([0, N + 1000], [-5, N]):
        assert all_same(call_with_seq(seq), ref), seq
