"""The cases of tests/test_ipo_state_gpu.py, defined once for the three places that run them: the GPU test itself (unpinned: the
half-wave kernel at these row counts), its two child processes (ZEDO_IPO_KERNEL=half|row) and tests/test_ipo_state_ref.py, which
holds the float64 oracle - the arbiter of all of them - to the conditions the GPU test relies on.

Problems and states are those of test_ipo_single_iterations_on_general_intrinsics: problem(J, N, H, general=True), IPO_T, IPO_MIN,
IPO_MAX, normaliser N k 2, states from O.ipo_fit(dtype=float64, trace=, init=, it0=) handed over rounded to fp32.  Nothing of
zedo_hip is imported here: the functions that launch take the module as their first argument."""
import functools
import hashlib

import numpy as np

from _shared import IPO_MAX, IPO_MIN, IPO_T, KEYS, initial_state, oracle_args, oracle_resume, oracle_run, problem

N8 = 8
AXES8 = ["", "x", "y", "z", "xy", "xz", "yz", "xyz"]

# ---- the scale on, beside and beyond the clamp ----------------------------------------------------------------------------------

F = np.float32
CLAMP_SCALES = [("0.3", F(0.3)), ("below_min", np.nextafter(F(IPO_MIN), F(0))), ("min", F(IPO_MIN)), ("max", F(IPO_MAX)),
                ("above_max", np.nextafter(F(IPO_MAX), F(3))), ("2.4", F(2.4))]
CLAMP_KEYS = [KEYS[0], KEYS[1], KEYS[3]]
CLAMP_AXES = ["xyz", ""]
CLAMP_STATES = [0, 10, 30]
CLAMP_ITERS = [1, 4]


def clamp_state(J, kl, axes, it_state, value):
    """The oracle's float64 state after it_state iterations with the scale of ALL poses set to value (an fp32 number: handing the
    state over in fp32 does not move it)."""
    s = oracle_run(J, tuple(kl), N8, axes)[0][it_state].copy()
    s[:, 4] = np.float64(value)
    return s


@functools.lru_cache(maxsize=None)
def clamp_reference(J, kl, axes, it_state, value, iters):
    """What ``iters`` iterations from clamp_state(...) with it_begin = it_state must give, from the oracle alone:
    (handed state float64, float64 end state, fp32 oracle's end state, clear poses, T0 [8,3] in float64).
    A pose is clear when its residuals are >= 1e-3 px in every one of the iterations (a key joint at the root is not counted).

    it_state = 0: zedo_ipo_fit_resume ignores the content of a state handed in with it_begin = 0 and starts from RotOpt's initial
    values, so the injected scale cannot reach the fit; the expectation is the oracle's fit from the initial state, whatever value is."""
    kl = list(kl)
    args, norm = oracle_args(J, kl, N8), N8 * len(kl) * 2
    handed = clamp_state(J, kl, axes, it_state, value)
    start = handed if it_state > 0 else initial_state(N8)
    want, _, _, res = oracle_resume(args, axes, norm, start, it_state, iters)
    o32 = oracle_resume(args, axes, norm, start, it_state, iters, np.float32)[0]
    moving = np.abs(problem(J, N8)[0][0][kl]).max(-1) > 0
    clear = (res[:, :, moving, :].reshape(iters, N8, -1).min(2) >= 1e-3).all(0)
    return handed, want, o32, clear, args[1].reshape(N8, 3)


def clamp_cases(J, kl, axes):
    return [(it_state, tag, value, iters) for it_state in CLAMP_STATES for tag, value in CLAMP_SCALES for iters in CLAMP_ITERS]


# ---- launching ---------------------------------------------------------------------------------------------------------------------

class Problem:
    """problem(J, N, H) on the device with its key list and normaliser."""

    def __init__(self, J, kl, N, H=1):
        from _shared import dev
        cl, uv, K = problem(J, N, H)
        self.J, self.kl, self.N, self.H, self.norm = J, list(kl), N, H, N * len(kl) * 2
        self.x0, self.uv, self.K = dev(cl), dev(uv), dev(K)

    def fit(self, zh, axes, iters, B, state=None, it_begin=0, row_offset=0):
        """-> (R, T, q, scale); state is updated in place."""
        return zh.ipo_fit(self.x0, self.uv, self.K, self.kl, axes, IPO_T, IPO_MIN, IPO_MAX, iters, self.norm, B, row_offset=row_offset,
                          return_params=True, state=state, it_begin=it_begin)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- two calls equal one -------------------------------------------------------------------------------------------------------------

TOTAL = 60
SPLITS = [(1, 59), (25, 35), (59, 1), (20, 20, 20)]
# tag, N, H, B, row_offset.  The shard is cut from H = 3: rows [5, 19) do not exist in the 16 rows of H = 2, the entry point refuses them
ROWS = [("B16", N8, 2, 16, 0), ("B7", N8, 2, 7, 0), ("B14_offset5", N8, 3, 14, 5)]
ROWS_FULL_BLOCK = ("B131", 131, 1, 131, 0)                # one full 128-lane workgroup of the lane-per-row kernel and a tail of 3
SPLIT_AXES = ["", "xy", "xyz"]
PAD = 2                                                   # rows of the state tensor behind row B - 1: never touched
SEAM_FROM, SEAM_STATE, SEAM_TOTAL, SEAM_SPLITS = 2040, 20, 16, [(8, 8), (5, 11)]


def dirty_state(B):
    """[B + PAD, 15] fp32 whose every byte is 0xFF (a NaN with all payload bits set)."""
    import torch
    return torch.full((B + PAD, 15), -1, dtype=torch.int32, device="cuda").view(torch.float32)


def chain(zh, prob, axes, B, row_offset, parts, st, it_begin):
    """The fit in len(parts) calls, each resuming the state the one before wrote -> (R, T, q, scale) of the last call."""
    out = None
    for n in parts:
        out = prob.fit(zh, axes, n, B, state=st, it_begin=it_begin, row_offset=row_offset)
        it_begin += n
    return out


def round_trip(zh, prob, axes, B, row_offset, tag):
    """TOTAL iterations in one call against every split of SPLITS, in R, T, q, scale and all 15 state columns, bit for bit; the
    state buffer arrives with every byte 0xFF and is larger than B rows.  Also: the call without a state gives the same bits,
    and iters = 0 with it_begin = TOTAL returns the state unchanged and R, T of its parameters.  -> the digest of the unsplit fit."""
    import torch
    names = ("R", "T", "q", "scale", "state")
    bare = prob.fit(zh, axes, TOTAL, B, row_offset=row_offset)
    st1 = dirty_state(B)
    one = prob.fit(zh, axes, TOTAL, B, state=st1, it_begin=0, row_offset=row_offset) + (st1,)
    assert bool(torch.isfinite(st1[:B]).all()), (tag, "the state of a fit from it_begin = 0 keeps bytes of the buffer it was given")
    for name, a, b in zip(names, bare, one):
        assert same_bits(a, b), (tag, "with and without a state buffer", name)
    assert bool((st1[B:].view(torch.int32) == -1).all()), (tag, "rows behind B were written")
    assert same_bits(one[2], st1[:B, 0:4]) and same_bits(one[3], st1[:B, 4]), (tag, "q / scale are not the state's parameters")
    for parts in SPLITS:
        st = dirty_state(B)
        got = chain(zh, prob, axes, B, row_offset, parts, st, 0) + (st,)
        for name, a, b in zip(names, one, got):
            if not same_bits(a, b):
                rows = torch.nonzero((a.reshape(a.shape[0], -1).view(torch.int32) != b.reshape(b.shape[0], -1).view(torch.int32)).any(1))
                raise AssertionError((tag, "split " + "+".join(map(str, parts)), name, "rows", [int(r) for r in rows.flatten()[:8]]))
    st0 = st1.clone()
    idle = prob.fit(zh, axes, 0, B, state=st0, it_begin=TOTAL, row_offset=row_offset) + (st0,)
    for name, a, b in zip(names, one, idle):
        assert same_bits(a, b), (tag, "iters = 0 from the written state", name)
    return digest(*one)


def seam_state():
    J, kl = KEYS[0]
    return oracle_run(J, tuple(kl), N8, "xyz")[0][SEAM_STATE].astype(np.float32)


def round_trip_across_the_table_end(zh, s20):
    """The state after SEAM_STATE iterations (KEYS[0], N = 8, "xyz"), declared to be the state after SEAM_FROM: SEAM_TOTAL
    iterations in one call against the splits, bit for bit.  -> the digest of the unsplit fit."""
    import torch
    from _shared import dev
    J, kl = KEYS[0]
    prob = Problem(J, kl, N8)

    def run(parts):
        st = torch.cat([dev(s20), dirty_state(0)])
        return chain(zh, prob, "xyz", N8, 0, parts, st, SEAM_FROM) + (st,)

    one = run((SEAM_TOTAL,))
    assert bool(torch.isfinite(one[4][:N8]).all()) and not same_bits(one[4][:N8], dev(s20))
    for parts in SEAM_SPLITS:
        for name, a, b in zip(("R", "T", "q", "scale", "state"), one, run(parts)):
            assert same_bits(a, b), ("table end", "split " + "+".join(map(str, parts)), name)
    return digest(*one)


def split_cases(with_full_block=True):
    return [(J, kl, axes, row) for J, kl in KEYS for axes in SPLIT_AXES for row in ROWS + ([ROWS_FULL_BLOCK] if with_full_block else [])]


def split_id(J, kl, axes, row):
    return f"split_J{J}_k{len(kl)}_{axes or 'none'}_{row[0]}"


# ---- what a child process runs under its pin ---------------------------------------------------------------------------------------

def write_child_inputs(path):
    """The fp32 states the children resume from - computed by the parent from the oracle, so that both children read the same bytes
    and neither runs the oracle: singles_<case> [51,8,15], the states of test_ipo_single_iterations_on_general_intrinsics at N = 8;
    clamp_<case> [8,15]; seam [8,15]."""
    out = {"seam": seam_state()}
    for J, kl in KEYS:
        for axes in AXES8:
            out[f"singles_J{J}_k{len(kl)}_{axes or 'none'}"] = np.stack(oracle_run(J, tuple(kl), N8, axes)[0]).astype(np.float32)
    for J, kl in CLAMP_KEYS:
        for axes in CLAMP_AXES:
            for it_state in CLAMP_STATES:
                for tag, value in CLAMP_SCALES:
                    out[f"clamp_J{J}_k{len(kl)}_{axes or 'none'}_s{it_state}_{tag}"] = clamp_state(J, kl, axes, it_state, value).astype(np.float32)
    np.savez(path, **out)


def child_main(path):
    """Every launch of tests/test_ipo_state_gpu.py in the kernel ZEDO_IPO_KERNEL pins -> {case: SHA-256 over R, T, q, scale and the
    state}.  The round trips are asserted here as well: a state written by a iterations and resumed for b gives the bits of a + b."""
    import json
    import torch
    import zedo_hip as zh
    from _shared import dev
    inp = np.load(path)
    out = {}
    for J, kl in KEYS:
        prob = Problem(J, kl, N8)
        for axes in AXES8:
            name = f"singles_J{J}_k{len(kl)}_{axes or 'none'}"
            h = hashlib.sha256()
            for it in range(50):
                st = dev(inp[name][it])
                h.update(digest(*prob.fit(zh, axes, 1, N8, state=st, it_begin=it), st).encode())
            out[name] = h.hexdigest()
        if (J, kl) in CLAMP_KEYS:
            for axes in CLAMP_AXES:
                for it_state, tag, value, iters in clamp_cases(J, kl, axes):
                    st = dev(inp[f"clamp_J{J}_k{len(kl)}_{axes or 'none'}_s{it_state}_{tag}"])
                    res = prob.fit(zh, axes, iters, N8, state=st, it_begin=it_state)
                    assert bool(torch.isfinite(st).all())
                    out[f"clamp_J{J}_k{len(kl)}_{axes or 'none'}_s{it_state}_{tag}_i{iters}"] = digest(*res, st)
    probs = {}
    for J, kl, axes, row in split_cases():
        tag, N, H, B, off = row
        if (J, tuple(kl), N, H) not in probs:
            probs[(J, tuple(kl), N, H)] = Problem(J, kl, N, H)
        out[split_id(J, kl, axes, row)] = round_trip(zh, probs[(J, tuple(kl), N, H)], axes, B, off, split_id(J, kl, axes, row))
    out["seam"] = round_trip_across_the_table_end(zh, inp["seam"])
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(out))


# ---- tests/test_ipo_key_lists_gpu.py: every key-list length in the kernel ZEDO_IPO_KERNEL pins ------------------------------------------

KEY_LIST_ITERS = 500


def key_list_cases():
    from _shared import IPO_FORM_IDS, IPO_FORM_KEYS, IPO_LENGTH_KEYS
    names = [f"k{len(kl)}" for _, kl in IPO_LENGTH_KEYS] + IPO_FORM_IDS
    return [(name, J, kl, N, axes) for name, (J, kl) in zip(names, IPO_LENGTH_KEYS + IPO_FORM_KEYS) for N in (8, 64) for axes in ("z", "xyz")]


def key_lists_child_main():
    """make_ipo_problem(21, N, H = 2) with every list of IPO_LENGTH_KEYS and IPO_FORM_KEYS, N = 8 and 64, axes "z" and "xyz":
    KEY_LIST_ITERS iterations through zedo_ipo_fit_resume from it_begin = 0 with a state buffer that arrives dirty
    -> {case: SHA-256 over R, T, q, scale and all 15 state columns}; every output finite."""
    import json
    import torch
    import zedo_hip as zh
    from _shared import dev, make_ipo_problem
    out, probs = {}, {}
    for name, J, kl, N, axes in key_list_cases():
        if (J, N) not in probs:
            probs[(J, N)] = tuple(dev(a) for a in make_ipo_problem(J, N, H=2))
        x0, uv, K = probs[(J, N)]
        B = 2 * N
        st = dirty_state(B)
        res = zh.ipo_fit(x0, uv, K, kl, axes, IPO_T, IPO_MIN, IPO_MAX, KEY_LIST_ITERS, N * len(kl) * 2, B, return_params=True, state=st,
                         it_begin=0)
        assert all(bool(torch.isfinite(t).all()) for t in res) and bool(torch.isfinite(st[:B]).all()), (name, N, axes)
        assert bool((st[B:].view(torch.int32) == -1).all()), (name, N, axes, "rows behind B were written")
        out[f"{name}_N{N}_{axes}"] = digest(*res, st[:B])
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(out))
