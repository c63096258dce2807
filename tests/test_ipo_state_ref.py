"""CPU: the arbiter of tests/test_ipo_state_gpu.py held to what that file relies on.  The float64 oracle (oracle/zedo_oracle.py) decides
there what a resumed IPO fit must return; here, without a GPU: its gradient mask at the clamp agrees with torch.clamp's autograd at
exactly the six scale values the GPU test injects, in float32 and float64; its own resume interface (init=, it0=) splits a fit
without changing a bit; the injected states leave the share of clear poses the GPU test needs, so that it cannot go vacuous; and each
injected value does what its case is for (beyond the clamp the gradient of the scale is an exact zero, on it it is not)."""
import numpy as np
import pytest
import torch

import _ipo_state as S
from _shared import IPO_MAX, IPO_MIN, KEYS, initial_state, oracle_args, oracle_resume, oracle_run, unpack

CLAMP_IDS = [f"J{J}-k{len(kl)}-{axes or 'none'}" for J, kl in S.CLAMP_KEYS for axes in S.CLAMP_AXES]
CLAMP_PARAMS = [(J, kl, axes) for J, kl in S.CLAMP_KEYS for axes in S.CLAMP_AXES]


def test_the_injected_values_are_what_they_are_called():
    v = dict(S.CLAMP_SCALES)
    assert all(x.dtype == np.float32 for x in v.values()) and len(v) == 6
    assert v["0.3"] < v["below_min"] < v["min"] == np.float32(0.5) < v["max"] == np.float32(2.0) < v["above_max"] < v["2.4"]
    assert v["min"] - v["below_min"] == np.float32(2.0 ** -25) and v["above_max"] - v["max"] == np.float32(2.0 ** -22)
    assert (IPO_MIN, IPO_MAX) == (0.5, 2.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_the_gradient_mask_of_the_oracle_is_torch_clamps_at_the_six_values(dtype):
    """torch.clamp's backward passes the gradient where min <= x <= max, both ends included; the oracle spells that mask by hand
    (ipo_loss_and_grads).  At each injected value: the oracle's g_scale is the unmasked gradient (the same call with the bounds at
    -inf / +inf, nonzero on every pose) times d clamp / d x of torch's autograd on the CPU, exactly."""
    import zedo_oracle as O
    J, kl = KEYS[0]
    args = [np.asarray(a, dtype) for a in oracle_args(J, kl, S.N8)]
    q = unpack(oracle_run(J, tuple(kl), S.N8, "xyz")[0][10])[0].astype(dtype)
    tdt = torch.float32 if dtype is np.float32 else torch.float64
    passes = {}
    for tag, value in S.CLAMP_SCALES:
        scale = np.full(S.N8, value, dtype)
        x = torch.tensor(scale, dtype=tdt, requires_grad=True)
        torch.clamp(x, IPO_MIN, IPO_MAX).sum().backward()
        mask = x.grad.numpy()
        assert set(np.unique(mask)) <= {0.0, 1.0} and len(np.unique(mask)) == 1
        passes[tag] = bool(mask[0])
        clip = np.clip(scale, dtype(IPO_MIN), dtype(IPO_MAX))
        g = O.ipo_loss_and_grads(q, scale, args[0], args[1].reshape(-1, 3), args[2], args[3], "xyz", IPO_MIN, IPO_MAX, S.N8 * len(kl) * 2)[2]
        free = O.ipo_loss_and_grads(q, clip, args[0], args[1].reshape(-1, 3), args[2], args[3], "xyz", -np.inf, np.inf, S.N8 * len(kl) * 2)[2]
        assert (free != 0).all() and g.dtype == dtype
        assert np.array_equal(g, free * mask.astype(dtype)), tag
    assert passes == {"0.3": False, "below_min": False, "min": True, "max": True, "above_max": False, "2.4": False}


@pytest.mark.parametrize("axes", ["", "xy", "xyz"])
@pytest.mark.parametrize("J,kl", KEYS, ids=[f"J{J}-k{len(kl)}" for J, kl in KEYS])
def test_the_oracle_resumed_is_the_oracle_unsplit(J, kl, axes):
    """iters = a, then init=, it0 = a, iters = b, against iters = a + b: every one of the 15 state columns, R and T bit for bit in
    float64, for the splits the GPU test runs; from the initial state and from a state declared to be the one after 2040."""
    args, norm = oracle_args(J, kl, S.N8), S.N8 * len(kl) * 2
    for start, it0, total, splits in ((initial_state(S.N8), 0, S.TOTAL, S.SPLITS),
                                      (oracle_run(J, tuple(kl), S.N8, axes)[0][S.SEAM_STATE], S.SEAM_FROM, S.SEAM_TOTAL, S.SEAM_SPLITS)):
        one = oracle_resume(args, axes, norm, start, it0, total)
        assert not np.array_equal(one[0], start)
        for parts in splits:
            st, it = start, it0
            for n in parts:
                st, R, T, _ = oracle_resume(args, axes, norm, st, it, n)
                it += n
            assert it == it0 + total
            for a, b in zip(one[:3], (st, R, T)):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (parts, it0)


@pytest.mark.parametrize("J,kl,axes", CLAMP_PARAMS, ids=CLAMP_IDS)
def test_the_clamp_cases_leave_clear_poses_and_do_what_they_are_for(J, kl, axes):
    """For every state the GPU test hands over (after 0, 10 and 30 iterations x six scales x 1 and 4 iterations in one call): at most
    5 % of the pose-iterations are left out (the project's cap), and every single call keeps at least one clear pose.  From the
    states after 10 and 30: one iteration moves the scale's first moment by exactly 0.9 beyond the clamp (g = 0) and by something
    else on it, the scale itself moves in every case, and the float64 end states of the six values differ from each other.  With ""
    the three axis slots stay exact zeros.  After 0 iterations the state is not read (it_begin = 0): one expectation for all six."""
    left_out, total = 0, 0
    for it_state in S.CLAMP_STATES:
        ends = []
        for tag, value in S.CLAMP_SCALES:
            for iters in S.CLAMP_ITERS:
                handed, want, o32, clear, T0 = S.clamp_reference(J, tuple(kl), axes, it_state, value, iters)
                left_out, total = left_out + iters * int((~clear).sum()), total + iters * S.N8
                assert clear.any(), (it_state, tag, iters)
                assert (handed[:, 4] == np.float64(value)).all() and np.isfinite(want).all() and np.isfinite(o32).all()
                if axes == "":
                    assert (want[:, [1, 2, 3, 6, 7, 8, 11, 12, 13]] == 0).all()
                if iters == 1:
                    ends.append(want)
                    if it_state > 0:
                        inside = IPO_MIN <= value <= IPO_MAX
                        decayed = want[:, 9] == handed[:, 9] + (0.0 - handed[:, 9]) * (1 - 0.9)
                        assert decayed.all() if not inside else not decayed.any(), (it_state, tag)
                        assert (want[:, 4] != handed[:, 4]).all() and (handed[:, 9] != 0).all() and (handed[:, 14] > 0).all()
                        if tag in ("0.3", "2.4"):                       # one step stays beyond the clamp: the returned scale shows it unclamped
                            assert ((want[:, 4] < IPO_MIN - 0.05) | (want[:, 4] > IPO_MAX + 0.05)).all(), (it_state, tag)
        distinct = len({e.tobytes() for e in ends})
        assert distinct == (len(S.CLAMP_SCALES) if it_state > 0 else 1), (it_state, distinct)
    assert left_out <= 0.05 * total, (left_out, total)
