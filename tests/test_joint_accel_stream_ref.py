"""CPU: the numpy reference of the fixed-lag streaming selection under the second-order model (tests/_joint_accel_stream_ref.py) on its
own.  fixed_lag is held to what defines it: the path at frame n is that of the OFFLINE reference (_joint_accel_ref.joint_accel_ref - itself
pinned against the enumeration of all paths - run again on the truncated inputs) on the clip cut after frame min(n + lag, last), exactly,
and the cost is that reference's emin at the end of n's chain there, bit for bit (of a chain of one frame: its cost, the minimum of u).
Then the condition the exact comparisons of the GPU tests rest on, and the order of the shares at which the lag changes the decision."""
import numpy as np
import pytest

from _joint_accel_ref import GAP_MIN, joint_accel_ref
from _joint_accel_stream_ref import (BIG, BIG_WEIGHTS, GPU_CASES, LAGS, WEIGHTS, case, check_gaps, clips, dead_joint_case, differ_share, fixed_lag, forward, tables)

SMALL = [(1, 1, 1, 1), (1, 7, 2, 7), (5, 12, 3, 4), (1, 20, 17, 20), (3, 40, 64, 9)]


def truncated(x, T, u, N, a, e):
    """The frames a .. e of a case as a problem of their own: rows (h, n) h-major."""
    H = x.shape[0] // N
    rows = (np.arange(H)[:, None] * N + np.arange(a, e + 1)[None, :]).reshape(-1)
    return x[rows], T[rows], u[rows]


def hold_to_truncated_clips(x, T, u, N, seq, lam_v, lam_a, tab):
    """One offline reference per truncation serves every lag: the frame n = e - lag, and at the clip's last frame every n >= e - lag."""
    fixed = {lag: fixed_lag(tab, seq, lag) for lag in LAGS}
    J = x.shape[1]
    for a, b in zip(seq[:-1], seq[1:]):
        for e in range(a, b):
            xt, Tt, ut = truncated(x, T, u, N, a, e)
            r = joint_accel_ref(ut, xt, Tt, [0, e + 1 - a], lam_v, lam_a)
            dead = ~np.isfinite(r["cost"])
            for lag in LAGS:
                path, cost = fixed[lag]
                for n in (range(max(a, e - lag), b) if e == b - 1 else ([e - lag] if e - lag >= a else [])):
                    assert np.array_equal(path[n], r["path"][n - a]), (lag, n, e)
                    for j in range(J):
                        if dead[n - a, j]:
                            assert np.isposinf(cost[n, j])
                            continue
                        c = n - a                                  # the end of n's chain on the truncated clip
                        while c + 1 <= e - a and not dead[c + 1, j]:
                            c += 1
                        one = (c == 0 or dead[c - 1, j])            # a chain of one frame: emin is not formed, the cost is min u
                        want = r["cost"][c, j] if one else r["emin"][c, j]
                        assert cost[n, j].view(np.int64) == np.float64(want).view(np.int64), (lag, n, j, e)


@pytest.mark.parametrize("lam_v,lam_a", WEIGHTS)
@pytest.mark.parametrize("J,N,H,L", SMALL, ids=lambda v: str(v))
def test_every_frame_is_the_offline_reference_on_the_truncated_clip(J, N, H, L, lam_v, lam_a):
    x, T, u = case(J, N, H)
    hold_to_truncated_clips(x, T, u, N, clips(N, L), lam_v, lam_a, tables(J, N, H, L, lam_v, lam_a))


@pytest.mark.parametrize("lam_v,lam_a", WEIGHTS)
def test_dead_joint_case_on_truncated_clips(lam_v, lam_a):
    """A dead (frame, joint) inside the lag window, chains that end before the horizon; the dead entry reports 0 and +inf."""
    x, T, u, j = dead_joint_case()
    tab = forward(u, x, T, [0, 9], lam_v, lam_a)
    hold_to_truncated_clips(x, T, u, 9, [0, 9], lam_v, lam_a, tab)
    for lag in LAGS:
        p, c = fixed_lag(tab, [0, 9], lag)
        assert p[4, j] == 0 and np.isposinf(c[4, j]) and np.isfinite(np.delete(c[:, j], 4)).all()


def test_a_lag_that_covers_the_clip_is_the_offline_path_and_lag_zero_the_arg_min_pair():
    for lam_v, lam_a in WEIGHTS:
        for J, N, H, L in ((3, 130, 7, 130), (5, 12, 3, 4)):
            x, T, u = case(J, N, H)
            tab, seq = tables(J, N, H, L, lam_v, lam_a), clips(N, L)
            r = joint_accel_ref(u, x, T, seq, lam_v, lam_a)
            for lag in (L - 1, L, 10 * L):
                assert np.array_equal(fixed_lag(tab, seq, lag)[0], r["path"])
            p0, c0 = fixed_lag(tab, seq, 0)
            assert np.array_equal(p0, np.where(tab["start"], tab["argq"], tab["argq"] % H)) and np.array_equal(c0, tab["argv"])


def test_the_inputs_are_what_the_exact_comparison_assumes():
    """At every live (n, j) of every case and weight pair the GPU tests use, the two smallest entries of E[n] (u at a chain's first
    frame) are more than GAP_MIN apart: no arg-min is left out of any comparison.  (The inner minima: _joint_accel_ref.check_inputs.)"""
    g = min(check_gaps(GPU_CASES), check_gaps([BIG], weights=(BIG_WEIGHTS,)))
    print(f"smallest gap between the two best entries at any horizon: {g:.3g}")
    assert g > GAP_MIN


def test_the_lag_matters_on_these_inputs():
    """The shares of (frame, joint) at which the fixed-lag decision differs from the whole-clip path, (17,70,50,35) in clips of 35: only
    their order is asserted - 0 at a lag that covers the clip, non-increasing from lag 0 to 8."""
    for lam_v, lam_a in WEIGHTS:
        shares = {lag: differ_share(17, 70, 50, 35, lam_v, lam_a, lag) for lag in LAGS + (34,)}
        print(f"differs from the whole-clip path at ({lam_v:g}, {lam_a:g}): " + ", ".join(f"lag {k}: {100 * v:.1f} %" for k, v in shares.items()))
        assert shares[34] == 0 and shares[8] > 0
        assert all(shares[a] >= shares[b] for a, b in zip(LAGS[:-1], LAGS[1:]))
