"""CPU: the numpy reference of the fixed-lag streaming fusion (tests/_joint_stream_marginal_ref.py) pinned on its own, before any kernel
is held to it: a row is the offline reference on the truncated clip, bit for bit; a lag that covers the clip is the offline reference;
small chains against the enumeration of every path; the inputs of the GPU comparisons leave no arg-max in doubt; and the measured
distance to the whole-clip answer does not grow with the lag."""
import numpy as np
import pytest

from _joint_marginal_ref import brute_force_chain, joint_marginal_ref, marg_bound
from _joint_marginal_ref import reference as offline_reference
from _joint_stream_marginal_ref import LAGS, check_inputs, distance_table, fixed_lag_marginal, horizons, reference
from _joint_temporal_ref import camera_frame, case, dead_joint_case
from _temporal_ref import clips

KEYS = ("w", "mean", "cov", "hmax", "wmax", "logz")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def cut(u, x, T, N, a, e):
    """The frames a .. e of the case as a clip of its own: rows (h, n) h-major."""
    H = x.shape[0] // N
    rows = (np.arange(H)[:, None] * N + np.arange(a, e + 1)[None, :]).reshape(-1)
    return u[rows], x[rows], T[rows]


@pytest.mark.parametrize("lag", (3, 8))
def test_a_row_is_the_offline_reference_on_the_truncated_clip(lag):
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    r = reference(J, N, H, L, 100.0, 1.0, lag)
    for a in (0, 35):
        for n in (0, 5, 17, 31, 34):
            e = min(n + lag, L - 1)
            assert (r["e"][a + n] == a + e).all()
            ut, xt, Tt = cut(u, x, T, N, a, a + e)
            o = joint_marginal_ref(ut, xt, Tt, [0, e + 1], 100.0, 1.0)
            for k in KEYS + ("A", "B"):
                assert same_bits(r[k][a + n], o[k][n]), (a, n, k)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (5, 12, 3, 4), (2, 30, 130, 13)], ids=lambda v: str(v))
def test_a_lag_that_covers_the_clip_is_the_offline_reference(J, N, H, L):
    r, o = reference(J, N, H, L, 100.0, 1.0, L - 1), offline_reference(J, N, H, L, 100.0, 1.0)
    for k in KEYS + ("A", "B", "dead"):
        assert same_bits(r[k], o[k]), k
    x, T, u, _ = dead_joint_case()
    r, o = fixed_lag_marginal(u, x, T, [0, 9], 100.0, 1.0, 8), joint_marginal_ref(u, x, T, [0, 9], 100.0, 1.0)
    for k in KEYS + ("A", "B", "dead"):
        assert same_bits(r[k], o[k]), k


def test_horizons_stop_at_a_dead_frame_and_at_the_clip_end():
    dead = np.zeros((9, 2), bool)
    dead[4, 1] = True
    e = horizons(dead, [0, 6, 9], 2)
    assert e[:, 0].tolist() == [2, 3, 4, 5, 5, 5, 8, 8, 8]
    assert e[:, 1].tolist() == [2, 3, 3, 3, -1, 5, 8, 8, 8]


@pytest.mark.parametrize("lag", (0, 1, 2))
def test_small_chains_match_the_enumeration_of_every_path(lag):
    """(5, 12, 3, 4): chains of four frames; dead_joint_case: a chain of nine split by a dead (frame, joint) - every row against
    brute_force_chain of the chain cut at the row's horizon, log-marginals within marg_bound."""
    for (x, T, u), seq in ((case(5, 12, 3), clips(12, 4)), (dead_joint_case()[:3], [0, 9])):
        N, H, J = seq[-1], 3, 5
        r = fixed_lag_marginal(u, x, T, seq, 100.0, 1.0, lag)
        X = camera_frame(x, T, N)
        uu = np.asarray(u, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()
        uu[~np.isfinite(uu)] = np.inf
        beta = marg_bound(max(b - a for a, b in zip(seq[:-1], seq[1:])), H, r["G"])
        checked, brute = 0, {}
        for n, j in zip(*np.nonzero(~r["dead"])):
            s = n
            while s - 1 >= max(a for a in seq[:-1] if a <= n) and not r["dead"][s - 1, j]:
                s -= 1
            e = r["e"][n, j]
            if (s, e, j) not in brute:                                # the frames of one chain that share a horizon share the enumeration
                brute[s, e, j] = brute_force_chain(uu[s:e + 1, j], X[:, s:e + 1, j].transpose(1, 0, 2), 100.0, 1.0)
            w, lz = brute[s, e, j]
            pos = w[n - s] > 0
            assert np.array_equal(pos, r["w"][n, j] > 0)
            assert np.abs(np.log(r["w"][n, j][pos]) - np.log(w[n - s][pos])).max() <= beta and abs(r["logz"][n, j] - lz) <= beta
            checked += 1
        assert checked == (60 if N == 12 else 44)


def test_the_inputs_leave_no_arg_max_in_doubt():
    gap, two_beta = check_inputs()
    assert gap > 1e-6 and two_beta < 1e-8


def test_a_longer_lag_is_closer_to_the_whole_clip_answer():
    rows = distance_table()
    for lag, dm, tv, diff in rows:
        print(f"lag {lag}: median |mean - whole-clip mean| = {dm * 1e3:.3g} mm, median total variation = {tv:.3g}, arg-max differs on "
              f"{100 * diff:.1f} %")
    d = [row[1] for row in rows]
    assert [row[0] for row in rows] == [0, 1, 3, 8, 34]
    assert d[0] >= d[1] >= d[2] >= d[3] >= d[4] == 0.0 and rows[4][2] == 0.0 and rows[4][3] == 0.0
    assert tuple(LAGS) == (0, 1, 3, 8)
