"""CPU: the numpy reference of the fixed-lag streaming fusion under the second-order motion model
(tests/_joint_accel_stream_marginal_ref.py) pinned on its own - every row against joint_accel_marginal_ref on the clip cut at the row's
horizon, bit for bit; against the enumeration of every path of the cut clip; a lag that covers the clip against the offline reference;
the check of the inputs that lets the GPU tests compare every arg-max; and the lag table of README.md, of which only the order is
asserted.  Whether a fixed-lag second-order fusion is closer to ground truth on real video is not measured here or anywhere."""
import numpy as np
import pytest

from _joint_accel_marginal_ref import WEIGHTS, accel_marg_bound, brute_force_chain, joint_accel_marginal_ref
from _joint_accel_marginal_ref import reference as offline_reference
from _joint_accel_stream_marginal_ref import LAGS, SMALL, check_inputs, distance_table, fixed_lag_accel_marginal, reference
from _joint_temporal_ref import camera_frame, case, dead_joint_case
from _temporal_ref import clips

EPS = 2.0 ** -53
KEYS = ("w", "mean", "cov", "hmax", "wmax", "logz")


def bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cut_rows(u, x, T, N, a, e):
    """The rows (h, n) of the frames a .. e of a case of N frames, h-major."""
    H = x.shape[0] // N
    rows = (np.arange(H)[:, None] * N + np.arange(a, e + 1)[None]).reshape(-1)
    return u[rows], x[rows], None if T is None else T[rows]


def held_to_the_cuts(u, x, T, N, seq, lam_v, lam_a, tau, lag):
    """Every row of fixed_lag_accel_marginal equals, bit for bit, the row of joint_accel_marginal_ref on its clip cut after frame
    min(n + lag, the clip's last)."""
    r = fixed_lag_accel_marginal(u, x, T, seq, lam_v, lam_a, tau, lag, N)
    for a, b in zip(seq[:-1], seq[1:]):
        for cut in range(a, b):
            ns = [n for n in range(a, b) if min(n + lag, b - 1) == cut]
            if not ns:
                continue
            ut, xt, Tt = cut_rows(u, x, T, N, a, cut)
            o = joint_accel_marginal_ref(ut, xt, Tt, [0, cut - a + 1], lam_v, lam_a, tau)
            for n in ns:
                for k in KEYS:
                    assert bits(r[k][n], o[k][n - a]), (lag, n, cut, k)
    return r


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (2, 11, 4, 3), (1, 20, 17, 20), (3, 26, 7, 26)], ids=lambda v: str(v))
def test_every_row_is_the_offline_reference_on_the_clip_cut_at_its_horizon(J, N, H, L):
    x, T, u = case(J, N, H)
    for lam_v, lam_a, tau in WEIGHTS[:2] if H > 7 else WEIGHTS:
        for lag in LAGS + (L - 1,):
            held_to_the_cuts(u, x, T, N, clips(N, L), lam_v, lam_a, tau, lag)


def test_a_dead_frame_joint_and_excluded_entries_on_the_cut_clips():
    """dead_joint_case: a chain that ends before the horizon, chains of one and two frames so far, excluded hypotheses."""
    x, T, u, j = dead_joint_case()
    for lag in LAGS:
        r = held_to_the_cuts(u, x, T, 9, [0, 9], 30.0, 100.0, 1.0, lag)
        assert r["dead"][4, j] and r["dead"].sum() == 1 and np.isnan(r["mean"][4, j]).all() and np.isneginf(r["logz"][4, j])
        assert r["e"][3, j] == 3 and r["e"][4, j] == -1 and r["e"][5, j] == min(5 + lag, 8)


def test_against_the_enumeration_of_all_paths():
    """(5, 12, 3, 4): per clip, frame and lag the 3^(e+1) paths of the clip cut after e = min(n + lag, 3)."""
    J, N, H, L = 5, 12, 3, 4
    x, T, u = case(J, N, H)
    X = camera_frame(x, T, N)
    for lam_v, lam_a, tau in ((0.0, 100.0, 1.0), (30.0, 300.0, 0.5)):
        for lag in (0, 1, 2, 3):
            r = fixed_lag_accel_marginal(u, x, T, clips(N, L), lam_v, lam_a, tau, lag)
            tol = accel_marg_bound(L, H, r["G"]) + 2.0 * (H ** L + 6.0 * L * r["G"] + 8.0) * EPS
            worst = 0.0
            for a in (0, 4, 8):
                for n in range(a, a + L):
                    e = min(n + lag, a + L - 1)
                    for j in range(J):
                        uj = u.reshape(H, N, J)[:, a:e + 1, j].T.copy()
                        w, lz = brute_force_chain(uj, X[:, a:e + 1, j].transpose(1, 0, 2), lam_v, lam_a, tau)
                        worst = max(worst, float(np.abs(np.log(r["w"][n, j]) - np.log(w[n - a])).max()), abs(r["logz"][n, j] - lz))
            print(f"lag {lag} lambda_v={lam_v:g} lambda_a={lam_a:g} tau={tau:g}: max |log w, logZ - enumeration| = {worst:.3e} (tolerance {tol:.3e})")
            assert worst <= tol


@pytest.mark.parametrize("J,N,H,L", SMALL, ids=lambda v: str(v))
def test_a_lag_that_covers_the_clip_is_the_offline_reference(J, N, H, L):
    lam_v, lam_a, tau = WEIGHTS[1]
    r, o = reference(J, N, H, L, lam_v, lam_a, tau, L - 1), offline_reference(J, N, H, L, lam_v, lam_a, tau)
    for k in KEYS:
        assert bits(r[k], o[k]), k
    assert r["G"] == o["G"]


def test_no_arg_max_is_left_out_of_a_comparison():
    """check_inputs: on SMALL at every lag and weight set the log-gap between the two largest marginals of every live (n, j) exceeds 1e-6
    and 100 x twice the largest accel_marg_bound."""
    gap, beta2 = check_inputs()
    assert gap > 1e-6 and gap > 100 * beta2


def test_the_lag_table_orders_as_expected():
    """The table of README.md at (lambda_v, lambda_a, tau) = (30, 100, 1), on a shape the numpy reference finishes in seconds: the
    distance to the whole-clip answer does not grow with the lag and is exactly zero once the lag covers the clip."""
    rows = distance_table()
    for lag, d_mean, tv, share in rows:
        print(f"lag {lag:2d}: median |mean - whole-clip mean| = {1000 * d_mean:.4f} mm, median total variation = {tv:.5f}, arg-max share = {share:.4f}")
    assert rows[-1][1:] == (0.0, 0.0, 1.0)
    assert rows[0][1] >= rows[-2][1] >= rows[-1][1] and rows[0][2] >= rows[-2][2] >= rows[-1][2] and rows[0][3] <= rows[-1][3]
