"""CPU: the numpy reference of the fusion along a video under the second-order motion model (tests/_joint_accel_marginal_ref.py) pinned
on its own - against the enumeration of every path, at lambda_a = 0 against the first-order reference of tests/_joint_marginal_ref.py,
chains of one and two frames, the order of the sums, the limit tau -> 0 against the paths of tests/_joint_accel_ref.py, the rules for
excluded entries and a dead (frame, joint), the property the model is built for - at lambda_v = 0 a common constant velocity changes no
marginal beyond the rounding of the moved positions - and the figure that motivates it.  Whether the fused second-order pose is closer to
ground truth on real video is not measured here or anywhere: these tests hold the arithmetic."""
import numpy as np
import pytest

from _joint_accel_marginal_ref import (COLD_CASES, COLD_TAU, accel_marg_bound, brute_force_chain, check_inputs, joint_accel_marginal_ref,
                                       reference)
from _joint_accel_ref import joint_accel_ref, moving_case
from _joint_marginal_ref import joint_marginal_ref, marg_bound, softmax_ref
from _joint_temporal_ref import camera_frame, case, dead_joint_case
from _temporal_ref import clips

EPS = 2.0 ** -53


def log_diff(w, w_ref, floor=1e-300):
    """max |log w - log w_ref| over the entries where the reference is above `floor`; the others must be tiny in w as well."""
    big = w_ref > floor
    assert (w[big] > 0).all()
    return float(np.abs(np.log(w[big]) - np.log(w_ref[big])).max())


@pytest.mark.parametrize("H,L", [(3, 6), (2, 10), (4, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("exclude", [False, True], ids=["all-finite", "one-excluded"])
def test_forward_backward_over_pairs_is_the_enumeration_of_all_paths(H, L, exclude):
    """Every joint of one clip of L frames against the enumeration of its H^L paths at two weight pairs: the marginals and logZ.  The
    enumeration adds H^L path weights (H^L eps relative) of energies accumulated over 3 L terms (under 6 L G eps on a path's -E / tau):
    the tolerance is accel_marg_bound plus twice that."""
    J = 2
    x, T, u = case(J, L, H)
    u = u.reshape(H, L, J).copy()
    if exclude:
        u[H - 1, L // 2, 0] = np.nan
        u[0, 0, 1] = np.inf
    u = u.reshape(H * L, J)
    X = camera_frame(x, T, L)
    for lam_v, lam_a, tau in ((0.0, 100.0, 1.0), (30.0, 300.0, 0.5)):
        r = joint_accel_marginal_ref(u, x, T, [0, L], lam_v, lam_a, tau)
        tol = accel_marg_bound(L, H, r["G"]) + 2.0 * (H ** L + 6.0 * L * r["G"] + 8.0) * EPS
        for j in range(J):
            uj = u.reshape(H, L, J)[:, :, j].T.copy()
            uj[~np.isfinite(uj)] = np.inf
            w, lz = brute_force_chain(uj, X[:, :, j].transpose(1, 0, 2), lam_v, lam_a, tau)
            e_w, e_z = log_diff(r["w"][:, j], w), float(np.abs(r["logz"][:, j] - lz).max())
            print(f"H={H} L={L} joint {j} lambda_v={lam_v:g} lambda_a={lam_a:g} tau={tau:g}: max |log w - enumeration| = {e_w:.3e}, "
                  f"|logZ - enumeration| = {e_z:.3e} (tolerance {tol:.3e})")
            assert e_w <= tol and e_z <= tol
            assert np.array_equal(r["w"][:, j] == 0.0, ~np.isfinite(uj)) and np.array_equal(w == 0.0, ~np.isfinite(uj))
            assert (np.abs(r["w"][:, j].sum(1) - 1.0) <= tol).all()


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (3, 130, 7, 130), (2, 9, 63, 9)], ids=lambda v: str(v))
def test_without_the_second_order_term_the_marginals_are_the_first_order_ones(J, N, H, L):
    """lambda_a = 0: the chain over pairs is the first-order chain - the log-marginals and logZ of joint_marginal_ref within the sum of the
    two bounds, with and without T."""
    x, T, u = case(J, N, H)
    for Tq, lam, tau in ((T, 100.0, 1.0), (None, 30.0, 0.25)):
        first = joint_marginal_ref(u, x, Tq, clips(N, L), lam, tau)
        r = joint_accel_marginal_ref(u, x, Tq, clips(N, L), lam, 0.0, tau)
        tol = marg_bound(min(L, N), H, first["G"]) + accel_marg_bound(min(L, N), H, r["G"])
        e_w, e_z = log_diff(r["w"], first["w"]), float(np.abs(r["logz"] - first["logz"]).max())
        print(f"lambda_a = 0, J={J} N={N} H={H} L={L} lambda={lam:g} tau={tau:g}: max |log w - first order| = {e_w:.3e}, |logZ| {e_z:.3e} "
              f"(sum of the bounds {tol:.3e})")
        assert e_w <= tol and e_z <= tol
        assert np.array_equal(r["hmax"], first["hmax"])


def test_chains_of_one_frame_are_a_softmax_and_chains_of_two_are_first_order():
    """Clips of one frame: w is the per-(frame, joint) softmax of -u / tau, whatever the weights.  Clips of two frames have no second
    difference: the first-order marginals, whatever lambda_a."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    sm = softmax_ref(u, N, 0.5)
    r = joint_accel_marginal_ref(u, x, T, clips(N, 1), 30.0, 1e6, 0.5)
    tol = accel_marg_bound(1, H, r["G"]) + 2.0 ** -52 * max(1.0, float(np.abs(np.log(sm)).max()))
    assert log_diff(r["w"], sm) <= tol and np.isnan(r["A2"]).all()
    u3 = u.reshape(H, N, J).transpose(1, 2, 0)
    assert np.array_equal(r["hmax"], np.argmin(u3, axis=2))
    first = joint_marginal_ref(u, x, T, clips(N, 2), 30.0, 0.5)
    for lam_a in (0.0, 100.0, 1e6):
        two = joint_accel_marginal_ref(u, x, T, clips(N, 2), 30.0, lam_a, 0.5)
        tol = marg_bound(2, H, first["G"]) + accel_marg_bound(2, H, two["G"])
        assert log_diff(two["w"], first["w"]) <= tol and np.abs(two["logz"] - first["logz"]).max() <= tol
    # the marginals of a chain of two do not depend on lambda_a at all: no term carries it
    a, b = joint_accel_marginal_ref(u, x, T, clips(N, 2), 30.0, 0.0, 0.5), joint_accel_marginal_ref(u, x, T, clips(N, 2), 30.0, 1e6, 0.5)
    assert np.array_equal(a["w"], b["w"])


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (1, 20, 17, 20), (3, 130, 7, 130), (2, 9, 63, 9)], ids=lambda v: str(v))
def test_the_order_of_the_sums_stays_inside_the_bound(J, N, H, L):
    x, T, u = case(J, N, H)
    up = joint_accel_marginal_ref(u, x, T, clips(N, L), 30.0, 100.0, 1.0)
    down = joint_accel_marginal_ref(u, x, T, clips(N, L), 30.0, 100.0, 1.0, descending=True)
    beta = accel_marg_bound(min(L, N), H, up["G"])
    e = max(log_diff(down["w"], up["w"]), float(np.abs(down["logz"] - up["logz"]).max()), float(np.abs(down["w"].sum(2) - 1.0).max()))
    print(f"J={J} N={N} H={H} L={L}: ascending against descending sums: {e:.3e} of a bound of {beta:.3e} ({100 * e / beta:.2f} %)")
    assert e <= beta


def test_the_inputs_are_what_the_exact_comparisons_assume():
    check_inputs()


@pytest.mark.parametrize("J,N,H,L", COLD_CASES, ids=lambda v: str(v))
def test_a_cold_chain_is_the_second_order_viterbi_path(J, N, H, L):
    """tau = 1e-9 on every case the GPU test uses for this limit: first wmax >= 0.99 on EVERY live (frame, joint) - the condition under
    which the comparison means something - then the arg-max is joint_accel_ref's path, everywhere."""
    x, T, u = case(J, N, H)
    r = reference(J, N, H, L, 30.0, 100.0, COLD_TAU)
    live = ~r["dead"]
    assert live.all() and (r["wmax"][live] >= 0.99).all()
    path = joint_accel_ref(u, x, T, clips(N, L), 30.0, 100.0)["path"]
    assert np.array_equal(r["hmax"], path)


def test_a_dead_frame_joint_and_excluded_entries():
    """The hand-built case of _joint_temporal_ref.dead_joint_case ((frame 4, joint 2) dead, excluded entries at frames 2 and 6): the dead
    entry reports NaN, 0, 0 and -inf and a row of zeros, that joint's chain splits there (two values of logz), excluded entries have w = 0
    exactly, and the other joints return the bits of the untouched unaries.  With (frame 1, joint 2) dead as well the joint has chains
    of one and of two frames, which give those chains' own answers."""
    x, T, u, j = dead_joint_case()
    H, N, J = 3, 9, 5
    clean = case(J, N, H)[2]
    for lam_v, lam_a in ((0.0, 100.0), (30.0, 100.0)):
        r = joint_accel_marginal_ref(u, x, T, [0, N], lam_v, lam_a, 1.0)
        c = joint_accel_marginal_ref(clean, x, T, [0, N], lam_v, lam_a, 1.0)
        others = np.arange(J) != j
        for k in ("w", "mean", "cov", "hmax", "wmax", "logz"):
            assert np.array_equal(r[k][:, others], c[k][:, others]), k
        dead = np.zeros((N, J), bool)
        dead[4, j] = True
        assert np.array_equal(r["dead"], dead)
        assert np.array_equal(np.isnan(r["mean"]).any(2), dead) and np.array_equal(np.isnan(r["cov"]).any(2), dead)
        assert np.array_equal(np.isneginf(r["logz"]), dead) and r["hmax"][4, j] == 0 and r["wmax"][4, j] == 0.0 and (r["w"][4, j] == 0.0).all()
        assert len(set(r["logz"][:4, j].tolist())) == 1 and len(set(r["logz"][5:, j].tolist())) == 1 and r["logz"][3, j] != r["logz"][5, j]
        excluded = ~np.isfinite(u.reshape(H, N, J).transpose(1, 2, 0))
        assert excluded.sum() == 5 and (r["w"][excluded] == 0.0).all() and (r["w"][~excluded & ~dead[:, :, None]] > 0.0).all()
        assert (np.abs(r["w"].sum(2)[~dead] - 1.0) <= accel_marg_bound(N, H, r["G"])).all()
        v = u.reshape(H, N, J).copy()
        v[:, 1, j] = np.nan                                          # joint j: chains [0, 1), [2, 4) and [5, 9)
        v = v.reshape(H * N, J)
        r2 = joint_accel_marginal_ref(v, x, T, [0, N], lam_v, lam_a, 1.0)
        with np.errstate(invalid="ignore"):                          # the dead (frame, joint) of v: inf - inf, not looked at
            sm = softmax_ref(v, N, 1.0)
        assert log_diff(r2["w"][0, j], sm[0, j]) <= accel_marg_bound(1, H, r2["G"]) + 2.0 ** -51 * max(1.0, float(np.abs(np.log(sm[0, j][sm[0, j] > 0])).max()))
        first = joint_marginal_ref(v, x, T, [0, N], lam_v, 1.0)
        assert log_diff(r2["w"][2:4, j], first["w"][2:4, j]) <= marg_bound(2, H, first["G"]) + accel_marg_bound(2, H, r2["G"])
        assert np.array_equal(r2["w"][5:, j], r["w"][5:, j]) and np.array_equal(r2["logz"][5:, j], r["logz"][5:, j])


def velocity_bound(L, c_a, rho):
    """How far a log-marginal can move when every coordinate of X is perturbed by at most rho: a second difference moves by at most
    (1 + 2 + 1) rho per coordinate, its norm by sqrt(3) 4 rho, a path's energy over tau by c_a times that per frame, over at most L
    frames; a log-marginal is the difference of two log-sums of path weights, each of which moves by at most what a path's does."""
    return 2.0 * L * c_a * 4.0 * np.sqrt(3.0) * rho


def test_a_constant_velocity_changes_no_marginal_at_lambda_v_zero():
    """lambda_v = 0: n v added to the float64 camera-frame X of every hypothesis (v = 10 cm per frame on every coordinate).  The second
    difference of n v is zero, so only the rounding of X + n v remains: at most 2^-53 (max|X| + N v) per coordinate.  The bound is
    velocity_bound at that perturbation plus the evaluation bound of the two runs."""
    J, N, H, L = 3, 60, 12, 60
    x, T, u = case(J, N, H)
    X = camera_frame(x, T, N)
    v = 0.10
    Xv = X + v * np.arange(N)[None, :, None, None]
    a = joint_accel_marginal_ref(u, X.reshape(H * N, J, 3), None, [0, N], 0.0, 100.0, 1.0)
    b = joint_accel_marginal_ref(u, Xv.reshape(H * N, J, 3), None, [0, N], 0.0, 100.0, 1.0)
    rho = EPS * (float(np.abs(X).max()) + N * v)
    tol = velocity_bound(L, 100.0, rho) + accel_marg_bound(L, H, max(a["G"], b["G"]))
    e = max(log_diff(b["w"], a["w"], 1e-250), float(np.abs(b["logz"] - a["logz"]).max()))
    print(f"J={J} N={N} H={H}: 10 cm per frame of common velocity at lambda_v = 0 moves a log-marginal by at most {e:.3e} (bound {tol:.3e})")
    assert e <= tol
    # the first-order chain is not blind to it
    f0, fv = (joint_marginal_ref(u, Y.reshape(H * N, J, 3), None, [0, N], 100.0, 1.0) for Y in (X, Xv))
    assert log_diff(fv["w"], f0["w"], 1e-250) > 1e3 * tol


def test_the_motivating_statistic():
    """moving_case(3, 60, 12, v) at v = 0 and v = 10 cm per frame, tau = 1: the median over (frame, joint) of the largest marginal, for
    the first-order reference (lambda = 100) and for this one (lambda_v = 0, lambda_a = 100).  Printed; asserted is only the direction the
    model implies: the second-order median does not drop with v beyond what the one fp32 rounding of the moved x (2^-24 (max|X| + N v) per
    coordinate) can move a marginal by - velocity_bound in the exponent."""
    J, N, H = 3, 60, 12
    med = {}
    for v in (0.0, 0.10):
        x, T, u = moving_case(J, N, H, v)
        med["first", v] = float(np.median(joint_marginal_ref(u, x, T, [0, N], 100.0, 1.0)["wmax"]))
        r = joint_accel_marginal_ref(u, x, T, [0, N], 0.0, 100.0, 1.0)
        med["second", v] = float(np.median(r["wmax"]))
        xmax = float(np.abs(camera_frame(x, T, N)).max())
    tol = float(np.expm1(velocity_bound(N, 100.0, 2.0 ** -24 * (xmax + N * 0.10)) + accel_marg_bound(N, H, r["G"])))
    print(f"J={J} N={N} H={H}, tau 1, 10 cm per frame of common velocity: median largest marginal, first order (lambda 100) "
          f"{med['first', 0.0]:.4f} -> {med['first', 0.10]:.4f}; second order (lambda_v 0, lambda_a 100) {med['second', 0.0]:.4f} -> "
          f"{med['second', 0.10]:.4f} (allowed drop {tol:.4f})")
    assert med["second", 0.10] >= med["second", 0.0] - tol
