"""CPU: the numpy reference of the joint-wise selection with a second-order motion model (tests/_joint_accel_ref.py) pinned on its own -
against the enumeration of every path, at lambda_a = 0 against the first-order reference of tests/_joint_temporal_ref.py, the rules for
excluded entries and a dead (frame, joint), the condition on the shared inputs that makes an exact comparison of paths honest, the
property the model is built for - a common constant velocity changes the first-order selection and not the second-order one - and the
driver's argument checks.  Whether the second-order paths are closer to ground truth on real video is not measured here or anywhere:
these tests hold the arithmetic."""
import numpy as np
import pytest

from _joint_accel_ref import brute_force, check_inputs, cost_bound, joint_accel_ref, moving_case
from _joint_temporal_ref import case, dead_joint_case, joint_temporal_ref, per_frame_argmin
from _temporal_ref import clips, switch_rate

PAIRS = ((0.0, 100.0), (30.0, 300.0), (100.0, 0.0))                          # (lambda_v, lambda_a)


@pytest.mark.parametrize("J,N,H,L", [(2, 7, 2, 7), (2, 12, 3, 4), (1, 6, 4, 6), (1, 5, 5, 5)], ids=lambda v: str(v))
def test_the_dynamic_programme_over_pairs_finds_the_best_of_all_paths(J, N, H, L):
    """Every clip of every joint against the enumeration of its H^L paths (the last clip may be shorter): the same path, and the
    re-accumulated cost of the last frame is the enumeration's total, bit for bit - the same additions in the same order."""
    x, T, u = case(J, N, H)
    x4, T3, u3 = x.reshape(H, N, J, 3), T.reshape(H, N, 3), u.reshape(H, N, J)
    seq = clips(N, L)
    for lam_v, lam_a in PAIRS:
        r = joint_accel_ref(u, x, T, seq, lam_v, lam_a)
        assert r["gap"] > 1e-8
        for a, b in zip(seq[:-1], seq[1:]):
            xs, Ts, us = (np.ascontiguousarray(v[:, a:b]).reshape((-1,) + v.shape[2:]) for v in (x4, T3, u3))
            for j in range(J):
                total, path = brute_force(us, xs, Ts, b - a, j, lam_v, lam_a)
                assert np.array_equal(r["path"][a:b, j], path), (lam_v, lam_a, a, j)
                assert r["cost"][b - 1, j] == total
                # E is accumulated in another order than the cost along the path: equal up to rounding
                assert abs(r["emin"][b - 1, j] - total) <= cost_bound(b - a, total)


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (17, 70, 50, 35), (3, 130, 7, 130), (2, 9, 63, 9)], ids=lambda v: str(v))
def test_without_the_second_order_term_the_paths_are_the_first_order_ones(J, N, H, L):
    """lambda_a = 0: the chain over pairs minimises the objective of joint_temporal_ref - the same paths, with and without T, and costs
    within 8 L 2^-53 relative (the first-order cost is D along the path: the same terms, associated differently)."""
    x, T, u = case(J, N, H)
    for with_T, lam in ((True, 100.0), (False, 30.0)):
        first = joint_temporal_ref(u, x, T if with_T else None, clips(N, L), lam)
        r = joint_accel_ref(u, x, T if with_T else None, clips(N, L), lam, 0.0)
        assert first["gap"] > 1e-6 and r["gap"] > 1e-8
        assert np.array_equal(r["path"], first["path"])
        assert (np.abs(r["cost"] - first["cost"]) <= cost_bound(L, first["cost"])).all()


def test_the_limits():
    """Clips of one and two frames: no second difference exists - a clip of one frame keeps the per-frame joint arg-min and its unary, a
    clip of two is the first-order chain whatever lambda_a; lambda_v = lambda_a = 0 is the per-frame arg-min at any clip length."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    idx, best = per_frame_argmin(u, N), u.reshape(H, N, J).min(0)
    r = joint_accel_ref(u, x, T, clips(N, 1), 30.0, 100.0)
    assert np.array_equal(r["path"], idx) and np.array_equal(r["cost"], best)
    two = joint_accel_ref(u, x, T, clips(N, 2), 30.0, 1e6)
    first = joint_temporal_ref(u, x, T, clips(N, 2), 30.0)
    assert np.array_equal(two["path"], first["path"]) and (np.abs(two["cost"] - first["cost"]) <= cost_bound(2, first["cost"])).all()
    assert np.array_equal(joint_accel_ref(u, x, T, clips(N, 4), 0.0, 0.0)["path"], idx)


def test_a_dead_frame_joint_splits_only_that_joints_chain():
    """The hand-built case of _joint_temporal_ref.dead_joint_case: (frame 4, joint 2) is dead, frames 2 and 6 have excluded entries.  The
    other joints are untouched; the dead entry reports 0 and +inf; no excluded entry is on the path; that joint's two halves are the
    halves run alone; and dead entries placed so that chains of one and of two frames arise give those chains' own answers."""
    x, T, u, j = dead_joint_case()
    H, N, J = 3, 9, 5
    clean = case(J, N, H)[2]
    x4, T3, u3 = x.reshape(H, N, J, 3), T.reshape(H, N, 3), u.reshape(H, N, J)
    for lam_v, lam_a in ((0.0, 100.0), (30.0, 100.0)):
        r = joint_accel_ref(u, x, T, [0, N], lam_v, lam_a)
        c = joint_accel_ref(clean, x, T, [0, N], lam_v, lam_a)
        others = np.arange(J) != j
        assert np.array_equal(r["path"][:, others], c["path"][:, others]) and np.array_equal(r["cost"][:, others], c["cost"][:, others])
        assert r["path"][4, j] == 0 and np.isposinf(r["cost"][4, j])
        ok = np.arange(N) != 4
        assert np.isfinite(r["cost"][ok, j]).all() and np.isfinite(u3[r["path"][ok, j], np.arange(N)[ok], j]).all()
        for lo, hi in ((0, 4), (5, 9)):
            half = joint_accel_ref(u3[:, lo:hi].reshape(-1, J), x4[:, lo:hi].reshape(-1, J, 3), T3[:, lo:hi].reshape(-1, 3), [0, hi - lo],
                                   lam_v, lam_a)
            assert np.array_equal(half["path"][:, j], r["path"][lo:hi, j]) and np.array_equal(half["cost"][:, j], r["cost"][lo:hi, j])
        # frames 1 and 4 dead: joint j's chains are [0, 1) - one frame -, [2, 4) - two frames - and [5, 9)
        v = u3.copy()
        v[:, 1, j] = np.nan
        r = joint_accel_ref(v.reshape(-1, J), x, T, [0, N], lam_v, lam_a)
        assert r["path"][0, j] == per_frame_argmin(v.reshape(-1, J), N)[0, j] and r["cost"][0, j] == np.nanmin(v[:, 0, j])
        first = joint_temporal_ref(v.reshape(-1, J), x, T, [0, N], lam_v)
        assert np.array_equal(r["path"][2:4, j], first["path"][2:4, j])
        assert (np.abs(r["cost"][2:4, j] - first["cost"][2:4, j]) <= cost_bound(2, first["cost"][2:4, j])).all()
        assert r["path"][1, j] == 0 and np.isposinf(r["cost"][[1, 4], j]).all()


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs()


def test_a_common_velocity_moves_the_first_order_selection_and_not_the_second_order_one():
    """Every hypothesis of a case gets n v added (v = 10 cm per frame, the shifted case built in float64 and rounded to fp32 once).  The
    first-order reference then switches hypothesis more often: the common motion sits under its square root and makes a switch cheap.
    The second-order reference at lambda_v = 0 keeps its path on at least 99 % of (frame, joint): the second difference of n v is zero,
    and the fp32 rounding of the shifted x is the only source of change."""
    J, N, H, lam = 3, 60, 12, 100.0
    x, T, u = case(J, N, H)
    x0, _, _ = moving_case(J, N, H, 0.0)
    assert np.array_equal(x0, x)                                   # the same draws
    xv, _, _ = moving_case(J, N, H, 0.10)
    seq = [0, N]
    rate = lambda p: float(np.mean([switch_rate(p[:, j], seq) for j in range(J)]))
    f0, fv = joint_temporal_ref(u, x, T, seq, lam)["path"], joint_temporal_ref(u, xv, T, seq, lam)["path"]
    s0, sv = joint_accel_ref(u, x, T, seq, 0.0, lam)["path"], joint_accel_ref(u, xv, T, seq, 0.0, lam)["path"]
    same = float((s0 == sv).mean())
    print(f"J={J} N={N} H={H}, lambda 100, 10 cm per frame of common velocity: first-order switches {100 * rate(f0):.0f} % -> "
          f"{100 * rate(fv):.0f} % of transitions; second-order {100 * rate(s0):.0f} % -> {100 * rate(sv):.0f} %, the same hypothesis on "
          f"{100 * same:.1f} % of (frame, joint)")
    assert rate(fv) > rate(f0)
    assert same >= 0.99


def test_driver_accepts_accel_with_joints_temporal_only():
    """Argument checks that need no GPU: --accel is a switch of --select joints-temporal, has no default, leaves --smooth at its default of
    100, and refuses a negative or non-finite value; every other --select refuses it in words of its own."""
    from run._driver import build_parser, check_select_args
    p = build_parser("t", inference=True)
    base = ["--config", "c.py", "--select", "joints-temporal"]
    a = p.parse_args(base)
    check_select_args(a)
    assert a.accel is None and a.smooth == 100.0
    a = p.parse_args(base + ["--accel", "250"])
    check_select_args(a)
    assert a.accel == 250.0 and a.smooth == 100.0 and a.seq_len is None
    a = p.parse_args(base + ["--accel", "0", "--smooth", "0", "--seq_len", "7"])
    check_select_args(a)
    assert a.accel == 0.0 and a.smooth == 0.0 and a.seq_len == 7
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(base + ["--accel", bad]))
        assert "--accel" in str(e.value)
    for sel in ("none", "reproj", "joints", "temporal", "joints-fused"):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(["--config", "c.py", "--select", sel, "--accel", "100"]))
        assert "--accel is a switch of --select joints-temporal" in str(e.value)
    with pytest.raises(SystemExit) as e:                                # run.opt_main has the switch in its parser and refuses it too
        check_select_args(build_parser("t").parse_args(["--config", "c.py", "--accel", "100"]))
    assert "--accel" in str(e.value)
