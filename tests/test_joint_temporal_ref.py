"""CPU: the numpy reference of the joint-wise temporal selection (tests/_joint_temporal_ref.py) pinned on its own - against the pose-level
reference of tests/_temporal_ref.py on every one-joint slice of x + T, against the enumeration of every path, the rules for excluded
entries and a dead (frame, joint) on a hand-built case, the conditions on the shared inputs that make an exact comparison of paths
honest, and the driver's argument checks.  Whether joint-wise temporal paths are closer to ground truth than the per-frame joint-wise
arg-min is not measured here or anywhere: these tests hold the arithmetic."""
import numpy as np
import pytest

from _joint_temporal_ref import (ALL_CASES, IDS, camera_frame, case, check_inputs, dead_joint_case, joint_temporal_ref, per_frame_argmin,
                                 reference)
from _temporal_ref import brute_force, clips, temporal_ref


def joint_slice(x, T, u, N, j):
    """Joint j as a one-joint problem of the pose-level reference: (x + T in float64 [H N,1,3], unaries [H N])."""
    X = camera_frame(x, T, N)
    return np.ascontiguousarray(X[:, :, j:j + 1, :]).reshape(-1, 1, 3), np.ascontiguousarray(u[:, j])


@pytest.mark.parametrize("J,N,H,L", ALL_CASES, ids=IDS)
def test_every_joint_is_the_pose_level_reference_on_its_slice(J, N, H, L):
    """With one joint the mean over the joints is that joint's term (0 + m, divided by 1: exact), so the two references evaluate the same
    statements: the same bits, with and without T."""
    x, T, u = case(J, N, H)
    for with_T, lam in ((True, 100.0), (False, 30.0)):
        r = reference(J, N, H, L, lam, with_T)
        for j in range(J):
            xs, us = joint_slice(x, T if with_T else None, u, N, j)
            t = temporal_ref(us, xs, clips(N, L), lam)
            assert np.array_equal(r["path"][:, j], t["path"]) and np.array_equal(r["cost"][:, j], t["cost"]), (j, with_T)
            assert np.array_equal(r["back"][:, j], t["back"]) and np.array_equal(r["D"][:, j], t["D"])


@pytest.mark.parametrize("J,H,L", [(3, 3, 4), (2, 2, 6), (1, 3, 3)])
@pytest.mark.parametrize("lam", [0.0, 30.0, 100.0])
def test_the_dynamic_programme_finds_the_best_of_all_paths_of_every_joint(J, H, L, lam):
    x, T, u = case(J, L, H)
    r = joint_temporal_ref(u, x, T, [0, L], lam)
    for j in range(J):
        xs, us = joint_slice(x, T, u, L, j)
        total, path = brute_force(us, xs, L, lam)
        assert np.array_equal(r["path"][:, j], path)
        assert r["cost"][-1, j] == total                            # the same additions in the same order: the same bits


def test_the_limits():
    """lambda = 0 and clips of one frame: the per-frame joint-wise arg-min; clips of one frame also return the unary itself."""
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    idx = per_frame_argmin(u, N)
    assert np.array_equal(joint_temporal_ref(u, x, T, clips(N, L), 0.0)["path"], idx)
    r = joint_temporal_ref(u, x, T, clips(N, 1), 100.0)
    best = u.reshape(H, N, J).min(0)
    assert np.array_equal(r["path"], idx) and np.array_equal(r["cost"], best) and (r["back"] == -1).all()


def test_a_dead_frame_joint_splits_only_that_joints_chain():
    x, T, u, j = dead_joint_case()
    H, N, J = 3, 9, 5
    clean = case(J, N, H)[2]
    for lam in (0.0, 100.0):
        r = joint_temporal_ref(u, x, T, [0, N], lam)
        c = joint_temporal_ref(clean, x, T, [0, N], lam)
        others = np.arange(J) != j
        assert np.array_equal(r["path"][:, others], c["path"][:, others]) and np.array_equal(r["cost"][:, others], c["cost"][:, others])
        assert r["path"][4, j] == 0 and np.isposinf(r["cost"][4, j]) and np.isposinf(r["D"][4, j]).all()
        ok = np.arange(N) != 4
        assert np.isfinite(r["cost"][ok, j]).all() and np.isfinite(r["cost"][:, others]).all()
        u3 = u.reshape(H, N, J)
        assert np.isfinite(u3[r["path"][ok, j], np.arange(N)[ok], j]).all()                   # an excluded entry is never on the path
        assert (r["back"][5, j] == -1).all() and (r["back"][0, j] == -1).all() and (r["back"][6, j] >= 0).all()
        assert (r["back"][5, others] >= 0).all()                                              # the other chains run through frame 4
        # that joint's two halves are the recurrence of the halves run alone, and the same as two clips cut at the dead frame
        x4, T3 = x.reshape(H, N, J, 3), T.reshape(H, N, 3)
        for lo, hi in ((0, 4), (5, 9)):
            half = joint_temporal_ref(u3[:, lo:hi].reshape(-1, J), x4[:, lo:hi].reshape(-1, J, 3), T3[:, lo:hi].reshape(-1, 3), [0, hi - lo], lam)
            assert np.array_equal(half["path"][:, j], r["path"][lo:hi, j]) and np.array_equal(half["cost"][:, j], r["cost"][lo:hi, j])
        cut = joint_temporal_ref(u, x, T, [0, 4, 5, N], lam)
        assert np.array_equal(cut["path"][:, j], r["path"][:, j]) and np.array_equal(cut["cost"][:, j], r["cost"][:, j])
    r = joint_temporal_ref(u, x, T, [0, N], 0.0)
    assert np.array_equal(r["path"][ok], per_frame_argmin(u, N)[ok])


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs()


def test_driver_accepts_joints_temporal_with_its_switches():
    """Argument checks that need no GPU: --select joints-temporal takes --smooth / --seq_len (default 100), refuses bad values; the other
    choices keep refusing the two switches."""
    from run._driver import build_parser, check_select_args
    p = build_parser("t", inference=True)
    base = ["--config", "c.py", "--select", "joints-temporal"]
    a = p.parse_args(base)
    check_select_args(a)
    assert a.select == "joints-temporal" and a.smooth == 100.0 and a.seq_len is None
    a = p.parse_args(base + ["--smooth", "0", "--seq_len", "7"])
    check_select_args(a)
    assert a.smooth == 0.0 and a.seq_len == 7
    for extra in (["--smooth", "-1"], ["--smooth", "nan"], ["--smooth", "inf"], ["--seq_len", "0"]):
        with pytest.raises(SystemExit):
            check_select_args(p.parse_args(base + extra))
    for sel in ("none", "reproj", "joints"):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(["--config", "c.py", "--select", sel, "--seq_len", "4"]))
        assert "--select temporal" in str(e.value) and "joints-temporal" in str(e.value)
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "c.py", "--select", "joint-temporal"])
