"""CPU: the float64 reference of the joint-wise aggregation (tests/_joint_ref.py) pinned on facts that hold by construction, so that the
GPU tests compare the kernels with something that has been checked itself."""
import numpy as np
import pytest

from _joint_ref import CASES, IDS, case, check_inputs, compose_ref, joint_reproj_ref, joint_select_ref
from _select_ref import reproj_ref, select_ref


def test_the_inputs_are_what_the_bounds_assume():
    check_inputs()


@pytest.mark.parametrize("J,N,H", CASES, ids=IDS)
def test_the_unweighted_row_mean_is_the_row_level_reference(J, N, H):
    x, T, uv, K, _ = case(J, N, H)
    d = joint_reproj_ref(x, T, uv, K)
    assert d.shape == (H * N, J)
    assert np.abs(d.mean(1) - reproj_ref(x, T, uv, K, None)).max() <= 1e-12
    lo = (H * N) // 3
    assert np.array_equal(joint_reproj_ref(x[lo:], T[lo:], uv, K, row_offset=lo), d[lo:])


@pytest.mark.parametrize("J,N,H", CASES, ids=IDS)
def test_the_mean_of_the_minima_is_at_most_the_minimum_of_the_means(J, N, H):
    """... for every pose, unweighted and with the clamped confidences as weights: a bound of the pose-level selection."""
    x, T, uv, K, conf = case(J, N, H)
    d = joint_reproj_ref(x, T, uv, K)
    best, idx = joint_select_ref(d, N)
    assert np.array_equal(best, d.reshape(H, N, J).min(0)) and np.array_equal(idx, d.reshape(H, N, J).argmin(0))
    assert (best.mean(1) <= d.mean(1).reshape(H, N).min(0)).all()
    w = np.clip(conf, np.float32(1e-4), 1).astype(np.float64)
    pose_level, _ = select_ref(reproj_ref(x, T, uv, K, conf), N)
    assert ((w * best).sum(1) / w.sum(1) <= pose_level + 1e-12).all()


def test_one_joint_behind_the_camera_is_infinite_alone_and_nan_falls_through():
    x, T, uv, K, _ = (a.copy() for a in case(5, 3, 5))
    full = joint_reproj_ref(x, T, uv, K)
    x[4, 1, 2] = -1.0 - T[4, 2]
    x[7, 2, 0] = np.nan
    d = joint_reproj_ref(x, T, uv, K)
    assert np.isposinf(d[4, 1]) and np.isnan(d[7, 2])
    mask = np.ones(d.shape, bool)
    mask[4, 1] = mask[7, 2] = False
    assert np.array_equal(d[mask], full[mask])
    assert np.isposinf(reproj_ref(x, T, uv, K)[4])                                  # the row-level call: the whole row
    best, idx = joint_select_ref(d, 3)
    assert np.isnan(best[7 % 3, 2]) and idx[7 % 3, 2] == 7 // 3 and idx[4 % 3, 1] != 4 // 3
    best, idx = joint_select_ref(d[4:6], 3, row_offset=4)                            # rows 4, 5 = (h 1, n 1), (h 1, n 2)
    assert (idx[0] == -1).all() and np.isposinf(best[0]).all() and (idx[1:] == 1).all() and np.isposinf(best[1, 1])


def test_compose_with_every_joint_from_the_reference_hypothesis_returns_its_x_exactly():
    J, N, H = 17, 70, 5
    x, T, uv, K, _ = case(J, N, H)
    g = np.random.Generator(np.random.Philox(key=[79, 1]))
    ref = g.integers(0, H, N).astype(np.int32)
    pose = compose_ref(x, T, np.repeat(ref[:, None], J, 1), ref)
    assert pose.dtype == np.float32 and np.array_equal(pose.view(np.int32), x.reshape(H, N, J, 3)[ref, np.arange(N)].view(np.int32))
    jh = g.integers(0, H, (N, J)).astype(np.int32)
    cam = compose_ref(x, T, jh)
    n, j = 11, 5
    want = x.reshape(H, N, J, 3)[jh[n, j], n, j].astype(np.float64) + T.reshape(H, N, 3)[jh[n, j], n].astype(np.float64)
    assert np.array_equal(cam[n, j], want.astype(np.float32))
    rel = compose_ref(x, T, jh, ref)
    assert np.array_equal(rel[n, j], (want - T.reshape(H, N, 3)[ref[n], n].astype(np.float64)).astype(np.float32))
    same = jh == ref[:, None]
    assert same.any() and np.array_equal(rel[same], x.reshape(H, N, J, 3)[ref, np.arange(N)][same])


def test_the_parser_accepts_select_joints():
    import run.inference as inf
    import run.opt_main as om
    assert inf.parse_args(["prog", "--config", "c.py", "--select", "joints"]).select == "joints"
    assert om.parse_args(["prog", "--config", "c.py", "--select", "joints"]).select == "joints"      # (refused when it runs)
    assert inf.parse_args(["prog", "--config", "c.py"]).select == "none"
