"""CPU: the numpy reference of the temporal selection (tests/_temporal_ref.py) pinned on its own - the dynamic programme against the
enumeration of every path, its limits (lambda = 0, clips of one frame), the rules for excluded rows and dead frames on a hand-built
case, and the conditions on the shared inputs that make an exact comparison of paths honest.  Whether a temporally consistent path is
closer to ground truth than the per-frame arg-min is not measured here or anywhere: these tests hold the arithmetic."""
import numpy as np
import pytest

from _select_ref import select_ref
from _temporal_ref import brute_force, case, check_inputs, clips, dead_frame_case, temporal_ref


@pytest.mark.parametrize("J,H,L", [(5, 3, 6), (1, 2, 7), (17, 4, 5)])
@pytest.mark.parametrize("lam", [0.0, 30.0, 100.0])
def test_the_dynamic_programme_finds_the_best_of_all_paths(J, H, L, lam):
    x, u = case(J, L, H)
    r = temporal_ref(u, x, [0, L], lam)
    total, path = brute_force(u, x, L, lam)
    assert np.array_equal(r["path"], path)
    assert r["cost"][-1] == total                                   # the same additions in the same order: the same bits
    # cost[n] is the best total of the paths that end in path[n] at frame n: non-decreasing by at least the frame's unary
    un = u.reshape(H, L)[r["path"], np.arange(L)]
    assert (np.diff(r["cost"]) >= un[1:] - 1e-12).all()


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (5, 12, 3, 4), (1, 7, 2, 7)])
def test_without_a_motion_cost_the_path_is_the_per_frame_arg_min(J, N, H, L):
    x, u = case(J, N, H)
    _, idx = select_ref(u, N)
    assert np.array_equal(temporal_ref(u, x, clips(N, L), 0.0)["path"], idx)


@pytest.mark.parametrize("lam", [0.0, 100.0, 1e6])
def test_clips_of_one_frame_are_decided_per_frame(lam):
    J, N, H = 17, 70, 50
    x, u = case(J, N, H)
    best, idx = select_ref(u, N)
    r = temporal_ref(u, x, clips(N, 1), lam)
    assert np.array_equal(r["path"], idx) and np.array_equal(r["cost"], best) and (r["back"] == -1).all()


def test_excluded_rows_and_dead_frames():
    x, u = dead_frame_case()
    H, N = 3, 9
    for lam in (0.0, 100.0):
        r = temporal_ref(u, x, [0, N], lam)
        assert r["path"][4] == 0 and np.isposinf(r["cost"][4]) and np.isposinf(r["D"][4]).all()
        ok = np.arange(N) != 4
        assert np.isfinite(r["cost"][ok]).all()
        u2 = u.reshape(H, N)
        assert np.isfinite(u2[r["path"][ok], np.arange(N)[ok]]).all()                       # an excluded row is never on the path
        assert (r["back"][5] == -1).all() and (r["back"][0] == -1).all() and (r["back"][6] >= 0).all()
        # both sides of the dead frame are the recurrence of the two halves run alone
        x4 = x.reshape(H, N, 5, 3)
        for lo, hi in ((0, 4), (5, 9)):
            half = temporal_ref(u2[:, lo:hi].reshape(-1), x4[:, lo:hi].reshape(-1, 5, 3), [0, hi - lo], lam)
            assert np.array_equal(half["path"], r["path"][lo:hi]) and np.array_equal(half["cost"], r["cost"][lo:hi])
        # and the same as two clips cut at the dead frame
        cut = temporal_ref(u, x, [0, 4, 5, N], lam)
        assert np.array_equal(cut["path"], r["path"]) and np.array_equal(cut["cost"], r["cost"])
    # at lambda = 0 the winner of frames 2 and 6 is the best of the rows that are left
    r = temporal_ref(u, x, [0, N], 0.0)
    v = np.where(np.isfinite(u.reshape(H, N)), u.reshape(H, N), np.inf)
    assert np.array_equal(r["path"][ok], np.argmin(v, axis=0)[ok])


def test_the_inputs_are_what_the_exact_comparison_assumes():
    check_inputs()


def test_dataset_clip_offsets(tmp_path):
    """CustomDataset: seq_start from the constructor or the npz, [0, N] without one; an array that is not strictly ascending from 0 to N
    is a ValueError, and so is sample_interval together with seq_start."""
    from lib.dataset.custom import CustomDataset
    N = 6
    db2, K = np.zeros((N, 17, 3), np.float32), np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
    assert CustomDataset(db2, K).seq_start.tolist() == [0, N] and CustomDataset(db2, K).seq_start.dtype == np.int32
    assert CustomDataset(db2, K, seq_start=[0, 2, 6]).seq_start.tolist() == [0, 2, 6]
    for bad in ([0, 2], [1, 6], [0, 3, 3, 6], [0, 4, 2, 6], [0, 7], [6], [[0, 6]], [0, 2.5, 6]):
        with pytest.raises(ValueError):
            CustomDataset(db2, K, seq_start=bad)
    with pytest.raises(ValueError):
        CustomDataset(db2, K, sample_interval=2, seq_start=[0, 2, 6])
    np.savez(tmp_path / "a.npz", db_2d=db2, camera_param=K, seq_start=np.array([0, 1, 6]))
    np.savez(tmp_path / "b.npz", db_2d=db2, camera_param=K)
    assert CustomDataset.from_npz(tmp_path / "a.npz").seq_start.tolist() == [0, 1, 6]
    assert CustomDataset.from_npz(tmp_path / "b.npz").seq_start.tolist() == [0, N]
    with pytest.raises(ValueError):
        CustomDataset.from_npz(tmp_path / "a.npz", sample_interval=2)
    assert CustomDataset.from_npz(tmp_path / "b.npz", sample_interval=2).seq_start.tolist() == [0, 3]


def test_driver_refuses_the_temporal_switches_where_they_do_not_apply():
    """Argument checks that need no GPU: --smooth / --seq_len without --select temporal, and non-positive values."""
    from run._driver import build_parser, check_select_args
    p = build_parser("t", inference=True)
    base = ["--config", "c.py"]
    for extra in (["--smooth", "50"], ["--seq_len", "5"], ["--select", "reproj", "--smooth", "50"], ["--select", "joints", "--seq_len", "4"]):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(base + extra))
        assert "--select temporal" in str(e.value)
    for extra in (["--select", "temporal", "--smooth", "-1"], ["--select", "temporal", "--smooth", "nan"], ["--select", "temporal", "--seq_len", "0"]):
        with pytest.raises(SystemExit):
            check_select_args(p.parse_args(base + extra))
    a = p.parse_args(base + ["--select", "temporal"])
    check_select_args(a)
    assert a.smooth == 100.0 and a.seq_len is None
    a = p.parse_args(base + ["--select", "temporal", "--smooth", "0", "--seq_len", "7"])
    check_select_args(a)
    assert a.smooth == 0.0 and a.seq_len == 7
