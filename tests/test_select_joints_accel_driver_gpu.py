"""GPU: `run.inference --select joints-temporal --accel LAMBDA2` - the J joint-wise chains of --select joints-temporal run with a
second-order motion term (zedo_joint_accel_select, lambda_v = --smooth, lambda_a = --accel); everything else of the run is what
--select joints-temporal does.  results.npy stays what it is; <out>_selected.npz holds joints-temporal's arrays plus `accel`,
joint_hypothesis is what the binding returns on the run's own rows (and what the numpy reference returns), joint_path_cost the
re-accumulated cost, the pose joint_compose of the paths.  --accel 0 gives the paths of the run without --accel; --seq_len 1 is --select
joints; the refusals.  Without --accel the driver's path is untouched: tests/test_select_joints_temporal_driver_gpu.py holds that.
Whether a second-order term lowers the error on real video is not measured: the inputs here are synthetic and the weights random.  The
selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _joint_accel_ref import cost_bound, joint_accel_ref
from _joint_ref import joint_reproj_ref
from _shared import _problem, _rows_and_T, cfg_path, dev, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S, L, LAM, ACC = 12, 3, 10, 5, 100.0, 100.0
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]
JT = ["--select", "joints-temporal", "--seq_len", str(L), "--smooth", "100"]
JT_ARRAYS = ("pose", "joint_hypothesis", "joint_hypothesis_per_frame", "joint_reproj_px", "joint_path_cost", "hypothesis", "T", "reproj_px",
             "reproj_px_pose_level", "seq_start", "smooth")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One process, five runs: without --select, joints-temporal without --accel, with --accel 100, with --accel 0, and --select joints."""
    import run.inference as inf
    d = tmp_path_factory.mktemp("accel")
    go = lambda name, extra: inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / name)] + extra))[0]
    res = {"plain": go("plain.npy", []), "first": go("first.npy", JT), "accel": go("accel.npy", JT + ["--accel", "100"]),
           "zero": go("zero.npy", JT + ["--accel", "0"]), "joints": go("joints.npy", ["--select", "joints"])}
    return d, res


def test_selected_npz_gains_accel_beside_an_unchanged_results_file(runs):
    import zedo_hip as zh
    d, res = runs
    a = np.load(d / "accel.npy")
    assert a.shape == (N, H, 17, 3) and a.tobytes() == np.load(d / "plain.npy").tobytes() == np.load(d / "first.npy").tobytes()
    assert np.array_equal(res["accel"], res["plain"])
    first, sel = np.load(d / "first_selected.npz"), np.load(d / "accel_selected.npz")
    assert sorted(first.files) == sorted(JT_ARRAYS) and sorted(sel.files) == sorted(JT_ARRAYS + ("accel",))
    assert sel["accel"].dtype == np.float64 and sel["accel"].shape == () and float(sel["accel"]) == ACC and float(sel["smooth"]) == LAM
    seq = clips(N, L)
    # what does not hang on the joint paths is the run without --accel, byte for byte
    for k in ("joint_hypothesis_per_frame", "hypothesis", "T", "reproj_px_pose_level", "seq_start", "smooth"):
        assert sel[k].dtype == first[k].dtype and sel[k].tobytes() == first[k].tobytes(), k
    # the joint paths and their costs: the binding on the run's own rows
    x, Tall = _rows_and_T(N, H, S)
    assert np.array_equal(x.reshape(H, N, 17, 3).permute(1, 0, 2, 3).cpu().numpy(), a)
    uv, K, conf = (dev(v) for v in _problem(N))
    jerr = zh.joint_reproj(x, Tall, uv, K, return_rows=True)[2]
    jpath, jcost = zh.joint_accel_select(jerr, x, Tall, seq, N, LAM, ACC)
    jh, jpc, hyp = sel["joint_hypothesis"], sel["joint_path_cost"], sel["hypothesis"]
    assert jh.dtype == np.int32 and jh.shape == (N, 17) and jpc.dtype == np.float64 and jpc.shape == (N, 17)
    assert np.array_equal(jh, jpath.cpu().numpy()) and jpc.tobytes() == jcost.cpu().numpy().tobytes()
    # independent of the library: float64 distances and the recurrence over pairs in numpy (the kernel's distances differ by at most
    # 1e-9 px: the reference's gap must be well above that, and a cost may differ by L times 1e-9 more than its bound)
    xn, Tn = x.cpu().numpy(), Tall.cpu().numpy()
    u_ref = joint_reproj_ref(xn, Tn, uv.cpu().numpy(), K.cpu().numpy())
    assert np.abs(jerr.cpu().numpy() - u_ref).max() <= 1e-9
    r = joint_accel_ref(u_ref, xn, Tn, seq, LAM, ACC)
    dlt = np.abs(jpc - r["cost"])
    print(f"joint paths against the numpy reference: gap {r['gap']:.3e}, max |joint_path_cost - ref| = {dlt.max():.3e}; they differ from the "
          f"run without --accel on {int((jh != first['joint_hypothesis']).sum())} of {N * 17} (frame, joint)")
    assert r["gap"] > 1e-6
    assert np.array_equal(jh, r["path"]) and (dlt <= cost_bound(L, r["cost"]) + L * 1e-9).all()
    # the pose is joint_compose of the written indices; the errors hang on them
    e3 = jerr.reshape(H, N, 17).cpu().numpy()
    assert sel["joint_reproj_px"].tobytes() == np.ascontiguousarray(e3[jh, np.arange(N)[:, None], np.arange(17)[None, :]]).tobytes()
    pose = zh.joint_compose(x, Tall, dev(jh, torch.int32), dev(hyp, torch.int32))
    assert sel["pose"].dtype == np.float32 and np.array_equal(sel["pose"].view(np.int32), pose.cpu().numpy().view(np.int32))
    _, again, _ = zh.min_reproj(pose, dev(sel["T"]), uv, K, conf)
    assert again.cpu().numpy().tobytes() == sel["reproj_px"].tobytes()


def test_accel_zero_gives_the_paths_of_the_run_without_accel(runs):
    d, _ = runs
    first, zero = np.load(d / "first_selected.npz"), np.load(d / "zero_selected.npz")
    assert float(zero["accel"]) == 0.0 and sorted(zero.files) == sorted(JT_ARRAYS + ("accel",))
    for k in JT_ARRAYS:
        if k != "joint_path_cost":                                   # the same terms, associated differently
            assert zero[k].dtype == first[k].dtype and zero[k].tobytes() == first[k].tobytes(), k
    assert (np.abs(zero["joint_path_cost"] - first["joint_path_cost"]) <= cost_bound(L, first["joint_path_cost"])).all()


def test_clips_of_one_frame_are_select_joints(runs, tmp_path):
    import run.inference as inf
    d, _ = runs
    inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(tmp_path / "single.npy"), "--select", "joints-temporal", "--seq_len", "1",
                                               "--accel", "100"]))
    single, joints = np.load(tmp_path / "single_selected.npz"), np.load(d / "joints_selected.npz")
    assert single["seq_start"].tolist() == list(range(N + 1)) and float(single["accel"]) == 100.0
    for k in ("joint_hypothesis", "hypothesis", "pose", "T", "reproj_px", "reproj_px_pose_level", "joint_reproj_px"):
        assert single[k].dtype == joints[k].dtype and single[k].tobytes() == joints[k].tobytes(), k
    assert single["joint_path_cost"].tobytes() == joints["joint_reproj_px"].tobytes()              # a chain of one frame costs its unary


def test_the_refusals():
    import run.inference as inf
    import run.opt_main as om
    go = lambda extra: inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy"] + extra))
    for sel in ("none", "reproj", "joints", "temporal", "joints-fused"):
        with pytest.raises(SystemExit) as e:
            go(["--select", sel, "--accel", "100"])
        assert "--accel is a switch of --select joints-temporal" in str(e.value), sel
    for bad in ("-2", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            go(JT + ["--accel", bad])
        assert "--accel" in str(e.value) and "finite weight >= 0" in str(e.value)
    with pytest.raises(SystemExit) as e:
        go(JT + ["--accel", "100", "--prune", "5:2"])
    assert "--prune with --select joints-temporal" in str(e.value)
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + JT + ["--accel", "100"]))
    assert "run.inference only" in str(e.value)
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + ["--accel", "100"]))
    assert "--accel is a switch of --select joints-temporal" in str(e.value)
