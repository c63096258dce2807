"""GPU: `run.inference --select joints-temporal` - the frames are a video and the pose is assembled joint by joint: per clip and per joint
the hypothesis sequence that minimises that joint's reprojection distance plus --smooth times that joint's displacement in the camera
frame (zedo_joint_reproj + zedo_joint_temporal_select + zedo_joint_compose), written in the frame of the pose-level temporal path
(zedo_min_reproj + zedo_temporal_select).  results.npy stays what it is; beside it <out>_selected.npz holds the assembled pose, both
paths, what --select joints would keep, the errors, the path costs, the clips and the weight.  --seq_len 1 is --select joints; --eval;
the refusals; two real ranks on one GPU (gloo rehearsal transport) against the one-rank run.
The weighted reprojection error of the assembled pose and the switch rates are PRINTED, not asserted: nobody has measured them on this
path, and whether joint-wise temporal paths are closer to ground truth on real video is not measured at all - the inputs here are
synthetic and the weights random.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import os

import numpy as np
import pytest

from _joint_ref import compose_ref, joint_reproj_ref
from _joint_temporal_ref import joint_temporal_ref
from _shared import _inference, _problem, _rows_and_T, cfg_path, dev, run_two_ranks, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)
from _temporal_ref import clips, cost_bound, switch_rate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S, L, LAM = 12, 3, 10, 5, 100.0
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]
JT = ["--select", "joints-temporal", "--seq_len", str(L), "--smooth", "100"]
ARRAYS = ("pose", "joint_hypothesis", "joint_hypothesis_per_frame", "joint_reproj_px", "joint_path_cost", "hypothesis", "T", "reproj_px",
          "reproj_px_pose_level", "seq_start", "smooth")


def _check_selected(sel, results, seq, lam=LAM):
    """The eleven arrays with their dtypes and shapes, and every one of them recomputed through the binding from results.npy and the
    loop's translations; the joint paths and their costs also by the numpy references in float64 on the run's rows (distances of
    _joint_ref.joint_reproj_ref, recurrence of _joint_temporal_ref.joint_temporal_ref): a driver that handed the call no T, or a library
    that ignored it, does not pass."""
    import zedo_hip as zh
    assert sorted(sel.files) == sorted(ARRAYS)
    pose, jh, jpf, jpx, jpc, hyp, T, px, px_pose, ss, smooth = (sel[k] for k in ARRAYS)
    assert pose.shape == (N, 17, 3) and pose.dtype == np.float32 and T.shape == (N, 3) and T.dtype == np.float32
    for a in (jh, jpf):
        assert a.shape == (N, 17) and a.dtype == np.int32 and ((a >= 0) & (a < H)).all()
    for a in (jpx, jpc):
        assert a.shape == (N, 17) and a.dtype == np.float64 and np.isfinite(a).all()
    assert hyp.shape == (N,) and hyp.dtype == np.int32 and ((hyp >= 0) & (hyp < H)).all()
    assert px.shape == (N,) and px.dtype == np.float64 and px_pose.shape == (N,) and px_pose.dtype == np.float64
    assert ss.dtype == np.int32 and ss.tolist() == list(seq) and smooth.dtype == np.float64 and smooth.shape == () and float(smooth) == lam
    x, Tall = _rows_and_T(N, H, S)
    assert np.array_equal(x.reshape(H, N, 17, 3).permute(1, 0, 2, 3).cpu().numpy(), results)
    uv, K, conf = (dev(a) for a in _problem(N))
    best0, idx0, jerr = zh.joint_reproj(x, Tall, uv, K, return_rows=True)
    err = zh.min_reproj(x, Tall, uv, K, conf)[0]
    path, _ = zh.temporal_select(err, x, seq, N, lam)
    jpath, jcost = zh.joint_temporal_select(jerr, x, Tall, seq, N, lam)
    assert np.array_equal(jh, jpath.cpu().numpy()) and jpc.tobytes() == jcost.cpu().numpy().tobytes()
    assert np.array_equal(jpf, idx0.cpu().numpy()) and np.array_equal(hyp, path.cpu().numpy())
    # independent of the library: float64 distances and recurrence in numpy (the kernel's distances differ by at most 1e-9 px, so an
    # exact comparison of paths needs the reference's gap well above that, and a cost may differ by L times 1e-9 more than its bound)
    u_ref = joint_reproj_ref(x.cpu().numpy(), Tall.cpu().numpy(), uv.cpu().numpy(), K.cpu().numpy())
    assert np.abs(jerr.cpu().numpy() - u_ref).max() <= 1e-9
    r = joint_temporal_ref(u_ref, x.cpu().numpy(), Tall.cpu().numpy(), seq, lam)
    Lmax = int(np.diff(seq).max())
    d = np.abs(jpc - r["cost"])
    with_no_T = joint_temporal_ref(u_ref, x.cpu().numpy(), None, seq, lam)["path"]
    print(f"joint paths against the numpy reference: gap {r['gap']:.3e}, max |joint_path_cost - ref| = {d.max():.3e}; the reference "
          f"without T differs on {int((with_no_T != r['path']).sum())} of {N * 17} (frame, joint)")
    assert r["gap"] > 1e-6
    assert np.array_equal(jh, r["path"]) and (d <= cost_bound(1, Lmax, r["cost"]) + Lmax * 1e-9).all()
    e3 = jerr.reshape(H, N, 17).cpu().numpy()
    assert jpx.tobytes() == np.ascontiguousarray(e3[jh, np.arange(N)[:, None], np.arange(17)[None, :]]).tobytes()
    assert px_pose.tobytes() == np.ascontiguousarray(err.reshape(H, N).cpu().numpy()[hyp, np.arange(N)]).tobytes()
    assert np.array_equal(T, Tall.reshape(H, N, 3).cpu().numpy()[hyp, np.arange(N)])
    # pose = joint_compose of the written indices, and the compose formula in numpy
    assert np.array_equal(pose.view(np.int32), zh.joint_compose(x, Tall, dev(jh, torch.int32), dev(hyp, torch.int32)).cpu().numpy().view(np.int32))
    assert np.array_equal(pose.view(np.int32), compose_ref(x.cpu().numpy(), Tall.cpu().numpy(), jh, hyp).view(np.int32))
    own = jh == hyp[:, None]                                         # a joint taken from the frame's own hypothesis is results' bits
    assert np.array_equal(pose[own].view(np.int32), results[np.arange(N), hyp][own].view(np.int32))
    _, again, _ = zh.min_reproj(dev(pose), dev(T), uv, K, conf)     # the assembled poses as a one-hypothesis problem
    assert again.cpu().numpy().tobytes() == px.tobytes()
    return jh, jpf, px, px_pose


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """The one-rank runs with --select joints-temporal (clips of L and of one frame) and --select joints, in this process."""
    import run.inference as inf
    d = tmp_path_factory.mktemp("one_rank")
    res, _ = inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "results.npy")] + JT))
    inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "joints.npy"), "--select", "joints"]))
    inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "single.npy"), "--select", "joints-temporal", "--seq_len", "1"]))
    return d, res


def test_selected_npz_beside_an_unchanged_results_file(one_rank, tmp_path, capsys):
    d, res = one_rank
    plain, errs, out_plain = _inference(BASE + ["--out", str(tmp_path / "results.npy")], capsys)
    assert errs is None and sorted(os.listdir(tmp_path)) == ["results.npy"]
    res_b, _, out_sel = _inference(BASE + ["--out", str(tmp_path / "again.npy")] + JT, capsys)
    assert out_sel == out_plain                                                                     # nothing more on stdout
    assert np.array_equal(res_b, res) and np.array_equal(res, plain)
    a = np.load(d / "results.npy")
    assert a.shape == (N, H, 17, 3) and a.tobytes() == np.load(tmp_path / "results.npy").tobytes()
    assert a.tobytes() == np.load(d / "joints.npy").tobytes()
    sel = np.load(d / "results_selected.npz")
    seq = clips(N, L)
    jh, jpf, px, px_pose = _check_selected(sel, a, seq)
    again = np.load(tmp_path / "again_selected.npz")
    for k in ARRAYS:
        assert again[k].tobytes() == sel[k].tobytes(), k
    joints = np.load(d / "joints_selected.npz")
    assert jpf.tobytes() == joints["joint_hypothesis"].tobytes()                                    # what --select joints keeps
    # --smooth 0: figures only (nobody has measured them on this path)
    _inference(BASE + ["--out", str(tmp_path / "zero.npy"), "--select", "joints-temporal", "--smooth", "0", "--seq_len", str(L)], capsys)
    zero = np.load(tmp_path / "zero_selected.npz")
    assert float(zero["smooth"]) == 0.0 and np.array_equal(zero["joint_hypothesis"], zero["joint_hypothesis_per_frame"])
    rate = lambda p: float(np.mean([switch_rate(p[:, j], seq) for j in range(17)]))
    with capsys.disabled():
        print(f"\njoints-temporal, {N} frames in clips of {L}, H = {H}: weighted reprojection error of the assembled pose {px.mean():.3f} px "
              f"(--smooth 0: {zero['reproj_px'].mean():.3f} px, pose level {px_pose.mean():.3f} px); joint paths switch at {100 * rate(jh):.0f} % "
              f"of transitions at --smooth 100, {100 * rate(zero['joint_hypothesis']):.0f} % at --smooth 0; they leave the per-frame arg-min on "
              f"{100 * float((jh != jpf).mean()):.0f} % of (frame, joint)")
    # without --seq_len a synthetic run is one clip
    _inference(BASE + ["--out", str(tmp_path / "one.npy"), "--select", "joints-temporal"], capsys)
    one = np.load(tmp_path / "one_selected.npz")
    assert one["seq_start"].tolist() == [0, N] and float(one["smooth"]) == 100.0
    _check_selected(one, a, [0, N])


def test_clips_of_one_frame_are_select_joints(one_rank):
    """--seq_len 1: every chain is one frame long - joint_hypothesis, hypothesis and the bits of pose (and what hangs on them) are those
    of --select joints on the same run."""
    d, _ = one_rank
    single, joints = np.load(d / "single_selected.npz"), np.load(d / "joints_selected.npz")
    assert single["seq_start"].tolist() == list(range(N + 1))
    for k in ("joint_hypothesis", "hypothesis", "pose", "T", "reproj_px", "reproj_px_pose_level", "joint_reproj_px"):
        assert single[k].dtype == joints[k].dtype and single[k].tobytes() == joints[k].tobytes(), k
    assert single["joint_hypothesis_per_frame"].tobytes() == joints["joint_hypothesis"].tobytes()
    assert single["joint_path_cost"].tobytes() == joints["joint_reproj_px"].tobytes()              # a chain of one frame costs its unary


def test_eval_prints_the_assembled_pose_after_the_best_of_h_lines(tmp_path, capsys):
    _, errs, out = _inference(BASE + ["--out", str(tmp_path / "a.npy"), "--eval"], capsys)
    _, errs_s, out_s = _inference(BASE + ["--out", str(tmp_path / "b.npy"), "--eval"] + JT, capsys)
    lines, lines_s = out.splitlines(), out_s.splitlines()
    assert lines_s[:len(lines)] == lines and len(lines_s) == len(lines) + 2                        # the existing lines have not moved
    assert lines_s[-2].startswith("joints-temporal MPJPE : ") and lines_s[-1].startswith("joints-temporal PA-MPJPE : ")
    at = lambda key: [i for i, l in enumerate(lines_s) if l.startswith(key)]
    assert len(at("mean MPJPE : ")) == 1 and len(at("mean PA-MPJPE : ")) == 1
    assert at("mean MPJPE : ")[0] < at("mean PA-MPJPE : ")[0] < len(lines_s) - 2
    assert len(errs) == 2 and errs_s[:2] == errs and len(errs_s) == 4
    s1, s2 = float(lines_s[-2].split(" : ")[1]), float(lines_s[-1].split(" : ")[1])
    assert (s1, s2) == errs_s[2:] and np.isfinite([s1, s2]).all() and s2 <= s1 + 1e-9


def test_the_refusals():
    import run.inference as inf
    import run.opt_main as om
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + ["--select", "joints-temporal"]))
    assert "run.inference only" in str(e.value) and "--select joints-temporal" in str(e.value)
    with pytest.raises(SystemExit) as e:
        inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy", "--prune", "5:2"] + JT))
    assert "--prune with --select joints-temporal" in str(e.value)
    for extra in (["--smooth", "-2"], ["--seq_len", "0"]):
        with pytest.raises(SystemExit):
            inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy", "--select", "joints-temporal"] + extra))
    with pytest.raises(SystemExit) as e:
        inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy", "--select", "joints", "--smooth", "50"]))
    assert "--select temporal" in str(e.value)


def test_two_ranks_on_one_gpu_write_the_one_rank_file(one_rank, tmp_path):
    """Two fresh processes, two members of one gloo process group on device 0, each on its own row shard (18 rows each of 36): rank 0's
    _selected.npz is byte for byte the one-rank run's in all eleven arrays, results.npy as well."""
    d, _ = one_rank
    run_two_ranks(BASE + ["--out", str(tmp_path / "results.npy")] + JT, tmp_path)
    assert np.load(tmp_path / "results.npy").tobytes() == np.load(d / "results.npy").tobytes()
    one, two = np.load(d / "results_selected.npz"), np.load(tmp_path / "results_selected.npz")
    assert sorted(two.files) == sorted(ARRAYS)
    for k in ARRAYS:
        assert one[k].dtype == two[k].dtype and one[k].shape == two[k].shape and one[k].tobytes() == two[k].tobytes(), k
