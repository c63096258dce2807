"""GPU: `run.inference --select joints-fused` - the frames are a video and the hypotheses are FUSED joint by joint: per clip and per joint
the posterior mean position under the chain model of --select joints-temporal at --temperature (zedo_joint_reproj + zedo_joint_marginal),
written in the frame of the pose-level temporal path (zedo_min_reproj + zedo_temporal_select).  results.npy stays what it is; beside it
<out>_selected.npz holds the fused pose, the covariance and the spread of every joint, the most probable hypothesis with its probability,
the log-partition values, the Viterbi paths of the same model, the clips and the two weights.  --eval; the refusals; a cold chain is
--select joints-temporal's path; two real ranks on one GPU (gloo rehearsal transport) against the one-rank run.
The spreads and the probabilities are PRINTED, not asserted: whether the fused pose is closer to ground truth than a selected one is not
measured at all - the inputs here are synthetic and the weights random.  The fusion does not depend on the arithmetic mode of the dense
layers: one session runs it."""
import os

import numpy as np
import pytest

from _shared import _inference, _problem, _rows_and_T, cfg_path, dev, run_two_ranks, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S, L, LAM = 12, 3, 10, 5, 100.0
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]
JF = ["--select", "joints-fused", "--seq_len", str(L), "--smooth", "100"]
ARRAYS = ("pose", "joint_cov", "joint_spread_m", "joint_hypothesis", "joint_weight", "joint_logz", "joint_hypothesis_viterbi", "hypothesis",
          "T", "reproj_px_pose_level", "seq_start", "smooth", "temperature")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """In this process: the plain run, --select joints-fused at the default temperature and at 1e-9, and --select joints-temporal."""
    import run.inference as inf
    d = tmp_path_factory.mktemp("fused")
    plain, _ = inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "plain.npy")]))
    res, _ = inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "results.npy")] + JF))
    inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "cold.npy"), "--temperature", "1e-9"] + JF))
    inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "viterbi.npy"), "--select", "joints-temporal", "--seq_len", str(L), "--smooth", "100"]))
    return d, res, plain


def test_selected_npz_beside_an_unchanged_results_file(runs):
    import zedo_hip as zh
    d, res, plain = runs
    assert sorted(f for f in os.listdir(d) if f.startswith("plain")) == ["plain.npy"]
    a = np.load(d / "results.npy")
    assert np.array_equal(res, plain) and a.shape == (N, H, 17, 3) and a.tobytes() == np.load(d / "plain.npy").tobytes()
    sel = np.load(d / "results_selected.npz")
    assert sorted(sel.files) == sorted(ARRAYS)
    pose, cov, spread, jh, jw, jlz, jv, hyp, T, px_pose, ss, smooth, temperature = (sel[k] for k in ARRAYS)
    assert pose.shape == (N, 17, 3) and pose.dtype == np.float32 and T.shape == (N, 3) and T.dtype == np.float32
    assert cov.shape == (N, 17, 6) and cov.dtype == np.float64 and spread.shape == (N, 17) and spread.dtype == np.float64
    for i in (jh, jv):
        assert i.shape == (N, 17) and i.dtype == np.int32 and ((i >= 0) & (i < H)).all()
    for f in (jw, jlz):
        assert f.shape == (N, 17) and f.dtype == np.float64 and np.isfinite(f).all()
    assert hyp.shape == (N,) and hyp.dtype == np.int32 and px_pose.shape == (N,) and px_pose.dtype == np.float64
    seq = clips(N, L)
    assert ss.dtype == np.int32 and ss.tolist() == seq
    for v, want in ((smooth, LAM), (temperature, 1.0)):
        assert v.dtype == np.float64 and v.shape == () and float(v) == want
    # every array again through the binding, from results.npy's rows and the loop's translations
    x, Tall = _rows_and_T(N, H, S)
    assert np.array_equal(x.reshape(H, N, 17, 3).permute(1, 0, 2, 3).cpu().numpy(), a)
    uv, K, conf = (dev(v) for v in _problem(N))
    jerr = zh.joint_reproj(x, Tall, uv, K, return_rows=True)[2]
    err = zh.min_reproj(x, Tall, uv, K, conf)[0]
    path, _ = zh.temporal_select(err, x, seq, N, LAM)
    mean, kcov, hmax, wmax, logz = (t.cpu().numpy() for t in zh.joint_marginal(jerr, x, Tall, seq, N, LAM, 1.0))
    jpath, _ = zh.joint_temporal_select(jerr, x, Tall, seq, N, LAM)
    assert np.array_equal(hyp, path.cpu().numpy()) and np.array_equal(jh, hmax) and np.array_equal(jv, jpath.cpu().numpy())
    assert cov.tobytes() == kcov.tobytes() and jw.tobytes() == wmax.tobytes() and jlz.tobytes() == logz.tobytes()
    assert np.array_equal(T, Tall.reshape(H, N, 3).cpu().numpy()[hyp, np.arange(N)])
    assert px_pose.tobytes() == np.ascontiguousarray(err.reshape(H, N).cpu().numpy()[hyp, np.arange(N)]).tobytes()
    assert spread.tobytes() == np.sqrt(kcov[:, :, 0] + kcov[:, :, 3] + kcov[:, :, 5]).tobytes()
    # pose is the kernel's mean in the frame of the pose-level temporal path: fl32(mean - T[path]); pose + T is the mean to fp32 rounding
    assert np.array_equal(pose.view(np.int32), (mean - T.astype(np.float64)[:, None, :]).astype(np.float32).view(np.int32))
    back = pose.astype(np.float64) + T.astype(np.float64)[:, None, :]
    assert np.abs(back - mean).max() <= 2.0 ** -24 * np.abs(mean - T.astype(np.float64)[:, None, :]).max() + 1e-15
    # the fused joint lies in the hull of the hypotheses' joints
    X = (x.to(torch.float64) + Tall.to(torch.float64)[:, None, :]).reshape(H, N, 17, 3).cpu().numpy()
    assert (mean >= X.min(0) - 1e-12).all() and (mean <= X.max(0) + 1e-12).all()
    print(f"\njoints-fused, {N} frames in clips of {L}, H = {H}, temperature 1 px: the largest marginal has median {np.median(jw):.2f}, minimum "
          f"{jw.min():.2f}; spread sqrt(trace cov) median {1e3 * np.median(spread):.1f} mm, largest {1e3 * spread.max():.1f} mm; the most probable "
          f"hypothesis leaves the Viterbi path on {100 * float((jh != jv).mean()):.0f} % of (frame, joint)")


def test_a_cold_chain_keeps_the_path_of_select_joints_temporal(runs):
    """--temperature 1e-9: joint_hypothesis == joint_hypothesis_viterbi, which is what --select joints-temporal writes; the fused pose is that
    run's assembled pose to the weight the runner-up paths keep."""
    d, _, _ = runs
    cold, vit = np.load(d / "cold_selected.npz"), np.load(d / "viterbi_selected.npz")
    assert float(cold["temperature"]) == 1e-9 and np.array_equal(cold["joint_hypothesis"], cold["joint_hypothesis_viterbi"])
    assert np.array_equal(cold["joint_hypothesis_viterbi"], vit["joint_hypothesis"]) and np.array_equal(cold["hypothesis"], vit["hypothesis"])
    assert np.array_equal(np.load(d / "results_selected.npz")["joint_hypothesis_viterbi"], vit["joint_hypothesis"])
    assert cold["joint_weight"].min() > 0.99
    assert np.abs(cold["pose"] - vit["pose"]).max() <= 1e-2 * np.abs(vit["pose"]).max()


def test_eval_prints_the_fused_pose_after_the_best_of_h_lines(tmp_path, capsys):
    _, errs, out = _inference(BASE + ["--out", str(tmp_path / "a.npy"), "--eval"], capsys)
    _, errs_s, out_s = _inference(BASE + ["--out", str(tmp_path / "b.npy"), "--eval"] + JF, capsys)
    lines, lines_s = out.splitlines(), out_s.splitlines()
    assert lines_s[:len(lines)] == lines and len(lines_s) == len(lines) + 2                        # the existing lines have not moved
    assert lines_s[-2].startswith("joints-fused MPJPE : ") and lines_s[-1].startswith("joints-fused PA-MPJPE : ")
    assert len(errs) == 2 and errs_s[:2] == errs and len(errs_s) == 4
    s1, s2 = float(lines_s[-2].split(" : ")[1]), float(lines_s[-1].split(" : ")[1])
    assert (s1, s2) == errs_s[2:] and np.isfinite([s1, s2]).all() and s2 <= s1 + 1e-9


def test_the_refusals():
    import run.inference as inf
    import run.opt_main as om
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + ["--select", "joints-fused"]))
    assert "run.inference only" in str(e.value) and "--select joints-fused" in str(e.value)
    with pytest.raises(SystemExit) as e:
        inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy", "--prune", "5:2"] + JF))
    assert "--prune with --select joints-fused" in str(e.value)
    for extra in (["--smooth", "-2"], ["--seq_len", "0"], ["--temperature", "0"], ["--temperature", "nan"]):
        with pytest.raises(SystemExit):
            inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy", "--select", "joints-fused"] + extra))
    for sel in ("none", "joints-temporal"):
        with pytest.raises(SystemExit) as e:
            inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy", "--select", sel, "--temperature", "2"]))
        assert "--temperature is a switch of --select joints-fused" in str(e.value)


def test_two_ranks_on_one_gpu_write_the_one_rank_file(runs, tmp_path):
    """Two fresh processes, two members of one gloo process group on device 0, each on its own row shard: rank 0's _selected.npz is byte
    for byte the one-rank run's in all thirteen arrays, results.npy as well."""
    d, _, _ = runs
    run_two_ranks(BASE + ["--out", str(tmp_path / "results.npy")] + JF, tmp_path)
    assert np.load(tmp_path / "results.npy").tobytes() == np.load(d / "results.npy").tobytes()
    one, two = np.load(d / "results_selected.npz"), np.load(tmp_path / "results_selected.npz")
    assert sorted(two.files) == sorted(ARRAYS)
    for k in ARRAYS:
        assert one[k].dtype == two[k].dtype and one[k].shape == two[k].shape and one[k].tobytes() == two[k].tobytes(), k
