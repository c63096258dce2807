"""GPU: `run.inference --select joints` - the joint-wise, label-free aggregation as a stage of the driver.  results.npy stays what it is;
beside it <out>_selected.npz holds, per detection, the pose assembled from the joints whose reprojection is closest to their detections
(zedo_joint_reproj + zedo_joint_compose), in the frame of the pose-level winner (zedo_min_reproj), with both selections' indices and
errors.  Fused and step-wise route, --eval, the refusal of run.opt_main, and two real ranks on one GPU (gloo rehearsal transport) against
the one-rank run.  Whether the assembled pose is closer to ground truth on real data is not measured: the inputs here are synthetic.
The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import os

import numpy as np
import pytest

from _joint_ref import compose_ref
from _shared import _inference, _problem, _rows_and_T, cfg_path, dev, run_two_ranks, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S = 8, 3, 10
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]
ARRAYS = ("pose", "joint_hypothesis", "joint_reproj_px", "hypothesis", "T", "reproj_px", "reproj_px_pose_level")


def _check_selected(sel, sel_reproj, results, uv, K, conf, n=N, h=H):
    """The seven arrays; the per-joint winners recomputed from results.npy and the selected frame; the pose-level arrays are those of
    --select reproj; the assembled pose reprojects at least as close as the pose-level winner (+ 1e-3 px for the fp32 rounding of the
    composed coordinates)."""
    import zedo_hip as zh
    assert sorted(sel.files) == sorted(ARRAYS)
    pose, jh, jpx, hyp, T, px, px_pose = (sel[k] for k in ARRAYS)
    assert pose.shape == (n, 17, 3) and pose.dtype == np.float32
    assert jh.shape == (n, 17) and jh.dtype == np.int32 and jpx.shape == (n, 17) and jpx.dtype == np.float64
    assert hyp.shape == (n,) and hyp.dtype == np.int32 and T.shape == (n, 3) and T.dtype == np.float32
    assert px.shape == (n,) and px.dtype == np.float64 and px_pose.shape == (n,) and px_pose.dtype == np.float64
    assert ((jh >= 0) & (jh < h)).all() and ((hyp >= 0) & (hyp < h)).all()
    for k, kr in (("hypothesis", "hypothesis"), ("T", "T"), ("reproj_px_pose_level", "reproj_px")):
        assert sel[k].dtype == sel_reproj[kr].dtype and sel[k].tobytes() == sel_reproj[kr].tobytes(), k
    print(f"selected: max (reproj_px - pose level) = {(px - px_pose).max():.3e} px (bound 1e-3); mean {px.mean():.3f} vs {px_pose.mean():.3f} px")
    assert (px <= px_pose + 1e-3).all()
    # results.npy is [n, h, 17, 3] root-relative to each row's own T; a joint taken from the frame's own hypothesis is results' bits
    own = jh == hyp[:, None]
    assert np.array_equal(pose[own].view(np.int32), results[np.arange(n), hyp][own].view(np.int32))
    # every row's T is not in the file: the driver's own loop again (same kernels, same bits) gives them - see the caller
    return pose, jh, jpx, hyp, T


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """The one-rank runs with --select joints and --select reproj (in this process), shared by the tests below: (directory, results)."""
    import run.inference as inf
    d = tmp_path_factory.mktemp("one_rank")
    res, _ = inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "results.npy"), "--select", "joints"]))
    inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "reproj.npy"), "--select", "reproj"]))
    return d, res


def test_selected_npz_beside_an_unchanged_results_file(one_rank, tmp_path, capsys):
    import zedo_hip as zh
    d, res = one_rank
    plain, errs, out_plain = _inference(BASE + ["--out", str(tmp_path / "results.npy")], capsys)
    assert errs is None and sorted(os.listdir(tmp_path)) == ["results.npy"]
    res_b, _, out_sel = _inference(BASE + ["--out", str(tmp_path / "again.npy"), "--select", "joints"], capsys)
    assert out_sel == out_plain                                                                     # nothing more on stdout
    assert np.array_equal(res_b, res) and np.array_equal(res, plain)
    a, b = np.load(d / "results.npy"), np.load(tmp_path / "results.npy")
    assert a.shape == (N, H, 17, 3) and a.tobytes() == b.tobytes() and a.tobytes() == np.load(d / "reproj.npy").tobytes()
    uv, K, conf = _problem(N)
    sel = np.load(d / "results_selected.npz")
    pose, jh, jpx, hyp, T = _check_selected(sel, np.load(d / "reproj_selected.npz"), a, uv, K, conf)
    # pose recomputed from results.npy + every row's T gives joint_hypothesis again through zh.joint_reproj
    x, Tall = _rows_and_T(N, H, S)
    assert np.array_equal(x.reshape(H, N, 17, 3).permute(1, 0, 2, 3).cpu().numpy(), a)
    rows = dev(np.ascontiguousarray(a.transpose(1, 0, 2, 3)).reshape(H * N, 17, 3))
    best, idx = zh.joint_reproj(rows, Tall, dev(uv), dev(K))
    assert np.array_equal(idx.cpu().numpy(), jh) and best.cpu().numpy().tobytes() == jpx.tobytes()
    assert np.array_equal(T, Tall.reshape(H, N, 3).cpu().numpy()[hyp, np.arange(N)])
    want = compose_ref(rows.cpu().numpy(), Tall.cpu().numpy(), jh, hyp)
    assert np.array_equal(pose.view(np.int32), want.view(np.int32))
    # reproj_px is zedo_min_reproj on the assembled poses as a one-hypothesis problem
    _, px, _ = zh.min_reproj(dev(pose), dev(T), dev(uv), dev(K), dev(conf))
    assert px.cpu().numpy().tobytes() == sel["reproj_px"].tobytes()


def test_eval_prints_the_aggregated_pose_after_the_best_of_h_lines(tmp_path, capsys):
    _, errs, out = _inference(BASE + ["--out", str(tmp_path / "a.npy"), "--eval"], capsys)
    _, errs_s, out_s = _inference(BASE + ["--out", str(tmp_path / "b.npy"), "--eval", "--select", "joints"], capsys)
    lines, lines_s = out.splitlines(), out_s.splitlines()
    assert lines_s[:len(lines)] == lines and len(lines_s) == len(lines) + 2                        # the existing lines have not moved
    assert lines_s[-2].startswith("joints-aggregated MPJPE : ") and lines_s[-1].startswith("joints-aggregated PA-MPJPE : ")
    at = lambda key: [i for i, l in enumerate(lines_s) if l.startswith(key)]
    assert len(at("mean MPJPE : ")) == 1 and len(at("mean PA-MPJPE : ")) == 1
    assert at("mean MPJPE : ")[0] < at("mean PA-MPJPE : ")[0] < len(lines_s) - 2
    assert len(errs) == 2 and errs_s[:2] == errs and len(errs_s) == 4
    s1, s2 = float(lines_s[-2].split(" : ")[1]), float(lines_s[-1].split(" : ")[1])
    assert (s1, s2) == errs_s[2:] and np.isfinite([s1, s2]).all() and s2 <= s1 + 1e-9
    # --select reproj keeps its lines
    _, _, out_r = _inference(BASE + ["--out", str(tmp_path / "c.npy"), "--eval", "--select", "reproj"], capsys)
    lines_r = out_r.splitlines()
    assert lines_r[:len(lines)] == lines and len(lines_r) == len(lines) + 2
    assert lines_r[-2].startswith("reproj-selected MPJPE : ") and lines_r[-1].startswith("reproj-selected PA-MPJPE : ")


def test_the_stepwise_route_aggregates_too(tmp_path, capsys):
    """A sampler configuration outside the fused pipeline (reverse-diffusion predictor): stepwise_loop(return_T=True) hands the final T
    of every row to the same aggregation."""
    cfg = tmp_path / "cfg_rd.py"
    cfg.write_text("import importlib.util\n"
                   f"_s = importlib.util.spec_from_file_location('base_cfg', r'{cfg_path('pw3d')}')\n"
                   "_m = importlib.util.module_from_spec(_s); _s.loader.exec_module(_m)\n"
                   "def get_config():\n"
                   "    c = _m.get_config()\n"
                   "    c.sampling.predictor = 'reverse_diffusion'\n"
                   "    return c\n")
    argv = ["--config", str(cfg), "--synthetic", "5", "--hypo", "2", "--oil_iterations", "4"]
    plain, _, out_plain = _inference(argv + ["--out", str(tmp_path / "p.npy")], capsys)
    res, _, out = _inference(argv + ["--out", str(tmp_path / "r.npy"), "--select", "joints"], capsys)
    assert "outside the fused pipeline" in out and out == out_plain and np.array_equal(res, plain)
    _inference(argv + ["--out", str(tmp_path / "q.npy"), "--select", "reproj"], capsys)
    uv, K, conf = _problem(5, str(cfg))
    _check_selected(np.load(tmp_path / "r_selected.npz"), np.load(tmp_path / "q_selected.npz"), np.load(tmp_path / "r.npy"), uv, K, conf, n=5, h=2)


def test_opt_main_refuses_the_switch():
    import run.opt_main as om
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + ["--select", "joints"]))
    assert "run.inference only" in str(e.value) and "--select joints" in str(e.value)


def test_two_ranks_on_one_gpu_write_the_one_rank_file(one_rank, tmp_path):
    """Two fresh processes, two members of one gloo process group on device 0, each on its own row shard (12 rows each of 24): rank 0's
    _selected.npz is byte for byte the one-rank run's in all seven arrays, results.npy as well."""
    d, _ = one_rank
    run_two_ranks(BASE + ["--out", str(tmp_path / "results.npy"), "--select", "joints"], tmp_path)
    assert np.load(tmp_path / "results.npy").tobytes() == np.load(d / "results.npy").tobytes()
    one, two = np.load(d / "results_selected.npz"), np.load(tmp_path / "results_selected.npz")
    assert sorted(two.files) == sorted(ARRAYS)
    for k in ARRAYS:
        assert one[k].dtype == two[k].dtype and one[k].shape == two[k].shape and one[k].tobytes() == two[k].tobytes(), k
