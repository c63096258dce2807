"""GPU: `run.inference --select temporal` - the frames are a video; per clip the hypothesis sequence that minimises reprojection error
plus --smooth times the mean joint displacement between consecutive frames (zedo_min_reproj + zedo_temporal_select) as a stage of the
driver.  results.npy stays what it is; beside it <out>_selected.npz holds the kept rows, the Viterbi path, what --select reproj would
keep, every row's reprojection error, the path costs, the clips and the weight.  Fused and step-wise route, --eval, the refusals, clips
from a 'wild' npz, and two real ranks on one GPU (gloo rehearsal transport) against the one-rank run.  Whether the temporal path is
closer to ground truth on real video is not measured: the inputs here are synthetic and the weights random.
The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import os

import numpy as np
import pytest

from _shared import _inference, cfg_path, run_two_ranks, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)
from _temporal_ref import clips, cost_bound, temporal_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S, L, LAM = 12, 3, 10, 5, 100.0
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]
TEMPORAL = ["--select", "temporal", "--seq_len", str(L), "--smooth", "100"]
ARRAYS = ("pose", "hypothesis", "hypothesis_per_frame", "reproj_px", "reproj_px_all", "path_cost", "T", "seq_start", "smooth")


def _check_selected(sel, sel_reproj, results, seq, lam=LAM, n=N, h=H):
    """The nine arrays with their dtypes and shapes; hypothesis and path_cost recomputed by the numpy reference from results.npy and
    reproj_px_all (exact: the reference's gap is asserted first); pose = the bits of results[n, hypothesis[n]]; the per-frame
    selection and what hangs on it are the bytes --select reproj writes."""
    assert sorted(sel.files) == sorted(ARRAYS)
    pose, hyp, hpf, px, px_all, pc, T, ss, smooth = (sel[k] for k in ARRAYS)
    assert pose.shape == (n, 17, 3) and pose.dtype == np.float32 and T.shape == (n, 3) and T.dtype == np.float32
    assert hyp.shape == (n,) and hyp.dtype == np.int32 and hpf.shape == (n,) and hpf.dtype == np.int32
    assert px.shape == (n,) and px.dtype == np.float64 and px_all.shape == (n, h) and px_all.dtype == np.float64
    assert pc.shape == (n,) and pc.dtype == np.float64 and ss.dtype == np.int32 and ss.tolist() == list(seq)
    assert smooth.dtype == np.float64 and smooth.shape == () and float(smooth) == lam
    assert ((hyp >= 0) & (hyp < h)).all() and np.isfinite(px_all).all()
    rows = np.ascontiguousarray(results.transpose(1, 0, 2, 3)).reshape(h * n, 17, 3)
    r = temporal_ref(np.ascontiguousarray(px_all.T).reshape(-1), rows, seq, lam)
    assert r["gap"] > 1e-6
    assert np.array_equal(hyp, r["path"])
    Lmax = int(np.diff(seq).max())
    err = np.abs(pc - r["cost"])
    print(f"selected: max |path_cost - ref| = {err.max():.3e}; path differs from the per-frame arg-min on {int((hyp != hpf).sum())} of {n} frames")
    assert (err <= cost_bound(17, Lmax, r["cost"])).all()
    assert np.array_equal(pose.view(np.int32), results[np.arange(n), hyp].view(np.int32))
    assert np.array_equal(px.view(np.int64), px_all[np.arange(n), hyp].view(np.int64))
    # what --select reproj keeps
    assert hpf.tobytes() == sel_reproj["hypothesis"].tobytes()
    assert px_all[np.arange(n), hpf].tobytes() == sel_reproj["reproj_px"].tobytes()
    keep = hyp == hpf
    assert np.array_equal(T[keep].view(np.int32), sel_reproj["T"][keep].view(np.int32))
    return hyp, hpf


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """The one-rank runs with --select temporal and --select reproj (in this process), shared by the tests below: (directory, results)."""
    import run.inference as inf
    d = tmp_path_factory.mktemp("one_rank")
    res, _ = inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "results.npy")] + TEMPORAL))
    inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "reproj.npy"), "--select", "reproj"]))
    return d, res


def test_selected_npz_beside_an_unchanged_results_file(one_rank, tmp_path, capsys):
    d, res = one_rank
    plain, errs, out_plain = _inference(BASE + ["--out", str(tmp_path / "results.npy")], capsys)
    assert errs is None and sorted(os.listdir(tmp_path)) == ["results.npy"]
    res_b, _, out_sel = _inference(BASE + ["--out", str(tmp_path / "again.npy")] + TEMPORAL, capsys)
    assert out_sel == out_plain                                                                     # nothing more on stdout
    assert np.array_equal(res_b, res) and np.array_equal(res, plain)
    a, b = np.load(d / "results.npy"), np.load(tmp_path / "results.npy")
    assert a.shape == (N, H, 17, 3) and a.tobytes() == b.tobytes() and a.tobytes() == np.load(d / "reproj.npy").tobytes()
    sel = np.load(d / "results_selected.npz")
    _check_selected(sel, np.load(d / "reproj_selected.npz"), a, clips(N, L))
    again = np.load(tmp_path / "again_selected.npz")
    for k in ARRAYS:
        assert again[k].tobytes() == sel[k].tobytes(), k
    # without --seq_len a synthetic run is one clip; --smooth 0 is the per-frame selection
    _inference(BASE + ["--out", str(tmp_path / "one.npy"), "--select", "temporal"], capsys)
    one = np.load(tmp_path / "one_selected.npz")
    _check_selected(one, np.load(d / "reproj_selected.npz"), a, [0, N])
    _inference(BASE + ["--out", str(tmp_path / "zero.npy"), "--select", "temporal", "--smooth", "0", "--seq_len", str(L)], capsys)
    zero = np.load(tmp_path / "zero_selected.npz")
    assert np.array_equal(zero["hypothesis"], zero["hypothesis_per_frame"]) and float(zero["smooth"]) == 0.0


def test_eval_prints_the_temporal_pose_after_the_best_of_h_lines(tmp_path, capsys):
    _, errs, out = _inference(BASE + ["--out", str(tmp_path / "a.npy"), "--eval"], capsys)
    _, errs_s, out_s = _inference(BASE + ["--out", str(tmp_path / "b.npy"), "--eval"] + TEMPORAL, capsys)
    lines, lines_s = out.splitlines(), out_s.splitlines()
    assert lines_s[:len(lines)] == lines and len(lines_s) == len(lines) + 2                        # the existing lines have not moved
    assert lines_s[-2].startswith("temporal-selected MPJPE : ") and lines_s[-1].startswith("temporal-selected PA-MPJPE : ")
    at = lambda key: [i for i, l in enumerate(lines_s) if l.startswith(key)]
    assert len(at("mean MPJPE : ")) == 1 and len(at("mean PA-MPJPE : ")) == 1
    assert at("mean MPJPE : ")[0] < at("mean PA-MPJPE : ")[0] < len(lines_s) - 2
    assert len(errs) == 2 and errs_s[:2] == errs and len(errs_s) == 4
    s1, s2 = float(lines_s[-2].split(" : ")[1]), float(lines_s[-1].split(" : ")[1])
    assert (s1, s2) == errs_s[2:]
    assert s1 >= errs[0] - 1e-12 and s2 >= errs[1] - 1e-12 and s2 <= s1 + 1e-9                      # one kept pose cannot beat the best of H


def test_the_stepwise_route_selects_too(tmp_path, capsys):
    """A sampler configuration outside the fused pipeline (reverse-diffusion predictor): stepwise_loop(return_T=True) hands the final T
    of every row to the same selection."""
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
    res, _, out = _inference(argv + ["--out", str(tmp_path / "r.npy"), "--select", "temporal", "--seq_len", "3", "--smooth", "30"], capsys)
    assert "outside the fused pipeline" in out and out == out_plain and np.array_equal(res, plain)
    _inference(argv + ["--out", str(tmp_path / "q.npy"), "--select", "reproj"], capsys)
    _check_selected(np.load(tmp_path / "r_selected.npz"), np.load(tmp_path / "q_selected.npz"), np.load(tmp_path / "r.npy"), [0, 3, 5],
                    lam=30.0, n=5, h=2)


def test_the_refusals():
    import run.inference as inf
    import run.opt_main as om
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + ["--select", "temporal"]))
    assert "run.inference only" in str(e.value) and "--select temporal" in str(e.value)
    for extra in (["--smooth", "50"], ["--seq_len", "4"], ["--select", "reproj", "--smooth", "50"]):
        with pytest.raises(SystemExit) as e:
            inf.main(inf.parse_args(["prog"] + BASE + ["--out", "unused.npy"] + extra))
        assert "--select temporal" in str(e.value)
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + ["--smooth", "50"]))
    assert "--select temporal" in str(e.value)


def test_clips_from_a_wild_npz(tmp_path, weights0, monkeypatch, capsys):
    """The 'wild' dataset fed from files: `seq_start` in the npz gives the file --seq_len gives for the same clips; without either the
    frames are one clip; a seq_start that is not ascending is refused on the host."""
    from lib.algorithms.advanced.model import ScoreModelFC_Adv
    from lib.algorithms.ema import ExponentialMovingAverage
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    d = syn.make_poses(N, seed=12, conf_mode="uniform")
    arrays = dict(db_2d=d["db_2d"], camera_param=d["camera_param"], db_3d=d["db_3d"])
    np.savez(tmp_path / "plain.npz", **arrays)
    np.savez(tmp_path / "clips.npz", seq_start=np.array(clips(N, L)), **arrays)
    np.savez(tmp_path / "bad.npz", seq_start=np.array([0, 7, 5, N]), **arrays)
    os.makedirs(tmp_path / "clusters")
    np.save(tmp_path / "clusters" / f"h36m_cluster{H}.npy", syn.make_clusters(H, seed=4))
    cfg_file = tmp_path / "cfg_wild_small.py"
    cfg_file.write_text("import importlib.util\n"
                        f"_s = importlib.util.spec_from_file_location('base_cfg', r'{cfg_path('wild')}')\n"
                        "_m = importlib.util.module_from_spec(_s); _s.loader.exec_module(_m)\n"
                        "def get_config():\n"
                        "    c = _m.get_config()\n"
                        f"    c.ZeDO.batch = {N}\n"
                        "    return c\n")
    model = ScoreModelFC_Adv(load_config(str(cfg_file)), n_joints=17, joint_dim=3, hidden_dim=1024, embed_dim=512, cond_dim=3)
    sd = {k: torch.tensor(v) for k, v in weights0.items()}
    sd["sigmas"] = torch.tensor(syn.sigmas_buffer())
    model.load_state_dict(sd)
    os.makedirs(tmp_path / "ckpt")
    torch.save({"model_state_dict": {"module." + k: v for k, v in model.state_dict().items()},
                "ema": ExponentialMovingAverage(model.parameters(), decay=0.9999).state_dict(), "step": 1}, tmp_path / "ckpt" / "c.pth")
    monkeypatch.chdir(tmp_path)
    base = ["--config", str(cfg_file), "--ckpt_dir", "ckpt", "--ckpt_name", "c.pth", "--hypo", str(H), "--oil_iterations", str(S)]
    _inference(base + ["--data", "clips.npz", "--out", "a.npy", "--select", "temporal"], capsys)
    _inference(base + ["--data", "plain.npz", "--out", "b.npy", "--select", "temporal", "--seq_len", str(L)], capsys)
    _inference(base + ["--data", "plain.npz", "--out", "c.npy", "--select", "temporal"], capsys)
    _inference(base + ["--data", "clips.npz", "--out", "e.npy", "--select", "temporal", "--seq_len", str(N)], capsys)      # --seq_len overrides
    _inference(base + ["--data", "plain.npz", "--out", "r.npy", "--select", "reproj"], capsys)
    a, b, c, e = (np.load(f"{k}_selected.npz") for k in "abce")
    assert a["seq_start"].tolist() == clips(N, L) and c["seq_start"].tolist() == [0, N] and e["seq_start"].tolist() == [0, N]
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        assert c[k].tobytes() == e[k].tobytes(), k
    _check_selected(a, np.load("r_selected.npz"), np.load("a.npy"), clips(N, L))
    _check_selected(c, np.load("r_selected.npz"), np.load("c.npy"), [0, N])
    with pytest.raises(ValueError):
        _inference(base + ["--data", "bad.npz", "--out", "x.npy", "--select", "temporal"], capsys)


def test_two_ranks_on_one_gpu_write_the_one_rank_file(one_rank, tmp_path):
    """Two fresh processes, two members of one gloo process group on device 0, each on its own row shard (18 rows each of 36): rank 0's
    _selected.npz is byte for byte the one-rank run's in all nine arrays, results.npy as well."""
    d, _ = one_rank
    run_two_ranks(BASE + ["--out", str(tmp_path / "results.npy")] + TEMPORAL, tmp_path)
    assert np.load(tmp_path / "results.npy").tobytes() == np.load(d / "results.npy").tobytes()
    one, two = np.load(d / "results_selected.npz"), np.load(tmp_path / "results_selected.npz")
    assert sorted(two.files) == sorted(ARRAYS)
    for k in ARRAYS:
        assert one[k].dtype == two[k].dtype and one[k].shape == two[k].shape and one[k].tobytes() == two[k].tobytes(), k
