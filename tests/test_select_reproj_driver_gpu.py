"""GPU: `run.inference --select reproj` - the label-free selection as a stage of the driver.  results.npy stays what it is; beside it
<out>_selected.npz holds, per detection, the hypothesis whose x + T reprojects closest to the 2D detections (zedo_min_reproj), its
root-relative pose, its translation and its error in pixels.  Fused and step-wise route, --eval, the refusal of run.opt_main, and two
real ranks on one GPU (gloo rehearsal transport) against the one-rank run.
The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import os

import numpy as np
import pytest

from _select_ref import reproj_ref
from _shared import _inference, _problem, cfg_path, run_two_ranks, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S = 8, 3, 10
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]
ARRAYS = ("pose", "hypothesis", "reproj_px", "T")


def _check_selected(sel, results, uv, K, conf, n=N, h=H):
    assert sorted(sel.files) == sorted(ARRAYS)
    pose, hyp, px, T = (sel[k] for k in ARRAYS)
    assert pose.shape == (n, 17, 3) and pose.dtype == np.float32 and hyp.shape == (n,) and hyp.dtype == np.int32
    assert px.shape == (n,) and px.dtype == np.float64 and T.shape == (n, 3) and T.dtype == np.float32
    assert ((hyp >= 0) & (hyp < h)).all()
    assert np.array_equal(pose.view(np.int32), results[np.arange(n), hyp].view(np.int32))          # the bits of results[n, hypothesis[n]]
    d = np.abs(px - reproj_ref(pose, T, uv, K, conf)).max()
    print(f"selected: max |reproj_px - ref| = {d:.3e} px (bound 1e-9)")
    assert d <= 1e-9


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """The one-rank run with --select reproj (in this process), shared by the tests below: (directory, results)."""
    import run.inference as inf
    d = tmp_path_factory.mktemp("one_rank")
    res, _ = inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / "results.npy"), "--select", "reproj"]))
    return d, res


def test_selected_npz_beside_an_unchanged_results_file(one_rank, tmp_path, capsys):
    d, res = one_rank
    plain, errs, out_plain = _inference(BASE + ["--out", str(tmp_path / "results.npy")], capsys)
    assert errs is None and sorted(os.listdir(tmp_path)) == ["results.npy"]                        # no --select: no extra file
    res_b, _, out_sel = _inference(BASE + ["--out", str(tmp_path / "again.npy"), "--select", "reproj"], capsys)
    assert out_sel == out_plain                                                                     # ... and nothing more on stdout
    assert np.array_equal(res_b, res) and np.array_equal(res, plain)
    a, b = np.load(d / "results.npy"), np.load(tmp_path / "results.npy")
    assert a.shape == (N, H, 17, 3) and a.tobytes() == b.tobytes()                                  # results.npy bit for bit
    sel = np.load(d / "results_selected.npz")
    uv, K, conf = _problem(N)
    _check_selected(sel, a, uv, K, conf)
    # the hypothesis kept is the arg-min over ALL rows: the same loop again (same kernels, same bits) for every row's T
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    cfg = load_config(cfg_path("pw3d"))
    z = cfg.ZeDO
    pipe = Pipeline(syn.make_weights(seed=cfg.seed), ZeDOConfig(z.IPO_iterations, z.IPO_keylist, z.RotAxes, z.IPO_T, z.IPO_minScaleT, z.IPO_maxScaleT,
                                                                S, z.sampling_eps, 0.1, 1000, 0.1, 20.0), "cuda")
    x, T = pipe.load(syn.make_clusters(H, seed=cfg.seed), np.concatenate([uv, conf[:, :, None]], -1), K).run()
    assert np.array_equal(x.reshape(H, N, 17, 3).permute(1, 0, 2, 3).cpu().numpy(), a)
    e = reproj_ref(x.cpu().numpy(), T.cpu().numpy(), uv, K, conf).reshape(H, N)
    assert np.isfinite(e).all()
    assert np.abs(sel["reproj_px"] - e.min(0)).max() <= 1e-9 and (e[sel["hypothesis"], np.arange(N)] <= e.min(0) + 2e-9).all()
    assert np.array_equal(sel["T"], T.reshape(H, N, 3).cpu().numpy()[sel["hypothesis"], np.arange(N)])


def test_eval_prints_the_selected_pose_after_the_best_of_h_lines(tmp_path, capsys):
    _, errs, out = _inference(BASE + ["--out", str(tmp_path / "a.npy"), "--eval"], capsys)
    _, errs_s, out_s = _inference(BASE + ["--out", str(tmp_path / "b.npy"), "--eval", "--select", "reproj"], capsys)
    lines, lines_s = out.splitlines(), out_s.splitlines()
    assert lines_s[:len(lines)] == lines and len(lines_s) == len(lines) + 2                        # the existing lines have not moved
    assert lines_s[-2].startswith("reproj-selected MPJPE : ") and lines_s[-1].startswith("reproj-selected PA-MPJPE : ")
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
    res, _, out = _inference(argv + ["--out", str(tmp_path / "r.npy"), "--select", "reproj"], capsys)
    assert "outside the fused pipeline" in out and out == out_plain and np.array_equal(res, plain)
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    d = syn.make_poses(5, seed=load_config(str(cfg)).seed)
    _check_selected(np.load(tmp_path / "r_selected.npz"), np.load(tmp_path / "r.npy"), d["db_2d"][:, :, :2], d["camera_param"],
                    d["db_2d"][:, :, 2], n=5, h=2)


def test_stepwise_loop_keeps_its_return_value_by_default():
    import inspect
    from run._driver import stepwise_loop
    p = inspect.signature(stepwise_loop).parameters["return_T"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_opt_main_refuses_the_switch():
    import run.opt_main as om
    with pytest.raises(SystemExit) as e:
        om.main(om.parse_args(["prog"] + BASE + ["--select", "reproj"]))
    assert "run.inference only" in str(e.value)
    with pytest.raises(SystemExit):
        om.parse_args(["prog"] + BASE + ["--select", "gt"])                                        # not a choice at all


def test_two_ranks_on_one_gpu_write_the_one_rank_file(one_rank, tmp_path):
    """Two fresh processes, two members of one gloo process group on device 0, each on its own row shard (12 rows each of 24): rank 0's
    _selected.npz is byte for byte the one-rank run's in all four arrays, results.npy as well."""
    d, _ = one_rank
    run_two_ranks(BASE + ["--out", str(tmp_path / "results.npy"), "--select", "reproj"], tmp_path)
    assert np.load(tmp_path / "results.npy").tobytes() == np.load(d / "results.npy").tobytes()
    one, two = np.load(d / "results_selected.npz"), np.load(tmp_path / "results_selected.npz")
    assert sorted(two.files) == sorted(ARRAYS)
    for k in ARRAYS:
        assert one[k].dtype == two[k].dtype and one[k].shape == two[k].shape and one[k].tobytes() == two[k].tobytes(), k
