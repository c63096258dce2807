"""GPU: `run.inference --select joints-tree-fused [--bone MU] [--temperature TAU]` - the soft answer of the skeleton-coupled aggregation
as a stage of the driver.  results.npy stays what it is; beside it <out>_selected.npz holds, per detection, the posterior mean of every
joint under the model of --select joints-tree at the temperature TAU (zedo_joint_tree_marginal on the confidence-weighted reprojection
distances), in the frame of the pose-level winner, its covariance and spread, the most probable hypothesis with its probability, the
log-partition value, every bone's expected mismatch and, for comparison, the assignment --select joints-tree keeps.  One process runs
none, joints-tree, joints-tree-fused at the defaults and at --temperature 1e-9 once; the tests share those runs.  The written pose,
covariance and log-partition value are held to the numpy reference of tests/_joint_tree_marginal_ref.py on the run's own arrays, within
its bounds.  Whether the fused pose is closer to ground truth on real data is not measured: the inputs here are synthetic.  The fusion
does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

import _joint_tree_marginal_ref as M
import _joint_tree_ref as R
from _shared import _inference, _problem, _rows_and_T, _sel, cfg_path, dev, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S = 8, 3, 10
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]
KEYS = ("pose", "joint_cov", "joint_spread_m", "joint_hypothesis", "joint_weight", "joint_logz", "joint_bone_m", "joint_hypothesis_tree",
        "hypothesis", "T", "reproj_px_pose_level", "bone", "temperature")
RUNS = {"none": [], "tree": ["--select", "joints-tree"], "fused": ["--select", "joints-tree-fused"],
        "cold": ["--select", "joints-tree-fused", "--temperature", "1e-9"]}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every run once, in this process: name -> (results array, path of the out file, stdout)."""
    import contextlib
    import io

    import run.inference as inf
    d = tmp_path_factory.mktemp("treefused")
    out = {}
    for name, extra in RUNS.items():
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res, _ = inf.main(inf.parse_args(["prog"] + BASE + ["--out", str(d / f"{name}.npy")] + extra))
        out[name] = (res, d / f"{name}.npy", buf.getvalue())
    return out


@pytest.fixture(scope="module")
def arrays():
    """The run's own arrays again (same kernels, same bits): rows x, T, the per-(row, joint) distances, the detections."""
    import zedo_hip as zh
    uv, K, conf = _problem(N)
    x, T = _rows_and_T(N, H, S)
    _, _, jerr = zh.joint_reproj(x, T, dev(uv), dev(K), return_rows=True)
    return dict(x=x.cpu().numpy(), T=T.cpu().numpy(), jerr=jerr.cpu().numpy(), conf=conf)


def test_results_file_is_unchanged_and_the_key_set_is_the_documented_one(runs):
    plain = np.load(runs["none"][1])
    assert plain.shape == (N, H, 17, 3)
    for name in RUNS:
        assert np.load(runs[name][1]).tobytes() == plain.tobytes(), name
        assert runs[name][2] == runs["none"][2], name                 # nothing more on stdout
    for name in ("fused", "cold"):
        sel = _sel(runs, name)
        assert sorted(sel.files) == sorted(KEYS)
        assert sel["pose"].shape == (N, 17, 3) and sel["pose"].dtype == np.float32
        assert sel["joint_cov"].shape == (N, 17, 6) and sel["joint_cov"].dtype == np.float64
        for k in ("joint_hypothesis", "joint_hypothesis_tree"):
            assert sel[k].shape == (N, 17) and sel[k].dtype == np.int32 and ((sel[k] >= 0) & (sel[k] < H)).all()
        for k in ("joint_spread_m", "joint_weight", "joint_logz", "joint_bone_m"):
            assert sel[k].shape == (N, 17) and sel[k].dtype == np.float64 and np.isfinite(sel[k]).all()
        assert sel["bone"].shape == () and float(sel["bone"]) == 100.0 and sel["temperature"].shape == ()
        c = sel["joint_cov"]
        assert np.allclose(sel["joint_spread_m"], np.sqrt(c[:, :, 0] + c[:, :, 3] + c[:, :, 5]), rtol=1e-15, atol=0.0)
        assert (sel["joint_weight"] > 0).all() and (sel["joint_weight"] <= 1.0 + 1e-3).all() and (sel["joint_bone_m"] >= 0).all()
    assert float(_sel(runs, "fused")["temperature"]) == 1.0 and float(_sel(runs, "cold")["temperature"]) == 1e-9
    t, f = _sel(runs, "tree"), _sel(runs, "fused")
    for k in ("hypothesis", "T", "reproj_px_pose_level"):              # the pose-level arrays are those of --select joints-tree
        assert f[k].dtype == t[k].dtype and f[k].tobytes() == t[k].tobytes(), k


def test_the_min_sum_assignment_rides_along_and_a_cold_run_is_it(runs, arrays):
    """At 1e-9 the arg-max is the joints-tree assignment and the written pose is the joints-tree pose within fp32 rounding of the mean:
    three fp32 roundings of numbers below the largest coordinate (x + T and - T in the composed pose, one in the fused one) and what
    the weights themselves leave off the kept hypothesis (concentrated_mean_bound on the call's own d_w, whose other outputs are the
    file's bits); joint_bone_m is the joints-tree bone within concentrated_bone_bound.  Neither tolerance scales with marg_bound,
    which is wide at this temperature."""
    import zedo_hip as zh
    t, f, c = _sel(runs, "tree"), _sel(runs, "fused"), _sel(runs, "cold")
    assert np.array_equal(f["joint_hypothesis_tree"], t["joint_hypothesis"]) and np.array_equal(c["joint_hypothesis_tree"], t["joint_hypothesis"])
    assert np.array_equal(c["joint_hypothesis"], t["joint_hypothesis"])
    a = arrays
    out = zh.joint_tree_marginal(dev(a["jerr"], torch.float64), dev(a["x"]), dev(a["T"]), R.H36M_PARENTS, N, 100.0, 1e-9, dev(a["conf"]),
                                 return_weights=True)
    mean, _, hmax, wmax, _, bone, w = (v.cpu().numpy() for v in out)
    assert np.array_equal(hmax, c["joint_hypothesis"]) and wmax.tobytes() == c["joint_weight"].tobytes() and bone.tobytes() == c["joint_bone_m"].tobytes()
    r = M.joint_tree_marginal_ref(a["jerr"], a["x"], a["T"], R.H36M_PARENTS, 100.0, 1e-9, N, a["conf"])
    X = M.camera_frame(a["x"], a["T"], N)
    xmax = float(np.abs(X).max())
    tol = M.concentrated_mean_bound(w, t["joint_hypothesis"], X) + 3 * 2.0 ** -23 * xmax
    d = np.abs(c["pose"].astype(np.float64) - t["pose"]).max(2)
    bb = M.concentrated_bone_bound(w, t["joint_hypothesis"], R.H36M_PARENTS, t["joint_bone_m"], M.marg_bound(17, H, r["G"]), r["G"], r["bmax"], r["lmax"])
    e_bone = np.abs(c["joint_bone_m"] - t["joint_bone_m"])
    print(f"driver joints-tree-fused at 1e-9 against joints-tree: max |pose - pose| = {d.max():.3e} m (largest allowed {tol.max():.3e}, of which "
          f"fp32 rounding {3 * 2.0 ** -23 * xmax:.3e}); max |bone - bone| = {e_bone.max():.3e} m (largest allowed {bb.max():.3e}); smallest "
          f"largest marginal {c['joint_weight'].min():.9f}")
    assert (d <= tol).all() and c["joint_weight"].min() > 0.99
    assert (e_bone <= bb).all()


def test_the_written_arrays_are_the_reference_on_the_runs_own_arrays(runs, arrays):
    a, sel = arrays, _sel(runs, "fused")
    assert np.array_equal(np.load(runs["fused"][1]), a["x"].reshape(H, N, 17, 3).transpose(1, 0, 2, 3))
    r = M.joint_tree_marginal_ref(a["jerr"], a["x"], a["T"], R.H36M_PARENTS, 100.0, 1.0, N, a["conf"])
    beta = M.marg_bound(17, H, r["G"])
    spread, xmax = M.spread_of(a["x"], a["T"], N)
    T_sel = sel["T"].astype(np.float64)
    want = r["mean"] - T_sel[:, None, :]
    e_pose = float(np.abs(sel["pose"] - want).max())
    e_cov = np.abs(sel["joint_cov"] - r["cov"])
    e_lz = float(np.abs(sel["joint_logz"] - r["logz"]).max())
    e_bone = float(np.abs(sel["joint_bone_m"] - r["bone"]).max())
    print(f"driver joints-tree-fused: max |pose - ref| = {e_pose:.3e} m, |cov - ref| = {e_cov.max():.3e} m^2, |logz - ref| = {e_lz:.3e} (bound "
          f"{beta:.3e}), |bone - ref| = {e_bone:.3e} m; largest marginal median {np.median(sel['joint_weight']):.2f}")
    assert e_pose <= M.mean_bound(beta, xmax) + 2.0 ** -23 * xmax     # the mean's bound and the rounding to fp32 of a number below xmax
    assert (e_cov <= M.cov_bound(beta, spread, xmax)[:, :, None]).all() and e_lz <= beta
    assert e_bone <= M.bone_bound(beta, r["bmax"], r["lmax"])
    clear = M.clear_argmax(r, beta)
    assert np.array_equal(sel["joint_hypothesis"][clear], r["hmax"][clear])
    assert np.abs(sel["joint_weight"] - r["wmax"]).max() <= np.expm1(beta)


def test_eval_prints_the_fused_pose_after_the_best_of_h_lines(tmp_path, capsys):
    _, errs, out = _inference(BASE + ["--out", str(tmp_path / "a.npy"), "--eval"], capsys)
    _, errs_s, out_s = _inference(BASE + ["--out", str(tmp_path / "b.npy"), "--eval", "--select", "joints-tree-fused"], capsys)
    lines, lines_s = out.splitlines(), out_s.splitlines()
    assert lines_s[:len(lines)] == lines and len(lines_s) == len(lines) + 2                        # the existing lines have not moved
    assert lines_s[-2].startswith("joints-tree-fused MPJPE : ") and lines_s[-1].startswith("joints-tree-fused PA-MPJPE : ")
    assert len(errs) == 2 and errs_s[:2] == errs and len(errs_s) == 4
    s1, s2 = float(lines_s[-2].split(" : ")[1]), float(lines_s[-1].split(" : ")[1])
    assert (s1, s2) == errs_s[2:] and np.isfinite([s1, s2]).all() and s2 <= s1 + 1e-9


def test_refusals_through_main(tmp_path):
    import run.inference as inf
    import run.opt_main as om
    out = ["--out", str(tmp_path / "r.npy")]

    def refused(argv, words, mod=inf):
        with pytest.raises(SystemExit) as e:
            mod.main(mod.parse_args(["prog"] + BASE + argv))
        assert words in str(e.value), (argv, str(e.value))

    fused = out + ["--select", "joints-tree-fused"]
    for bad in ("-1", "nan", "inf"):
        refused(fused + ["--bone", bad], "a finite weight >= 0 expected")
    for bad in ("0", "-1", "nan", "inf"):
        refused(fused + ["--temperature", bad], "a finite temperature > 0 expected")
    refused(fused + ["--smooth", "10"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal")
    refused(fused + ["--seq_len", "4"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal")
    refused(fused + ["--accel", "10"], "--accel is a switch of --select joints-temporal")
    refused(fused + ["--prune", "5:2"], "--prune with --select joints-tree-fused is not supported yet")
    refused(["--select", "joints-tree-fused"], "run.inference only", om)
    refused(fused + ["--hypo", "188"], "--select joints-tree-fused admits at most 187 hypotheses per pose at 17 joints")   # max_h(17) + 1
    assert not (tmp_path / "r.npy").exists()
