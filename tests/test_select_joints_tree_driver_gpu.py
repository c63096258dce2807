"""GPU: `run.inference --select joints-tree [--bone MU]` - the joint-wise, label-free aggregation with the skeleton as a coupling, as a
stage of the driver.  results.npy stays what it is; beside it <out>_selected.npz holds, per detection, the pose assembled from the
assignment zedo_joint_tree_select keeps (confidence-weighted reprojection distances plus MU times the bones' length mismatch, exact
min-sum over the dataset's bone tree), in the frame of the pose-level winner.  One process runs none, joints, joints-tree, --bone 0,
--bone 1e9 and --bone 3 (a weight at which these far-apart synthetic hypotheses may still be mixed) once; the tests share those runs.
The written assignment, cost and bone lengths are held to the numpy reference of tests/_joint_tree_ref.py on the run's own arrays.  Whether the coupled pose is closer to ground truth on real data is not measured: the
inputs here are synthetic.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

import _joint_tree_ref as R
from _joint_ref import compose_ref
from _shared import _inference, _problem, _rows_and_T, _sel, cfg_path, dev, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S = 8, 3, 10
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]

KEYS = ("pose", "joint_hypothesis", "joint_hypothesis_per_joint", "joint_reproj_px", "joint_bone_m", "tree_cost", "hypothesis", "T", "reproj_px",
        "reproj_px_pose_level", "bone")
RUNS = {"none": [], "joints": ["--select", "joints"], "tree": ["--select", "joints-tree"], "tree0": ["--select", "joints-tree", "--bone", "0"],
        "tree1e9": ["--select", "joints-tree", "--bone", "1e9"], "tree3": ["--select", "joints-tree", "--bone", "3"]}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every run once, in this process: name -> (results array, path of the out file, stdout)."""
    import contextlib
    import io

    import run.inference as inf
    d = tmp_path_factory.mktemp("tree")
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
    _, idx, jerr = zh.joint_reproj(x, T, dev(uv), dev(K), return_rows=True)
    return dict(x=x.cpu().numpy(), T=T.cpu().numpy(), jerr=jerr.cpu().numpy(), idx=idx.cpu().numpy(), uv=uv, K=K, conf=conf)


def test_results_file_is_unchanged_and_the_key_set_is_the_documented_one(runs):
    plain = np.load(runs["none"][1])
    assert plain.shape == (N, H, 17, 3)
    for name in RUNS:
        assert np.load(runs[name][1]).tobytes() == plain.tobytes(), name
        assert runs[name][2] == runs["none"][2], name                 # nothing more on stdout
    for name in ("tree", "tree0", "tree1e9", "tree3"):
        sel = _sel(runs, name)
        assert sorted(sel.files) == sorted(KEYS)
        assert sel["pose"].shape == (N, 17, 3) and sel["pose"].dtype == np.float32
        for k in ("joint_hypothesis", "joint_hypothesis_per_joint"):
            assert sel[k].shape == (N, 17) and sel[k].dtype == np.int32 and ((sel[k] >= 0) & (sel[k] < H)).all()
        for k in ("joint_reproj_px", "joint_bone_m"):
            assert sel[k].shape == (N, 17) and sel[k].dtype == np.float64
        assert sel["tree_cost"].shape == (N,) and sel["tree_cost"].dtype == np.float64
        assert sel["bone"].shape == () and sel["bone"].dtype == np.float64
    assert float(_sel(runs, "tree")["bone"]) == 100.0 and float(_sel(runs, "tree0")["bone"]) == 0.0 and float(_sel(runs, "tree1e9")["bone"]) == 1e9
    # what --select joints writes is what it wrote: the pose-level arrays and the per-joint arg-min are shared
    j, t = _sel(runs, "joints"), _sel(runs, "tree")
    for k, kj in (("hypothesis", "hypothesis"), ("T", "T"), ("reproj_px_pose_level", "reproj_px_pose_level"), ("joint_hypothesis_per_joint", "joint_hypothesis")):
        assert t[k].dtype == j[kj].dtype and t[k].tobytes() == j[kj].tobytes(), k


@pytest.mark.parametrize("name,mu", [("tree", 100.0), ("tree0", 0.0), ("tree1e9", 1e9), ("tree3", 3.0)])
def test_the_written_assignment_is_the_reference_on_the_runs_own_arrays(runs, arrays, name, mu):
    import zedo_hip as zh
    a, sel = arrays, _sel(runs, name)
    assert np.array_equal(np.load(runs[name][1]), a["x"].reshape(H, N, 17, 3).transpose(1, 0, 2, 3))
    r = R.joint_tree_ref(a["jerr"], a["x"], a["T"], R.H36M_PARENTS, mu, N, a["conf"])
    assert r["gap"] > R.GAP_MIN
    jh = sel["joint_hypothesis"]
    print(f"driver joints-tree bone={mu:g}: max |tree_cost - ref| = {np.abs(sel['tree_cost'] - r['cost']).max():.3e}, max |bone - ref| = "
          f"{np.abs(sel['joint_bone_m'] - r['bone']).max():.3e}; gap {r['gap']:.3e}; hypotheses per pose {np.mean([len(set(v)) for v in jh]):.2f}")
    assert np.array_equal(jh, r["joint_h"])
    if mu <= 300.0:
        bound = R.cost_bound(17, r["scale"])
        assert (np.abs(sel["tree_cost"] - r["cost"]) <= bound).all()
        assert (mu * np.abs(sel["joint_bone_m"] - r["bone"]) <= bound[:, None]).all()
    hyp = sel["hypothesis"]
    want = compose_ref(a["x"], a["T"], jh, hyp)
    assert np.array_equal(sel["pose"].view(np.int32), want.view(np.int32))
    assert sel["joint_reproj_px"].tobytes() == a["jerr"].reshape(H, N, 17)[jh, np.arange(N)[:, None], np.arange(17)[None, :]].tobytes()
    _, px, _ = zh.min_reproj(dev(sel["pose"]), dev(sel["T"]), dev(a["uv"]), dev(a["K"]), dev(a["conf"]))
    assert px.cpu().numpy().tobytes() == sel["reproj_px"].tobytes()
    if mu == 0.0:                                                     # --select joints
        assert np.array_equal(jh, _sel(runs, "joints")["joint_hypothesis"]) and np.array_equal(jh, a["idx"])
        assert sel["pose"].tobytes() == _sel(runs, "joints")["pose"].tobytes()
    if mu == 1e9:                                                     # one whole hypothesis per pose, in the pose-level winner's frame
        assert (jh == jh[:, :1]).all() and (sel["joint_bone_m"] == 0).all()
        whole = np.argmin(R.unaries(a["jerr"], N, a["conf"]).sum(1), axis=1)
        assert np.array_equal(jh[:, 0], whole)
        assert np.array_equal(sel["pose"].view(np.int32), compose_ref(a["x"], a["T"], np.repeat(whole[:, None].astype(np.int32), 17, 1), hyp).view(np.int32))


def test_eval_prints_the_coupled_pose_after_the_best_of_h_lines(tmp_path, capsys):
    _, errs, out = _inference(BASE + ["--out", str(tmp_path / "a.npy"), "--eval"], capsys)
    _, errs_s, out_s = _inference(BASE + ["--out", str(tmp_path / "b.npy"), "--eval", "--select", "joints-tree"], capsys)
    lines, lines_s = out.splitlines(), out_s.splitlines()
    assert lines_s[:len(lines)] == lines and len(lines_s) == len(lines) + 2                        # the existing lines have not moved
    assert lines_s[-2].startswith("joints-tree MPJPE : ") and lines_s[-1].startswith("joints-tree PA-MPJPE : ")
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

    for sel in ("none", "reproj", "joints", "temporal", "joints-temporal", "joints-fused"):
        refused(out + ["--select", sel, "--bone", "100"], "--bone is a switch of --select joints-tree")
    refused(out + ["--bone", "100"], "--bone is a switch of --select joints-tree")
    for bad in ("-1", "nan", "inf"):
        refused(out + ["--select", "joints-tree", "--bone", bad], "a finite weight >= 0 expected")
    tree = out + ["--select", "joints-tree"]
    refused(tree + ["--smooth", "10"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal")
    refused(tree + ["--seq_len", "4"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal")
    refused(tree + ["--temperature", "2"], "--temperature is a switch of --select joints-fused")
    refused(tree + ["--accel", "10"], "--accel is a switch of --select joints-temporal")
    refused(tree + ["--prune", "5:2"], "--prune with --select joints-tree is not supported yet")
    refused(["--select", "joints-tree"], "run.inference only", om)
    refused(["--bone", "100"], "--bone is a switch of --select joints-tree", om)
    assert not (tmp_path / "r.npy").exists()
