"""GPU: `--prune PLAN` of run.inference and run.opt_main - hypotheses pruned during the loop as a switch of the driver.  With it
results.npy holds the K_final survivors of every pose in ascending hypothesis order, <out>_pruned.npz names them, --select reproj works on
the survivors and reports the original hypothesis, and the evaluation prints `best of K survivors` lines and the row-step fraction.
Without it nothing changes.  --select joints / temporal, more than one rank and the step-wise sampler route refuse the switch.
The switch does not depend on the arithmetic mode of the dense layers: one session runs it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _shared import ROOT, _inference, cfg_path, free_port, one_arithmetic_mode  # noqa: F401  (one_arithmetic_mode: autouse fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, H, S, PLAN, KF = 9, 6, 40, "7:4,8:2", 2
BASE = ["--config", cfg_path("pw3d"), "--synthetic", str(N), "--hypo", str(H), "--oil_iterations", str(S)]


@pytest.fixture(scope="module")
def pipe():
    """The driver's pipeline on the driver's synthetic problem, built in this process."""
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    cfg = load_config(cfg_path("pw3d"))
    z = cfg.ZeDO
    d = syn.make_poses(N, seed=cfg.seed)
    p = Pipeline(syn.make_weights(seed=cfg.seed), ZeDOConfig(z.IPO_iterations, z.IPO_keylist, z.RotAxes, z.IPO_T, z.IPO_minScaleT, z.IPO_maxScaleT,
                                                             S, z.sampling_eps, 0.1, 1000, 0.1, 20.0), "cuda")
    return p.load(syn.make_clusters(H, seed=cfg.seed), d["db_2d"], d["camera_param"])


def test_inference_writes_the_survivors_their_ids_and_the_selection(pipe, tmp_path, capsys):
    out = tmp_path / "results.npy"
    res, errs, text = _inference(BASE + ["--out", str(out), "--prune", PLAN, "--select", "reproj", "--eval"], capsys)
    assert sorted(os.listdir(tmp_path)) == ["results.npy", "results_pruned.npz", "results_selected.npz"]
    x, T, hyp = pipe.run_pruned(PLAN)
    want = x.reshape(KF, N, 17, 3).permute(1, 0, 2, 3).cpu().numpy()
    a = np.load(out)
    assert a.shape == (N, KF, 17, 3) and a.dtype == np.float32 and a.tobytes() == want.tobytes() and np.array_equal(res, a)
    pr = np.load(tmp_path / "results_pruned.npz")
    assert sorted(pr.files) == ["hypothesis", "stage_keep", "stage_step"]
    assert pr["hypothesis"].shape == (N, KF) and pr["hypothesis"].dtype == np.int32 and np.array_equal(pr["hypothesis"], hyp.cpu().numpy().T)
    assert (np.diff(pr["hypothesis"], axis=1) > 0).all()
    assert pr["stage_step"].tolist() == [7, 8] and pr["stage_keep"].tolist() == [4, 2]
    # the survivors are rows of the unpruned run
    xu, Tu = pipe.run()
    full = xu.reshape(H, N, 17, 3).cpu().numpy()
    assert np.array_equal(a.view(np.int32), full[pr["hypothesis"], np.arange(N)[:, None]].view(np.int32))
    # --select reproj: on the survivors, the id mapped through the table
    sel = np.load(tmp_path / "results_selected.npz")
    assert sorted(sel.files) == ["T", "hypothesis", "pose", "reproj_px"]
    best, slot = pipe.select_reproj(x, T)
    slot = slot.cpu().numpy()
    assert sel["hypothesis"].dtype == np.int32 and np.array_equal(sel["hypothesis"], pr["hypothesis"][np.arange(N), slot])
    assert np.array_equal(sel["pose"].view(np.int32), a[np.arange(N), slot].view(np.int32))
    assert np.array_equal(sel["reproj_px"], best.cpu().numpy())
    assert np.array_equal(sel["T"].view(np.int32), T.reshape(KF, N, 3).cpu().numpy()[slot, np.arange(N)].view(np.int32))
    assert np.array_equal(sel["pose"].view(np.int32), full[sel["hypothesis"], np.arange(N)].view(np.int32))
    # the printed lines
    lines = text.splitlines()
    at = lambda key: [i for i, l in enumerate(lines) if l.startswith(key)]
    i1, i2, i3 = at(f"best of {KF} survivors MPJPE : "), at(f"best of {KF} survivors PA-MPJPE : "), at(f"pruned {PLAN}: row-steps ")
    assert len(i1) == len(i2) == len(i3) == 1 and i1[0] + 1 == i2[0] and i2[0] + 1 == i3[0]
    done = (H * 7 + 4 * 1 + 2 * (S - 8)) * N
    assert lines[i3[0]] == f"pruned {PLAN}: row-steps {done} of {H * S * N} ({done / (H * S * N):.4f})"
    assert at("reproj-selected MPJPE : ")[0] > i3[0] and len(at("mean MPJPE : ")) == 1 and at("mean MPJPE : ")[0] < i1[0]
    assert float(lines[i1[0]].split(" : ")[1]) == errs[0] and float(lines[i2[0]].split(" : ")[1]) == errs[1] and len(errs) == 4
    assert errs[2] >= errs[0] - 1e-12                                                       # one kept pose cannot beat the best of the survivors


def test_without_the_switch_nothing_changes(pipe, tmp_path, capsys):
    res, errs, text = _inference(BASE + ["--out", str(tmp_path / "results.npy"), "--eval"], capsys)
    assert sorted(os.listdir(tmp_path)) == ["results.npy"] and "survivors" not in text and "pruned" not in text
    xu, _ = pipe.run()
    want = xu.reshape(H, N, 17, 3).permute(1, 0, 2, 3).cpu().numpy()
    a = np.load(tmp_path / "results.npy")
    assert a.shape == (N, H, 17, 3) and a.tobytes() == want.tobytes()
    # the identity plan writes the same array
    _inference(BASE + ["--out", str(tmp_path / "ident.npy"), "--prune", f"0:{H}"], capsys)
    assert np.load(tmp_path / "ident.npy").tobytes() == a.tobytes()
    assert np.array_equal(np.load(tmp_path / "ident_pruned.npz")["hypothesis"], np.broadcast_to(np.arange(H, dtype=np.int32), (N, H)))


def test_opt_main_prints_the_survivor_lines(capsys):
    import run.opt_main as om
    capsys.readouterr()
    errs = om.main(om.parse_args(["prog"] + BASE + ["--prune", "12:1"]))
    lines = capsys.readouterr().out.splitlines()
    done = (H * 12 + 1 * (S - 12)) * N
    assert f"best of 1 survivors MPJPE : {errs[0]}" in lines and f"best of 1 survivors PA-MPJPE : {errs[1]}" in lines
    assert lines[-1] == f"pruned 12:1: row-steps {done} of {H * S * N} ({done / (H * S * N):.4f})"


def test_the_refusals(tmp_path):
    import run.inference as inf
    import run.opt_main as om
    out = ["--out", str(tmp_path / "r.npy")]
    for sel in ("temporal", "joints"):
        with pytest.raises(SystemExit) as e:
            inf.main(inf.parse_args(["prog"] + BASE + out + ["--prune", PLAN, "--select", sel]))
        assert "--prune" in str(e.value) and sel in str(e.value) and "follow-up" in str(e.value)
    for bad in ("8:4,7:2", "7:0", f"7:{H + 1}", f"{S}:2", "junk"):
        with pytest.raises(SystemExit) as e:
            om.main(om.parse_args(["prog"] + BASE + ["--prune", bad]))
        assert "--prune" in str(e.value) and repr(bad.split(",")[-1]) in str(e.value)
    # the step-wise sampler route
    cfg = tmp_path / "cfg_rd.py"
    cfg.write_text("import importlib.util\n"
                   f"_s = importlib.util.spec_from_file_location('base_cfg', r'{cfg_path('pw3d')}')\n"
                   "_m = importlib.util.module_from_spec(_s); _s.loader.exec_module(_m)\n"
                   "def get_config():\n"
                   "    c = _m.get_config()\n"
                   "    c.sampling.predictor = 'reverse_diffusion'\n"
                   "    return c\n")
    with pytest.raises(SystemExit) as e:
        inf.main(inf.parse_args(["prog", "--config", str(cfg), "--synthetic", "5", "--hypo", "4", "--oil_iterations", "4"] + out + ["--prune", "1:2"]))
    assert "--prune" in str(e.value) and "fused pipeline" in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.endswith((".npy", ".npz"))]            # no refusal left a result file behind


def test_two_ranks_refuse_the_switch(tmp_path):
    """Two fresh processes of a gloo launch: both end at once with the message, before a process group or a GPU is touched."""
    # not _shared.run_two_ranks: that launcher asserts exit status 0 of both ranks, this launch must end with status 1
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ZEDO_FORCE_DIST", "ZEDO_BENCH_FORCE_DIST"):
        env.pop(k, None)
    env.update(ZEDO_SHARE_DEVICE="1", ZEDO_DIST_BACKEND="gloo", ZEDO_NO_BUILD="1", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(free_port()), PYTHONPATH=os.path.join(ROOT, "zedo-release_amd") + os.pathsep + env.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-m", "run.inference"] + BASE + ["--out", str(tmp_path / "results.npy"), "--prune", PLAN]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), cwd=str(tmp_path), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    done = [p.communicate() + (p.returncode,) for p in procs]
    for r, (out, err, rc) in enumerate(done):
        assert rc == 1 and "--prune runs on one rank only" in err, (r, rc, out[-2000:], err[-4000:])
    assert os.listdir(tmp_path) == []
