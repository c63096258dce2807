"""CPU: `python bench.py --gpus N` is a real launcher (one fresh process per GPU, RCCL rendezvous on 127.0.0.1) and the
row arithmetic of the eval surface's device-side subsampling."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env_without_ranks():
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    return e


def test_dry_launch_describes_one_rank_per_gpu():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "3", "--dry-launch"], capture_output=True, text=True,
                       env=_env_without_ranks(), timeout=300)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["dry_launch"] and d["gpus"] == 4 and len(d["ranks"]) == 4
    assert "--dry-launch" not in d["cmd"] and d["cmd"][-4:] == ["--gpus", "4", "--steps", "3"]
    ports = {x["MASTER_PORT"] for x in d["ranks"]}
    assert len(ports) == 1 and 1024 < int(ports.pop()) < 65536
    for i, x in enumerate(d["ranks"]):
        assert x["RANK"] == x["LOCAL_RANK"] == str(i) and x["WORLD_SIZE"] == "4" and x["MASTER_ADDR"] == "127.0.0.1"
        assert x["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and x["ZEDO_NO_BUILD"] == "1"     # the parent builds, never a rank


def test_launcher_refuses_more_ranks_than_gpus_instead_of_benchmarking_one():
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs visible")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, env=_env_without_ranks(), timeout=300)
    assert r.returncode != 0 and "GPU(s) are visible" in r.stderr and not r.stdout.strip()


def test_launcher_propagates_a_failing_rank():
    """bench.launch_ranks itself (the test used to re-implement its loop): two "ranks" that are plain python
    processes - rank 1 fails with code 7, the launcher must end rank 0 (which would sleep for a minute) and return 7."""
    sys.path.insert(0, ROOT)
    import time
    import bench
    code = "import os,sys,time; r=int(os.environ['RANK']); assert os.environ['ZEDO_NO_BUILD']=='1'; time.sleep(0.3 if r else 60); sys.exit(7 if r else 0)"
    old = dict(os.environ)
    os.environ.update(ZEDO_SHARE_DEVICE="1", ZEDO_DIST_BACKEND="gloo")      # no GPU count check on this CPU box
    try:
        real = bench.torch.cuda.device_count
        bench.torch.cuda.device_count = lambda: 1
        t0 = time.time()
        rc = bench.launch_ranks(2, [], cmd=[sys.executable, "-c", code], build=False)   # launcher logic only: no hipcc, no tree edits
        dt = time.time() - t0
    finally:
        bench.torch.cuda.device_count = real
        os.environ.clear()
        os.environ.update(old)
    assert rc == 7 and dt < 30, (rc, dt)
    # every rank exits 0 -> 0; a rank killed by a signal -> 1
    procs = [subprocess.Popen([sys.executable, "-c", "pass"]) for _ in range(3)]
    assert bench.supervise(procs, poll_s=0.05) == 0
    procs = [subprocess.Popen([sys.executable, "-c", "import os,signal; os.kill(os.getpid(), signal.SIGKILL)"]),
             subprocess.Popen([sys.executable, "-c", "import time; time.sleep(60)"])]
    assert bench.supervise(procs, poll_s=0.05) == 1 and procs[1].poll() is not None


def test_share_device_needs_the_gloo_transport():
    sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))
    e = _env_without_ranks()
    e.update(ZEDO_SHARE_DEVICE="1")
    e.pop("ZEDO_DIST_BACKEND", None)
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'zedo-release_amd'); from zedo_hip import pipeline as p; p.local_device_index()"],
                       capture_output=True, text=True, env=e, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "ZEDO_DIST_BACKEND=gloo" in r.stderr


def test_missing_library_is_built_once_under_a_lock_or_refused(tmp_path):
    """zedo_build.ensure_library: N ranks that find no library build it ONCE (exclusive lock; VERDICT r3: N concurrent
    `make`s into the same objects), a rank of a launcher that has built already (ZEDO_NO_BUILD=1) fails loudly instead."""
    import importlib.util
    import shutil
    pkg = tmp_path / "pkg"
    (pkg / "csrc").mkdir(parents=True)
    (pkg / "zedo_hip").mkdir()
    shutil.copy(os.path.join(ROOT, "zedo-release_amd", "zedo_build.py"), pkg / "zedo_build.py")
    # a stand-in Makefile that counts its invocations and takes a while, like hipcc does
    (pkg / "csrc" / "Makefile").write_text("all:\n\techo x >> builds.log\n\tsleep 1\n\ttouch ../zedo_hip/libzedo_hip.so.tmp && mv ../zedo_hip/libzedo_hip.so.tmp ../zedo_hip/libzedo_hip.so\n")
    code = f"import sys; sys.path.insert(0, {str(pkg)!r}); import zedo_build; print(zedo_build.ensure_library())"
    e = _env_without_ranks()
    e["ZEDO_NO_BUILD"] = "1"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=60)
    assert r.returncode != 0 and "ZEDO_NO_BUILD=1" in r.stderr and not (pkg / "csrc" / "builds.log").exists()
    e.pop("ZEDO_NO_BUILD")
    procs = [subprocess.Popen([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, text=True) for _ in range(6)]
    outs = [p.communicate(timeout=120)[0].strip() for p in procs]
    assert all(p.returncode == 0 for p in procs) and all(o.endswith("libzedo_hip.so") for o in outs), outs
    assert (pkg / "csrc" / "builds.log").read_text().count("x") == 1


def test_strong_scaling_projection_reads_the_one_gpu_shard_measurements():
    """bench.py --scaling strong reports efficiency_vs_projection against what ONE GPU measured for a rank's shard
    (profiles/strong_shards_r04.jsonl); the self-check problem is fixed and small."""
    sys.path.insert(0, ROOT)
    import bench
    r8, ms8, src = bench.strong_projection(6344, "f32")      # configs[2] over 8 ranks: 6 344 rows on rank 0, measured at 6 350
    assert r8 == 6350 and 400 < ms8 < 600 and src.startswith("profiles/strong_shards_r")
    assert bench.strong_projection(6344, "f16x3")[1] < ms8       # the alt-mode time of the same record
    assert bench.strong_projection(12688, "f32")[0] == 12700 and bench.strong_projection(25375, "f32")[0] == 25400
    assert bench.strong_projection(9000, "f32") is None          # nothing measured within 2 %
    assert bench.SELFCHECK == dict(poses=64, hypo=5, oil=20)


def test_workload_table_matches_the_baseline_configs():
    sys.path.insert(0, ROOT)
    import bench
    b = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert "1000 steps" in b["configs"][2] and "H=50" in b["configs"][2]
    assert bench.WORKLOADS[2]["poses"] == 1015 and bench.WORKLOADS[2]["default_scaling"] == "weak"
    assert bench.WORKLOADS[3]["poses"] == 567040 and bench.WORKLOADS[3]["weak"] * 8 == 567040
    assert "100k" in b["configs"][4] and bench.WORKLOADS[4]["poses"] == 100000 and bench.WORKLOADS[4]["weak"] * 8 == 100000


@pytest.mark.parametrize("N,H,k", [(10, 3, 3), (7, 2, 2), (9, 4, 1), (5, 3, 7)])
def test_device_side_subsampling_of_row_shards(N, H, k):
    """eval_multi(sample_interval=k) on ("rows", ...) shards == on the [N,H,J,3] layout (reference h36m.py:386-387): the kept
    rows of every contiguous shard are the contiguous shard [new_offset, ...) of the subsampled problem."""
    sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))
    from lib.dataset._eval import subsample
    rows = torch.arange(H * N * 2 * 3, dtype=torch.float32).reshape(H * N, 2, 3)        # row = h*N + n
    gt = np.arange(N * 2 * 3, dtype=np.float64).reshape(N, 2, 3)
    dense = rows.reshape(H, N, 2, 3).permute(1, 0, 2, 3)                                   # [N,H,J,3]
    ref_p, ref_gt, _ = subsample(dense, gt, k)
    ref_rows = ref_p.permute(1, 0, 2, 3).reshape(-1, 2, 3)                                 # rows of the subsampled problem
    for lo in range(0, H * N):
        for cnt in (1, 4, H * N - lo):
            cnt = min(cnt, H * N - lo)
            (tag, got), g2, off = subsample(("rows", rows[lo:lo + cnt]), gt, k, lo)
            assert tag == "rows" and np.array_equal(g2, ref_gt)
            assert torch.equal(got, ref_rows[off:off + got.shape[0]]), (lo, cnt, off)


def test_valid_ind_mask_is_one_scatter_and_scales_to_the_full_test_set():
    """eval_multi(valid_ind=...) (reference h36m.py:396-397): the mask over device rows is built from ONE flat index list
    and ONE scatter (a Python statement per pose took minutes at configs[3]'s 567 040 poses).  Equal to
    the per-pose loop on every shard of a small problem; half a million poses in well under ten seconds on a CPU."""
    import time
    sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))
    from lib.dataset._eval import valid_rows_mask
    rng = np.random.default_rng(3)
    N, H = 23, 7
    vi = [sorted(rng.choice(H + 2, size=rng.integers(0, H), replace=False).tolist()) for _ in range(N)]     # some indices >= H, some poses empty
    ok = np.zeros((H, N), bool)
    for n in range(N):
        for h in vi[n]:
            if 0 <= h < H:
                ok[h, n] = True
    flat = ok.reshape(-1)
    for lo, cnt in ((0, H * N), (5, 40), (H * N - 9, 9), (17, 1)):
        got = valid_rows_mask(vi, N, lo, cnt, torch.device("cpu")).numpy()
        assert np.array_equal(got, flat[lo:lo + cnt]), (lo, cnt)
        # the reference only ever evaluates `valid_ind[idx]`: a mapping {pose: hypotheses}, sets and generators-per-pose are as valid as a list
        as_dict = {n: set(vi[n]) for n in range(N)}
        assert np.array_equal(valid_rows_mask(as_dict, N, lo, cnt, torch.device("cpu")).numpy(), flat[lo:lo + cnt])
        as_arrays = np.array([np.asarray(v, dtype=np.int64) for v in vi], dtype=object)
        assert np.array_equal(valid_rows_mask(as_arrays, N, lo, cnt, torch.device("cpu")).numpy(), flat[lo:lo + cnt])
    N, H = 567040, 50
    vi = [(n % H, (n * 7) % H, (n * 13) % H) for n in range(N)]
    t0 = time.time()
    m = valid_rows_mask(vi, N, 0, H * N, torch.device("cpu"))
    dt = time.time() - t0
    assert int(m.sum()) == sum(len(set(v)) for v in vi) and m.shape == (H * N,)
    assert bool(m[(0 % H) * N + 0]) and bool(m[((5 * 7) % H) * N + 5]) and dt < 10.0, dt


def test_ulp_perturbation_and_tile_split_helpers():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))
    import bench
    from lib.dataset import synthetic as syn
    uv = syn.make_poses(50, seed=1)["db_2d"][:, :, :2]
    assert np.array_equal(syn.perturb_ulp(uv, 0), uv)
    p1, p1b, p2 = syn.perturb_ulp(uv, 5), syn.perturb_ulp(uv, 5), syn.perturb_ulp(uv, 6)
    assert np.array_equal(p1, p1b) and not np.array_equal(p1, p2) and p1.dtype == np.float32
    steps = (p1.view(np.int32).astype(np.int64) - uv.view(np.int32).astype(np.int64))
    assert set(np.unique(steps)) == {-1, 0, 1}                     # one unit in the last place at most (positive floats)
    for rows in (1, 64, 886, 2048, 2049, 6350, 8192, 12700, 20000, 50750, 1 << 20):
        sp = bench.f16x3_tile_split(rows)
        assert sum(r for _, _, r in sp) == -(-rows // 64) * 64 and all(r % bm == 0 for bm, _, r in sp)


def test_dump_outputs_are_float_arrays_a_fixed_sample_and_capped(tmp_path):
    """bench.py --dump-outputs: what a caller of the timed path receives, as float32 / float64 arrays; an output of more than
    DUMP_ROWS rows is the same seeded sample of its rows in every run (indices in <name>_rows); all files stay within DUMP_BYTES."""
    sys.path.insert(0, ROOT)
    import bench
    n, N = bench.DUMP_ROWS + 5, 7
    x = torch.arange(n * 51, dtype=torch.float32).reshape(n, 17, 3)
    T = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    out = {k: (torch.rand(N, dtype=torch.float64), torch.arange(N, dtype=torch.int32) % 3) for k in ("p1", "p2")}
    out.update(p1_actionwise=0.25, p2_actionwise=0.125)
    a, b = (bench.host_outputs(bench.output_arrays(bench.WORKLOADS[3], x, T, out)) for _ in range(2))
    assert set(a) == {"x", "x_rows", "T", "T_rows", "p1_best", "p1_hypothesis", "p2_best", "p2_hypothesis", "p1_actionwise", "p2_actionwise"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["x_rows"].astype(np.int64)
    assert a["x"].shape == (bench.DUMP_ROWS, 17, 3) and len(np.unique(rows)) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["x"], x.numpy()[rows]) and np.array_equal(a["T"], T.numpy()[rows])
    assert np.array_equal(a["p1_hypothesis"], out["p1"][1].numpy()) and a["p2_actionwise"].tolist() == [0.125]
    bench.write_outputs(a, str(tmp_path / "d"))
    for k, v in a.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v)
    g = bench.host_outputs(bench.output_arrays(bench.WORKLOADS[4], x, T, {"results": x[:10]}))
    assert set(g) == {"results"} and g["results"].shape == (10, 17, 3)
    with pytest.raises(SystemExit):
        bench.write_outputs({"big": np.zeros(bench.DUMP_BYTES // 8 + 1)}, str(tmp_path / "e"))
    assert not (tmp_path / "e").exists()
