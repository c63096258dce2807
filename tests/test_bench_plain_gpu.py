"""bench.py's plain run on an MI355X (-m gpu): the headline only - every object of --full is null - with --steps timed passes,
and --dump-outputs writes what the last timed pass computed; two runs with the same arguments write identical files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ZEDO_FORCE_DIST", "ZEDO_BENCH_FORCE_LAUNCH"):
        e.pop(k, None)
    return e


def test_plain_run_times_the_steps_and_dumps_the_last_pass(tmp_path, math_mode):
    N, H = 64, 3
    files, lines = [], []
    for run in range(2):
        d = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--poses", str(N),
               "--hypo", str(H), "--oil", "20", "--math", math_mode, "--dump-outputs", str(d)]
        r = subprocess.run(cmd, env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
        files.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a = lines[0]
    assert a["steps"] == 2 and a["warmup"] == 1 and a["full"] is False and a["higher_is_better"] is True and a["unit"] == "poses/s"
    assert a["dtype"] == "f32" if math_mode == "f32" else a["dtype"].startswith("f32 (hidden layers")
    assert a["ms_per_step"] > 0 and abs(a["value"] * a["ms_per_step"] / 1e3 - N) < 1e-2 * N        # value = poses / (ms_per_step / 1000)
    for k in ("roofline", "alt_mode", "geometry_kernels", "cpu_baseline", "kernel_time_ms_sampled_avg", "multi_rank_selfcheck", "strong"):
        assert a[k] is None, k
    f = files[0]
    assert set(f) == {"x", "T", "p1_best", "p1_hypothesis", "p2_best", "p2_hypothesis"}
    assert f["x"].shape == (H * N, 17, 3) and f["x"].dtype == np.float32 and f["T"].shape == (H * N, 3) and f["T"].dtype == np.float32
    for k in ("p1", "p2"):
        assert f[k + "_best"].shape == (N,) and f[k + "_best"].dtype == np.float64 and np.isfinite(f[k + "_best"]).all()
        assert set(np.unique(f[k + "_hypothesis"])) <= set(range(H))
    assert abs(float(f["p1_best"].mean()) - a["mpjpe_best_of_H_m"]) < 1e-6 and abs(float(f["p2_best"].mean()) - a["pa_mpjpe_best_of_H_m"]) < 1e-6
    assert all(np.array_equal(f[k], files[1][k]) for k in f), "two runs with the same arguments differ"
    assert lines[1]["selection_sha16"] == a["selection_sha16"]
