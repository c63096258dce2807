#!/usr/bin/env python3
"""Time the pruned OIL loop (Pipeline.run_pruned) against the unpruned pass (Pipeline.run) in ONE process on the seeded problem of
bench.py at BASELINE configs[2]'s shape: 1 015 poses x H = 50 hypotheses, IPO 500 iterations, S = 1000 OIL steps, 3DPW settings.

The plans `none`, `0:50` (the identity table: every hypothesis is kept, pure overhead), `100:10`, `0:10` and `0:25,200:5` ALTERNATE
--reps times after one warm-up pass of each; every pass is timed with device events around it on the launch stream.  No speed-up is
fixed in advance: the yardstick is the unpruned leg of the same process.  Reported per plan: median / min / max milliseconds per pass,
poses per second at the median, the row-step fraction of the plan (plain arithmetic), the measured time over the unpruned median, and
the share of poses whose unpruned select_reproj winner is among the plan's survivors - a property of the synthetic inputs (random-init
weights), recorded and not asserted.  Whether pruning costs accuracy on real data is NOT measured by this tool or anywhere.

One prune stage (zedo_min_reproj + zedo_prune_rank + zedo_prune_gather on 50 x 1015 rows, keep 10) alternates --stage_reps times with
ONE OIL step on the same rows; two conditions follow from the project's own figures and are recorded as booleans:

    identity_inside_spread   median(0:50) <= max(none) + the stage's median cost
    stage_below_one_step     median(stage) < median(one OIL step at the same row count)

    python tools/prune_timing.py [--reps 5] [--stage_reps 25] [--out profiles/prune.json]   (GPU box only)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))

import numpy as np
import torch

N, H, S = 1015, 50, 1000
PLANS = ("none", "0:50", "100:10", "0:10", "0:25,200:5")
STAGE_KEEP = 10


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def spread(v, nd=3):
    return dict(median=round(float(np.median(v)), nd), min=round(float(min(v)), nd), max=round(float(max(v)), nd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage_reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.reps < 3 or a.stage_reps < 20:
        ap.error("--reps must be at least 3 and --stage_reps at least 20")
    import zedo_hip as zh
    from lib.dataset import synthetic as syn
    from zedo_hip.pipeline import Pipeline, ZeDOConfig, parse_prune_plan, prune_row_steps
    dev = torch.device("cuda")
    d = syn.make_poses(N, seed=2024)
    pipe = Pipeline(syn.make_weights(seed=0), ZeDOConfig.pw3d(OIL_iterations=S), dev).load(syn.make_clusters(H, seed=2024), d["db_2d"],
                                                                                          d["camera_param"])
    ident = torch.arange(H, dtype=torch.int32, device=dev)[:, None].expand(H, N).contiguous()

    def one_pass(plan):
        if plan == "none":
            x, T = pipe.run()
            return x, T, ident
        return pipe.run_pruned(plan)

    for plan in PLANS:                                               # warm-up: code objects, allocator, clocks
        one_pass(plan)
    torch.cuda.synchronize()
    ms = {p: [] for p in PLANS}
    last = {}
    for _ in range(a.reps):
        for plan in PLANS:
            t, last[plan] = timed(lambda: one_pass(plan))
            ms[plan].append(t)
    xu, Tu, _ = last["none"]
    assert bool(torch.isfinite(xu).all()), "the unpruned pass is not finite"
    _, winner = pipe.select_reproj(xu, Tu)
    xi, Ti, hi = last["0:50"]
    assert torch.equal(xi, xu) and torch.equal(Ti, Tu) and torch.equal(hi, ident), "the identity plan changed a bit"

    # one prune stage against one OIL step on the same 50 x 1015 rows, alternating
    x0, T0 = xu.clone(), Tu.clone()
    step_at = S // 2

    def stage():
        err, _, _ = zh.min_reproj(x0, T0, pipe.uv, pipe.K, pipe.conf, N)
        return zh.prune_gather(zh.prune_rank(err, N, STAGE_KEEP), x0, T0)

    def parts():
        t1, r = timed(lambda: zh.min_reproj(x0, T0, pipe.uv, pipe.K, pipe.conf, N))
        t2, keep = timed(lambda: zh.prune_rank(r[0], N, STAGE_KEEP))
        t3, _ = timed(lambda: zh.prune_gather(keep, x0, T0))
        return t1 * 1e3, t2 * 1e3, t3 * 1e3

    xs, Ts = xu.clone(), Tu.clone()
    step = lambda: zh.oil_run(pipe.weights, pipe.sched, xs, pipe.geom, Ts, step_at, step_at + 1, S // 5)
    for _ in range(3):
        stage()
        step()
        parts()
    torch.cuda.synchronize()
    t_stage, t_step, t_parts = [], [], []
    for _ in range(a.stage_reps):
        t_stage.append(timed(stage)[0] * 1e3)
        t_step.append(timed(step)[0] * 1e3)
        t_parts.append(parts())
    st, sp = spread(t_stage, 1), spread(t_step, 1)
    pm = np.median(np.array(t_parts), axis=0)

    none = spread(ms["none"])
    rec = dict(tool="tools/prune_timing.py", device=torch.cuda.get_device_name(0), math=pipe.weights.math, N=N, H=H, S=S, reps=a.reps,
               stage_reps=a.stage_reps,
               accuracy="UNMEASURED: whether pruning by reprojection error costs accuracy cannot be measured with random-init weights and "
                        "synthetic poses",
               plans={})
    for plan in PLANS:
        steps = parse_prune_plan(plan, H, S) if plan != "none" else []
        done, total = prune_row_steps(steps, H, S)
        s = spread(ms[plan])
        hyp = last[plan][2]
        rec["plans"][plan] = dict(ms_per_pass=s, poses_per_s=round(N / s["median"] * 1e3, 1), row_step_fraction=round(done / total, 4),
                                  time_over_unpruned=round(s["median"] / none["median"], 4), survivors=int(hyp.shape[0]),
                                  unpruned_winner_survives_share=round(float((hyp == winner[None, :]).any(0).double().mean()), 4))
    rec["prune_stage"] = dict(rows=H * N, keep=STAGE_KEEP, stage_us=st, one_oil_step_us=sp,
                              parts_median_us=dict(min_reproj=round(float(pm[0]), 1), prune_rank=round(float(pm[1]), 1),
                                                   prune_gather=round(float(pm[2]), 1)),
                              stage_over_one_step=round(st["median"] / sp["median"], 4))
    rec["conditions"] = dict(
        identity_inside_spread=bool(rec["plans"]["0:50"]["ms_per_pass"]["median"] <= none["max"] + st["median"] * 1e-3),
        identity_minus_unpruned_median_ms=round(rec["plans"]["0:50"]["ms_per_pass"]["median"] - none["median"], 3),
        unpruned_spread_ms=round(none["max"] - none["min"], 3),
        stage_below_one_step=bool(st["median"] < sp["median"]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
