#!/usr/bin/env python3
"""Time the joint-wise aggregation (zedo_joint_reproj) on both of its routes against zedo_min_reproj on the SAME rows, in ONE process on
seeded inputs, at 1 015 x 50 = 50 750 rows (BASELINE configs[2]) and 70 880 x 50 = 3 544 000 rows (configs[3]'s per-GPU shard), J = 17.

The yardstick is zedo_min_reproj in the same run: existing code that reads the same x and T and does the same arithmetic per joint.  It
writes and re-reads an 8-byte error per row; the walking route of zedo_joint_reproj (no d_jerr) writes 12 bytes per (pose, joint) and
nothing per row; the row route (d_jerr given) writes and re-reads 8 bytes per (row, joint).

After a warm-up of the three calls they ALTERNATE --reps times (default 25, at least 20); each call is timed with device events around it
on the launch stream (binding included: the output allocations from torch's cache and one ctypes call).  Reported per size: median /
min / max of each call in microseconds, the algorithmic bytes of each (every operand addressed, counted once per launch that addresses
it) and the GB/s they imply at the median.  NO gate; recorded beside the numbers is the rule of DESIGN.md 8.4 for the walking route,

    within_rule  <=>  median(walking) <= median(min_reproj) + (max - min of min_reproj in this run)

This measures speed only.  Whether joint-wise aggregation lowers the error against ground truth on real data is not measured here or
anywhere in this repository (random-init weights and synthetic poses cannot tell).

    python tools/joint_reproj_timing.py [--reps 25] [--out profiles/joint_reproj.json]   (GPU box only)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))

import numpy as np
import torch

SIZES = ((1015, 50), (70880, 50))
J = 17


def inputs(N, H, dev):
    """The rows of tools/select_reproj_timing.py: the pose's root-relative ground truth + 8 cm of seeded noise, T = the pose's root + 5 cm
    of noise - like a finished optimisation; the dataset's detections, intrinsics and confidences."""
    from lib.dataset import synthetic as syn
    d = syn.make_poses(N, seed=11, conf_mode="uniform", dtype3d=np.float64)
    t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    gt = t(d["db_3d"] - d["db_3d"][:, 0:1], torch.float64)
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + N)
    x = gt.to(torch.float32).repeat(H, 1, 1)
    x += 0.08 * torch.randn(x.shape, generator=g, dtype=torch.float32, device=dev)
    T = t(d["db_3d"][:, 0, :]).repeat(H, 1)
    T += 0.05 * torch.randn(T.shape, generator=g, dtype=torch.float32, device=dev)
    return x.contiguous(), T.contiguous(), t(d["db_2d"][:, :, :2]), t(d["camera_param"]), t(d["db_2d"][:, :, 2])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(us, nbytes):
    med = float(np.median(us))
    return dict(median_us=round(med, 1), min_us=round(float(min(us)), 1), max_us=round(float(max(us)), 1),
                algorithmic_bytes=int(nbytes), gb_per_s_at_median=round(nbytes / med / 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import zedo_hip as zh
    dev = torch.device("cuda")
    rec = dict(tool="tools/joint_reproj_timing.py", J=J, reps=a.reps, device=torch.cuda.get_device_name(0),
               accuracy_on_real_data="not measured", sizes={})
    for N, H in SIZES:
        B = N * H
        x, T, uv, K, conf = inputs(N, H, dev)
        calls = dict(joint_reproj_walking=lambda: zh.joint_reproj(x, T, uv, K),
                     joint_reproj_rows=lambda: zh.joint_reproj(x, T, uv, K, return_rows=True),
                     min_reproj=lambda: zh.min_reproj(x, T, uv, K, conf))
        for _ in range(3):                                           # warm-up of the three calls: code objects, allocator
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        us, last = {k: [] for k in calls}, {}
        for _ in range(a.reps):
            for k, fn in calls.items():
                t, last[k] = timed(fn)
                us[k].append(t)
        wb, wi = last["joint_reproj_walking"]
        rb, ri, jerr = last["joint_reproj_rows"]
        assert torch.equal(wb.view(torch.int64), rb.view(torch.int64)) and torch.equal(wi, ri), f"{B} rows: the routes disagree"
        assert bool(torch.isfinite(jerr).all()) and bool((wi >= 0).all()), f"{B} rows: a joint distance is not finite"
        mixed = float((wi.min(1).values != wi.max(1).values).double().mean())
        # bytes: the rows (x 204, T 12 per row), the per-pose operands (uv 136, K 36; conf 68), and what each call writes and re-reads:
        # walking: best / idx 12 per (pose, joint); rows: jerr written and read 16 per (row, joint) + best / idx; min_reproj: err 16 per row
        s = dict(joint_reproj_walking=stats(us["joint_reproj_walking"], B * (204 + 12) + N * (136 + 36 + 12 * J)),
                 joint_reproj_rows=stats(us["joint_reproj_rows"], B * (204 + 12 + 16 * J) + N * (136 + 36 + 12 * J)),
                 min_reproj=stats(us["min_reproj"], B * (204 + 12 + 8 + 8) + N * (136 + 36 + 68 + 12)))
        spread = s["min_reproj"]["max_us"] - s["min_reproj"]["min_us"]
        rec["sizes"][f"{B}_rows"] = dict(
            N=N, H=H, median_joint_px=round(float(jerr.median()), 3), median_best_joint_px=round(float(wb.median()), 3),
            poses_with_joints_of_several_hypotheses=round(mixed, 4), **s, min_reproj_spread_us=round(spread, 1),
            walking_over_min_reproj=round(s["joint_reproj_walking"]["median_us"] / s["min_reproj"]["median_us"], 3),
            rows_over_min_reproj=round(s["joint_reproj_rows"]["median_us"] / s["min_reproj"]["median_us"], 3),
            walking_within_rule=bool(s["joint_reproj_walking"]["median_us"] <= s["min_reproj"]["median_us"] + spread))
        del x, T, uv, K, conf, last, wb, wi, rb, ri, jerr
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
