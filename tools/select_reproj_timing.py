#!/usr/bin/env python3
"""Time the label-free selection (zedo_min_reproj) against zedo_min_mpjpe(procrustes=0) on the SAME rows, in ONE process on seeded
inputs, at 1 015 x 50 = 50 750 rows (BASELINE configs[2]) and 70 880 x 50 = 3 544 000 rows (configs[3]'s per-GPU shard, the shard
size of tests/test_large_shards_gpu.py), J = 17, confidences given.

zedo_min_mpjpe reads the same pose bytes plus a LARGER per-pose operand (408 bytes of fp64 ground truth against 240 bytes of
detections, intrinsics and confidences) and does less arithmetic per joint (one fp64 sqrt against two divides and a sqrt); at
3 544 000 rows it runs a pose-major kernel that zedo_min_reproj does not have.

After a warm-up of both calls they ALTERNATE --reps times (default 25, at least 20); each call is timed with device events around
it on the launch stream (binding included: three output allocations from torch's cache and one ctypes call, the same for both).
Reported per size: median / min / max of each call in microseconds, the algorithmic bytes of each (every operand addressed,
counted once per launch that addresses it) and the GB/s they imply at the median, and the adoption rule of DESIGN.md 8.4:

    not slower  <=>  median(min_reproj) <= median(min_mpjpe) + (max - min of min_mpjpe in this run)

    python tools/select_reproj_timing.py [--reps 25] [--out profiles/select_reproj.json]   (GPU box only)
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


def inputs(N, H, dev):
    """Rows (h, n) = the pose's root-relative ground truth + 8 cm of seeded noise, T = the pose's root + 5 cm of noise - like a
    finished optimisation; the dataset's detections, intrinsics and confidences; centred ground truth in fp64 for zedo_min_mpjpe."""
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
    return x.contiguous(), T.contiguous(), t(d["db_2d"][:, :, :2]), t(d["camera_param"]), t(d["db_2d"][:, :, 2]), gt


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
    rec = dict(tool="tools/select_reproj_timing.py", J=17, reps=a.reps, device=torch.cuda.get_device_name(0), sizes={})
    for N, H in SIZES:
        B = N * H
        x, T, uv, K, conf, gt = inputs(N, H, dev)
        mpjpe = lambda: zh.min_mpjpe(x, gt, N, False)
        reproj = lambda: zh.min_reproj(x, T, uv, K, conf)
        for _ in range(3):                                           # warm-up of both calls: code objects, allocator
            mpjpe()
            reproj()
        torch.cuda.synchronize()
        tm, tr = [], []
        for _ in range(a.reps):
            us, rm = timed(mpjpe)
            tm.append(us)
            us, rr = timed(reproj)
            tr.append(us)
        err = rr[0]
        assert bool(torch.isfinite(err).all()) and bool((rr[2] >= 0).all()), f"{B} rows: a row error is not finite"
        # bytes: the rows (x 204, T 12), err written by the row kernel and read by the arg-min (8 + 8), the per-pose operands, best / idx
        sm = stats(tm, B * (204 + 8 + 8) + N * (408 + 12))
        sr = stats(tr, B * (204 + 12 + 8 + 8) + N * (136 + 36 + 68 + 12))
        spread = sm["max_us"] - sm["min_us"]
        rec["sizes"][f"{B}_rows"] = dict(
            N=N, H=H, median_reproj_px=round(float(err.median()), 3),
            min_mpjpe=sm, min_reproj=sr, min_mpjpe_spread_us=round(spread, 1),
            reproj_over_mpjpe=round(sr["median_us"] / sm["median_us"], 3),
            not_slower=bool(sr["median_us"] <= sm["median_us"] + spread))
        del x, T, uv, K, conf, gt, rm, rr, err
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
