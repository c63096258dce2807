#!/usr/bin/env python3
"""Time the one-pass selection (zedo_min_mpjpe_both) against the two zedo_min_mpjpe calls it replaces, in ONE process on
seeded inputs, at the two row counts bench.py's geometry_kernels uses: 1 015 x 50 = 50 750 rows (BASELINE configs[2]) and
70 880 x 50 = 3 544 000 rows (configs[3]'s per-GPU shard), J = 17.

After a warm-up of both forms they ALTERNATE --reps times (default 25, at least 20); each form is timed with device events
around its calls on the launch stream.  Reported per size: median / min / max of each form in microseconds, the algorithmic
bytes of each form (every operand addressed, counted once per launch that addresses it), whether the two forms' outputs are
bit-identical (asserted), and the adoption rule of Pipeline.select:

    not slower  <=>  median(one call) <= median(two calls) + (max - min of the two-call form in this run)

    python tools/selection_both_timing.py [--reps 25] [--out profiles/selection_both.json]   (GPU box only)
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


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def inputs(N, H, dev):
    """Rows (h, n) = the pose's ground truth + 8 cm of seeded noise, like a finished optimisation; centred ground truth in fp64."""
    from lib.dataset import synthetic as syn
    d = syn.make_poses(N, seed=11, dtype3d=np.float64)
    gt = torch.tensor(np.ascontiguousarray(d["db_3d"] - d["db_3d"][:, 0:1]), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + N)
    x = gt.to(torch.float32).repeat(H, 1, 1)
    x += 0.08 * torch.randn(x.shape, generator=g, dtype=torch.float32, device=dev)
    return x.contiguous(), gt


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(us):
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(float(min(us)), 1), max_us=round(float(max(us)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import zedo_hip as zh
    dev = torch.device("cuda")
    rec = dict(tool="tools/selection_both_timing.py", J=17, reps=a.reps, device=torch.cuda.get_device_name(0), sizes={})
    for N, H in SIZES:
        B = N * H
        x, gt = inputs(N, H, dev)
        two = lambda: (zh.min_mpjpe(x, gt, N, False), zh.min_mpjpe(x, gt, N, True))
        one = lambda: zh.min_mpjpe_both(x, gt, N)
        for _ in range(3):                                           # warm-up of both forms: code objects, allocator
            two()
            one()
        torch.cuda.synchronize()
        t2, t1 = [], []
        for _ in range(a.reps):
            us, r2 = timed(two)
            t2.append(us)
            us, r1 = timed(one)
            t1.append(us)
        same = all(torch.equal(bits(r1[k][s]), bits(r2[s][k])) for s in (0, 1) for k in (0, 1, 2))
        assert same, f"{B} rows: the one-call outputs are not the bits of the two calls"
        s2, s1 = stats(t2), stats(t1)
        spread = s2["max_us"] - s2["min_us"]
        rec["sizes"][f"{B}_rows"] = dict(
            N=N, H=H, nan_rows=int(torch.isnan(r1[0]).any(0).sum()),
            two_calls=dict(s2, algorithmic_bytes=2 * (B * (204 + 8 + 8) + N * (408 + 12))),
            one_call=dict(s1, algorithmic_bytes=B * (204 + 16 + 16) + N * (408 + 24)),
            bit_identical=bool(same), two_call_spread_us=round(spread, 1),
            one_over_two=round(s1["median_us"] / s2["median_us"], 3),
            not_slower=bool(s1["median_us"] <= s2["median_us"] + spread))
        del x, gt, r1, r2
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
