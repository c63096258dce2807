#!/usr/bin/env python3
"""Time the joint-wise temporal selection (zedo_joint_temporal_select) against the only route that reaches the same result without it: J
calls of zedo_temporal_select on one-joint slices (unary = junary[:, j], x = x[:, j:j+1, :], both made contiguous - J copies of each, 4
launches per call or more when the transition costs are chunked, and a table of H x H transition costs per frame and call).  ONE process,
seeded inputs, J = 17, H = 50, lambda = 100:

    50 750 rows   (1 015 frames, BASELINE configs[2])            as 29 clips of 35 frames and as ONE clip of 1 015 frames
    3 544 000 rows (70 880 frames, configs[3]'s per-GPU shard)   as 2 026 clips of 35 frames (the last one of 5)

The sliced route has no translation argument, so the comparison runs WITHOUT T (d_T = NULL), where the two routes return the same bits -
that is checked on every point and recorded (bit_identical).  The call WITH T, the one the driver makes, is timed beside them: it reads
12 more bytes per (frame, hypothesis).

Method: after a warm-up of three calls of each route they ALTERNATE --reps times (default 25, at least 20) in the same process; each call
is timed with device events on the launch stream around the whole call (binding, output and workspace allocation from torch's cache, and
for the sliced route the 2 J slice copies included - they are part of what that route costs).  Recorded per point: median / min / max in
microseconds of the three, the ratio of the medians, and the workspace each route needs.  The rule for a new call: its median must not
exceed the sliced route's at any point (native_not_slower).  One workgroup walks one (clip, joint): the single 1 015-frame clip is serial
in time on J = 17 compute units, and is reported as that.

This measures speed only.  Whether joint-wise temporal paths lower the error against ground truth on real video is not measured here or
anywhere in this repository (random-init weights and synthetic poses cannot tell).

    python tools/joint_temporal_timing.py [--reps 25] [--out profiles/joint_temporal.json]   (GPU box only)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

J, H, CLIP, LAM = 17, 50, 35, 100.0
POINTS = (("50750_rows_clips_of_35", 1015, CLIP), ("50750_rows_one_clip", 1015, 1015), ("3544000_rows_clips_of_35", 70880, CLIP))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(us):
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(float(min(us)), 1), max_us=round(float(max(us)), 1), reps=len(us))


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import zedo_hip as zh
    from joint_reproj_timing import inputs
    dev = torch.device("cuda")
    rec = dict(tool="tools/joint_temporal_timing.py", J=J, H=H, smooth=LAM, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="three warm-up calls of each route, then the routes alternate in one process; device events on the launch stream around "
                      "the whole call (binding, allocations from torch's cache, the sliced route's 2 J slice copies); microseconds",
               accuracy_on_real_data="not measured", points={})
    data = {}
    for name, N, clip in POINTS:
        if N not in data:
            data.clear()
            torch.cuda.empty_cache()
            x, T, uv, K, _ = inputs(N, H, dev)
            data[N] = (x, T, zh.joint_reproj(x, T, uv, K, return_rows=True)[2])
            del uv, K
        x, T, jerr = data[N]
        seq = list(range(0, N, clip)) + [N]
        sd = torch.tensor(seq, dtype=torch.int32, device=dev)

        def native():
            return zh.joint_temporal_select(jerr, x, None, sd, N=N, lam=LAM)

        def native_T():
            return zh.joint_temporal_select(jerr, x, T, sd, N=N, lam=LAM)

        def sliced():
            out = [zh.temporal_select(jerr[:, j].contiguous(), x[:, j:j + 1, :].contiguous(), sd, N=N, lam=LAM) for j in range(J)]
            return torch.stack([p for p, _ in out], 1), torch.stack([c for _, c in out], 1)

        for _ in range(3):
            rn, rt, rs = native(), native_T(), sliced()
        torch.cuda.synchronize()
        us_n, us_t, us_s = [], [], []
        for _ in range(a.reps):
            t, rn = timed(native)
            us_n.append(t)
            t, rs = timed(sliced)
            us_s.append(t)
            t, rt = timed(native_T)
            us_t.append(t)
        sn, ss, st = stats(us_n), stats(us_s), stats(us_t)
        per_frame = jerr.reshape(H, N, J).argmin(0)
        point = dict(N=N, H=H, J=J, clips=len(seq) - 1, longest_clip=min(clip, N), native_without_T=sn, sliced_calls=ss, native_with_T=st,
                     sliced_over_native=round(ss["median_us"] / sn["median_us"], 2), native_not_slower=bool(sn["median_us"] <= ss["median_us"]),
                     bit_identical=same(rn, rs),
                     share_of_frame_joints_where_the_path_with_T_leaves_the_per_frame_arg_min=round(float((rt[0] != per_frame).double().mean()), 4),
                     workspace_bytes_native=int(zh._lib.zedo_joint_temporal_workspace_bytes(N, H, J)),
                     workspace_bytes_one_sliced_call=int(zh._lib.zedo_temporal_workspace_bytes(N, H, 0)),
                     transition_table_bytes_the_sliced_route_writes=int(J) * (N - 1) * H * H * 8)
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del rn, rt, rs
    rec["native_not_slower_everywhere"] = all(p["native_not_slower"] for p in rec["points"].values())
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
