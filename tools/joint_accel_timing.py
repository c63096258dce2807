#!/usr/bin/env python3
"""Time the joint-wise selection with a second-order motion model (zedo_joint_accel_select) against two yardsticks: the first-order call
zedo_joint_temporal_select on the same inputs - H^2 transitions per (frame, joint) where this call has H^3, so a multiple of the order of
H is expected, not parity - and the same recurrence over pairs stated in plain torch (the clips of a point batched into one tensor, one
min over h'' per frame, the backward pass by gathers).  ONE process, seeded inputs, J = 17, H = 50, lambda_v = lambda_a = 100, with T:

    50 750 rows   (1 015 frames, BASELINE configs[2])            as 29 clips of 35 frames and as ONE clip of 1 015 frames
    3 544 000 rows (70 880 frames, configs[3]'s per-GPU shard)   as 2 026 clips of 35 frames (the last one of 5); back2 is 3.0 GB

The torch statement needs 8 H^3 J bytes of candidates per clip and frame: it runs at the first two points and NOT at the third (34 GB per
frame step unless the clips are chunked); that point compares the two native calls only.  The torch statement's paths are compared with
the call's on every point it runs at and recorded (paths_equal).

Method: after a warm-up of three calls of each route they ALTERNATE --reps times (default 25, at least 20) in the same process; each call
is timed with device events on the launch stream around the whole call (binding, output and workspace allocation from torch's cache).
Recorded per point: median / min / max in microseconds of every route, the ratios of the medians, and the workspace of both calls.  One
workgroup walks one (clip, joint): the single 1 015-frame clip is serial in time on J = 17 compute units, and is reported as that.

This measures speed only.  Whether second-order paths lower the error against ground truth on real video is not measured here or anywhere
in this repository (random-init weights and synthetic poses cannot tell).

    python tools/joint_accel_timing.py [--reps 25] [--out profiles/joint_accel.json]   (GPU box only)
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

J, H, CLIP, LAM_V, LAM_A = 17, 50, 35, 100.0, 100.0
# (name, frames, frames per clip, run the torch statement)
POINTS = (("50750_rows_clips_of_35", 1015, CLIP, True), ("50750_rows_one_clip", 1015, 1015, True),
          ("3544000_rows_clips_of_35", 70880, CLIP, False))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(us):
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(float(min(us)), 1), max_us=round(float(max(us)), 1), reps=len(us))


def norm3(d):
    return torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def torch_statement(jerr, x, T, N, L, lam_v, lam_a):
    """The recurrence over pairs of include/zedo_hip.h for clips of exactly L >= 3 frames without dead entries, all clips and joints at
    once -> path [N,J] int32."""
    C = N // L
    X = (x.double() + T.double()[:, None, :]).view(H, C, L, J, 3).permute(1, 3, 2, 0, 4)      # [C,J,L,H,3]
    u = jerr.view(H, C, L, J).permute(1, 3, 2, 0)                                             # [C,J,L,H]
    motion = lambda n: norm3(X[:, :, n, None, :, :] - X[:, :, n - 1, :, None, :])             # [C,J,h',h]
    E = u[:, :, 0, :, None] + (u[:, :, 1, None, :] + lam_v * motion(1))
    back = []
    for n in range(2, L):
        g = X[:, :, n, None, :, :] - 2.0 * X[:, :, n - 1, :, None, :]                         # [C,J,h',h,3]
        a = norm3(g[:, :, None] + X[:, :, n - 2, :, None, None, :])                           # [C,J,h'',h',h]
        best, arg = (E[:, :, :, :, None] + lam_a * a).min(dim=2)
        back.append(arg)
        E = u[:, :, n, None, :] + (lam_v * motion(n) + best)
    q = E.flatten(2).argmin(-1)                                                               # [C,J]
    path = torch.empty((C, J, L), dtype=torch.int64, device=x.device)
    path[:, :, L - 1], path[:, :, L - 2] = q % H, q // H
    for n in range(L - 1, 1, -1):
        idx = path[:, :, n - 1] * H + path[:, :, n]
        path[:, :, n - 2] = back[n - 2].flatten(2).gather(2, idx[:, :, None])[:, :, 0]
    return path.permute(0, 2, 1).reshape(N, J).to(torch.int32)


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
    rec = dict(tool="tools/joint_accel_timing.py", J=J, H=H, smooth=LAM_V, accel=LAM_A, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="three warm-up calls of each route, then the routes alternate in one process; device events on the launch stream around "
                      "the whole call (binding, allocations from torch's cache); microseconds",
               accuracy_on_real_data="not measured", points={})
    data = {}
    for name, N, clip, with_torch in POINTS:
        if N not in data:
            data.clear()
            torch.cuda.empty_cache()
            x, T, uv, K, _ = inputs(N, H, dev)
            data[N] = (x, T, zh.joint_reproj(x, T, uv, K, return_rows=True)[2])
            del uv, K
        x, T, jerr = data[N]
        seq = list(range(0, N, clip)) + [N]
        sd = torch.tensor(seq, dtype=torch.int32, device=dev)
        accel = lambda: zh.joint_accel_select(jerr, x, T, sd, N=N, lam=LAM_V, accel=LAM_A)
        first = lambda: zh.joint_temporal_select(jerr, x, T, sd, N=N, lam=LAM_V)
        plain = (lambda: torch_statement(jerr, x, T, N, clip, LAM_V, LAM_A)) if with_torch else None
        for _ in range(3):
            ra, rf = accel(), first()
            rt = plain() if plain else None
        torch.cuda.synchronize()
        us_a, us_f, us_t = [], [], []
        for _ in range(a.reps):
            t, ra = timed(accel)
            us_a.append(t)
            t, rf = timed(first)
            us_f.append(t)
            if plain:
                t, rt = timed(plain)
                us_t.append(t)
        sa, sf = stats(us_a), stats(us_f)
        point = dict(N=N, H=H, J=J, clips=len(seq) - 1, longest_clip=min(clip, N), accel_call=sa, first_order_call=sf,
                     accel_over_first_order=round(sa["median_us"] / sf["median_us"], 1),
                     share_of_frame_joints_where_the_two_calls_differ=round(float((ra[0] != rf[0]).double().mean()), 4),
                     workspace_bytes_accel=int(zh._lib.zedo_joint_accel_workspace_bytes(N, H, J)),
                     workspace_bytes_first_order=int(zh._lib.zedo_joint_temporal_workspace_bytes(N, H, J)))
        if plain:
            st = stats(us_t)
            point.update(torch_statement=st, torch_over_accel=round(st["median_us"] / sa["median_us"], 1),
                         accel_not_slower_than_torch=bool(sa["median_us"] <= st["median_us"]), paths_equal=bool(torch.equal(ra[0], rt)))
        else:
            point.update(torch_statement="not run: 8 H^3 J bytes of candidates per clip and frame, 34 GB per frame step at this point")
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del ra, rf, rt
    rec["accel_not_slower_than_torch_everywhere_it_ran"] = all(p.get("accel_not_slower_than_torch", True) for p in rec["points"].values())
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
