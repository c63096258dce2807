#!/usr/bin/env python3
"""Time the temporal selection (zedo_temporal_select) against a plain torch statement of the same recurrence on the GPU, in ONE process on
seeded inputs, at 1 015 x 50 = 50 750 rows (BASELINE configs[2]) and 70 880 x 50 = 3 544 000 rows (configs[3]'s per-GPU shard), J = 17,
each cut into clips of 35 frames (29 clips; 2 026 clips, the last one of 5 frames) and as ONE clip.

The torch route is what a user would write without this feature: the pairwise mean joint distances of consecutive frames in float64,
batched over chunks of frames; then a Python loop over the position inside a clip (all clips advance together: for clips of 35 the loop
has 35 iterations whatever their number, for one clip it has N), each iteration a broadcast add, a min over h' and two scatters; then the
same loop backwards.  The frame lists of every iteration are built before the clock starts.  The frames on which its path differs from the
native one are counted and recorded (expected: 0).

After a warm-up the two routes ALTERNATE --reps times (default 25, at least 20; the torch route of the single 70 880-frame clip takes
seconds per repetition: --torch_reps_long, default 5, is used there and recorded).  Each call is timed with device events on the launch
stream (binding included).  Recorded per point: median / min / max in microseconds of both routes and of zedo_min_reproj on the same rows,
and the native call's split between its kernels (torch.profiler device times of three calls; null if the profiler sees no kernels).
The rule for a new selection: the native median must not exceed the torch route's at any point (native_not_slower).

One workgroup walks one clip: the single 70 880-frame clip is serial in time on ONE compute unit, and is reported as that.
This measures speed only.  Whether a temporally consistent path lowers the error against ground truth on real video is not measured here
or anywhere in this repository (random-init weights and synthetic poses cannot tell).

    python tools/temporal_select_timing.py [--reps 25] [--out profiles/temporal_select.json]   (GPU box only)
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

SIZES = ((1015, 50), (70880, 50))
J, CLIP, LAM = 17, 35, 100.0
PAIR_CHUNK = 256                       # frames of pairwise differences the torch route holds at once ([chunk,H,H,J,3] float64: 261 MB)
# seconds per pass the README gives for these sizes (exact fp32, H = 50, S = 1000): the selection's cost is quoted as a share of it
README_PASS_S = {50750: 3.105}


def frame_lists(seq, dev):
    """Per position t inside a clip: the frames n = seq_start[s] + t of every clip long enough, and whether each is its clip's last."""
    a, b = np.asarray(seq[:-1]), np.asarray(seq[1:])
    out = []
    for t in range(int((b - a).max())):
        keep = a + t < b
        n = a[keep] + t
        out.append((torch.tensor(n, dtype=torch.int64, device=dev), torch.tensor(n + 1 == b[keep], device=dev)))
    return out


def torch_route(u, x4, lists, lam):
    """u [N,H] f64, x4 [H,N,J,3] f32 -> (path [N] i64, cost [N] f64).  No excluded rows or dead frames (the timing inputs have none)."""
    H, N = x4.shape[0], x4.shape[1]
    xd = x4.to(torch.float64)
    M = torch.empty((N, H, H), dtype=torch.float64, device=u.device)                     # M[n,h',h]
    for c0 in range(1, N, PAIR_CHUNK):
        c1 = min(N, c0 + PAIR_CHUNK)
        cur, prv = xd[:, c0:c1].permute(1, 0, 2, 3), xd[:, c0 - 1:c1 - 1].permute(1, 0, 2, 3)
        M[c0:c1] = (cur[:, None] - prv[:, :, None]).square().sum(-1).sqrt().mean(-1)
    D = torch.empty((N, H), dtype=torch.float64, device=u.device)
    back = torch.zeros((N, H), dtype=torch.int64, device=u.device)
    D[lists[0][0]] = u[lists[0][0]]
    for n, _ in lists[1:]:
        best, arg = (D[n - 1][:, :, None] + lam * M[n]).min(1)
        D[n] = u[n] + best
        back[n] = arg
    path = torch.zeros((N,), dtype=torch.int64, device=u.device)
    for n, last in reversed(lists):
        nxt = torch.where(last, n, n + 1).clamp_(max=N - 1)
        path[n] = torch.where(last, D[n].argmin(1), back[nxt].gather(1, path[nxt][:, None])[:, 0])
    return path, D.gather(1, path[:, None])[:, 0]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(us):
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(float(min(us)), 1), max_us=round(float(max(us)), 1), reps=len(us))


def kernel_split(fn, calls=3):
    """Device time per kernel of the native call (microseconds per call), by the kernel's name."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for key in ("temporal_dead", "temporal_transition", "temporal_scan", "temporal_backtrack"):
                if key in ev.name:
                    dt = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0) or getattr(ev, "device_time", 0)
                    out[key] = out.get(key, 0.0) + float(dt) / calls
        return {k: round(v, 1) for k, v in out.items()} or None
    except Exception as e:          # the profiler is a convenience of this tool, not of the measurement
        return dict(error=repr(e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--torch_reps_long", type=int, default=5, help="repetitions of the torch route where one takes seconds (one 70 880-frame clip)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import zedo_hip as zh
    from joint_reproj_timing import inputs
    dev = torch.device("cuda")
    rec = dict(tool="tools/temporal_select_timing.py", J=J, clip=CLIP, smooth=LAM, reps=a.reps, device=torch.cuda.get_device_name(0),
               accuracy_on_real_data="not measured", points={})
    for N, H in SIZES:
        B = N * H
        x, T, uv, K, conf = inputs(N, H, dev)
        for _ in range(3):
            err = zh.min_reproj(x, T, uv, K, conf)[0]
        us_reproj = [timed(lambda: zh.min_reproj(x, T, uv, K, conf))[0] for _ in range(a.reps)]
        u2 = err.reshape(H, N).t().contiguous()
        x4 = x.reshape(H, N, J, 3)
        for name, seq in ((f"clips_of_{CLIP}", list(range(0, N, CLIP)) + [N]), ("one_clip", [0, N])):
            sd = torch.tensor(seq, dtype=torch.int32, device=dev)
            lists = frame_lists(seq, dev)
            native = lambda: zh.temporal_select(err, x, sd, N=N, lam=LAM)
            torch_fn = lambda: torch_route(u2, x4, lists, LAM)
            long_torch = len(lists) > 5000
            for _ in range(3):
                native()
            tp, tc = torch_fn()
            torch.cuda.synchronize()
            us_n, us_t = [], []
            t_reps = a.torch_reps_long if long_torch else a.reps
            for i in range(a.reps):
                t, (p, c) = timed(native)
                us_n.append(t)
                if i < t_reps:
                    t, (tp, tc) = timed(torch_fn)
                    us_t.append(t)
            differ = int((p.to(torch.int64) != tp).sum())               # (torch sums the joints in its own order: a near tie may fall the other way)
            rel = float(((c - tc).abs() / tc).max())
            sn, st = stats(us_n), stats(us_t)
            point = dict(N=N, H=H, clips=len(seq) - 1, longest_clip=len(lists), native=sn, torch=st,
                         native_kernels_us=kernel_split(native), min_reproj_same_rows=stats(us_reproj),
                         torch_over_native=round(st["median_us"] / sn["median_us"], 2), native_not_slower=bool(sn["median_us"] <= st["median_us"]),
                         frames_where_the_routes_differ=differ, max_relative_cost_difference=rel, frames_where_path_leaves_the_per_frame_arg_min=round(float((p != u2.argmin(1)).double().mean()), 4),
                         workspace_bytes=int(zh._lib.zedo_temporal_workspace_bytes(N, H, 0)))
            if B in README_PASS_S:
                point["share_of_the_pass"] = round(sn["median_us"] * 1e-6 / README_PASS_S[B], 6)
            rec["points"][f"{B}_rows_{name}"] = point
            print(json.dumps({f"{B}_rows_{name}": point}), flush=True)
            del lists, tp, tc, p, c
        del x, T, uv, K, conf, err, u2, x4
        torch.cuda.empty_cache()
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
