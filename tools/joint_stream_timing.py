#!/usr/bin/env python3
"""Time the joint-wise selection on live streams (zedo_joint_stream_push) at J = 17, H = 50, lambda = 100, WITH T.  ONE process, seeded
inputs, the unaries are zedo_joint_reproj's distances.  H = 50 is the only hypothesis count timed: it is the one the package runs at, and
the recurrence's cost per frame is the offline call's, which tools/joint_temporal_timing.py covers.

  (1) whole clips, lag = L - 1 and a flush: ONE clip of 1 015 frames (S = 1) and 29 clips of 35 frames (S = 29), each in one push.  The
      yardstick is zedo_joint_temporal_select on the same tensors, which returns the same bits (checked, bit_identical).  The forward
      recurrence is the same; the difference is the emission - one wave per (frame, joint) walking up to L - 1 back pointers - against the
      offline backward pass.
  (2) the live shape: S = 16 streams, F = 1 frame per push, lag = 30, 300 pushes in a row; microseconds per push.  Beside it the route a
      user has without the call: zedo_joint_temporal_select on each stream's last lag + F frames (16 clips in one call) for every push,
      on a window assembled beforehand (its assembly is not timed).  THAT ROUTE COMPUTES A DIFFERENT ANSWER: it forgets everything before
      the window.  The figure says what the state saves, not that the two are interchangeable.
  (3) the same with F = 8.

Method: after a warm-up of three rounds the routes ALTERNATE --reps times (default 25, at least 20) in the same process; device events on
the launch stream around the whole call, or around the 300 pushes of a round (binding and output allocation from torch's cache included).
Recorded: median / min / max in microseconds and the ratio of the medians.  No ratio is required of the new call.

This measures speed only.  The choice of lag is untuned, and whether a fixed-lag path is closer to ground truth than the per-frame choice
on real video is not measured here or anywhere in this repository.

    python tools/joint_stream_timing.py [--reps 25] [--out profiles/joint_stream.json]   (GPU box only)
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

J, H, LAM = 17, 50, 100.0
WHOLE = (("one_clip_of_1015", 1, 1015), ("29_clips_of_35", 29, 35))
LIVE = (("live_S16_F1_lag30", 16, 1, 30, 300), ("live_S16_F8_lag30", 16, 8, 30, 300))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(us):
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(float(min(us)), 1), max_us=round(float(max(us)), 1), reps=len(us))


def rows_of(N, frames, dev):
    """frames [S,F] (a tensor of frame indices of a problem of N frames) -> the rows (h, n) of the chunk, h-major with n = s F + f."""
    return (torch.arange(H, device=dev)[:, None, None] * N + frames[None]).reshape(-1)


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
    rec = dict(tool="tools/joint_stream_timing.py", J=J, H=H, smooth=LAM, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="three warm-up rounds, then the routes alternate in one process; device events on the launch stream around the whole "
                      "call or the pushes of a round (binding, allocations from torch's cache); microseconds",
               accuracy_on_real_data="not measured", lag="untuned", points={})

    # (1) whole clips
    N = 1015
    x, T, uv, K, _ = inputs(N, H, dev)
    jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
    for name, S, L in WHOLE:
        sd = torch.tensor(list(range(0, N, L)) + [N], dtype=torch.int32, device=dev)
        js = zh.JointStream(S, H, J, L - 1, L, lam=LAM)
        fl = torch.ones(S, dtype=torch.int32, device=dev)

        def offline():
            return zh.joint_temporal_select(jerr, x, T, sd, N=N, lam=LAM)

        def stream():
            return js.push(jerr, x, T, flush=fl)

        for _ in range(3):
            ro, rs = offline(), stream()
        torch.cuda.synchronize()
        us_o, us_s = [], []
        for _ in range(a.reps):
            t, ro = timed(offline)
            us_o.append(t)
            t, rs = timed(stream)
            us_s.append(t)
        so, ss = stats(us_o), stats(us_s)
        same = bool(torch.equal(rs[2][:, :L].reshape(N, J), ro[0])
                    and torch.equal(rs[3][:, :L].reshape(N, J).view(torch.int64), ro[1].view(torch.int64)) and rs[1].tolist() == [L] * S)
        point = dict(S=S, F=L, lag=L - 1, offline_call=so, stream_push=ss, stream_over_offline=round(ss["median_us"] / so["median_us"], 3),
                     offline_spread=round(so["max_us"] / so["min_us"], 3), bit_identical=same, state_bytes=js.state_bytes,
                     offline_workspace_bytes=int(zh._lib.zedo_joint_temporal_workspace_bytes(N, H, J)))
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
    del x, T, uv, K, jerr

    # (2), (3) live: every stream walks its own run of `pushes * F` consecutive frames of one problem
    for name, S, F, lag, pushes in LIVE:
        per = pushes * F
        N = S * per
        torch.cuda.empty_cache()
        x, T, uv, K, _ = inputs(N, H, dev)
        jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
        base = torch.arange(S, device=dev)[:, None] * per
        chunks = []
        for i in range(pushes):
            r = rows_of(N, base + i * F + torch.arange(F, device=dev)[None], dev)
            chunks.append((jerr[r].contiguous(), x[r].contiguous(), T[r].contiguous()))
        W = lag + F                                                  # the window of the route without state, assembled once
        r = rows_of(N, base + torch.arange(W, device=dev)[None], dev)
        wu, wx, wT = jerr[r].contiguous(), x[r].contiguous(), T[r].contiguous()
        wsd = torch.arange(0, S * W + 1, W, dtype=torch.int32, device=dev)
        js = zh.JointStream(S, H, J, lag, F, lam=LAM)

        def stream_round():
            js.reset()
            for u, xx, TT in chunks:
                out = js.push(u, xx, TT)
            return out

        def window_round():
            for _ in range(pushes):
                out = zh.joint_temporal_select(wu, wx, wT, wsd, N=S * W, lam=LAM)
            return out

        for _ in range(3):
            stream_round(), window_round()
        torch.cuda.synchronize()
        us_s, us_w = [], []
        for _ in range(a.reps):
            t, _ = timed(stream_round)
            us_s.append(t / pushes)
            t, _ = timed(window_round)
            us_w.append(t / pushes)
        ss, sw = stats(us_s), stats(us_w)
        point = dict(S=S, F=F, lag=lag, pushes_per_round=pushes, stream_push_per_push=ss, offline_on_the_last_lag_plus_F_frames_per_push=sw,
                     window_over_stream=round(sw["median_us"] / ss["median_us"], 2),
                     the_window_route_computes_a_different_answer="it has no history before the window; its window is assembled beforehand, untimed",
                     frames_per_second_per_stream_at_the_median=round(F / (ss["median_us"] * 1e-6), 0), state_bytes=js.state_bytes)
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del x, T, uv, K, jerr, chunks, wu, wx, wT
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
