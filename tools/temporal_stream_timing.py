#!/usr/bin/env python3
"""Time the pose-level selection on live streams (zedo_temporal_stream_push) at J = 17, H = 50, lambda = 100.  ONE process, seeded inputs,
the unaries are zedo_min_reproj's errors.  H = 50 IS THE ONLY HYPOTHESIS COUNT TIMED: it is the one the package runs at; the transition
costs grow with H^2 and nothing here says how the figures move with H.

  (1) whole clips, lag = L - 1 and a flush: ONE clip of 1 015 frames (S = 1) and 29 clips of 35 frames (S = 29), each in one push.  The
      yardstick is zedo_temporal_select on the same tensors, which returns the same bits (ASSERTED before anything is timed).  The forward
      work is the same - the same transition tiles, the same resident scan -; the difference is the emission - one wave per frame
      walking up to L - 1 back pointers - against the offline backward pass.  The ratio is printed beside the offline call's own
      max / min of the run: a ratio outside that spread needs an explanation, none is required.
  (2) the live shape: S = 16 streams, lag = 30, 300 pushes in a row of F = 1 and of F = 8 frames; microseconds per push, beside
      zedo_joint_stream_push (J chains per stream, WITH T) on the same frames in the same run, and beside the route a user has without
      the call: zedo_temporal_select on each stream's last lag + F frames (16 clips in one call) for every push, on a window assembled
      beforehand (its assembly is not timed).  THE WINDOW ROUTE COMPUTES A DIFFERENT ANSWER: it forgets everything before the window.
  (3) Pipeline.push_live_joints at the same two shapes: both unaries, both streams, the window of pending frames and zedo_joint_compose.
      The problem of load() is the same S F poses at every push: the cost does not depend on the values.
  (4) the one derived condition - a steady-state push does O(F J H^2 + F lag) work whatever the clip holds: seven runs of 1 000 pushes of
      F = 1 (S = 16, lag = 30), a device event between any two pushes; the median of pushes 900 - 999 (over the seven runs) must lie
      inside the spread of the seven medians of pushes 100 - 199.  Recorded as steady_state.within_spread; the exit status is 1 if not.

Method: after a warm-up of three rounds the routes ALTERNATE --reps times (default 25, at least 20) in the same process; device events on
the launch stream around the whole call, or around the pushes of a round (binding and output allocation from torch's cache included).
Recorded: median / min / max in microseconds.  No ratio is required of the new call.

This measures speed only.  The choice of lag and lambda is UNTUNED, and whether a fixed-lag path is closer to ground truth than the
per-frame choice on real video is UNMEASURED here and anywhere in this repository.

    python tools/temporal_stream_timing.py [--reps 25] [--out profiles/temporal_stream.json]   (GPU box only)
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
STEADY = dict(S=16, F=1, lag=30, pushes=1000, runs=7, early=(100, 200), late=(900, 1000))


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


def alternate(reps, *fns):
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            us[k].append(timed(fn)[0])
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import zedo_hip as zh
    from joint_reproj_timing import inputs
    from lib.dataset import synthetic as syn
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    dev = torch.device("cuda")
    rec = dict(tool="tools/temporal_stream_timing.py", J=J, H=H, only_H_timed=H, smooth=LAM, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="three warm-up rounds, then the routes alternate in one process; device events on the launch stream around the whole "
                      "call or the pushes of a round (binding, allocations from torch's cache); microseconds",
               accuracy_on_real_data="UNMEASURED", lag="UNTUNED", smooth_weight="UNTUNED", points={})

    # (1) whole clips
    N = 1015
    x, T, uv, K, conf = inputs(N, H, dev)
    err = zh.min_reproj(x, T, uv, K, conf, N, 0)[0]
    for name, S, L in WHOLE:
        sd = torch.tensor(list(range(0, N, L)) + [N], dtype=torch.int32, device=dev)
        ts = zh.TemporalStream(S, H, J, L - 1, L, lam=LAM)
        fl = torch.ones(S, dtype=torch.int32, device=dev)

        def offline():
            return zh.temporal_select(err, x, sd, N=N, lam=LAM)

        def stream():
            return ts.push(err, x, flush=fl)

        ro, rs = offline(), stream()
        torch.cuda.synchronize()
        assert torch.equal(rs[2][:, :L].reshape(N), ro[0]) and rs[1].tolist() == [L] * S
        assert torch.equal(rs[3][:, :L].reshape(N).view(torch.int64), ro[1].view(torch.int64)), "the stream must return the offline bits"
        us_o, us_s = alternate(a.reps, offline, stream)
        so, ss = stats(us_o), stats(us_s)
        point = dict(S=S, F=L, lag=L - 1, offline_call=so, stream_push=ss, stream_over_offline=round(ss["median_us"] / so["median_us"], 3),
                     offline_spread_max_over_min=round(so["max_us"] / so["min_us"], 3), bit_identical=True, state_bytes=ts.state_bytes,
                     offline_workspace_bytes=int(zh._lib.zedo_temporal_workspace_bytes(N, H, 0)))
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del ts
    del x, T, uv, K, conf, err

    # (2), (3) live: every stream walks its own run of `pushes * F` consecutive frames of one problem
    weights = zh.Weights(syn.make_weights(seed=0))
    for name, S, F, lag, pushes in LIVE:
        per = pushes * F
        N = S * per
        torch.cuda.empty_cache()
        x, T, uv, K, conf = inputs(N, H, dev)
        err = zh.min_reproj(x, T, uv, K, conf, N, 0)[0]
        jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
        base = torch.arange(S, device=dev)[:, None] * per
        chunks = []
        for i in range(pushes):
            r = rows_of(N, base + i * F + torch.arange(F, device=dev)[None], dev)
            chunks.append((err[r].contiguous(), jerr[r].contiguous(), x[r].contiguous(), T[r].contiguous()))
        W = lag + F                                                  # the window of the route without state, assembled once
        r = rows_of(N, base + torch.arange(W, device=dev)[None], dev)
        wu, wx = err[r].contiguous(), x[r].contiguous()
        wsd = torch.arange(0, S * W + 1, W, dtype=torch.int32, device=dev)
        ts = zh.TemporalStream(S, H, J, lag, F, lam=LAM)
        js = zh.JointStream(S, H, J, lag, F, lam=LAM)
        first = (base[:, :1] + torch.arange(F, device=dev)[None]).reshape(-1)                 # the poses of the first chunk
        d2 = torch.cat([uv[first], conf[first][:, :, None]], -1)
        pipe = Pipeline(weights, ZeDOConfig.h36m(OIL_iterations=10)).load(torch.zeros((H, J, 3)), d2, K[first])
        lj = pipe.open_live_joints(S, lag, F, lam=LAM)

        def stream_round():
            ts.reset()
            for u, _, xx, _ in chunks:
                out = ts.push(u, xx)
            return out

        def joint_round():
            js.reset()
            for _, ju, xx, TT in chunks:
                out = js.push(ju, xx, TT)
            return out

        def window_round():
            for _ in range(pushes):
                out = zh.temporal_select(wu, wx, wsd, N=S * W, lam=LAM)
            return out

        def live_round():
            lj.reset()
            for _, _, xx, TT in chunks:
                out = pipe.push_live_joints(lj, xx, TT)
            return out

        us = alternate(a.reps, stream_round, joint_round, window_round, live_round)
        ss, sj, sw, sl = (stats([t / pushes for t in u]) for u in us)
        point = dict(S=S, F=F, lag=lag, pushes_per_round=pushes, temporal_stream_push_per_push=ss, joint_stream_push_per_push=sj,
                     offline_on_the_last_lag_plus_F_frames_per_push=sw, push_live_joints_per_push=sl,
                     window_over_stream=round(sw["median_us"] / ss["median_us"], 2),
                     pose_stream_over_joint_stream=round(ss["median_us"] / sj["median_us"], 2),
                     the_window_route_computes_a_different_answer="it has no history before the window; its window is assembled beforehand, untimed",
                     push_live_joints_includes="zedo_min_reproj, zedo_joint_reproj, both pushes, the window of pending frames (torch), zedo_joint_compose",
                     frames_per_second_per_stream_at_the_median=round(F / (ss["median_us"] * 1e-6), 0), state_bytes=ts.state_bytes)
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del x, T, uv, K, conf, err, jerr, chunks, wu, wx, ts, js, lj, pipe

    # (4) steady state: the cost of a push does not grow with the clip
    S, F, lag, pushes = (STEADY[k] for k in ("S", "F", "lag", "pushes"))
    N = S * pushes
    torch.cuda.empty_cache()
    x, T, uv, K, conf = inputs(N, H, dev)
    err = zh.min_reproj(x, T, uv, K, conf, N, 0)[0]
    base = torch.arange(S, device=dev)[:, None] * pushes
    chunks = []
    for i in range(pushes):
        r = rows_of(N, base + i, dev)
        chunks.append((err[r].contiguous(), x[r].contiguous()))
    ts = zh.TemporalStream(S, H, J, lag, F, lam=LAM)
    early, late = [], []
    for run in range(STEADY["runs"] + 1):                            # the first run warms up and is not recorded
        ts.reset()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(pushes + 1)]
        ev[0].record()
        for i, (u, xx) in enumerate(chunks):
            ts.push(u, xx)
            ev[i + 1].record()
        torch.cuda.synchronize()
        us = np.array([ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(pushes)])
        if run:
            early.append(float(np.median(us[slice(*STEADY["early"])])))
            late.append(float(np.median(us[slice(*STEADY["late"])])))
    late_median = float(np.median(late))
    within = min(early) <= late_median <= max(early)
    rec["steady_state"] = dict(STEADY, medians_of_pushes_100_to_199_us=[round(v, 1) for v in early],
                               medians_of_pushes_900_to_999_us=[round(v, 1) for v in late], median_of_the_late_medians_us=round(late_median, 1),
                               within_spread=bool(within), events="one device event between any two pushes; host-bound pushes measure the host")
    print(json.dumps(dict(steady_state=rec["steady_state"])), flush=True)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if within else 1


if __name__ == "__main__":
    sys.exit(main())
