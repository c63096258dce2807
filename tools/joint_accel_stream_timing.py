#!/usr/bin/env python3
"""Time the second-order joint-wise selection on live streams (zedo_joint_accel_stream_push) at J = 17, H = 50, (lambda_v, lambda_a) =
(30, 100), WITH T.  ONE process, seeded inputs, the unaries are zedo_joint_reproj's distances.  H = 50 is the only hypothesis count timed.

  (1) whole clips, lag = L - 1 and a flush: ONE clip of 1 015 frames (S = 1) and 29 clips of 35 frames (S = 29), each in one push, against
      zedo_joint_accel_select on the same tensors.  The paths are asserted equal BEFORE anything is timed.  The forward recurrence is the
      same H^3 walk; the stream adds one block reduction per frame and stores E, X and u of its last frame; its emission - one wave per
      (frame, joint) - stands against the offline backward and cost kernels.  The ratio is reported beside the offline call's own
      max / min of the same run.
  (2) the live shape: S = 16 streams, lag = 30, 300 pushes in a row, at F = 1 and F = 8; microseconds per push.  Beside it
      - zedo_joint_stream_push, the first-order chain, on the same inputs: the price of the second-order model;
      - zedo_joint_accel_select on each stream's last lag + F frames (16 clips in one call) for every push, on a window assembled
        beforehand (its assembly is not timed).  THAT ROUTE COMPUTES A DIFFERENT ANSWER: it forgets everything before the window.
  (3) the derived condition - a steady-state push does O(F H^3 + F lag) work whatever the clip already holds: 1 000 pushes of F = 1 in
      a row (the 300 chunks of (2), cycled), every push between its own pair of events; the medians of pushes 100-199 and 900-999 of every
      repetition, and the spread of the earlier window's medians across the repetitions.

Method: after a warm-up of three rounds the routes ALTERNATE --reps times (default 25, at least 20) in the same process; device events on
the launch stream around the whole call, or around the 300 pushes of a round (binding and output allocation from torch's cache included).
Recorded: median / min / max in microseconds and the ratios of the medians.  No ratio is required of the new call.  What bounds the scan
has not been profiled, for the offline call either.

This measures speed only.  lambda_v, lambda_a and the lag are untuned, and accuracy on real video is not measured here or anywhere in this
repository.

    python tools/joint_accel_stream_timing.py [--reps 25] [--out profiles/joint_accel_stream.json]   (GPU box only)
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

from joint_stream_timing import rows_of, stats, timed

J, H, LAM_V, LAM_A = 17, 50, 30.0, 100.0
WHOLE = (("one_clip_of_1015", 1, 1015), ("29_clips_of_35", 29, 35))
LIVE = (("live_S16_F1_lag30", 16, 1, 30, 300), ("live_S16_F8_lag30", 16, 8, 30, 300))
STEADY_PUSHES, STEADY_REPS = 1000, 7


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
    rec = dict(tool="tools/joint_accel_stream_timing.py", J=J, H=H, smooth=LAM_V, accel=LAM_A, reps=a.reps,
               device=torch.cuda.get_device_name(0),
               method="three warm-up rounds, then the routes alternate in one process; device events on the launch stream around the whole "
                      "call or the pushes of a round (binding, allocations from torch's cache); microseconds",
               accuracy_on_real_data="not measured", lag_and_weights="untuned", only_H_timed=H,
               what_bounds_the_scan="not profiled (for the offline call either)", points={})

    # (1) whole clips
    N = 1015
    x, T, uv, K, _ = inputs(N, H, dev)
    jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
    for name, S, L in WHOLE:
        sd = torch.tensor(list(range(0, N, L)) + [N], dtype=torch.int32, device=dev)
        js = zh.JointAccelStream(S, H, J, L - 1, L, lam=LAM_V, accel=LAM_A)
        fl = torch.ones(S, dtype=torch.int32, device=dev)

        def offline():
            return zh.joint_accel_select(jerr, x, T, sd, N=N, lam=LAM_V, accel=LAM_A)

        def stream():
            return js.push(jerr, x, T, flush=fl)

        ro, rs = offline(), stream()
        torch.cuda.synchronize()
        assert torch.equal(rs[2][:, :L].reshape(N, J), ro[0]) and rs[1].tolist() == [L] * S, name        # before anything is timed
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
        point = dict(S=S, F=L, lag=L - 1, offline_call=so, stream_push=ss, stream_over_offline=round(ss["median_us"] / so["median_us"], 3),
                     offline_max_over_min=round(so["max_us"] / so["min_us"], 3), paths_equal=True, state_bytes=js.state_bytes,
                     offline_workspace_bytes=int(zh._lib.zedo_joint_accel_workspace_bytes(N, H, J)))
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del js
    del x, T, uv, K, jerr

    # (2) live: every stream walks its own run of `pushes * F` consecutive frames of one problem
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
        ja = zh.JointAccelStream(S, H, J, lag, F, lam=LAM_V, accel=LAM_A)
        j1 = zh.JointStream(S, H, J, lag, F, lam=LAM_V)

        def rounds_of(st):
            def go():
                st.reset()
                for u, xx, TT in chunks:
                    out = st.push(u, xx, TT)
                return out
            return go

        def window_round():
            for _ in range(pushes):
                out = zh.joint_accel_select(wu, wx, wT, wsd, N=S * W, lam=LAM_V, accel=LAM_A)
            return out

        routes = dict(accel_stream_push=rounds_of(ja), first_order_stream_push=rounds_of(j1),
                      accel_select_on_the_last_lag_plus_F_frames=window_round)
        for _ in range(3):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                us[k].append(timed(fn)[0] / pushes)
        st = {k: stats(v) for k, v in us.items()}
        point = dict(S=S, F=F, lag=lag, pushes_per_round=pushes, per_push=st,
                     accel_stream_over_first_order_stream=round(st["accel_stream_push"]["median_us"] / st["first_order_stream_push"]["median_us"], 2),
                     window_over_accel_stream=round(st["accel_select_on_the_last_lag_plus_F_frames"]["median_us"] / st["accel_stream_push"]["median_us"], 2),
                     the_window_route_computes_a_different_answer="it has no history before the window; its window is assembled beforehand, untimed",
                     frames_per_second_per_stream_at_the_median=round(F / (st["accel_stream_push"]["median_us"] * 1e-6), 0),
                     state_bytes=ja.state_bytes)
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)

        # (3) on the F = 1 shape: 1 000 pushes in a row, each between its own events
        if F == 1:
            early, late = [], []
            for rep in range(STEADY_REPS + 1):
                ja.reset()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(STEADY_PUSHES + 1)]
                ev[0].record()
                for i in range(STEADY_PUSHES):
                    ja.push(*chunks[i % pushes])
                    ev[i + 1].record()
                torch.cuda.synchronize()
                if rep == 0:
                    continue                                         # warm-up
                t = np.array([ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(STEADY_PUSHES)])
                early.append(float(np.median(t[100:200])))
                late.append(float(np.median(t[900:1000])))
            point = dict(S=S, F=F, lag=lag, pushes=STEADY_PUSHES, reps=STEADY_REPS,
                         median_us_of_pushes_100_199=[round(v, 1) for v in early], median_us_of_pushes_900_999=[round(v, 1) for v in late],
                         median_of_medians_early=round(float(np.median(early)), 1), median_of_medians_late=round(float(np.median(late)), 1),
                         spread_of_the_early_medians=round(max(early) - min(early), 1),
                         late_minus_early=round(float(np.median(late)) - float(np.median(early)), 1))
            rec["points"]["steady_state_S16_F1_lag30"] = point
            print(json.dumps({"steady_state_S16_F1_lag30": point}), flush=True)
        del x, T, uv, K, jerr, chunks, wu, wx, wT, ja, j1
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
