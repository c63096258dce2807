#!/usr/bin/env python3
"""Time the joint-wise fusion on live streams (zedo_joint_stream_marginal_push) at J = 17, H = 50, lambda = 100, tau = 1, WITH T.  ONE
process, seeded inputs, the unaries are zedo_joint_reproj's distances.  H = 50 is the only hypothesis count timed: it is the one the
package runs at.

  (1) whole clips, lag = L - 1 and a flush, each in one push: ONE clip of 1 015 frames, ONE clip of 127 frames, and 29 clips of 35 frames
      (S = 29).  The yardstick is zedo_joint_marginal on the same tensors, which returns the same bits (asserted before anything is
      timed).  The forward recurrence is the same; the emission is one backward walk per (stream, joint) - the frames of a flushed clip
      share their horizon - beside L J - J workgroups that return at once.
      DERIVED CONDITION (asserted): (push time at 1 015) / (push time at 127) <= 2 x the same quotient of the offline call in this
      process.  The shared-horizon walk is linear in L like the offline pass; a walk per emitted frame would be quadratic and make the
      quotient about 4 times larger (1 015 / 127 = 8, half of it on average).  Both quotients are recorded.
  (2) the live shape: S = 16 streams, F = 1 frame per push, lag = 30, 300 pushes in a row; microseconds per push, against
      (a) zedo_joint_stream_push at the same shape - the price of the soft answer: the hard emission reads back pointers where this one
          runs a recurrence of lag frames per emitted frame, so a multiple of the order of lag is expected of the emission;
      (b) zedo_joint_marginal on each stream's last lag + F frames (16 clips in one call) for every push, on a window assembled
          beforehand (its assembly is not timed).  THAT ROUTE COMPUTES A DIFFERENT, HISTORY-FREE ANSWER: it forgets everything before
          the window.
  (3) the same with F = 8.

Method: after a warm-up of three rounds the routes ALTERNATE --reps times (default 25, at least 20) in the same process; device events on
the launch stream around the whole call, or around the 300 pushes of a round (binding and output allocation from torch's cache included).
Recorded: median / min / max in microseconds and the ratios of the medians.  No ratio is required of the new call except the derived
condition of (1).

This measures speed only.  lag, lambda and tau are untuned, and whether a fixed-lag fused pose is closer to ground truth than a selected
one on real video is not measured here or anywhere in this repository.

    python tools/joint_stream_marginal_timing.py [--reps 25] [--out profiles/joint_stream_marginal.json]   (GPU box only)
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

J, H, LAM, TAU = 17, 50, 100.0, 1.0
WHOLE = (("one_clip_of_1015", 1015, 1, 1015), ("one_clip_of_127", 127, 1, 127), ("29_clips_of_35", 1015, 29, 35))
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


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def rows_of(N, frames, dev):
    """frames [S,F] (a tensor of frame indices of a problem of N frames) -> the rows (h, n) of the chunk, h-major with n = s F + f."""
    return (torch.arange(H, device=dev)[:, None, None] * N + frames[None]).reshape(-1)


def alternate(routes, reps, per=1):
    """routes: callables; three warm-up rounds, then they alternate reps times -> [stats], microseconds / per."""
    for _ in range(3):
        for f in routes:
            f()
    torch.cuda.synchronize()
    us = [[] for _ in routes]
    for _ in range(reps):
        for i, f in enumerate(routes):
            us[i].append(timed(f)[0] / per)
    return [stats(u) for u in us]


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
    rec = dict(tool="tools/joint_stream_marginal_timing.py", J=J, H=H, smooth=LAM, temperature=TAU, reps=a.reps,
               device=torch.cuda.get_device_name(0), hypothesis_counts_timed="H = 50 only",
               method="three warm-up rounds, then the routes alternate in one process; device events on the launch stream around the whole "
                      "call or the pushes of a round (binding, allocations from torch's cache); microseconds",
               accuracy_on_real_data="not measured", lag="untuned", points={})

    # (1) whole clips
    for name, N, S, L in WHOLE:
        x, T, uv, K, _ = inputs(N, H, dev)
        jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
        sd = torch.tensor(list(range(0, N, L)) + [N], dtype=torch.int32, device=dev)
        js = zh.JointMarginalStream(S, H, J, L - 1, L, lam=LAM, tau=TAU)
        fl = torch.ones(S, dtype=torch.int32, device=dev)
        if S > 1:                                                    # rows (h, n) with n = s L + f: the problem's own order
            assert N == S * L
        offline = lambda: zh.joint_marginal(jerr, x, T, sd, N=N, lam=LAM, tau=TAU, return_weights=True)
        stream = lambda: js.push(jerr, x, T, flush=fl, return_weights=True)
        ro, rs = offline(), stream()
        torch.cuda.synchronize()
        assert rs[1].tolist() == [L] * S
        for o, s in zip(ro, rs[2:]):                                 # equality before anything is timed
            assert torch.equal(bits(s[:, :L].reshape(o.shape)), bits(o)), name
        so, ss = alternate((offline, stream), a.reps)
        point = dict(S=S, F=L, lag=L - 1, offline_call=so, stream_push=ss, stream_over_offline=round(ss["median_us"] / so["median_us"], 3),
                     offline_spread=round(so["max_us"] / so["min_us"], 3), bit_identical=True, state_bytes=js.state_bytes,
                     offline_workspace_bytes=int(zh._lib.zedo_joint_marginal_workspace_bytes(N, H, J)))
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del x, T, uv, K, jerr, js
    p_long, p_short = rec["points"]["one_clip_of_1015"], rec["points"]["one_clip_of_127"]
    q_push = p_long["stream_push"]["median_us"] / p_short["stream_push"]["median_us"]
    q_off = p_long["offline_call"]["median_us"] / p_short["offline_call"]["median_us"]
    rec["linear_in_L"] = dict(push_1015_over_127=round(q_push, 3), offline_1015_over_127=round(q_off, 3),
                              condition="push quotient <= 2 x offline quotient", holds=bool(q_push <= 2.0 * q_off))
    print(json.dumps(dict(linear_in_L=rec["linear_in_L"])), flush=True)

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
        jm = zh.JointMarginalStream(S, H, J, lag, F, lam=LAM, tau=TAU)
        jh = zh.JointStream(S, H, J, lag, F, lam=LAM)

        def soft_round():
            jm.reset()
            for u, xx, TT in chunks:
                out = jm.push(u, xx, TT)
            return out

        def hard_round():
            jh.reset()
            for u, xx, TT in chunks:
                out = jh.push(u, xx, TT)
            return out

        def window_round():
            for _ in range(pushes):
                out = zh.joint_marginal(wu, wx, wT, wsd, N=S * W, lam=LAM, tau=TAU)
            return out

        ss, sh, sw = alternate((soft_round, hard_round, window_round), a.reps, pushes)
        point = dict(S=S, F=F, lag=lag, pushes_per_round=pushes, stream_marginal_push_per_push=ss, stream_push_per_push=sh,
                     offline_fusion_on_the_last_lag_plus_F_frames_per_push=sw,
                     soft_over_hard=round(ss["median_us"] / sh["median_us"], 2), window_over_soft=round(sw["median_us"] / ss["median_us"], 2),
                     the_window_route_computes_a_different_answer="it has no history before the window; its window is assembled beforehand, untimed",
                     frames_per_second_per_stream_at_the_median=round(F / (ss["median_us"] * 1e-6), 0), state_bytes=jm.state_bytes,
                     hard_state_bytes=jh.state_bytes)
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del x, T, uv, K, jerr, chunks, wu, wx, wT
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    assert rec["linear_in_L"]["holds"], rec["linear_in_L"]


if __name__ == "__main__":
    main()
