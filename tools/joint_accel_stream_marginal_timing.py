#!/usr/bin/env python3
"""Time the second-order joint-wise fusion on live streams (zedo_joint_accel_stream_marginal_push) at J = 17, H = 50, (lambda_v, lambda_a,
tau) = (30, 100, 1), WITH T.  ONE process, seeded inputs, the unaries are zedo_joint_reproj's distances.  H = 50 is the only hypothesis
count timed: it is the one the package runs at.

  whole   whole clips, lag = L - 1 and a flush, each in one push: ONE clip of 1 015 frames, ONE clip of 127 frames, and 29 clips of 35
          frames (S = 29), against zedo_joint_accel_marginal on the same tensors, which returns the same bits (asserted before anything is
          timed).  The ratio is reported beside the offline call's own max / min of the same run.
          DERIVED CONDITION (asserted): (median push time at 1 015) / (median push time at 127) <= the same quotient of the offline call
          with that call's own spread in it: its slowest repetition at 1 015 over its fastest at 127 - the largest value the yardstick's
          own quotient takes in this process.  The shared-horizon walk is linear in L like the offline pass; a walk per
          emitted frame would be quadratic and make the quotient about 4 times larger (1 015 / 127 = 8, half of it on average).
  live1   the live shape: S = 16 streams, F = 1 frame per push, lag = 30, 300 pushes in a row; microseconds per push, against
          (a) zedo_joint_accel_stream_push at the same shape - the price of the soft answer: the hard emission reads back one byte per
              frame of lag where this one runs a recurrence over pairs;
          (b) zedo_joint_stream_marginal_push at the same shape - the price of the second-order model;
          (c) zedo_joint_accel_marginal on each stream's last lag + F frames (16 clips in one call) for every push, on a window assembled
              beforehand (its assembly is not timed).  THAT ROUTE COMPUTES A DIFFERENT, HISTORY-FREE ANSWER: it forgets everything
              before the window.
  live8   the same with F = 8.
  steady  DERIVED CONDITION (asserted): a steady-state push does the same work whatever the clip already holds.  1 000 pushes of F = 1 in
          a row (the 300 chunks of live1, cycled), every push between its own pair of events; the medians of pushes 100-199 and 900-999 of
          each of seven repetitions; the medians of the two windows over the repetitions differ by no more than the spread (max - min) of
          the earlier window's medians.

Method: after a warm-up of three rounds (one for the live shapes) the routes ALTERNATE --reps times (default 25, at least 20; --live8-reps
for live8, whose round takes seconds) in the same process; device events on the launch stream around the whole call, or around the 300
pushes of a round (binding and output allocation from torch's cache included).  Recorded: median / min / max in microseconds and the
ratios of the medians.  No ratio is required of the new call except the two derived conditions.

This measures speed only.  lambda_v, lambda_a, tau and the lag are untuned, and accuracy on real video is not measured here or anywhere
in this repository.

    python tools/joint_accel_stream_marginal_timing.py [--only whole,live1,live8,steady] [--reps 25] [--out profiles/joint_accel_stream_marginal.json]
(GPU box only; --out is merged into: a run of some sections keeps the others' records)
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

from joint_stream_marginal_timing import bits, rows_of, stats, timed

J, H, LAM_V, LAM_A, TAU = 17, 50, 30.0, 100.0, 1.0
WHOLE = (("one_clip_of_1015", 1015, 1, 1015), ("one_clip_of_127", 127, 1, 127), ("29_clips_of_35", 1015, 29, 35))
LIVE = dict(live1=("live_S16_F1_lag30", 16, 1, 30, 300), live8=("live_S16_F8_lag30", 16, 8, 30, 300))
STEADY = dict(pushes=1000, early=(100, 200), late=(900, 1000), repetitions=7)


def live_inputs(zh, S, F, lag, pushes, dev):
    """-> (the chunks [(u, x, T)] of `pushes` pushes of F frames of S streams, the window (u, x, T, seq) of lag + F frames per stream)."""
    from joint_reproj_timing import inputs
    per = pushes * F
    N = S * per
    x, T, uv, K, _ = inputs(N, H, dev)
    jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
    base = torch.arange(S, device=dev)[:, None] * per
    chunks = []
    for i in range(pushes):
        r = rows_of(N, base + i * F + torch.arange(F, device=dev)[None], dev)
        chunks.append((jerr[r].contiguous(), x[r].contiguous(), T[r].contiguous()))
    W = lag + F
    r = rows_of(N, base + torch.arange(W, device=dev)[None], dev)
    window = (jerr[r].contiguous(), x[r].contiguous(), T[r].contiguous(), torch.arange(0, S * W + 1, W, dtype=torch.int32, device=dev))
    return chunks, window


def whole(zh, reps, dev, rec):
    from joint_reproj_timing import inputs
    for name, N, S, L in WHOLE:
        x, T, uv, K, _ = inputs(N, H, dev)
        jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
        sd = torch.tensor(list(range(0, N, L)) + [N], dtype=torch.int32, device=dev)
        js = zh.JointAccelMarginalStream(S, H, J, L - 1, L, lam=LAM_V, accel=LAM_A, tau=TAU)
        fl = torch.ones(S, dtype=torch.int32, device=dev)
        assert N == S * L                                            # rows (h, n) with n = s L + f: the problem's own order
        offline = lambda: zh.joint_accel_marginal(jerr, x, T, sd, N=N, lam=LAM_V, accel=LAM_A, tau=TAU, return_weights=True)
        stream = lambda: js.push(jerr, x, T, flush=fl, return_weights=True)
        ro, rs = offline(), stream()
        torch.cuda.synchronize()
        assert rs[1].tolist() == [L] * S
        for o, s in zip(ro, rs[2:]):                                 # equality before anything is timed
            assert torch.equal(bits(s[:, :L].reshape(o.shape)), bits(o)), name
        so, ss = alternate((offline, stream), reps)
        point = dict(S=S, F=L, lag=L - 1, offline_call=so, stream_push=ss, stream_over_offline=round(ss["median_us"] / so["median_us"], 3),
                     offline_spread=round(so["max_us"] / so["min_us"], 3), bit_identical=True, state_bytes=js.state_bytes,
                     offline_workspace_bytes=int(zh._lib.zedo_joint_accel_marginal_workspace_bytes(N, H, J)))
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del x, T, uv, K, jerr, js
        torch.cuda.empty_cache()
    p_long, p_short = rec["points"]["one_clip_of_1015"], rec["points"]["one_clip_of_127"]
    q_push = p_long["stream_push"]["median_us"] / p_short["stream_push"]["median_us"]
    q_off = p_long["offline_call"]["median_us"] / p_short["offline_call"]["median_us"]
    q_off_max = p_long["offline_call"]["max_us"] / p_short["offline_call"]["min_us"]      # the largest quotient the offline call's own repetitions span
    rec["linear_in_L"] = dict(push_1015_over_127=round(q_push, 3), offline_1015_over_127=round(q_off, 3),
                              offline_1015_over_127_at_its_own_spread=round(q_off_max, 3),
                              condition="push quotient (medians) <= offline quotient with that call's own spread: its max at 1 015 over its min at 127",
                              holds=bool(q_push <= q_off_max))
    print(json.dumps(dict(linear_in_L=rec["linear_in_L"])), flush=True)


def live(zh, key, reps, dev, rec):
    name, S, F, lag, pushes = LIVE[key]
    torch.cuda.empty_cache()
    chunks, (wu, wx, wT, wsd) = live_inputs(zh, S, F, lag, pushes, dev)
    W = lag + F
    soft2 = zh.JointAccelMarginalStream(S, H, J, lag, F, lam=LAM_V, accel=LAM_A, tau=TAU)
    hard2 = zh.JointAccelStream(S, H, J, lag, F, lam=LAM_V, accel=LAM_A)
    soft1 = zh.JointMarginalStream(S, H, J, lag, F, lam=100.0, tau=TAU)

    def round_of(js):
        def run():
            js.reset()
            for u, xx, TT in chunks:
                out = js.push(u, xx, TT)
            return out
        return run

    def window_round():
        for _ in range(pushes):
            out = zh.joint_accel_marginal(wu, wx, wT, wsd, N=S * W, lam=LAM_V, accel=LAM_A, tau=TAU)
        return out

    s2, h2, s1, sw = alternate((round_of(soft2), round_of(hard2), round_of(soft1), window_round), reps, pushes, warm=1)
    point = dict(S=S, F=F, lag=lag, pushes_per_round=pushes, accel_stream_marginal_push_per_push=s2, accel_stream_push_per_push=h2,
                 stream_marginal_push_per_push=s1, offline_fusion_on_the_last_lag_plus_F_frames_per_push=sw,
                 soft_over_hard=round(s2["median_us"] / h2["median_us"], 2), second_over_first_order=round(s2["median_us"] / s1["median_us"], 2),
                 window_over_stream=round(sw["median_us"] / s2["median_us"], 2),
                 the_window_route_computes_a_different_answer="it has no history before the window; its window is assembled beforehand, untimed",
                 microseconds_per_walk_frame_if_the_walks_run_in_rounds_of_256=round(s2["median_us"] / lag / max(1.0, np.ceil(S * J * F / 256.0)), 1),
                 workgroups_per_push=S * J * F, frames_per_second_per_stream_at_the_median=round(F / (s2["median_us"] * 1e-6), 0),
                 state_bytes=soft2.state_bytes, hard_state_bytes=hard2.state_bytes, first_order_state_bytes=soft1.state_bytes)
    rec["points"][name] = point
    print(json.dumps({name: point}), flush=True)


def steady(zh, dev, rec):
    name, S, F, lag, pushes = LIVE["live1"]
    torch.cuda.empty_cache()
    chunks, _ = live_inputs(zh, S, F, lag, pushes, dev)
    js = zh.JointAccelMarginalStream(S, H, J, lag, F, lam=LAM_V, accel=LAM_A, tau=TAU)
    n, (e0, e1), (l0, l1) = STEADY["pushes"], STEADY["early"], STEADY["late"]
    early, late = [], []
    for rep in range(STEADY["repetitions"] + 1):                     # (the first repetition warms up and is dropped)
        js.reset()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            js.push(*chunks[i % pushes])
            ev[i + 1].record()
        torch.cuda.synchronize()
        us = [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(n)]
        if rep:
            early.append(float(np.median(us[e0:e1])))
            late.append(float(np.median(us[l0:l1])))
    m_early, m_late, spread = float(np.median(early)), float(np.median(late)), max(early) - min(early)
    rec["steady_state"] = dict(S=S, F=F, lag=lag, pushes=n, repetitions=STEADY["repetitions"], pushes_100_199_median_us=stats(early),
                               pushes_900_999_median_us=stats(late), difference_us=round(abs(m_late - m_early), 1),
                               spread_of_the_earlier_window_us=round(spread, 1),
                               condition="|median of pushes 900-999 - median of pushes 100-199| <= the spread of the earlier window's medians",
                               holds=bool(abs(m_late - m_early) <= spread))
    print(json.dumps(dict(steady_state=rec["steady_state"])), flush=True)


def alternate(routes, reps, per=1, warm=3):
    """routes: callables; `warm` warm-up rounds, then they alternate reps times -> [stats], microseconds / per."""
    for _ in range(warm):
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
    ap.add_argument("--live8-reps", type=int, default=None, help="repetitions of live8 (default: --reps)")
    ap.add_argument("--only", default="whole,live1,live8,steady")
    ap.add_argument("--out", default=None, help="also merge the JSON record into this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    only = a.only.split(",")
    import zedo_hip as zh
    dev = torch.device("cuda")
    rec = dict(points={})
    if a.out and os.path.exists(a.out):
        rec = json.load(open(a.out))
    rec.update(tool="tools/joint_accel_stream_marginal_timing.py", J=J, H=H, smooth=LAM_V, accel=LAM_A, temperature=TAU, reps=a.reps,
               device=torch.cuda.get_device_name(0), hypothesis_counts_timed="H = 50 only",
               method="warm-up rounds, then the routes alternate in one process; device events on the launch stream around the whole call or "
                      "the pushes of a round (binding, allocations from torch's cache); microseconds",
               accuracy_on_real_data="not measured", lag="untuned")
    if "whole" in only:
        whole(zh, a.reps, dev, rec)
    if "live1" in only:
        live(zh, "live1", a.reps, dev, rec)
    if "live8" in only:
        rec["live8_reps"] = a.live8_reps or a.reps
        live(zh, "live8", a.live8_reps or a.reps, dev, rec)
    if "steady" in only:
        steady(zh, dev, rec)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    assert "linear_in_L" not in rec or rec["linear_in_L"]["holds"], rec["linear_in_L"]
    assert "steady_state" not in rec or rec["steady_state"]["holds"], rec["steady_state"]


if __name__ == "__main__":
    main()
