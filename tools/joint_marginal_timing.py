#!/usr/bin/env python3
"""Time the joint-wise fusion along a video (zedo_joint_marginal) against two yardsticks, in ONE process on seeded inputs, J = 17, H = 50,
lambda = 100, tau = 1:

    torch_statement   the same recurrences stated in plain torch, float64, with torch.logsumexp: all clips and joints of one time offset in
                      one batched step ([clips, J, H, H'] transition costs per step), forward, then backward with the marginals, the mean
                      and the covariance - what a user would write without the kernel (finite unaries only: no dead entries here);
    viterbi           zedo_joint_temporal_select on the same inputs - the max-product twin: one square root per pair where the fusion
                      takes two square roots and one exponential, one pass where the fusion takes two.

    50 750 rows   (1 015 frames, BASELINE configs[2])            as 29 clips of 35 frames and as ONE clip of 1 015 frames
    3 544 000 rows (70 880 frames, configs[3]'s per-GPU shard)   as 2 026 clips of 35 frames (the last one of 5)

Method: after a warm-up of three calls of each route they ALTERNATE --reps times (default 25, at least 20) in the same process; each call
is timed with device events on the launch stream around the whole call (binding, output and workspace allocation from torch's cache).
Recorded per point: median / min / max in microseconds of the three, the ratios of the medians, the largest difference between the
kernel's and the torch statement's outputs, and the workspace.  No ratio is promised: what is measured is recorded, also where the
kernel is not the faster one (native_not_slower_than_torch).  One workgroup walks one (clip, joint): the single 1 015-frame clip is
serial in time on J = 17 compute units, and is reported as that.

This measures speed only.  Whether the fused pose is closer to ground truth than a selected one on real video is not measured here or
anywhere in this repository (random-init weights and synthetic poses cannot tell).

    python tools/joint_marginal_timing.py [--reps 25] [--out profiles/joint_marginal.json]   (GPU box only)
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

J, H, CLIP, LAM, TAU = 17, 50, 35, 100.0, 1.0
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


def torch_statement(junary, x, T, starts, lens, N, lam, tau):
    """-> (mean [N,J,3], cov [N,J,6], hmax [N,J], w [N,J,H]) float64; starts / lens: int64 tensors of the clips."""
    Hh = x.shape[0] // N
    X = (x.double() + T.double()[:, None, :]).reshape(Hh, N, -1, 3).permute(1, 2, 0, 3).contiguous()      # [N, J, H, 3]
    l = (-junary / tau).reshape(Hh, N, -1).permute(1, 2, 0).contiguous()                                 # [N, J, H]
    c = lam / tau
    A, LB = torch.empty_like(l), torch.empty_like(l)                                                     # LB = l + B
    Bv = torch.zeros_like(l)
    Lmax = int(lens.max().item())
    for t in range(Lmax):
        i = starts[lens > t] + t
        if t == 0:
            A[i] = l[i]
        else:
            m = (X[i][:, :, :, None, :] - X[i - 1][:, :, None, :, :]).square().sum(-1).sqrt()            # [C, J, h, h']
            A[i] = l[i] + torch.logsumexp(A[i - 1][:, :, None, :] - c * m, dim=-1)
    ends = starts + lens - 1
    for t in range(Lmax):                                                                                # t frames before the clip's end
        live = lens > t
        i = ends[live] - t
        if t > 0:
            m = (X[i + 1][:, :, None, :, :] - X[i][:, :, :, None, :]).square().sum(-1).sqrt()            # [C, J, h, h']
            Bv[i] = torch.logsumexp(LB[i + 1][:, :, None, :] - c * m, dim=-1)
        LB[i] = l[i] + Bv[i]
    lz = torch.logsumexp(A[ends], dim=-1)                                                                # [clips, J]
    logz = torch.repeat_interleave(lz, lens, dim=0)                                                      # clips are consecutive
    w = (A + Bv - logz[:, :, None]).exp()
    mean = (w[..., None] * X).sum(2)
    d = X - mean[:, :, None, :]
    cov = torch.stack([(w * d[..., p] * d[..., q]).sum(2) for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], -1)
    return mean, cov, w.argmax(2), w


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
    rec = dict(tool="tools/joint_marginal_timing.py", J=J, H=H, smooth=LAM, temperature=TAU, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="three warm-up calls of each route, then the routes alternate in one process; device events on the launch stream around "
                      "the whole call (binding, allocations from torch's cache); microseconds",
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
        starts = sd[:-1].to(torch.int64)
        lens = (sd[1:] - sd[:-1]).to(torch.int64)

        def native():
            return zh.joint_marginal(jerr, x, T, sd, N=N, lam=LAM, tau=TAU, return_weights=True)

        def plain():
            return torch_statement(jerr, x, T, starts, lens, N, LAM, TAU)

        def viterbi():
            return zh.joint_temporal_select(jerr, x, T, sd, N=N, lam=LAM)

        for _ in range(3):
            rn, rp, rv = native(), plain(), viterbi()
        torch.cuda.synchronize()
        us_n, us_p, us_v = [], [], []
        for _ in range(a.reps):
            t, rn = timed(native)
            us_n.append(t)
            t, rp = timed(plain)
            us_p.append(t)
            t, rv = timed(viterbi)
            us_v.append(t)
        sn, sp, sv = stats(us_n), stats(us_p), stats(us_v)
        point = dict(N=N, H=H, J=J, clips=len(seq) - 1, longest_clip=min(clip, N), native=sn, torch_statement=sp, viterbi=sv,
                     torch_over_native=round(sp["median_us"] / sn["median_us"], 2), native_over_viterbi=round(sn["median_us"] / sv["median_us"], 2),
                     native_not_slower_than_torch=bool(sn["median_us"] <= sp["median_us"]),
                     max_abs_marginal_difference_to_torch=float((rn[5] - rp[3]).abs().max()),
                     max_abs_mean_difference_to_torch_m=float((rn[0] - rp[0]).abs().max()),
                     max_abs_cov_difference_to_torch_m2=float((rn[1] - rp[1]).abs().max()),
                     median_largest_marginal=round(float(rn[3].median()), 4),
                     share_of_frame_joints_where_the_most_probable_hypothesis_leaves_the_viterbi_path=round(float((rn[2] != rv[0]).double().mean()), 4),
                     workspace_bytes_native=int(zh._lib.zedo_joint_marginal_workspace_bytes(N, H, J)),
                     workspace_bytes_viterbi=int(zh._lib.zedo_joint_temporal_workspace_bytes(N, H, J)))
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del rn, rp, rv
    rec["native_not_slower_than_torch_everywhere"] = all(p["native_not_slower_than_torch"] for p in rec["points"].values())
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
