#!/usr/bin/env python3
"""Time the pose-level fusion along a video (zedo_temporal_marginal) against two yardsticks, in ONE process on seeded inputs, J = 17,
H = 50, lambda = 100, tau = 1:

    torch_statement   the same two recurrences stated in plain torch, float64, with torch.logsumexp: all clips of one time offset in one
                      batched step ([clips, H, H'] transition costs per step from a [clips, H, H', J, 3] difference), forward, then
                      backward, then the marginals, the mean and the covariance - what a user would write without the kernel (finite
                      unaries only: no dead frames here);
    viterbi           zedo_temporal_select on the same inputs - the max-product twin.  The arithmetic predicts a small multiple of it:
                      two scans where it has one, two walks over a column of transition costs in each, one exp per pair, and every
                      transition cost computed twice (once per scan, in the layout that scan reads).

    50 750 rows   (1 015 frames, BASELINE configs[2])            as 29 clips of 35 frames and as ONE clip of 1 015 frames
    3 544 000 rows (70 880 frames, configs[3]'s per-GPU shard)   as 2 026 clips of 35 frames (the last one of 5)

Before anything is timed the kernel's outputs are ASSERTED equal to the torch statement's within the bounds of
tests/_temporal_marginal_ref.py (beta on the log-marginals and logZ, mean_bound, cov_bound), with G read off the torch statement's A.
Method: after a warm-up of three calls of each route they ALTERNATE --reps times (default 25, at least 20) in the same process; each call
is timed with device events on the launch stream around the whole call (binding, output and workspace allocation from torch's cache).
Recorded per point: median / min / max in microseconds of the three, the ratios of the medians, the largest differences, the workspace.
One more pair alternates at the 29-clip shape: chunk_frames = N against a chunk that cuts the frames into three - what the chunking
itself costs (both recompute every transition cost once: the backward scan reads the transposed table).  No ratio is promised: what is
measured is recorded, also where the kernel is not the faster one (native_not_slower_than_torch).  One workgroup walks one clip: the
single 1 015-frame clip is serial in time on ONE compute unit, and is reported as that.

This measures speed only.  Whether the fused pose is closer to ground truth than a selected one on real video is not measured here or
anywhere in this repository (random-init weights and synthetic poses cannot tell).

    python tools/temporal_marginal_timing.py [--reps 25] [--out profiles/temporal_marginal.json]   (GPU box only)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

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


def torch_statement(unary, x, T, starts, lens, N, lam, tau):
    """-> (mean [N,J,3], cov [N,J,6], hmax [N], w [N,H], logz [N], A [N,H]) float64; starts / lens: int64 tensors of the clips."""
    Hh = x.shape[0] // N
    xs = x.double().reshape(Hh, N, -1, 3).permute(1, 0, 2, 3).contiguous()                               # [N, H, J, 3]: the motion term
    X = (x.double() + T.double()[:, None, :]).reshape(Hh, N, -1, 3).permute(1, 0, 2, 3).contiguous()     # the moments
    l = (-unary / tau).reshape(Hh, N).t().contiguous()                                                   # [N, H]
    c = lam / tau
    A, LB = torch.empty_like(l), torch.empty_like(l)                                                     # LB = l + B
    Bv = torch.zeros_like(l)
    Lmax = int(lens.max().item())
    motion = lambda cur, prev: (xs[cur][:, :, None] - xs[prev][:, None, :]).square().sum(-1).sqrt().mean(-1)   # [C, h of cur, h' of prev]
    for t in range(Lmax):
        i = starts[lens > t] + t
        if t == 0:
            A[i] = l[i]
        else:
            A[i] = l[i] + torch.logsumexp(A[i - 1][:, None, :] - c * motion(i, i - 1), dim=-1)
    ends = starts + lens - 1
    for t in range(Lmax):                                                                                # t frames before the clip's end
        i = ends[lens > t] - t
        if t > 0:
            Bv[i] = torch.logsumexp(LB[i + 1][:, None, :] - c * motion(i + 1, i).transpose(1, 2), dim=-1)
        LB[i] = l[i] + Bv[i]
    lz = torch.logsumexp(A[ends], dim=-1)                                                                # [clips]
    logz = torch.repeat_interleave(lz, lens, dim=0)                                                      # clips are consecutive
    w = ((A + Bv) - logz[:, None]).exp()
    mean = (w[:, :, None, None] * X).sum(1)
    d = X - mean[:, None]
    cov = torch.stack([(w[:, :, None] * d[..., p] * d[..., q]).sum(1) for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], -1)
    return mean, cov, w.argmax(1), w, logz, A


def assert_equal_within_the_bounds(rn, rp, x, T, N, L):
    """The kernel's (mean, cov, hmax, wmax, logz, w) against the torch statement's outputs; -> the observed figures."""
    from _temporal_marginal_ref import cov_bound, marg_bound, mean_bound
    mean, cov, hmax, wmax, logz, w = rn
    pmean, pcov, phmax, pw, plogz, pA = rp
    G = float(pA.abs().max())
    beta = marg_bound(L, H, J, G)
    big = pw > 1e-300
    e_lw = float((w[big].log() - pw[big].log()).abs().max())
    e_lz = float((logz - plogz).abs().max())
    X = (x.double() + T.double()[:, None, :]).reshape(H, N, J, 3)
    xmax = float(X.abs().max())
    spread = (X.amax(0) - X.amin(0)).amax(-1)                                                            # [N, J]
    mb = float(mean_bound(beta, xmax))
    cb = torch.as_tensor(cov_bound(beta, spread.cpu().numpy(), xmax), device=cov.device)[:, :, None]
    e_mean, e_cov = float((mean - pmean).abs().max()), (cov - pcov).abs()
    seen = dict(G=G, beta=beta, max_abs_log_marginal_difference_to_torch=e_lw, share_of_beta=e_lw / beta, max_abs_logz_difference_to_torch=e_lz,
                max_abs_mean_difference_to_torch_m=e_mean, mean_bound_m=mb, max_abs_cov_difference_to_torch_m2=float(e_cov.max()),
                hmax_differs_from_torch=int((hmax != phmax).sum()))
    assert e_lw <= beta and e_lz <= beta and e_mean <= mb and bool((e_cov <= cb).all()), seen
    return seen


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
    rec = dict(tool="tools/temporal_marginal_timing.py", J=J, H=H, smooth=LAM, temperature=TAU, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="equality with the torch statement asserted within the derived bounds first; three warm-up calls of each route, then the "
                      "routes alternate in one process; device events on the launch stream around the whole call (binding, allocations from "
                      "torch's cache); microseconds",
               accuracy_on_real_data="not measured", points={})
    data = {}
    for name, N, clip in POINTS:
        if N not in data:
            data.clear()
            torch.cuda.empty_cache()
            x, T, uv, K, conf = inputs(N, H, dev)
            data[N] = (x, T, zh.min_reproj(x, T, uv, K, conf, N, 0)[0])
            del uv, K, conf
        x, T, err = data[N]
        seq = list(range(0, N, clip)) + [N]
        sd = torch.tensor(seq, dtype=torch.int32, device=dev)
        starts = sd[:-1].to(torch.int64)
        lens = (sd[1:] - sd[:-1]).to(torch.int64)

        def native(chunk=0):
            return zh.temporal_marginal(err, x, T, sd, N=N, lam=LAM, tau=TAU, chunk_frames=chunk, return_weights=True)

        def plain():
            return torch_statement(err, x, T, starts, lens, N, LAM, TAU)

        def viterbi():
            return zh.temporal_select(err, x, sd, N=N, lam=LAM)

        seen = assert_equal_within_the_bounds(native(), plain(), x, T, N, min(clip, N))
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
                     native_not_slower_than_torch=bool(sn["median_us"] <= sp["median_us"]), **seen,
                     median_largest_marginal=round(float(rn[3].median()), 4),
                     share_of_frames_where_the_most_probable_hypothesis_leaves_the_viterbi_path=round(float((rn[2] != rv[0]).double().mean()), 4),
                     chunk_frames_native=int(min(N, max(1, (256 << 20) // (8 * H * H)))),
                     workspace_bytes_native=int(zh.temporal_marginal_workspace_bytes(N, H, 0)),
                     workspace_bytes_viterbi=int(zh._lib.zedo_temporal_workspace_bytes(N, H, 0)))
        if name == POINTS[0][0]:                                     # what cutting the frames into three chunks costs
            third = (N + 2) // 3
            for _ in range(3):
                ra, rb = native(N), native(third)
            assert all(torch.equal(p, q) for p, q in zip(ra, rb))
            us_a, us_b = [], []
            for _ in range(a.reps):
                us_a.append(timed(lambda: native(N))[0])
                us_b.append(timed(lambda: native(third))[0])
            sa, sb = stats(us_a), stats(us_b)
            point["chunking"] = dict(one_chunk=sa, three_chunks=sb, chunk_frames_three=third,
                                     three_over_one=round(sb["median_us"] / sa["median_us"], 3), same_bits=True,
                                     workspace_bytes_three=int(zh.temporal_marginal_workspace_bytes(N, H, third)))
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
