#!/usr/bin/env python3
"""Time the fusion along a video under the second-order motion model (zedo_joint_accel_marginal) against three yardsticks on the same
inputs: its hard twin zedo_joint_accel_select (one pass of H^3 transitions with a min where this call has two passes of two walks each,
with an exp per transition in the second walk: a small multiple is expected, not parity), the first-order fusion zedo_joint_marginal (H^2
transitions per (frame, joint): a multiple of the order of H is expected), and the same pair recurrences stated in plain torch (float64,
torch.logsumexp, the clips of a point batched into one tensor).  ONE process, seeded inputs, J = 17, H = 50, lambda_v = lambda_a = 100,
tau = 1, with T:

    50 750 rows   (1 015 frames, BASELINE configs[2])            as 29 clips of 35 frames and as ONE clip of 1 015 frames
    3 544 000 rows (70 880 frames, configs[3]'s per-GPU shard)   as 2 026 clips of 35 frames (the last one of 5)

The workspace of this call is 8 N J H^2 bytes: 345 MB at the first two points and 24 GB at the third, where the recording is therefore
cut into SPLIT = 8 calls of 254 whole clips (8 890 frames, 3.0 GB of workspace each; the last call has 248 clips).  The rows of every
part are gathered into contiguous tensors BEFORE anything is timed (the ABI wants the rows of a call h-major and contiguous); the time of
the split route is the sum of its calls.  The two native yardsticks run unsplit.  The torch statement needs 8 H^3 J bytes per clip and
frame step: it runs at the first two points and NOT at the third.  Where it runs, the call's marginals, log Z, mean and covariance are
checked against it within accel_marg_bound (tests/_joint_accel_marginal_ref.py) and what follows from it BEFORE anything is timed; a miss
ends the tool.

Method: after a warm-up of three calls of each route they ALTERNATE --reps times (default 25, at least 20) in the same process; each call
is timed with device events on the launch stream around the whole call (binding, output and workspace allocation from torch's cache).
Recorded per point: median / min / max in microseconds of every route and the ratios of the medians.  One workgroup walks one (clip,
joint): the single 1 015-frame clip is serial in time on J = 17 compute units, and is reported as that.  What bounds the kernels (fp64
rate, the LDS, the exp) is NOT profiled here.

This measures speed only.  The weights are the untuned defaults.  Whether the fused second-order pose is closer to ground truth on real
video is not measured here or anywhere in this repository (random-init weights and synthetic poses cannot tell).

    python tools/joint_accel_marginal_timing.py [--reps 25] [--out profiles/joint_accel_marginal.json]   (GPU box only)
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

J, H, CLIP, LAM_V, LAM_A, TAU, SPLIT = 17, 50, 35, 100.0, 100.0, 1.0, 8
# (name, frames, frames per clip, run the torch statement, calls the recording is cut into)
POINTS = (("50750_rows_clips_of_35", 1015, CLIP, True, 1), ("50750_rows_one_clip", 1015, 1015, True, 1),
          ("3544000_rows_clips_of_35", 70880, CLIP, False, SPLIT))


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


def torch_statement(jerr, x, T, N, L, lam_v, lam_a, tau):
    """The recurrences over pairs of include/zedo_hip.h for clips of exactly L >= 3 frames without dead or excluded entries, all clips and
    joints at once -> (mean [N,J,3], cov [N,J,6], hmax [N,J], w [N,J,H], logz [N,J], G)."""
    C = N // L
    c_v, c_a = lam_v / tau, lam_a / tau
    X = (x.double() + T.double()[:, None, :]).view(H, C, L, J, 3).permute(1, 3, 2, 0, 4)      # [C,J,L,H,3]
    l = -jerr.view(H, C, L, J).permute(1, 3, 2, 0) / tau                                      # [C,J,L,H]
    motion = lambda n: norm3(X[:, :, n, None, :, :] - X[:, :, n - 1, :, None, :])             # [C,J,h',h]
    A2 = [None, l[:, :, 0, :, None] + (l[:, :, 1, None, :] - c_v * motion(1))]
    for n in range(2, L):
        g = X[:, :, n, None, :, :] - 2.0 * X[:, :, n - 1, :, None, :]                         # [C,J,h',h,3]
        a = norm3(g[:, :, None] + X[:, :, n - 2, :, None, None, :])                           # [C,J,h'',h',h]
        A2.append(l[:, :, n, None, :] + (-c_v * motion(n) + torch.logsumexp(A2[n - 1][:, :, :, :, None] - c_a * a, dim=2)))
    lz = torch.logsumexp(A2[L - 1].flatten(2), dim=-1)                                        # [C,J]
    G = max(float(l.abs().max()), max(float(t.abs().max()) for t in A2[1:]), 4.0 * 3.0 ** 0.5 * float(X.abs().max()) * (c_v + c_a))
    w = torch.empty((C, J, L, H), dtype=torch.float64, device=x.device)
    B2 = torch.zeros_like(A2[1])
    for n in range(L - 1, 0, -1):
        if n < L - 1:
            M = (l[:, :, n + 1, None, :] - c_v * motion(n + 1)) + B2                          # [C,J,h,h+]
            g = X[:, :, n - 1, :, None, :] - 2.0 * X[:, :, n, None, :, :]                     # [C,J,h',h,3]
            a = norm3(g[:, :, :, :, None, :] + X[:, :, n + 1, None, None, :, :])              # [C,J,h',h,h+]
            B2 = torch.logsumexp(M[:, :, None] - c_a * a, dim=-1)
        pi = (A2[n] + B2 - lz[:, :, None, None]).exp()
        w[:, :, n] = pi.sum(2)
        if n == 1:
            w[:, :, 0] = pi.sum(3)
    mean = (w[..., None] * X).sum(3)                                                          # [C,J,L,3]
    d = X - mean[:, :, :, None, :]
    cov = torch.stack([(w * d[..., p] * d[..., q]).sum(3) for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], -1)
    flat = lambda t: t.permute(0, 2, 1, *range(3, t.dim())).reshape((N, J) + tuple(t.shape[3:]))
    return flat(mean), flat(cov), flat(w).argmax(2), flat(w), lz[:, None, :].expand(C, L, J).reshape(N, J), G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import zedo_hip as zh
    from _joint_accel_marginal_ref import accel_marg_bound
    from _joint_marginal_ref import cov_bound, mean_bound
    from joint_reproj_timing import inputs
    dev = torch.device("cuda")
    rec = dict(tool="tools/joint_accel_marginal_timing.py", J=J, H=H, smooth=LAM_V, accel=LAM_A, temperature=TAU, reps=a.reps,
               device=torch.cuda.get_device_name(0),
               method="three warm-up calls of each route, then the routes alternate in one process; device events on the launch stream around "
                      "the whole call (binding, allocations from torch's cache); microseconds; the split route: its parts gathered beforehand, "
                      "the sum of its calls",
               what_bounds_the_kernels="not profiled", accuracy_on_real_data="not measured", weights="untuned defaults", points={})
    data = {}
    for name, N, clip, with_torch, split in POINTS:
        if N not in data:
            data.clear()
            torch.cuda.empty_cache()
            x, T, uv, K, _ = inputs(N, H, dev)
            data[N] = (x, T, zh.joint_reproj(x, T, uv, K, return_rows=True)[2])
            del uv, K
        x, T, jerr = data[N]
        seq = list(range(0, N, clip)) + [N]
        sd = torch.tensor(seq, dtype=torch.int32, device=dev)
        n_clips = len(seq) - 1
        per = -(-n_clips // split)                                   # whole clips per call
        parts = []
        for k in range(0, n_clips, per):
            n0, n1 = seq[k], seq[min(k + per, n_clips)]
            cut = lambda t: t.view((H, N) + tuple(t.shape[1:]))[:, n0:n1].reshape((H * (n1 - n0),) + tuple(t.shape[1:])).contiguous()
            parts.append((cut(jerr), cut(x), cut(T), torch.tensor([s - n0 for s in seq[k:min(k + per, n_clips) + 1]], dtype=torch.int32, device=dev),
                          n1 - n0) if split > 1 else (jerr, x, T, sd, N))

        def fused():
            return [zh.joint_accel_marginal(u_, x_, T_, s_, N=n_, lam=LAM_V, accel=LAM_A, tau=TAU, return_weights=with_torch)
                    for u_, x_, T_, s_, n_ in parts]

        select = lambda: zh.joint_accel_select(jerr, x, T, sd, N=N, lam=LAM_V, accel=LAM_A)
        first = lambda: zh.joint_marginal(jerr, x, T, sd, N=N, lam=LAM_V, tau=TAU)
        plain = (lambda: torch_statement(jerr, x, T, N, clip, LAM_V, LAM_A, TAU)) if with_torch else None
        point = dict(N=N, H=H, J=J, clips=n_clips, longest_clip=min(clip, N), calls_of_the_fused_route=len(parts),
                     workspace_bytes_fused_per_call=int(zh._lib.zedo_joint_accel_marginal_workspace_bytes(parts[0][4], H, J)),
                     workspace_bytes_fused_unsplit=8 * N * J * H * H + (4 * N * J + 7) // 8 * 8,
                     workspace_bytes_select=int(zh._lib.zedo_joint_accel_workspace_bytes(N, H, J)),
                     workspace_bytes_first_order_fusion=int(zh._lib.zedo_joint_marginal_workspace_bytes(N, H, J)))
        if plain:                                                    # equal within the bounds, or nothing is timed
            mean, cov, hmax, wmax, logz, w = fused()[0]
            pm, pc, ph, pw, plz, G = plain()
            beta = accel_marg_bound(min(clip, N), H, G)
            big = pw > 1e-300
            e_lw = float((w[big].log() - pw[big].log()).abs().max())
            e_lz = float((logz - plz).abs().max())
            X = x.double().view(H, N, J, 3) + T.double().view(H, N, 1, 3)
            xmax = float(X.abs().max())
            spread = (X.max(0).values - X.min(0).values).max(-1).values.cpu().numpy()
            e_mean, e_cov = float((mean - pm).abs().max()), (cov - pc).abs().cpu().numpy()
            ok = (e_lw <= beta and e_lz <= beta and e_mean <= mean_bound(beta, xmax)
                  and bool((e_cov <= cov_bound(beta, spread, xmax)[:, :, None]).all()))
            point.update(G=G, bound_on_log_marginals=beta, max_abs_log_marginal_difference_to_torch=e_lw, max_abs_logz_difference_to_torch=e_lz,
                         max_abs_mean_difference_to_torch_m=e_mean, mean_bound_m=float(mean_bound(beta, xmax)),
                         max_abs_cov_difference_to_torch_m2=float(e_cov.max()), equal_to_torch_within_the_bounds=ok,
                         share_of_frame_joints_where_hmax_differs_from_torch=round(float((hmax.long() != ph).double().mean()), 6))
            if not ok:
                print(json.dumps({name: point}), flush=True)
                sys.exit(f"{name}: the call and the torch statement differ by more than the bounds; nothing was timed")
            del mean, cov, hmax, wmax, logz, w, pm, pc, ph, pw, plz, X
        for _ in range(3):
            rf, rs, r1 = fused(), select(), first()
            rt = plain() if plain else None
        torch.cuda.synchronize()
        us_f, us_s, us_1, us_t = [], [], [], []
        for _ in range(a.reps):
            t, rf = timed(fused)
            us_f.append(t)
            t, rs = timed(select)
            us_s.append(t)
            t, r1 = timed(first)
            us_1.append(t)
            if plain:
                t, rt = timed(plain)
                us_t.append(t)
        sf, ss, s1 = stats(us_f), stats(us_s), stats(us_1)
        hm = torch.cat([r[2] for r in rf])
        point.update(fused_call=sf, select_call=ss, first_order_fusion_call=s1,
                     fused_over_select=round(sf["median_us"] / ss["median_us"], 2),
                     fused_over_first_order_fusion=round(sf["median_us"] / s1["median_us"], 1),
                     median_largest_marginal=round(float(torch.cat([r[3] for r in rf]).median()), 4),
                     median_largest_marginal_first_order=round(float(r1[3].median()), 4),
                     share_of_frame_joints_where_the_most_probable_hypothesis_leaves_the_select_path=round(float((hm != rs[0]).double().mean()), 4))
        if plain:
            st = stats(us_t)
            point.update(torch_statement=st, torch_over_fused=round(st["median_us"] / sf["median_us"], 1),
                         fused_not_slower_than_torch=bool(sf["median_us"] <= st["median_us"]))
        else:
            point.update(torch_statement="not run: 8 H^3 J bytes per clip and frame step, 34 GB at this point")
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del rf, rs, r1, rt, parts
    rec["fused_not_slower_than_torch_everywhere_it_ran"] = all(p.get("fused_not_slower_than_torch", True) for p in rec["points"].values())
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
