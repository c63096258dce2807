#!/usr/bin/env python3
"""Time the skeleton-coupled fusion per pose (zedo_joint_tree_marginal) against (a) the same two passes stated in plain torch - float64,
all poses batched, one [N,H,H] tensor of terms per bone, torch.logsumexp - and (b) zedo_joint_tree_select, the min-sum call on the same
inputs.  No ratio is fixed in advance: the figures are recorded as they come, slower included.  ONE process, seeded inputs, J = 17,
H = 50 (the only hypothesis count timed), the H36M tree, mu = 100, tau = 1, with T and confidences, the unaries zedo_joint_reproj's
distances:

    50 750 rows    (1 015 poses, BASELINE configs[2])
    3 544 000 rows (70 880 poses, configs[3]'s per-GPU shard)

Before anything is timed the torch statement's outputs are compared with the call's on every point it runs at: the log-marginals and
logz within 4 J (H + 8 + 28 G) 2^-53 (tests/_joint_tree_marginal_ref.py's marg_bound, G taken from the torch statement's own messages),
the mean, the covariance and the bone within the bounds that follow; the point records the differences and `within_bounds`, and a point
out of bounds is not timed.  The torch statement holds a handful of [N,H,H] float64 tensors at once - 1.4 GB each at the large point.  If
the device does not have room for it the point records that and compares nothing; the call itself needs no workspace at all.

Method: after a warm-up of three calls of each route they ALTERNATE --reps times (default 25, at least 20) in the same process; each call
is timed with device events on the launch stream around the whole call (binding, output allocation from torch's cache).  Recorded per
point: median / min / max in microseconds of the three routes and the ratios of the medians.

This measures speed only.  Whether the fused pose is closer to ground truth is not measured here or anywhere in this repository
(random-init weights and synthetic poses cannot tell).

    python tools/joint_tree_marginal_timing.py [--reps 25] [--out profiles/joint_tree_marginal.json]   (GPU box only)
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zedo-release_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from joint_tree_timing import norm3, post_order, stats, timed

J, H, MU, TAU = 17, 50, 100.0, 1.0
POINTS = (("50750_rows", 1015), ("3544000_rows", 70880))
TORCH_TENSORS = 10         # [N,H,H] float64 tensors the statement below holds at its peak (differences, squares, sum, b, terms, pair marginals)


def torch_statement(jerr, x, T, weight, parent, N, mu, tau, magnitudes=False):
    """The two passes of include/zedo_hip.h for inputs without excluded entries, all poses at once -> (mean [N,J,3], cov [N,J,6], hmax, wmax,
    logz [N,J], bone [N,J], lw [N,J,H] = S + Dn - logZ[, G, bmax, lmax]).  E_g is the sum over the other children, as the header defines it."""
    X = (x.double() + T.double()[:, None, :]).view(H, N, J, 3).permute(2, 1, 0, 3).contiguous()       # [J,N,H,3]
    w = weight.clamp(1e-4, 1.0).double()                                                              # the clamp in fp32
    l = list(-(w[:, :, None] * jerr.view(H, N, J).permute(1, 2, 0)).permute(1, 0, 2).contiguous() / tau)   # J x [N,H]
    S, M, Dn = list(l), {}, [torch.zeros_like(l[0]) for _ in range(J)]
    c, order = mu / tau, post_order(parent)
    G = bmax = lmax = 0.0

    def bone_term(g, p):
        nonlocal bmax, lmax
        own = norm3(X[g], X[p])                                                                       # [N,H]
        mix = norm3(X[g][:, None, :, :], X[p][:, :, None, :])                                         # [N,hp,hc]
        half = 0.5 * (own[:, None, :] + own[:, :, None])
        b = (mix - half).abs()
        if magnitudes:
            bmax, lmax = max(bmax, float(b.max())), max(lmax, float((mix + half).max()))
        return b

    for g in order:
        p = parent[g]
        if p >= 0:
            M[g] = torch.logsumexp(S[g][:, None, :] - c * bone_term(g, p), dim=2)
            S[p] = S[p] + M[g]
    lz = [None] * J
    bone = torch.zeros((N, J), dtype=torch.float64, device=x.device)
    for g in reversed(order):
        p = parent[g]
        if p < 0:
            lz[g] = torch.logsumexp(S[g], dim=1)
            continue
        E = l[p]
        for k in range(J):
            if parent[k] == p and k != g:
                E = E + M[k]
        E = E + Dn[p]
        b = bone_term(g, p)
        t = E[:, :, None] - c * b                                                                     # [N,hp,hc]
        Dn[g] = torch.logsumexp(t, dim=1)
        lz[g] = lz[p]
        bone[:, g] = (torch.exp(t + S[g][:, None, :] - lz[g][:, None, None]) * b).sum(dim=(1, 2))
        if magnitudes:
            G = max(G, float(E.abs().max()))
    lw = torch.stack([S[j] + Dn[j] - lz[j][:, None] for j in range(J)], 1)                           # [N,J,H]
    wgt = torch.exp(lw)
    Xn = X.permute(1, 0, 2, 3)                                                                        # [N,J,H,3]
    mean = (wgt[..., None] * Xn).sum(2)
    d = Xn - mean[:, :, None, :]
    cov = torch.stack([(wgt * d[..., a] * d[..., b_]).sum(2) for a, b_ in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 2)
    wmax, hmax = wgt.max(dim=2)
    out = (mean, cov, hmax.to(torch.int32), wmax, torch.stack(lz, 1), bone, lw)
    if magnitudes:
        G = max([G, c * lmax] + [float(v.abs().max()) for v in S + Dn + lz + list(M.values())])
        out += (G, bmax, lmax)
    return out


def compare(rc, rt, x, T, N):
    """The call's outputs (with d_w) against the torch statement's, within the bounds of tests/_joint_tree_marginal_ref.py -> dict."""
    mean, cov, hmax, wmax, logz, bone, w = rc
    tmean, tcov, thmax, twmax, tlogz, tbone, tlw, G, bmax, lmax = rt
    eps = 2.0 ** -53
    beta = 4.0 * J * (H + 8.0 + 28.0 * G) * eps
    X = (x.double() + T.double()[:, None, :]).view(H, N, J, 3)
    xmax = float(X.abs().max())
    spread = float((X.max(0)[0] - X.min(0)[0]).max())
    mb = 2.0 * math.expm1(beta) * (1.0 + beta) * xmax
    cb = 2.0 * math.expm1(beta) * spread ** 2 + 2.0 * mb * math.expm1(beta) * spread + mb ** 2 * (1.0 + beta)
    bb = 2.0 * math.expm1(beta) * (1.0 + beta) * bmax + 40.0 * eps * lmax
    big = tlw > -600.0
    d = dict(G=round(G, 1), log_marginal=float((torch.log(w[big]) - tlw[big]).abs().max()), logz=float((logz - tlogz).abs().max()),
             bound=beta, mean_m=float((mean - tmean).abs().max()), mean_bound_m=mb, cov_m2=float((cov - tcov).abs().max()), cov_bound_m2=cb,
             bone_m=float((bone - tbone).abs().max()), bone_bound_m=bb, hmax_differs=int((hmax != thmax).sum()))
    d["within_bounds"] = bool(d["log_marginal"] <= beta and d["logz"] <= beta and d["mean_m"] <= mb and d["cov_m2"] <= cb and d["bone_m"] <= bb)
    return d


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
    parent = zh.skeleton_parents(zh.H36M_EDGES, J)
    rec = dict(tool="tools/joint_tree_marginal_timing.py", J=J, H=H, bone=MU, temperature=TAU, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="three warm-up calls of each route, then the routes alternate in one process; device events on the launch stream around "
                      "the whole call (binding, allocations from torch's cache); microseconds",
               yardstick="(a) the same two passes in plain torch, float64, all poses batched, one [N,H,H] tensor per bone, torch.logsumexp, "
                         "checked equal to the call within the derived bounds before timing; (b) zedo_joint_tree_select on the same inputs; "
                         "no ratio fixed in advance",
               only_H_timed=H, lds_bytes=48 * J * H + 16 * H + 8192, accuracy_on_real_data="not measured", points={})
    for name, N in POINTS:
        torch.cuda.empty_cache()
        x, T, uv, K, conf = inputs(N, H, dev)
        jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
        del uv, K
        call = lambda: zh.joint_tree_marginal(jerr, x, T, parent, N, MU, TAU, conf)
        minsum = lambda: zh.joint_tree_select(jerr, x, T, parent, N, MU, conf)
        free = torch.cuda.mem_get_info()[0]
        need = TORCH_TENSORS * N * H * H * 8
        plain = (lambda: torch_statement(jerr, x, T, conf, parent, N, MU, TAU)) if need < free else None
        point = dict(N=N, H=H, J=J, rows=N * H, workspace_bytes=0)
        if plain:
            rc = zh.joint_tree_marginal(jerr, x, T, parent, N, MU, TAU, conf, return_weights=True)
            point["against_torch"] = compare(rc, torch_statement(jerr, x, T, conf, parent, N, MU, TAU, magnitudes=True), x, T, N)
            del rc
            if not point["against_torch"]["within_bounds"]:
                point["not_timed"] = "the torch statement and the call differ by more than the bounds"
                rec["points"][name] = point
                print(json.dumps({name: point}), flush=True)
                continue
        for _ in range(3):
            rc = call()
            rm = minsum()
            rt = plain() if plain else None
        torch.cuda.synchronize()
        us_c, us_m, us_t = [], [], []
        for _ in range(a.reps):
            t, rc = timed(call)
            us_c.append(t)
            t, rm = timed(minsum)
            us_m.append(t)
            if plain:
                t, rt = timed(plain)
                us_t.append(t)
        sc, sm = stats(us_c), stats(us_m)
        point.update(call=sc, min_sum_call=sm, call_over_min_sum=round(sc["median_us"] / sm["median_us"], 2),
                     largest_marginal_median=round(float(rc[3].median()), 3),
                     expected_bone_mismatch_mm=round(1e3 * float(rc[5][:, [j for j in range(J) if parent[j] >= 0]].mean()), 3),
                     min_sum_bone_mismatch_mm=round(1e3 * float(rm[2][:, [j for j in range(J) if parent[j] >= 0]].mean()), 3),
                     spread_mm_median=round(1e3 * float((rc[1][:, :, 0] + rc[1][:, :, 3] + rc[1][:, :, 5]).sqrt().median()), 2))
        if plain:
            st = stats(us_t)
            point.update(torch_statement=st, torch_over_call=round(st["median_us"] / sc["median_us"], 2),
                         call_not_slower_than_torch=bool(sc["median_us"] <= st["median_us"]))
        else:
            point.update(torch_statement=f"not run: it holds about {TORCH_TENSORS} [N,H,H] float64 tensors, {need / 2 ** 30:.1f} GiB, and "
                                         f"{free / 2 ** 30:.1f} GiB were free")
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del rc, rm, rt, x, T, jerr, conf
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
