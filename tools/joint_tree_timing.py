#!/usr/bin/env python3
"""Time the skeleton-coupled joint-wise aggregation (zedo_joint_tree_select) against the same recurrence stated in plain torch: float64,
all poses batched, one [N,H,H] tensor of candidates per bone, the downward pass and the bone lengths by gathers.  No ratio is fixed in
advance: the torch statement is the yardstick and the figures are recorded as they come, slower included.  ONE process, seeded inputs,
J = 17, H = 50, the H36M tree, mu = 100, with T and confidences, the unaries zedo_joint_reproj's distances:

    50 750 rows    (1 015 poses, BASELINE configs[2])
    3 544 000 rows (70 880 poses, configs[3]'s per-GPU shard)

The torch statement holds a handful of [N,H,H] float64 tensors at once - 1.4 GB each at the large point.  If the device does not have
room for it the point records that and compares nothing; the call itself needs no workspace at all.  The torch statement's assignment is
compared with the call's on every point it runs at and recorded (assignment_equal), as are the largest differences of cost and bone.

Method: after a warm-up of three calls of each route they ALTERNATE --reps times (default 25, at least 20) in the same process; each call
is timed with device events on the launch stream around the whole call (binding, output allocation from torch's cache).  Recorded per
point: median / min / max in microseconds of both routes and the ratio of the medians.

This measures speed only.  Whether the coupled pose is closer to ground truth is not measured here or anywhere in this repository
(random-init weights and synthetic poses cannot tell).

    python tools/joint_tree_timing.py [--reps 25] [--out profiles/joint_tree.json]   (GPU box only)
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

J, H, MU = 17, 50, 100.0
POINTS = (("50750_rows", 1015), ("3544000_rows", 70880))
TORCH_TENSORS = 8          # [N,H,H] float64 tensors the statement below holds at its peak (three differences, squares, sum, b, candidates)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(us):
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(float(min(us)), 1), max_us=round(float(max(us)), 1), reps=len(us))


def norm3(a, b):
    d0, d1, d2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return torch.sqrt(d0 * d0 + d1 * d1 + d2 * d2)


def post_order(parent):
    kids = [[c for c in range(len(parent)) if parent[c] == j] for j in range(len(parent))]
    out = []

    def walk(j):
        for c in kids[j]:
            walk(c)
        out.append(j)

    for r in range(len(parent)):
        if parent[r] < 0:
            walk(r)
    return out


def torch_statement(jerr, x, T, weight, parent, N, mu):
    """The recurrence of include/zedo_hip.h for inputs without excluded entries, all poses at once -> (joint_h [N,J] i32, cost [N], bone [N,J])."""
    X = (x.double() + T.double()[:, None, :]).view(H, N, J, 3).permute(2, 1, 0, 3).contiguous()       # [J,N,H,3]
    w = weight.clamp(1e-4, 1.0).double()                                                              # the clamp in fp32
    S = list((w[:, :, None] * jerr.view(H, N, J).permute(1, 2, 0)).permute(1, 0, 2).contiguous())      # J x [N,H]
    order, back = post_order(parent), {}
    for g in order:
        p = parent[g]
        if p < 0:
            continue
        own = norm3(X[g], X[p])                                                                       # [N,H]
        b = (norm3(X[g][:, None, :, :], X[p][:, :, None, :]) - 0.5 * (own[:, None, :] + own[:, :, None])).abs()   # [N,hp,hc]
        M, back[g] = (S[g][:, None, :] + mu * b).min(dim=2)
        S[p] = S[p] + M
    sel = [None] * J
    cost = torch.zeros((N,), dtype=torch.float64, device=x.device)
    bone = torch.zeros((N, J), dtype=torch.float64, device=x.device)
    for j in range(J):
        if parent[j] < 0:
            m, sel[j] = S[j].min(dim=1)
            cost = cost + m
    pick = lambda Xj, h: Xj.gather(1, h[:, None, None].expand(N, 1, 3))[:, 0]                         # [N,3]
    for g in reversed(order):
        p = parent[g]
        if p < 0:
            continue
        sel[g] = back[g].gather(1, sel[p][:, None])[:, 0]
        gc, gp, pc, pp = pick(X[g], sel[g]), pick(X[g], sel[p]), pick(X[p], sel[g]), pick(X[p], sel[p])
        bone[:, g] = (norm3(gc, pp) - 0.5 * (norm3(gc, pc) + norm3(gp, pp))).abs()
    return torch.stack(sel, 1).to(torch.int32), cost, bone


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
    rec = dict(tool="tools/joint_tree_timing.py", J=J, H=H, bone=MU, reps=a.reps, device=torch.cuda.get_device_name(0),
               method="three warm-up calls of each route, then the routes alternate in one process; device events on the launch stream around "
                      "the whole call (binding, allocations from torch's cache); microseconds",
               yardstick="the same recurrence in plain torch, float64, all poses batched, one [N,H,H] tensor per bone; no ratio fixed in advance",
               accuracy_on_real_data="not measured", points={})
    for name, N in POINTS:
        torch.cuda.empty_cache()
        x, T, uv, K, conf = inputs(N, H, dev)
        jerr = zh.joint_reproj(x, T, uv, K, return_rows=True)[2]
        del uv, K
        call = lambda: zh.joint_tree_select(jerr, x, T, parent, N, MU, conf)
        free = torch.cuda.mem_get_info()[0]
        need = TORCH_TENSORS * N * H * H * 8
        plain = (lambda: torch_statement(jerr, x, T, conf, parent, N, MU)) if need < free else None
        for _ in range(3):
            rc = call()
            rt = plain() if plain else None
        torch.cuda.synchronize()
        us_c, us_t = [], []
        for _ in range(a.reps):
            t, rc = timed(call)
            us_c.append(t)
            if plain:
                t, rt = timed(plain)
                us_t.append(t)
        sc = stats(us_c)
        point = dict(N=N, H=H, J=J, rows=N * H, call=sc, workspace_bytes=0,
                     hypotheses_per_pose=round(float(np.mean([len(set(v)) for v in rc[0][:2000].cpu().numpy().tolist()])), 2),
                     mean_bone_mismatch_mm=round(1e3 * float(rc[2][:, [j for j in range(J) if parent[j] >= 0]].mean()), 3))
        if plain:
            st = stats(us_t)
            point.update(torch_statement=st, torch_over_call=round(st["median_us"] / sc["median_us"], 2),
                         call_not_slower_than_torch=bool(sc["median_us"] <= st["median_us"]), assignment_equal=bool(torch.equal(rc[0], rt[0])),
                         max_cost_difference=float((rc[1] - rt[1]).abs().max()), max_bone_difference=float((rc[2] - rt[2]).abs().max()))
        else:
            point.update(torch_statement=f"not run: it holds about {TORCH_TENSORS} [N,H,H] float64 tensors, {need / 2 ** 30:.1f} GiB, and "
                                         f"{free / 2 ** 30:.1f} GiB were free")
        rec["points"][name] = point
        print(json.dumps({name: point}), flush=True)
        del rc, rt, x, T, jerr, conf
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
