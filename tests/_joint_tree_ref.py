"""The float64 reference of the skeleton-coupled joint-wise aggregation (zedo_joint_tree_select, include/zedo_hip.h), stated directly in
numpy: the camera-frame positions, the weighted unaries, the bone term, the recurrence from the leaves to the roots and the downward pass
exactly as the header words them; the trees and the inputs the CPU and GPU tests share (those of _joint_temporal_ref, every frame read as
an independent pose); and the bound the kernel's cost and bone are held to.  Pinned on its own by tests/test_joint_tree_ref.py (against
the enumeration of all assignments); the GPU tests hold the kernel to it."""
import functools
import itertools

import numpy as np

from _joint_temporal_ref import camera_frame, case, per_frame_argmin  # noqa: F401  (re-exported to the tests)

H36M_PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15]
H36M_EDGES = [[0, 1], [1, 2], [2, 3], [0, 4], [4, 5], [5, 6], [0, 7], [7, 8], [8, 9], [9, 10], [8, 11], [11, 12], [12, 13], [8, 14], [14, 15],
              [15, 16]]

# (J, N, H): what the issue lists
CASES = [(1, 1, 1), (2, 3, 2), (5, 12, 3), (17, 70, 50), (17, 40, 64), (21, 20, 65), (17, 6, 128), (17, 4, 129), (64, 6, 5), (3, 8, 256), (2, 4, 257)]
# the smallest shapes on both sides of the constants of csrc/zedo_joint_tree.hip that the table above does not straddle:
#   the hc of a bone are split over 4 parts of the workgroup up to H = 64 and over 2 up to H = 128; above that a lane owns hp = t, t + 256,
#   ..: 64 | 65, 128 | 129 and 256 | 257 are all above;
#   a wave takes the roots' arg-min and the dead flags 64 hypotheses at a time, joints w, w + 4, ..: one-joint trees at 64 | 65, and a
#   forest of 5 roots (more roots than waves) below;
#   the LDS cap 34 J H + 16 H + 4096 <= 163840: H = 268 is the last that fits at J = 17, H = 72 at J = 64, and H = 1024 (the cap on H itself)
#   fits up to J = 4; the first sizes beyond each are refused (tests/test_joint_tree_gpu.py::test_refusals).
BOUNDARY_CASES = [(1, 3, 64), (1, 3, 65), (17, 2, 268), (64, 2, 72), (4, 2, 1024)]
TOO_LARGE = [(17, 269), (64, 73), (5, 1024), (1, 1025), (65, 2)]          # (J, H)
ALL_CASES = CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}" for J, N, H in ALL_CASES]
MUS = (30.0, 100.0, 300.0)
GAP_MIN = 1e-8     # no case falls under it with _joint_temporal_ref's seeds: none is re-seeded


def heap_tree(J):
    return [(j - 1) // 2 if j else -1 for j in range(J)]


def reversed_chain(J):
    """parent[j] = j + 1: every parent index is above its child's; the root is the last joint."""
    return [j + 1 if j + 1 < J else -1 for j in range(J)]


def two_roots(J):
    """A forest: joints 0 and 1 are roots, joint j >= 2 hangs under j - 2 (two chains)."""
    return [-1 if j < 2 else j - 2 for j in range(J)]


def five_roots(J):
    return [-1 if j < 5 else j - 5 for j in range(J)]


def default_tree(J):
    return list(H36M_PARENTS) if J == 17 else heap_tree(J)


def post_order(parent):
    """The processing order of the header: post-order from the roots in ascending index, children in ascending index."""
    J = len(parent)
    kids = [[c for c in range(J) if parent[c] == j] for j in range(J)]
    out = []

    def walk(j):
        for c in kids[j]:
            walk(c)
        out.append(j)

    for r in range(J):
        if parent[r] < 0:
            walk(r)
    assert len(out) == J, "not a forest"
    return out


def weights64(weight):
    """[N,J] float64: the clamp to 1e-4 .. 1 taken in fp32 (above 1 -> 1, below 1e-4 -> 1e-4, NaN stays NaN)."""
    c = np.asarray(weight, dtype=np.float32).copy()
    c[c > np.float32(1.0)] = np.float32(1.0)
    c[c < np.float32(1e-4)] = np.float32(1e-4)
    return c.astype(np.float64)


def unaries(junary, N, weight=None):
    """u [N,J,H] float64: w * junary where that product is finite, else +inf."""
    rows, J = junary.shape
    H = rows // N
    u = np.asarray(junary, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()
    if weight is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            u = weights64(weight)[:, :, None] * u
    u[~np.isfinite(u)] = np.inf
    return u


def dist3(a, b):
    """sqrt(d0^2 + d1^2 + d2^2), d = a - b: products, then the sum ascending in c."""
    d0, d1, d2 = (a[..., c] - b[..., c] for c in range(3))
    return np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)


def bone_table(Xn, g, p):
    """(b [hp, hc], mix [hp, hc], own [h]) of the bone g - p of one pose, Xn [H,J,3]."""
    own = dist3(Xn[:, g], Xn[:, p])
    mix = dist3(Xn[None, :, g], Xn[:, None, p])                   # [hp, hc]: X[hc,g] - X[hp,p]
    return np.abs(mix - 0.5 * (own[None, :] + own[:, None])), mix, own


def joint_tree_ref(junary, x, T, parent, mu, N, weight=None):
    """-> dict(joint_h [N,J] int32, cost [N] f64, bone [N,J] f64, live [N,J] bool, scale [N] f64, gap): the recurrence and the downward
    pass of the header, one pose after the other.  scale = sum_j u + mu * sum_bones (mix + own) at the kept assignment (what cost_bound
    multiplies); gap = the smallest difference between the best and the second-best candidate of any minimum taken."""
    parent = [int(v) for v in parent]
    J = len(parent)
    H = x.shape[0] // N
    u = unaries(junary, N, weight)
    X = camera_frame(x, T, N)                                      # [H,N,J,3]
    order = post_order(parent)
    hh = np.arange(H)
    joint_h, cost, bone = np.zeros((N, J), np.int32), np.full(N, np.inf), np.zeros((N, J))
    live_all, scale = np.zeros((N, J), bool), np.zeros(N)
    gap = np.inf

    def second_gap(g):
        nonlocal gap
        g = g[np.isfinite(g)]
        if g.size:
            gap = min(gap, float(g.min()))

    for n in range(N):
        Xn = X[:, n]
        S = u[n].copy()                                            # [J,H]
        live = np.isfinite(S).any(1)
        live_all[n] = live
        back = np.zeros((J, H), np.int64)
        coupled = [g for g in order if parent[g] >= 0 and live[g] and live[parent[g]]]
        for g in coupled:
            p = parent[g]
            b, _, _ = bone_table(Xn, g, p)
            cand = S[g][None, :] + mu * b                          # [hp, hc]
            back[g] = np.argmin(cand, axis=1)                      # the lowest hc that attains the minimum
            M = cand[hh, back[g]]
            if H > 1:
                cand[hh, back[g]] = np.inf
                second_gap(cand.min(axis=1) - M)
            S[p] = S[p] + M
        c, roots = 0.0, 0
        for j in range(J):                                         # ascending root index
            if live[j] and not (parent[j] >= 0 and live[parent[j]]):
                joint_h[n, j] = int(np.argmin(S[j]))
                c += S[j, joint_h[n, j]]
                roots += 1
                if H > 1:
                    second_gap(np.diff(np.partition(S[j], 1)[:2]))
        cost[n] = c if roots else np.inf
        for g in reversed(coupled):                                # parents before children
            joint_h[n, g] = back[g, joint_h[n, parent[g]]]
        sc = float(sum(u[n, j, joint_h[n, j]] for j in range(J) if live[j]))
        for g in coupled:
            b, mix, own = bone_table(Xn, g, parent[g])
            hp, hc = joint_h[n, parent[g]], joint_h[n, g]
            bone[n, g] = b[hp, hc]
            sc += mu * (mix[hp, hc] + 0.5 * (own[hc] + own[hp]))
        scale[n] = sc
    return dict(joint_h=joint_h, cost=cost, bone=bone, live=live_all, scale=scale, gap=gap)


def energy(junary, x, T, parent, mu, N, assign, weight=None):
    """[N] float64: the energy of the header for the given assignment [N,J] (dead joints and cut bones left out)."""
    J = len(parent)
    u = unaries(junary, N, weight)
    X = camera_frame(x, T, N)
    live = np.isfinite(u).any(2)
    out = np.zeros(N)
    for n in range(N):
        e = 0.0
        for j in range(J):
            if live[n, j]:
                e += u[n, j, assign[n, j]]
        for g in range(J):
            p = parent[g]
            if p >= 0 and live[n, g] and live[n, p]:
                e += mu * bone_table(X[:, n], g, p)[0][assign[n, p], assign[n, g]]
        out[n] = e
    return out


def enumerate_best(junary, x, T, parent, mu, N, weight=None):
    """(assign [N,J], energy [N]) by trying all H^J assignments of every pose (small cases only; every joint live)."""
    J = len(parent)
    H = x.shape[0] // N
    u = unaries(junary, N, weight)
    X = camera_frame(x, T, N)
    best_a, best_e = np.zeros((N, J), np.int32), np.full(N, np.inf)
    for n in range(N):
        tabs = {g: bone_table(X[:, n], g, parent[g])[0] for g in range(J) if parent[g] >= 0}
        for a in itertools.product(range(H), repeat=J):
            e = sum(u[n, j, a[j]] for j in range(J)) + mu * sum(t[a[parent[g]], a[g]] for g, t in tabs.items())
            if e < best_e[n]:
                best_e[n], best_a[n] = e, a
    return best_a, best_e


def cost_bound(J, scale):
    """What |cost - reference| and mu * |bone - reference| of a correct fp64 evaluation stay under: K_ROUND * J * 2^-53 * scale, scale = sum_j u +
    mu * sum_bones (mix + own) at the kept assignment (joint_tree_ref's `scale`: the magnitudes of the operands, not of the result - b is a
    difference of two lengths that nearly cancel).  K_ROUND counts the roundings one bone's term u + mu * |mix - 0.5 (own_c + own_p)| goes
    through, each at most 2^-53 of an operand no larger than the term's share of scale: a square root is 3 differences (X itself is exact: the
    sum of two fp32 values whose exponents are close), 3 products, 2 sums, 1 root = 9 roundings that each move the root by at most one
    relative 2^-53 -> 9 per length and three lengths (mix, own_c, own_p, the two own weighing a half each: 9 + 9 = 18 in units of the larger
    length); the sum own_c + own_p 1 (the half is exact), the difference 1, the product by mu 1, the sum with S 1, the sum into S[p] 1: 23.
    A cost is a sum of at most J such terms nested at most J deep, and every partial sum is below scale: the factor J covers the depth."""
    return K_ROUND * J * 2.0 ** -53 * np.asarray(scale)


K_ROUND = 23


def dead_joint_case():
    """case(5, 9, 3) read as 9 poses on the heap tree (1 and 2 under 0, 3 and 4 under 1): joint 1 of pose 4 has no finite unary (NaN,
    +inf, -inf), so joints 3 and 4 become roots there; pose 2 has a NaN and pose 6 a +inf in the row that would otherwise win joint 1.
    -> (x, T, u [27,5], parent, the joint)."""
    x, T, u = case(5, 9, 3)
    j = 1
    u = u.reshape(3, 9, 5).copy()
    u[:, 4, j] = [np.nan, np.inf, -np.inf]
    u[np.argmin(u[:, 2, j]), 2, j] = np.nan
    u[np.argmin(u[:, 6, j]), 6, j] = np.inf
    return x, T, u.reshape(27, 5), heap_tree(5), j


def confidences(N, J):
    """[N,J] float32 in 0 .. 1.2: both sides of the clamp at 1 occur, and three entries sit below 1e-4."""
    g = np.random.Generator(np.random.Philox(key=[77, 100 * N + J]))
    c = g.uniform(0.0, 1.2, (N, J)).astype(np.float32)
    c.reshape(-1)[:3] = [0.0, 5e-5, 1.2][:min(3, c.size)]
    return c


@functools.lru_cache(maxsize=None)
def reference(J, N, H, mu, tree="default", with_T=True, with_weight=False):
    x, T, u = case(J, N, H)
    parent = {"default": default_tree, "chain": reversed_chain, "forest": two_roots, "forest5": five_roots}[tree](J)
    return joint_tree_ref(u, x, T if with_T else None, parent, mu, N, confidences(N, J) if with_weight else None)


def mismatch(x, T, parent, N, joint_h):
    """Mean over the bones with both ends present of | assembled length - mean of the two hypotheses' lengths |, metres: the header's b at
    the given assignment, whatever produced it."""
    X = camera_frame(x, T, N)
    tot, cnt = 0.0, 0
    for n in range(N):
        for g, p in enumerate(parent):
            if p >= 0:
                tot += bone_table(X[:, n], g, p)[0][joint_h[n, p], joint_h[n, g]]
                cnt += 1
    return tot / max(cnt, 1)


def check_inputs(verbose=True):
    """On the reference alone: for every case and mu the smallest gap between the best and the second-best candidate of any minimum the
    recurrence takes is above 1e-8 - seven orders above the fp64 error of a cost, so assignments are compared exactly."""
    gaps = []
    for J, N, H in ALL_CASES:
        for mu in MUS:
            r = reference(J, N, H, mu)
            assert np.isfinite(r["cost"]).all() and ((r["joint_h"] >= 0) & (r["joint_h"] < H)).all()
            gaps.append(r["gap"])
            assert r["gap"] > GAP_MIN, (J, N, H, mu, r["gap"])
    if verbose:
        print(f"smallest best-to-second gap: {min(gaps):.3g}")
    return min(gaps)
