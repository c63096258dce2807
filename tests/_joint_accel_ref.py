"""The float64 reference of the joint-wise selection with a second-order motion model (zedo_joint_accel_select, include/zedo_hip.h), stated
directly in numpy: per joint a chain over PAIRS of hypotheses, the forward recurrence, the backward pass and the re-accumulated cost in
the statement order of the header; and the inputs the CPU and GPU tests share (the generator, the camera frame, the first-order motion
term and the hand-built dead case are those of _joint_temporal_ref.py).  Pinned on its own by tests/test_joint_accel_ref.py (against the
enumeration of all paths and, at lambda_a = 0, against joint_temporal_ref); the GPU tests hold the kernels to it."""
import functools
import itertools

import numpy as np

from _joint_temporal_ref import camera_frame, case, joint_motion
from _temporal_ref import clips

# (J, N, H, L): clips are consecutive runs of L frames, the last one shorter.
CASES = [(1, 1, 1, 1), (1, 7, 2, 7), (5, 12, 3, 4), (17, 70, 50, 35), (3, 40, 64, 9), (3, 130, 7, 130), (64, 6, 5, 3), (65, 5, 3, 5)]
# the smallest shapes on both sides of the constants of csrc/zedo_joint_accel.hip that the table above does not straddle:
#   the scan deals the H^2 pairs to 256 lanes, 1, 2, 4, 7, 10, 13 or 16 pairs per lane (seven instantiations, the smallest with
#   256 KA >= H^2): 16 | 17, 22 | 23, 32 | 33, 42 | 43, 50 | 51 (50 is above), 57 | 58; the cap of the call is H = 64 (above): 63;
#   the backward pass stages min(256, 32768 / H^2) frames of back2 per run: 256 up to H = 11, 227 at H = 12 - a clip of 230 frames takes
#   one run at H = 11 and two at H = 12; a clip of 300 frames at H = 3 takes two runs of 256 (and two runs of the cost kernel, 256 frames
#   each); at H = 64 a run is 8 frames, and (3, 40, 64, 9) above has clips of 9.
BOUNDARY_CASES = [(1, 20, 16, 20), (1, 20, 17, 20), (1, 6, 22, 6), (1, 6, 23, 6), (1, 6, 32, 6), (1, 6, 33, 6), (1, 6, 42, 6), (1, 6, 43, 6),
                  (1, 5, 51, 5), (1, 5, 57, 5), (1, 5, 58, 5), (2, 9, 63, 9), (1, 230, 11, 230), (1, 230, 12, 230), (2, 300, 3, 300)]
ALL_CASES = CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}-L{L}" for J, N, H, L in ALL_CASES]
WEIGHTS = ((0.0, 30.0), (0.0, 100.0), (0.0, 300.0), (30.0, 100.0))           # (lambda_v, lambda_a)
GAP_MIN = 1e-8


def accel_term(X, n, j):
    """a[n,j,h'',h',h] as [h'', h', h] float64: sqrt(e0^2 + e1^2 + e2^2), e_c = (X[h,n,j,c] - 2 X[h',n-1,j,c]) + X[h'',n-2,j,c]; the
    squares, then their sum ascending in c."""
    g = X[None, :, n, j, :] - 2.0 * X[:, None, n - 1, j, :]                                   # [h', h, c]: formed once per pair
    e0, e1, e2 = (g[None, :, :, c] + X[:, None, None, n - 2, j, c] for c in range(3))
    return np.sqrt(e0 * e0 + e1 * e1 + e2 * e2)


def chains(dead_j, a, b):
    """The maximal runs [c0, c1) of live frames of one joint inside the clip [a, b)."""
    out, c0 = [], None
    for n in range(a, b):
        if dead_j[n]:
            if c0 is not None:
                out.append((c0, n))
            c0 = None
        elif c0 is None:
            c0 = n
    if c0 is not None:
        out.append((c0, b))
    return out


def path_cost(u, X, j, c0, p, lam_v, lam_a):
    """The cost of the path p over the chain that starts at c0, re-accumulated along it in the order of the header: u[n, j, h] as
    u[n][h]; -> the running cost of every frame."""
    out = np.empty(len(p))
    out[0] = u[c0][p[0]]
    for i in range(1, len(p)):
        n = c0 + i
        d = [X[p[i], n, j, c] - X[p[i - 1], n - 1, j, c] for c in range(3)]
        w = lam_v * np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        if i >= 2:
            e = [(X[p[i], n, j, c] - 2.0 * X[p[i - 1], n - 1, j, c]) + X[p[i - 2], n - 2, j, c] for c in range(3)]
            w = w + lam_a * np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        out[i] = out[i - 1] + (u[n][p[i]] + w)
    return out


def joint_accel_ref(junary, x, T, seq_start, lam_v, lam_a, N=None):
    """-> dict(path [N,J] int32, cost [N,J] float64, emin [N,J] float64, gap): the recurrence over pairs, the backward pass and the
    re-accumulated cost of the header, one joint after the other; emin = the smallest E of a chain's last frame, on that frame (NaN
    elsewhere); gap = the smallest difference between the best and the second-best candidate of every minimum taken - the inner minima
    over h'', the final pair of every chain, the arg-min of a one-frame chain."""
    seq = [int(v) for v in seq_start]
    N = seq[-1] if N is None else int(N)
    H, J = x.shape[0] // N, x.shape[1]
    u = np.asarray(junary, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()       # u[n, j, h]
    u[~np.isfinite(u)] = np.inf
    X = camera_frame(x, T, N)
    dead = ~np.isfinite(u).any(2)                                                             # [N, J]
    path, cost, emin = np.zeros((N, J), np.int32), np.full((N, J), np.inf), np.full((N, J), np.nan)
    gap = np.inf

    def second_gap(v):
        """v: the candidates of one or many minima along axis 0; the second-best is the minimum with the arg-min struck out."""
        nonlocal gap
        if v.shape[0] < 2:
            return
        first = np.argmin(v, axis=0)[None]
        rest = v.copy()
        np.put_along_axis(rest, first, np.inf, axis=0)
        with np.errstate(invalid="ignore"):
            g = rest.min(axis=0) - np.take_along_axis(v, first, axis=0)[0]
        g = g[np.isfinite(g)]
        if g.size:
            gap = min(gap, float(g.min()))

    for j in range(J):
        for a, b in zip(seq[:-1], seq[1:]):
            for c0, c1 in chains(dead[:, j], max(0, min(a, N)), max(0, min(b, N))):
                if c1 - c0 == 1:
                    p = [int(np.argmin(u[c0, j]))]
                    second_gap(u[c0, j])
                else:
                    back2 = {}
                    E = u[c0, j][:, None] + (u[c0 + 1, j][None, :] + lam_v * joint_motion(X, c0 + 1, j).T)      # [h', h]
                    for n in range(c0 + 2, c1):
                        with np.errstate(invalid="ignore"):
                            cand = E[:, :, None] + lam_a * accel_term(X, n, j)                # [h'', h', h]
                        back2[n] = np.argmin(cand, axis=0)                                    # the lowest h'' that attains the minimum
                        second_gap(cand)
                        best = np.take_along_axis(cand, back2[n][None], axis=0)[0]
                        E = u[n, j][None, :] + (lam_v * joint_motion(X, n, j).T + best)
                    q = int(np.argmin(E))                                                     # ties to the lowest h' H + h
                    second_gap(E.reshape(-1))
                    emin[c1 - 1, j] = E.reshape(-1)[q]
                    p = [0] * (c1 - c0)
                    p[-1], p[-2] = q % H, q // H
                    for n in range(c1 - 1, c0 + 1, -1):
                        p[n - 2 - c0] = int(back2[n][p[n - 1 - c0], p[n - c0]])
                path[c0:c1, j] = p
                cost[c0:c1, j] = path_cost(u[:, j], X, j, c0, p, lam_v, lam_a)
    return dict(path=path, cost=cost, emin=emin, gap=gap)


def brute_force(junary, x, T, L, j, lam_v, lam_a):
    """One clip of L frames (N = L) of joint j, every one of the H^L paths: -> (the smallest total, its path), the totals accumulated by
    path_cost."""
    H, J = x.shape[0] // L, x.shape[1]
    u = np.asarray(junary, dtype=np.float64).reshape(H, L, J).transpose(1, 2, 0)[:, j]        # u[n][h]
    X = camera_frame(x, T, L)
    best, arg = np.inf, None
    for p in itertools.product(range(H), repeat=L):
        t = path_cost(u, X, j, 0, p, lam_v, lam_a)[-1]
        if t < best:
            best, arg = t, p
    return best, np.array(arg, np.int32)


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam_v, lam_a, with_T=True):
    x, T, u = case(J, N, H)
    return joint_accel_ref(u, x, T if with_T else None, clips(N, L), lam_v, lam_a)


def cost_bound(L, ref_cost):
    """8 L 2^-53 relative: every term is non-negative, a frame adds at most three of them and a term carries about six roundings."""
    return 8.0 * L * 2.0 ** -53 * np.abs(ref_cost)


def moving_case(J, N, H, v):
    """case(J, N, H) with a common constant velocity of v metres per frame added to every coordinate of every hypothesis: the draws of
    _joint_temporal_ref.case repeated in float64, n v added there, ONE rounding to float32 (v = 0 returns the bits of case()).
    -> (x, T, u)."""
    g = np.random.Generator(np.random.Philox(key=[93, 1000 * J + 10 * N + H]))
    cl = 0.03 * g.standard_normal((H, 1, J, 3))
    walk = np.cumsum(0.01 * g.standard_normal((1, N, J, 3)), axis=1)
    x64 = cl + walk + 0.01 * g.standard_normal((H, N, J, 3))
    x = (x64 + v * np.arange(N)[None, :, None, None]).astype(np.float32)
    _, T, u = case(J, N, H)
    return np.ascontiguousarray(x.reshape(H * N, J, 3)), T, u


def check_inputs(verbose=True):
    """On the reference alone: for every case and weight pair the smallest gap between the best and the second-best candidate of any
    minimum taken is above 1e-8 - five orders above the fp64 error of a cost of a few hundred, so paths are compared exactly."""
    gaps = []
    for J, N, H, L in ALL_CASES:
        for lam_v, lam_a in WEIGHTS:
            r = reference(J, N, H, L, lam_v, lam_a)
            assert np.isfinite(r["cost"]).all() and ((r["path"] >= 0) & (r["path"] < H)).all()
            gaps.append(r["gap"])
            assert r["gap"] > GAP_MIN, (J, N, H, L, lam_v, lam_a, r["gap"])
        if verbose:
            print(f"J={J} N={N} H={H} L={L}: smallest gap {min(gaps[-len(WEIGHTS):]):.3g}")
    if verbose:
        print(f"smallest best-to-second gap: {min(gaps):.3g}")
    return min(gaps)
