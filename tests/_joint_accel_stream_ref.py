"""The float64 reference of the fixed-lag streaming selection under the second-order motion model (zedo_joint_accel_stream_push,
include/zedo_hip.h), stated directly in numpy: ONE forward pass of the chain over pairs per case, which keeps per (frame, joint) the lowest
arg-min pair of E[n], its value and back2[n] - prefix quantities of a clip, which do not depend on how its frames were cut into pushes -
and the decision read off them as the header states it: frame n is decided at the horizon e = min(n + lag, the last frame of n's chain on
the clip), by the pair kept there and the bytes back2[e] .. back2[n+2]; the cost is min E[e].  The statements of E and back2 are those of
_joint_accel_ref.joint_accel_ref.  Pinned on its own by tests/test_joint_accel_stream_ref.py (against joint_accel_ref on every truncation
of every clip); the GPU tests hold the kernels to it."""
import functools

import numpy as np

from _joint_accel_ref import GAP_MIN, accel_term, chains
from _joint_stream_ref import chunkings, emitted  # noqa: F401  (re-exported: the tests of this stream cut and count as the hard stream's)
from _joint_temporal_ref import camera_frame, case, dead_joint_case, joint_motion  # noqa: F401
from _temporal_ref import clips

LAGS = (0, 1, 2, 3, 8)                                             # lag 2 is the first that reads back2
WEIGHTS = ((0.0, 100.0), (30.0, 100.0))                            # (lambda_v, lambda_a)
# every (J, N, H, L) tests/test_joint_accel_stream_gpu.py compares exactly against this reference, at both weight pairs: the smallest
# shapes on both sides of the seven pair dealings of the scan (H = 16 | 17, 22 | 23, 32 | 33, 42 | 43, 50 | 51, 57 | 58, 63 | 64), of
# J = 64 | 65, the smallest clips, and a clip that wraps a short ring many times; BIG, the shape of the timings, at BIG_WEIGHTS alone
GPU_CASES = [(1, 1, 1, 1), (1, 7, 2, 7), (5, 12, 3, 4), (1, 20, 16, 20), (1, 20, 17, 20), (1, 6, 22, 6), (1, 6, 23, 6), (1, 6, 32, 6),
             (1, 6, 33, 6), (1, 6, 42, 6), (1, 6, 43, 6), (1, 5, 50, 5), (1, 5, 51, 5), (1, 5, 57, 5), (1, 5, 58, 5), (2, 9, 63, 9),
             (3, 40, 64, 9), (64, 6, 5, 3), (65, 5, 3, 5), (3, 130, 7, 130)]
BIG, BIG_WEIGHTS = (17, 70, 50, 35), (30.0, 100.0)


def two_smallest_gap(v):
    """The difference between the two smallest entries of v (inf if it has fewer than two finite ones)."""
    v = np.sort(v.reshape(-1)[np.isfinite(v.reshape(-1))])
    return float(v[1] - v[0]) if v.size > 1 else np.inf


def forward(junary, x, T, seq_start, lam_v, lam_a, N=None):
    """-> dict(dead [N,J] bool, start [N,J] bool (the first frame of a chain), argq [N,J] int (the lowest arg-min pair h' H + h of E[n];
    at a chain's first frame the lowest arg-min h of u), argv [N,J] (that minimum; +inf where dead), back2 {(n, j): [h', h] int}, gap:
    the smallest distance between the two smallest entries of E[n] (of u at a chain's first frame) over every live (n, j))."""
    seq = [int(v) for v in seq_start]
    N = seq[-1] if N is None else int(N)
    H, J = x.shape[0] // N, x.shape[1]
    u = np.asarray(junary, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()       # u[n, j, h]
    u[~np.isfinite(u)] = np.inf
    X = camera_frame(x, T, N)
    dead = ~np.isfinite(u).any(2)
    start = np.zeros((N, J), bool)
    argq, argv, back2, gap = np.zeros((N, J), np.int64), np.full((N, J), np.inf), {}, np.inf
    for j in range(J):
        for a, b in zip(seq[:-1], seq[1:]):
            for c0, c1 in chains(dead[:, j], max(0, min(a, N)), max(0, min(b, N))):
                start[c0, j] = True
                argq[c0, j], argv[c0, j] = int(np.argmin(u[c0, j])), u[c0, j].min()
                gap = min(gap, two_smallest_gap(u[c0, j]))
                E = None
                for n in range(c0 + 1, c1):
                    if n == c0 + 1:
                        E = u[c0, j][:, None] + (u[n, j][None, :] + lam_v * joint_motion(X, n, j).T)            # [h', h]
                    else:
                        with np.errstate(invalid="ignore"):
                            cand = E[:, :, None] + lam_a * accel_term(X, n, j)                # [h'', h', h]
                        back2[n, j] = np.argmin(cand, axis=0)                                 # the lowest h'' that attains the minimum
                        best = np.take_along_axis(cand, back2[n, j][None], axis=0)[0]
                        E = u[n, j][None, :] + (lam_v * joint_motion(X, n, j).T + best)
                    argq[n, j], argv[n, j] = int(np.argmin(E)), E.min()                       # ties to the lowest h' H + h
                    gap = min(gap, two_smallest_gap(E))
    return dict(dead=dead, start=start, argq=argq, argv=argv, back2=back2, gap=gap, H=H)


def fixed_lag(tab, seq, lag):
    """tab: forward() on the clips `seq` -> (path [N,J] int32, cost [N,J] float64) of every clip streamed with this lag and flushed at
    its end; a dead (frame, joint): 0 and +inf."""
    dead, start, argq, argv, back2, H = (tab[k] for k in ("dead", "start", "argq", "argv", "back2", "H"))
    N, J = dead.shape
    path, cost = np.zeros((N, J), np.int32), np.full((N, J), np.inf)
    seq = [int(v) for v in seq]
    for a, b in zip(seq[:-1], seq[1:]):
        for j in range(J):
            for n in range(a, b):
                if dead[n, j]:
                    continue
                c = n                                              # c_j(n): the first m >= n whose successor is dead or absent
                while c + 1 < b and not dead[c + 1, j]:
                    c += 1
                e = min(n + lag, c)
                cost[n, j] = argv[e, j]
                if e == n and start[n, j]:                         # a chain of one frame so far
                    path[n, j] = argq[e, j]
                    continue
                p = {e - 1: int(argq[e, j]) // H, e: int(argq[e, j]) % H}
                for m in range(e, n + 1, -1):
                    p[m - 2] = int(back2[m, j][p[m - 1], p[m]])
                path[n, j] = p[n]
    return path, cost


@functools.lru_cache(maxsize=None)
def tables(J, N, H, L, lam_v, lam_a, with_T=True):
    x, T, u = case(J, N, H)
    return forward(u, x, T if with_T else None, clips(N, L), lam_v, lam_a)


@functools.lru_cache(maxsize=None)
def dead_tables(lam_v, lam_a):
    x, T, u, _ = dead_joint_case()
    return forward(u, x, T, [0, 9], lam_v, lam_a)


def check_gaps(cases, weights=WEIGHTS, verbose=True):
    """On the reference alone: at every live (n, j) of every case and weight pair - any of them can be a horizon - the two smallest
    entries of E[n] (of u at a chain's first frame) are more than GAP_MIN apart, and so on dead_joint_case.  -> the smallest gap."""
    gaps = []
    for J, N, H, L in cases:
        for lam_v, lam_a in weights:
            g = tables(J, N, H, L, lam_v, lam_a)["gap"]
            assert g > GAP_MIN, (J, N, H, L, lam_v, lam_a, g)
            gaps.append(g)
            if verbose:
                print(f"J={J} N={N} H={H} L={L} ({lam_v:g}, {lam_a:g}): smallest gap at a horizon {g:.3g}")
    for lam_v, lam_a in weights:
        g = dead_tables(lam_v, lam_a)["gap"]
        assert g > GAP_MIN, ("dead_joint_case", lam_v, lam_a, g)
        gaps.append(g)
    return min(gaps)


def differ_share(J, N, H, L, lam_v, lam_a, lag):
    """Share of (frame, joint) at which the fixed-lag decision differs from the whole-clip path (lag >= L - 1)."""
    t, seq = tables(J, N, H, L, lam_v, lam_a), clips(N, L)
    return float((fixed_lag(t, seq, lag)[0] != fixed_lag(t, seq, L - 1)[0]).mean())
