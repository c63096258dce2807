"""The float64 reference of the fixed-lag streaming selection (zedo_joint_stream_push, include/zedo_hip.h), stated directly in numpy on
the tables D and back of _joint_temporal_ref.joint_temporal_ref - prefix quantities of a clip, which do not depend on how its frames were
cut into pushes: frame n of a clip is decided at the horizon e = min(n + lag, the last frame of n's chain on the clip), by the lowest
arg-min of D[e,j,.] and the back pointers e .. n+1.  Also the count of frames a push emits, as the header states it, and the chunkings
the CPU and GPU tests share.  Pinned on its own by tests/test_joint_stream_ref.py (against the offline reference on truncated clips); the
GPU tests hold the kernels to it."""
import numpy as np

from _joint_temporal_ref import ALL_CASES, LAMBDAS, dead_joint_case, joint_temporal_ref, reference
from _temporal_ref import clips

LAGS = (0, 1, 3, 8)


def fixed_lag(ref_tables, seq, lag):
    """ref_tables: the dict of joint_temporal_ref on clips `seq` (D [N,J,H], back [N,J,H]) -> (path [N,J] int32, cost [N,J] float64) of
    every clip streamed with this lag and flushed at its end.  A (frame, joint) is dead where D has no finite entry."""
    D, back = ref_tables["D"], ref_tables["back"]
    N, J, _ = D.shape
    dead = ~np.isfinite(D).any(2)
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
                h = int(np.argmin(D[e, j]))                        # the lowest h that minimises D[e,j,.]
                for m in range(e, n, -1):
                    h = int(back[m, j, h])
                path[n, j], cost[n, j] = h, D[n, j, h]
    return path, cost


def emitted(t, F, lag, flush):
    """(first, count) of a push of F frames onto a clip that held t: the header's formula."""
    held = min(lag, t) + F
    return max(0, t - lag), held if flush else max(0, held - lag)


def chunkings(L):
    """The three ways the tests cut a clip of L frames: (a) one push, (b) frame by frame, (c) pushes of 1, 2, 3, .. frames."""
    c, k = [], 1
    while sum(c) < L:
        c.append(min(k, L - sum(c)))
        k += 1
    return {"whole": [L], "single": [1] * L, "growing": c}


def smallest_gap(D):
    """The smallest difference between the two smallest entries of D[n,j,.] over the live (n, j) (inf if H = 1 or nothing is live)."""
    if D.shape[2] < 2:
        return np.inf
    two = np.partition(D, 1, axis=2)[:, :, :2]
    live = np.isfinite(two[:, :, 0])
    with np.errstate(invalid="ignore"):
        g = (two[:, :, 1] - two[:, :, 0])[live]
    return float(g.min()) if g.size else np.inf


def check_inputs(verbose=True):
    """On the reference alone: the two smallest entries of D[n,j,.] at EVERY live (n, j) - any of them can be a horizon - are more than
    1e-6 apart, for every case and lambda, with and without T, and on dead_joint_case: every arg-min the streaming call adds is compared
    exactly.  -> the smallest gap."""
    gaps = []
    for J, N, H, L in ALL_CASES:
        for lam in LAMBDAS:
            for with_T in (True, False):
                g = smallest_gap(reference(J, N, H, L, lam, with_T)["D"])
                assert g > 1e-6, (J, N, H, L, lam, with_T, g)
                gaps.append(g)
    x, T, u, _ = dead_joint_case()
    dead_gap = min(smallest_gap(joint_temporal_ref(u, x, T, [0, 9], lam)["D"]) for lam in (0.0,) + LAMBDAS)
    assert dead_gap > 1e-6, dead_gap
    if verbose:
        print(f"smallest gap between the two best entries of D[n,j,.]: {min(gaps):.3g} (dead_joint_case: {dead_gap:.3g})")
    return min(gaps)


def differ_share(J, N, H, L, lam, lag):
    """Share of (frame, joint) at which the fixed-lag decision differs from the whole-clip path."""
    r = reference(J, N, H, L, lam)
    return float((fixed_lag(r, clips(N, L), lag)[0] != r["path"]).mean())
