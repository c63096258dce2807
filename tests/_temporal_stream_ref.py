"""The float64 reference of the fixed-lag pose-level streaming selection (zedo_temporal_stream_push, include/zedo_hip.h), stated directly
in numpy on the tables D and back of _temporal_ref.temporal_ref - prefix quantities of a clip, which do not depend on how its frames were
cut into pushes: frame n of a clip is decided at the horizon e = min(n + lag, the last frame of n's chain on the clip), by the lowest
arg-min of D[e,.] and the back pointers e .. n+1.  The count of frames a push emits and the chunkings are those of
tests/_joint_stream_ref.py (emitted, chunkings): the header gives both calls one formula.  Pinned on its own by
tests/test_temporal_stream_ref.py (against the offline reference on truncated clips); the GPU tests hold the kernels to it."""
import numpy as np

from _temporal_ref import BOUNDARY_CASES, CASES, LAMBDAS, clips, dead_frame_case, reference, switch_rate, temporal_ref

LAGS = (0, 1, 3, 8)
# the shapes the streaming call accepts (H <= 1024: the resident scan only) among those of tests/_temporal_ref.py; REFUSED is the other side
STREAM_CASES = CASES + [c for c in BOUNDARY_CASES if c[2] <= 1024]
STREAM_IDS = [f"J{J}-N{N}-H{H}-L{L}" for J, N, H, L in STREAM_CASES]
REFUSED = (1, 3, 1030, 3)


def fixed_lag(ref_tables, seq, lag):
    """ref_tables: the dict of temporal_ref on clips `seq` (D [N,H], back [N,H]) -> (path [N] int32, cost [N] float64) of every clip
    streamed with this lag and flushed at its end.  A frame is dead where D has no finite entry."""
    D, back = ref_tables["D"], ref_tables["back"]
    N = D.shape[0]
    dead = ~np.isfinite(D).any(1)
    path, cost = np.zeros(N, np.int32), np.full(N, np.inf)
    seq = [int(v) for v in seq]
    for a, b in zip(seq[:-1], seq[1:]):
        for n in range(a, b):
            if dead[n]:
                continue
            c = n                                                  # c(n): the first m >= n whose successor is dead or absent
            while c + 1 < b and not dead[c + 1]:
                c += 1
            e = min(n + lag, c)
            h = int(np.argmin(D[e]))                               # the lowest h that minimises D[e,.]
            for m in range(e, n, -1):
                h = int(back[m, h])
            path[n], cost[n] = h, D[n, h]
    return path, cost


def smallest_gap(D):
    """The smallest difference between the two smallest entries of D[n,.] over the live frames (inf if H = 1 or nothing is live)."""
    if D.shape[1] < 2:
        return np.inf
    two = np.partition(D, 1, axis=1)[:, :2]
    live = np.isfinite(two[:, 0])
    with np.errstate(invalid="ignore"):
        g = (two[:, 1] - two[:, 0])[live]                          # (+inf where one entry alone is finite)
    return float(g.min()) if g.size else np.inf


def check_inputs(verbose=True):
    """On the reference alone, for every STREAM_CASE and lambda and on dead_frame_case: the two smallest entries of D[n,.] at EVERY live
    frame - any of them can be a horizon - and the two best candidates of every minimum the recurrence takes (temporal_ref's gap) are
    more than 1e-8 apart, seven orders above the fp64 error of a cost: every arg-min is compared exactly, none is left out.
    -> (the smallest gap of D, the smallest gap of a minimum)."""
    dgap, mgap = [], []
    for J, N, H, L in STREAM_CASES:
        for lam in LAMBDAS:
            r = reference(J, N, H, L, lam)
            dgap.append(smallest_gap(r["D"]))
            mgap.append(r["gap"])
            assert dgap[-1] > 1e-8 and mgap[-1] > 1e-8, (J, N, H, L, lam, dgap[-1], mgap[-1])
    x, u = dead_frame_case()
    for lam in (0.0,) + LAMBDAS:
        r = temporal_ref(u, x, [0, 9], lam)
        assert smallest_gap(r["D"]) > 1e-8 and r["gap"] > 1e-8, (lam, smallest_gap(r["D"]), r["gap"])
    if verbose:
        print(f"smallest gap between the two best entries of D[n,.]: {min(dgap):.3g}; between the two best candidates of a minimum: "
              f"{min(mgap):.3g}")
    return min(dgap), min(mgap)


def lag_table(J, N, H, L, lam, lags):
    """{lag: (share of frames at which the fixed-lag decision differs from the whole-clip path, its switch rate)}"""
    r, seq = reference(J, N, H, L, lam), clips(N, L)
    out = {}
    for lag in lags:
        p = fixed_lag(r, seq, lag)[0]
        out[lag] = (float((p != r["path"]).mean()), switch_rate(p, seq))
    return out
