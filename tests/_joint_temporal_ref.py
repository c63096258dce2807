"""The float64 reference of the joint-wise temporal selection (zedo_joint_temporal_select, include/zedo_hip.h), stated directly in numpy:
per joint the camera-frame positions X = x + T, the motion term of one joint, the forward recurrence and the backward pass exactly as the
header words them; and the inputs the CPU and GPU tests share.  Pinned on its own by tests/test_joint_temporal_ref.py (against
_temporal_ref.temporal_ref on one-joint slices and against the enumeration of all paths); the GPU tests hold the kernels to it."""
import functools

import numpy as np

from _temporal_ref import clips, switch_rate

# (J, N, H, L): clips are consecutive runs of L frames, the last one shorter.
CASES = [(1, 1, 1, 1), (1, 7, 2, 7), (5, 12, 3, 4), (17, 70, 50, 35), (17, 40, 64, 9), (21, 20, 65, 20), (3, 130, 7, 130), (2, 30, 130, 13),
         (64, 6, 5, 3), (65, 5, 3, 5), (1, 6, 300, 3), (1, 3, 1024, 3)]
# the smallest shapes on both sides of the constants of csrc/zedo_joint_temporal.hip that the table above does not straddle:
#   the scan splits the h' over 4 parts of the workgroup up to H = 64 (64 | 65 are above), over 2 up to H = 128: 128 | 129;
#   above that a lane owns 1, 2 or 4 hypotheses h = t, t + 256, .. (three instantiations): 256 | 257 and 512 | 513;
#   the backward pass stages min(256, 8192 / H) frames of the back table per run: a clip of 300 frames at H = 3 takes two runs (every
#   clip above fits into one), and at H = 1024 a run is 8 frames: a clip of 9.
BOUNDARY_CASES = [(1, 4, 128, 2), (1, 4, 129, 4), (1, 3, 256, 3), (1, 3, 257, 3), (1, 3, 512, 3), (1, 3, 513, 3), (2, 300, 3, 300), (1, 9, 1024, 9)]
ALL_CASES = CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}-L{L}" for J, N, H, L in ALL_CASES]
LAMBDAS = (30.0, 100.0, 300.0)
# the cases check_inputs() holds to "not the per-frame selection"
SMOOTHING_CASES = [(17, 70, 50, 35), (17, 40, 64, 9), (21, 20, 65, 20), (3, 130, 7, 130), (2, 30, 130, 13)]
SEED = {}                                                      # (J, N, H) -> first key word, for a boundary case whose gap falls under 1e-6


@functools.lru_cache(maxsize=None)
def case(J, N, H):
    """-> (x [H N,J,3] float32, T [H N,3] float32, u [H N,J] float64), rows (h, n): H hypotheses that differ by a fixed offset of 3 cm per
    coordinate, a shared random walk of 1 cm per frame, 1 cm of independent noise; translations about (0.1, -0.2, 4) m that differ by 5 cm
    per hypothesis, walk 1 cm per frame and carry 5 mm of noise; unrelated unaries in 0.5 .. 8.  Read-only."""
    g = np.random.Generator(np.random.Philox(key=[SEED.get((J, N, H), 93), 1000 * J + 10 * N + H]))
    cl = 0.03 * g.standard_normal((H, 1, J, 3))
    walk = np.cumsum(0.01 * g.standard_normal((1, N, J, 3)), axis=1)
    x = (cl + walk + 0.01 * g.standard_normal((H, N, J, 3))).astype(np.float32)
    T = (np.array([0.1, -0.2, 4.0]) + 0.05 * g.standard_normal((H, 1, 3))
         + np.cumsum(0.01 * g.standard_normal((1, N, 3)), axis=1)
         + 0.005 * g.standard_normal((H, N, 3))).astype(np.float32)
    u = g.uniform(0.5, 8.0, (H, N, J))          # draws in exactly this order
    out = (np.ascontiguousarray(x.reshape(H * N, J, 3)), np.ascontiguousarray(T.reshape(H * N, 3)), np.ascontiguousarray(u.reshape(H * N, J)))
    for a in out:
        a.setflags(write=False)
    return out


def dead_joint_case():
    """_temporal_ref.dead_frame_case on joint 2 of 5 (H = 3, one clip of 9 frames): (frame 4, joint 2) has no finite unary (NaN, +inf,
    -inf), frame 2 has a NaN and frame 6 a +inf in the row that would otherwise win that joint; the other joints are untouched.
    -> (x [27,5,3], T [27,3], u [27,5], the joint)."""
    x, T, u = case(5, 9, 3)
    j = 2
    u = u.reshape(3, 9, 5).copy()
    u[:, 4, j] = [np.nan, np.inf, -np.inf]
    u[np.argmin(u[:, 2, j]), 2, j] = np.nan
    u[np.argmin(u[:, 6, j]), 6, j] = np.inf
    return x, T, u.reshape(27, 5), j


def camera_frame(x, T, N):
    """X [H,N,J,3] float64 = (double)x + (double)T (T None: x alone)."""
    H, J = x.shape[0] // N, x.shape[1]
    X = np.asarray(x, dtype=np.float64).reshape(H, N, J, 3)
    if T is not None:
        X = X + np.asarray(T, dtype=np.float64).reshape(H, N, 1, 3)
    return X


def joint_motion(X, n, j):
    """m[n,j,h',h] as [h, h'] float64: sqrt(d0^2 + d1^2 + d2^2), d_c = X[h,n,j,c] - X[h',n-1,j,c]; products, then the sum ascending in c."""
    d0, d1, d2 = (X[:, None, n, j, c] - X[None, :, n - 1, j, c] for c in range(3))
    return np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)


def joint_temporal_ref(junary, x, T, seq_start, lam, N=None):
    """-> dict(path [N,J] int32, cost [N,J] float64, D [N,J,H], back [N,J,H], gap): the recurrence and the backward pass of the header,
    one joint after the other; gap = the smallest difference between the best and the second-best predecessor cost over all (n, j, h) and
    between the two best final costs of any chain."""
    seq = [int(v) for v in seq_start]
    N = seq[-1] if N is None else int(N)
    H, J = x.shape[0] // N, x.shape[1]
    u = np.asarray(junary, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()       # u[n, j, h]
    u[~np.isfinite(u)] = np.inf
    X = camera_frame(x, T, N)
    dead = ~np.isfinite(u).any(2)                                                             # [N, J]
    D, back = np.full((N, J, H), np.inf), np.full((N, J, H), -1, np.int32)
    path, cost = np.zeros((N, J), np.int32), np.full((N, J), np.inf)
    gap = np.inf
    k = np.arange(H)

    def second_gap(g):
        nonlocal gap
        g = g[np.isfinite(g)]
        if g.size:
            gap = min(gap, float(g.min()))

    for j in range(J):
        for a, b in zip(seq[:-1], seq[1:]):
            for n in range(a, b):
                if dead[n, j]:
                    continue
                if n == a or dead[n - 1, j]:
                    D[n, j] = u[n, j]
                    continue
                with np.errstate(invalid="ignore"):
                    cand = D[n - 1, j][None, :] + lam * joint_motion(X, n, j)                 # [h, h']
                back[n, j] = np.argmin(cand, axis=1)                                          # the lowest h' that attains the minimum
                first = cand[k, back[n, j]]
                D[n, j] = u[n, j] + first
                if H > 1:
                    cand[k, back[n, j]] = np.inf
                    with np.errstate(invalid="ignore"):
                        second_gap(cand.min(axis=1) - first)
            have = False
            for n in range(b - 1, a - 1, -1):
                if dead[n, j]:
                    have = False
                    continue
                if have:
                    path[n, j] = back[n + 1, j, path[n + 1, j]]
                else:
                    path[n, j] = int(np.argmin(D[n, j]))
                    if H > 1:
                        with np.errstate(invalid="ignore"):
                            second_gap(np.diff(np.partition(D[n, j], 1)[:2]))
                cost[n, j] = D[n, j, path[n, j]]
                have = True
    return dict(path=path, cost=cost, D=D, back=back, gap=gap)


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam, with_T=True):
    x, T, u = case(J, N, H)
    return joint_temporal_ref(u, x, T if with_T else None, clips(N, L), lam)


def per_frame_argmin(u, N):
    """[N,J] int32: per (frame, joint) the lowest hypothesis with the smallest finite unary - what lambda = 0 and clips of one frame keep."""
    H, J = u.shape[0] // N, u.shape[1]
    v = np.asarray(u, dtype=np.float64).reshape(H, N, J).copy()
    v[~np.isfinite(v)] = np.inf
    return np.argmin(v, axis=0).astype(np.int32)


def check_inputs(verbose=True):
    """On the reference alone: for every case and lambda the smallest gap between the best and the second-best candidate of any minimum
    the recurrence takes is above 1e-6 - nine orders above the fp64 error of a cost, so paths are compared exactly; and, at lambda = 100
    for SMOOTHING_CASES, averaged over the joints, the selection is not the per-frame one: the paths differ from the per-frame joint
    arg-min on more than 25 % of the frames and switch hypothesis at fewer transitions than with lambda = 0."""
    gaps = []
    for J, N, H, L in ALL_CASES:
        x, T, u = case(J, N, H)
        seq = clips(N, L)
        for lam in LAMBDAS:
            r = reference(J, N, H, L, lam)
            assert np.isfinite(r["cost"]).all() and ((r["path"] >= 0) & (r["path"] < H)).all()
            gaps.append(r["gap"])
            assert r["gap"] > 1e-6, (J, N, H, L, lam, r["gap"])
        if (J, N, H, L) in SMOOTHING_CASES:
            p100, p0 = reference(J, N, H, L, 100.0)["path"], joint_temporal_ref(u, x, T, seq, 0.0)["path"]
            differ = float((p100 != per_frame_argmin(u, N)).mean())
            sw = float(np.mean([switch_rate(p100[:, j], seq) for j in range(J)]))
            sw0 = float(np.mean([switch_rate(p0[:, j], seq) for j in range(J)]))
            if verbose:
                print(f"J={J} N={N} H={H} L={L}: lambda 100 differs from the per-frame joint arg-min on {100 * differ:.0f} % of (frame, joint), "
                      f"switches at {100 * sw:.0f} % of transitions (lambda 0: {100 * sw0:.0f} %)")
            assert differ > 0.25 and sw < sw0
    if verbose:
        print(f"smallest best-to-second gap: {min(gaps):.3g}")
    return min(gaps)

