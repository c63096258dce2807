"""The float64 reference of the temporal selection (zedo_temporal_select, include/zedo_hip.h), stated directly in numpy: the motion term,
the forward recurrence and the backward pass exactly as the header words them, a brute-force enumeration of all H^L paths of one clip,
and the inputs the CPU and GPU tests share.  Pinned on its own by tests/test_temporal_ref.py; the GPU tests hold the kernels to it."""
import functools
import itertools

import numpy as np

# (J, N, H, L): clips are consecutive runs of L frames, the last one shorter.  H on both sides of one and two waves (50, 64, 65, 130), a
# short last clip (70 frames in clips of 9, 130 in clips of 50), a clip longer than a run of the backward pass's LDS staging (300), J != 17.
CASES = [(1, 1, 1, 1), (1, 7, 2, 7), (5, 12, 3, 4), (17, 64, 5, 64), (17, 70, 50, 35), (17, 70, 64, 9), (21, 40, 65, 40), (17, 300, 7, 300),
         (17, 130, 130, 50)]
# more hypotheses than the scan kernel keeps in the LDS at once (TS_CAP = 1024), where D[n-1,.] is walked in pieces
EXTRA_CASES = [(1, 3, 1030, 3)]
# the smallest shapes on the far side of the constants of csrc/zedo_temporal.hip that CASES and EXTRA_CASES stay below:
#   TT_J = 32 joints per staged piece: 33 (a second piece, one joint long), 64 (two full pieces; H = 17 also crosses the TT_P = 16 tile of
#   h') and 65 (three pieces);  256 < H <= TS_CAP: H = 300, a lane of the resident scan owns two h and its prefetch serves the first only,
#   clips of 13 frames end inside the backward pass's runs;  TB_INTS = 8192 ints of staged back rows: H = 4097 stages one frame per run,
#   H = 8193 walks the table in memory (one frame of transition costs is 537 MB).
BOUNDARY_CASES = [(33, 9, 5, 9), (64, 6, 17, 3), (65, 5, 3, 5), (17, 40, 300, 13), (1, 4, 4097, 2), (1, 3, 8193, 3)]
# check_inputs() holds them to the same conditions as the others; with the draws of case() as they are the smallest gap between the best
# and the second-best candidate over the three lambdas is 6.6e-6 (H = 300), 4.7e-6 (H = 4097) and 1.3e-5 (H = 8193): no other seed needed.
ALL_CASES = CASES + EXTRA_CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}-L{L}" for J, N, H, L in ALL_CASES]
LAMBDAS = (30.0, 100.0, 300.0)
REF_BLOCK = 1 << 19                                            # elements of the candidate block the reference holds at a time


def clips(N, L):
    """seq_start of consecutive clips of L frames, the last one shorter."""
    return list(range(0, N, L)) + [N]


@functools.lru_cache(maxsize=None)
def case(J, N, H):
    """-> (x [H N,J,3] float32 rows (h, n), u [H N] float64): H hypotheses that differ by a fixed offset of 3 cm per coordinate, a shared
    random walk of 1 cm per frame, 1 cm of independent noise per (hypothesis, frame); unrelated unaries in 0.5 .. 8.  Read-only."""
    g = np.random.Generator(np.random.Philox(key=[91, 1000 * J + 10 * N + H]))
    cl = 0.03 * g.standard_normal((H, 1, J, 3))
    walk = np.cumsum(0.01 * g.standard_normal((1, N, J, 3)), axis=1)
    x = (cl + walk + 0.01 * g.standard_normal((H, N, J, 3))).astype(np.float32)
    u = g.uniform(0.5, 8.0, (H, N))
    out = (np.ascontiguousarray(x.reshape(H * N, J, 3)), np.ascontiguousarray(u.reshape(H * N)))
    for a in out:
        a.setflags(write=False)
    return out


def dead_frame_case():
    """H = 3, one clip of 9 frames: frame 4 has no finite unary (NaN, +inf, -inf), frame 2 has a NaN and frame 6 a +inf in the row that
    would otherwise win.  -> (x [27,5,3], u [27])."""
    x, u = case(5, 9, 3)
    u = u.reshape(3, 9).copy()
    u[:, 4] = [np.nan, np.inf, -np.inf]
    u[np.argmin(u[:, 2]), 2] = np.nan
    u[np.argmin(u[:, 6]), 6] = np.inf
    return x, u.reshape(-1)


def motion_block(x4, n, h0, h1):
    """x4 [H,N,J,3] float64 -> [h1 - h0, H'] float64: m[n, h', h] for h in h0 .. h1-1, h-major (the candidates of one h are contiguous).
    (1/J) sum_j sqrt(sum_c (x[h,n,j,c] - x[h',n-1,j,c])^2), the sums ascending in c, then in j."""
    J = x4.shape[2]
    acc = np.zeros((h1 - h0, x4.shape[0]))
    for j in range(J):
        d0, d1, d2 = (x4[h0:h1, None, n, j, c] - x4[None, :, n - 1, j, c] for c in range(3))
        acc = acc + np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
    return acc / J


def motion_ref(x, N, n):
    """m[n] [H', H] float64, all of it at once."""
    H, J = x.shape[0] // N, x.shape[1]
    return motion_block(np.asarray(x, dtype=np.float64).reshape(H, N, J, 3), n, 0, H).T


def temporal_ref(unary, x, seq_start, lam, N=None):
    """-> dict(path [N] int32, cost [N] float64, D [N,H], back [N,H], gap): the recurrence and the backward pass of the header; gap = the
    smallest difference between the best and the second-best predecessor cost over all (n, h) and between the two best final costs."""
    seq = [int(v) for v in seq_start]
    N = seq[-1] if N is None else int(N)
    H = len(unary) // N
    u = np.asarray(unary, dtype=np.float64).reshape(H, N).T.copy()                         # u[n, h]
    u[~np.isfinite(u)] = np.inf
    x4 = np.asarray(x, dtype=np.float64).reshape(H, N, x.shape[1], 3)
    dead = ~np.isfinite(u).any(1)
    D, back = np.full((N, H), np.inf), np.full((N, H), -1, np.int32)
    path, cost = np.zeros(N, np.int32), np.full(N, np.inf)
    gap = np.inf

    def second_gap(g):
        nonlocal gap
        g = g[np.isfinite(g)]
        if g.size:
            gap = min(gap, float(g.min()))

    for a, b in zip(seq[:-1], seq[1:]):
        for n in range(a, b):
            if dead[n]:
                continue
            if n == a or dead[n - 1]:
                D[n] = u[n]
                continue
            # blocks of hypotheses h, so that 8193 of them need no H x H x 3 array: every element is computed as it would be at once
            step = max(1, REF_BLOCK // H)
            for h0 in range(0, H, step):
                h1 = min(H, h0 + step)
                k = np.arange(h1 - h0)
                with np.errstate(invalid="ignore"):
                    cand = D[n - 1][None, :] + lam * motion_block(x4, n, h0, h1)           # [h, h']
                back[n, h0:h1] = np.argmin(cand, axis=1)                                   # the lowest h' that attains the minimum
                first = cand[k, back[n, h0:h1]]
                D[n, h0:h1] = u[n, h0:h1] + first
                if H > 1:
                    cand[k, back[n, h0:h1]] = np.inf
                    with np.errstate(invalid="ignore"):
                        second_gap(cand.min(axis=1) - first)
        have = False
        for n in range(b - 1, a - 1, -1):
            if dead[n]:
                have = False
                continue
            if have:
                path[n] = back[n + 1, path[n + 1]]
            else:
                path[n] = int(np.argmin(D[n]))
                if H > 1:
                    with np.errstate(invalid="ignore"):
                        second_gap(np.diff(np.partition(D[n], 1)[:2]))
            cost[n] = D[n, path[n]]
            have = True
    return dict(path=path, cost=cost, D=D, back=back, gap=gap)


def brute_force(unary, x, L, lam):
    """One clip of L frames (N = L), every one of the H^L paths: -> (the smallest total, its path).  total = sum_n u[n, p_n] +
    lam sum_{n>=1} m[n, p_{n-1}, p_n], added in ascending n as the recurrence adds them."""
    H = len(unary) // L
    u = np.asarray(unary, dtype=np.float64).reshape(H, L).T
    m = [None] + [motion_ref(x, L, n) for n in range(1, L)]
    best, arg = np.inf, None
    for p in itertools.product(range(H), repeat=L):
        t = u[0, p[0]]
        for n in range(1, L):
            t = u[n, p[n]] + (t + lam * m[n][p[n - 1], p[n]])
        if t < best:
            best, arg = t, p
    return best, np.array(arg, np.int32)


def switch_rate(path, seq_start):
    """Share of the frame transitions inside clips at which the path changes hypothesis (nan when there is no transition)."""
    seq = [int(v) for v in seq_start]
    ch = tot = 0
    for a, b in zip(seq[:-1], seq[1:]):
        ch += int((path[a + 1:b] != path[a:b - 1]).sum())
        tot += max(0, b - a - 1)
    return ch / tot if tot else float("nan")


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam):
    x, u = case(J, N, H)
    return temporal_ref(u, x, clips(N, L), lam)


def cost_bound(J, L, ref_cost):
    """An fp64 evaluation of the recurrence differs from another by at most about 4 L (J + 4) 2^-53 relative: per frame J square roots of
    three-term sums, their sum, one product and two additions, over at most L frames of a clip."""
    return 4.0 * L * (J + 4) * 2.0 ** -53 * np.abs(ref_cost)


def check_inputs(verbose=True):
    """On the reference alone: for every case and lambda the smallest gap between the best and the second-best candidate of any minimum
    the recurrence takes is above 1e-6 - six orders above the fp64 error of a cost, so paths are compared exactly; and, at lambda = 100
    for every case with H >= 5, the selection is not the per-frame one: the path differs from the per-frame arg-min on more than 25 %
    of the frames, switches hypothesis at more than 5 % of the transitions, and at fewer than with lambda = 0."""
    gaps = []
    for J, N, H, L in ALL_CASES:
        x, u = case(J, N, H)
        seq = clips(N, L)
        for lam in LAMBDAS:
            r = reference(J, N, H, L, lam)
            assert np.isfinite(r["cost"]).all() and ((r["path"] >= 0) & (r["path"] < H)).all()
            gaps.append(r["gap"])
            assert r["gap"] > 1e-6, (J, N, H, L, lam, r["gap"])
        if H >= 5 and (J, N, H, L) in CASES:
            p100, p0 = reference(J, N, H, L, 100.0)["path"], temporal_ref(u, x, seq, 0.0)["path"]
            per_frame = np.argmin(u.reshape(H, N), axis=0)
            differ, sw, sw0 = float((p100 != per_frame).mean()), switch_rate(p100, seq), switch_rate(p0, seq)
            if verbose:
                print(f"J={J} N={N} H={H} L={L}: lambda 100 differs from the per-frame arg-min on {100 * differ:.0f} % of frames, switches at "
                      f"{100 * sw:.0f} % of transitions (lambda 0: {100 * sw0:.0f} %)")
            assert differ > 0.25 and sw > 0.05 and sw < sw0
    if verbose:
        print(f"smallest best-to-second gap: {min(gaps):.3g}")
