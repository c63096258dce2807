"""The float64 reference of the pose-level fusion along a video (zedo_temporal_marginal, include/zedo_hip.h), stated directly in numpy: the
forward and the backward recurrence in the log domain over whole hypotheses, the marginals, the posterior mean pose, every joint's
covariance from centred differences and the arg-max exactly as the header words them, every sum ascending in h; the enumeration of all
H^L paths of one clip; and beta, the bound on a log-marginal the GPU test holds the kernels to.  The inputs are those of _temporal_ref
(case, clips, dead_frame_case, motion_ref) plus a translation per (hypothesis, frame); the log-sum-exp, the bounds that follow from beta
and the one place the outputs are held to a reference are _joint_marginal_ref's.  Pinned on its own by tests/test_temporal_marginal_ref.py."""
import functools
import itertools

import numpy as np

from _joint_marginal_ref import cov_bound, hold_marginals, lse_ascending, mean_bound, softmax_bound, softmax_ref  # noqa: F401  (re-exported)
from _joint_marginal_ref import asc_sum
from _joint_temporal_ref import camera_frame
from _temporal_ref import case, clips, dead_frame_case, motion_ref  # noqa: F401  (re-exported)

# (J, N, H, L): the select call's tables (_temporal_ref.CASES and BOUNDARY_CASES) up to the resident recurrence's cap - both sides of TT_J
# = 32 joints per staged piece (33, 64, 65) and of TT_P = 16 (H = 17), one and two waves (50, 64 | 65, 130), 256 lanes with a lane that
# owns two h (300), chains across many chunks (300 frames), the cap itself (1024).
CASES = [(1, 1, 1, 1), (1, 7, 2, 7), (5, 12, 3, 4), (17, 64, 5, 64), (17, 70, 50, 35), (17, 70, 64, 9), (21, 40, 65, 40), (17, 300, 7, 300),
         (17, 130, 130, 50), (33, 9, 5, 9), (64, 6, 17, 3), (65, 5, 3, 5), (17, 40, 300, 13), (1, 3, 1024, 3)]
IDS = [f"J{J}-N{N}-H{H}-L{L}" for J, N, H, L in CASES]
LAMBDAS = (30.0, 100.0, 300.0)
TAUS = (1.0, 0.25)


@functools.lru_cache(maxsize=None)
def translation(N, H):
    """T [H N,3] float32, rows (h, n): about (0.1, -0.2, 4) m, 5 cm apart per hypothesis, a walk of 1 cm per frame, 5 mm of noise.  Read-only."""
    g = np.random.Generator(np.random.Philox(key=[92, 10 * N + H]))
    T = (np.array([0.1, -0.2, 4.0]) + 0.05 * g.standard_normal((H, 1, 3)) + np.cumsum(0.01 * g.standard_normal((1, N, 3)), axis=1)
         + 0.005 * g.standard_normal((H, N, 3))).astype(np.float32)
    T = np.ascontiguousarray(T.reshape(H * N, 3))
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def case_motion(J, N, H):
    """m[n] [H',H] of every frame n >= 1 of case(J, N, H) (index 0: None), computed once for all weights and clip lengths."""
    x = case(J, N, H)[0]
    return [None] + [motion_ref(x, N, n) for n in range(1, N)]


def chain_ref(unary, x, seq_start, lam, tau, N=None, descending=False, motion=None):
    """The chain alone -> dict(A, B, w [N,H], hmax [N] int32, wmax, logz [N], dead [N] bool, ok [N,H] bool, G): the recurrences and the
    marginals of the header.  G = the largest finite |A|.  descending: every sum over the hypotheses in the other order.  motion: m[n]
    for every n, if the caller has them (case_motion); otherwise motion_ref forms them."""
    lse = lambda t: lse_ascending(t, descending)
    seq = [int(v) for v in seq_start]
    N = seq[-1] if N is None else int(N)
    H = len(unary) // N
    u = np.asarray(unary, dtype=np.float64).reshape(H, N).T.copy()                            # u[n, h]
    ok = np.isfinite(u)
    with np.errstate(invalid="ignore"):
        l = np.where(ok, -u / tau, -np.inf)
    dead = ~ok.any(1)
    c = lam / tau
    A, B = np.full((N, H), -np.inf), np.zeros((N, H))
    w, logz = np.zeros((N, H)), np.full(N, -np.inf)
    hmax, wmax = np.zeros(N, np.int32), np.zeros(N)
    for a, b in zip(seq[:-1], seq[1:]):
        m = motion if motion is not None else {n: motion_ref(x, N, n) for n in range(a + 1, b)}    # m[n][h', h]
        for n in range(a, b):
            if dead[n]:
                continue
            if n == a or dead[n - 1]:
                A[n] = l[n]
            else:
                A[n] = l[n] + lse(A[n - 1][None, :] - c * m[n].T)                             # [h, h']
        lz = -np.inf
        for n in range(b - 1, a - 1, -1):
            if dead[n]:
                continue
            if n == b - 1 or dead[n + 1]:
                lz = float(lse(A[n]))
            else:
                B[n] = lse((l[n + 1] + B[n + 1])[None, :] - c * m[n + 1])                     # [h, h']
            logz[n] = lz
            with np.errstate(invalid="ignore"):
                w[n] = np.where(ok[n], np.exp((A[n] + B[n]) - lz), 0.0)
            hmax[n] = int(np.argmax(w[n]))                                                    # the lowest h with the largest marginal
            wmax[n] = w[n, hmax[n]]
    fin = np.isfinite(A)
    return dict(A=A, B=B, w=w, hmax=hmax, wmax=wmax, logz=logz, dead=dead, G=float(np.abs(A[fin]).max()) if fin.any() else 0.0)


def moments_ref(w, dead, x, T, N, descending=False):
    """-> (mean [N,J,3], cov [N,J,6]) of X = x + T (T None: x alone) under the marginals w [N,H]: sum_h w X and sum_h w (X - mean)(X -
    mean)^T from the centred differences (xx, xy, xz, yy, yz, zz), the sums ascending in h; NaN on a dead frame."""
    X = camera_frame(x, T, N)                                                                 # [H, N, J, 3]
    J = X.shape[2]
    mean, cov = np.full((N, J, 3), np.nan), np.full((N, J, 6), np.nan)
    for n in np.flatnonzero(~dead):
        Xn = X[:, n]                                                                          # [H, J, 3]
        mu = asc_sum(w[n][:, None, None] * Xn, descending)
        d = Xn - mu
        mean[n] = mu
        cov[n] = np.stack([asc_sum(w[n][:, None] * (d[:, :, p] * d[:, :, q]), descending)
                           for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], -1)
    return mean, cov


def temporal_marginal_ref(unary, x, T, seq_start, lam, tau, N=None, descending=False, motion=None):
    """-> chain_ref's dict with mean [N,J,3] and cov [N,J,6]: the definitions of the header.  T enters the positions the moments are
    taken of and nothing else."""
    r = chain_ref(unary, x, seq_start, lam, tau, N, descending, motion)
    r["mean"], r["cov"] = moments_ref(r["w"], r["dead"], x, T, r["w"].shape[0], descending)
    return r


@functools.lru_cache(maxsize=None)
def case_chain(J, N, H, L, lam, tau):
    x, u = case(J, N, H)
    return chain_ref(u, x, clips(N, L), lam, tau, motion=case_motion(J, N, H))


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam, tau, with_T=True):
    """The reference of a case of the table: the chain is computed once per (case, weights), the moments with T and without."""
    r = dict(case_chain(J, N, H, L, lam, tau))
    r["mean"], r["cov"] = moments_ref(r["w"], r["dead"], case(J, N, H)[0], translation(N, H) if with_T else None, N)
    return r


def brute_force_clip(unary, x, L, lam, tau):
    """One clip of L frames (N = L), every one of the H^L paths -> (w [L,H], logZ): a path's weight is exp(-(sum_n u[n,p_n] + lam
    sum_{n>=1} m[n,p_{n-1},p_n]) / tau), shifted by the smallest energy."""
    H = len(unary) // L
    u = np.asarray(unary, dtype=np.float64).reshape(H, L).T
    m = [None] + [motion_ref(x, L, n) for n in range(1, L)]
    paths = list(itertools.product(range(H), repeat=L))
    E = np.empty(len(paths))
    for i, p in enumerate(paths):
        e = u[0, p[0]]
        for n in range(1, L):
            e = e + u[n, p[n]] + lam * m[n][p[n - 1], p[n]]
        E[i] = e
    Emin = E.min()
    pw = np.exp(-(E - Emin) / tau)
    Z = pw.sum()
    w = np.zeros((L, H))
    for i, p in enumerate(paths):
        for n in range(L):
            w[n, p[n]] += pw[i] / Z
    return w, -Emin / tau + np.log(Z)


def marg_bound(L, H, J, G):
    """beta: the absolute bound on the difference between two float64 evaluations of a log-marginal A + B - logZ (and on |sum_h w - 1|):
    4 L (H + 8 + 2 (J + 5) G) 2^-53.

    It is _joint_marginal_ref.marg_bound's argument with the error of a term replaced.  One step of a recurrence is l + LSE_h'(t_h'),
    t = V[h'] - c m, and here m = (1/J) sum_j sqrt(sum_c d_c^2), d exact differences.  With eps = 2^-53:
      - the terms: one square root of a three-term sum of squares is good to about 3 eps relative (three products, two additions, the
        root: the root halves what went in); the sum of J such positive numbers in ANY order adds (J - 1) eps relative, the division
        by J one more: (J + 3) eps on m.  c m is one product more, (J + 4) eps |c m|, and the subtraction one rounding of t, eps |t|.
        |c m| = |V - t| <= |V| + |t|, so the term's absolute error is at most (J + 5) eps (|V| + |t|) <= 2 (J + 5) eps G, G the largest
        finite |A| (|t| <= G where the term carries weight: a term far below the maximum contributes its error times its vanishing
        weight).  An absolute error d in every term moves the LSE by at most d: 2 (J + 5) G eps.  (J = 1: 12 G eps, where the joint-wise
        bound has 8 G eps - it counts 4 eps on a term where this count has J + 5 = 6: the division by J and the looser square root.)
      - the exponentials and the sum of H positive terms: as there, 8 eps and H eps on the log.
    That is (H + 8 + 2 (J + 5) G) eps per step; the errors of the steps add along the chain: L steps forward for A, L backward for B;
    logZ is one more LSE over A, inside the forward budget of its chain end.  A + B - logZ therefore differs from the exact value by at
    most 2 L (H + 8 + 2 (J + 5) G) eps in each evaluation, and two evaluations from each other by twice that."""
    return 4.0 * L * (H + 8.0 + 2.0 * (J + 5.0) * G) * 2.0 ** -53


def over_joints(a, J):
    """A per-frame array [N, ...] as hold_marginals takes it: [N, J, ...], repeated over the joints."""
    return np.broadcast_to(a[:, None], (a.shape[0], J) + a.shape[1:])


def pose_reference(r, J):
    """The reference arrays of hold_marginals out of what temporal_marginal_ref returns: the per-frame w, hmax, logz and dead flags
    repeated over the J joints; log w = A + B - logZ."""
    with np.errstate(invalid="ignore"):                              # a dead frame: -inf - -inf, which nothing looks at
        log_w = (r["A"] + r["B"]) - r["logz"][:, None]
    return dict(log_w_ref=over_joints(log_w, J), logz_ref=over_joints(r["logz"], J), mean_ref=r["mean"], cov_ref=r["cov"],
                hmax_ref=over_joints(r["hmax"], J), w_ref=over_joints(r["w"], J), dead=over_joints(r["dead"], J))


def hold_pose_marginals(out, r, x, T, N, L, left_out_cap=0.0):
    """out = (mean [N,J,3], cov [N,J,6], hmax [N], wmax [N], logz [N], w [N,H]) of the pose-level call against the reference r through
    _joint_marginal_ref.hold_marginals, the per-frame outputs repeated over J; beta = marg_bound of the longest chain.  NO arg-max is
    left out of the comparison unless the caller says so.  -> what was observed."""
    mean, cov, hmax, wmax, logz, w = out
    J, H = mean.shape[1], w.shape[1]
    beta = marg_bound(min(L, N), H, J, r["G"])
    full = (mean, cov, np.ascontiguousarray(over_joints(hmax, J)), np.ascontiguousarray(over_joints(wmax, J)),
            np.ascontiguousarray(over_joints(logz, J)), np.ascontiguousarray(over_joints(w, J)))
    return hold_marginals(full, beta=beta, x=x, T=T, N=N, left_out_cap=left_out_cap, **pose_reference(r, J))


def top_two_gap(r):
    """The smallest difference between the two largest log-marginals of a live frame (inf with H = 1 or no live frame)."""
    w = r["w"][~r["dead"]]
    if w.shape[1] < 2 or not w.shape[0]:
        return np.inf
    top2 = np.sort(w, axis=1)[:, -2:]
    with np.errstate(divide="ignore"):
        return float((np.log(top2[:, 1]) - np.log(top2[:, 0])).min())


def check_inputs(verbose=True):
    """On the reference alone, for every case, lambda and tau of the tables: the two largest log-marginals of every live frame are more
    than 1e-4 apart and 2 beta is below 1e-5 - the arg-max of EVERY frame is compared exactly (left_out_cap = 0).
    -> (the smallest gap, the largest 2 beta)."""
    gaps, betas = [], []
    for J, N, H, L in CASES:
        for lam in LAMBDAS:
            for tau in TAUS:
                r = case_chain(J, N, H, L, lam, tau)
                gap, b2 = top_two_gap(r), 2.0 * marg_bound(min(L, N), H, J, r["G"])
                gaps.append(gap)
                betas.append(b2)
                assert gap > 1e-4 and b2 < 1e-5, (J, N, H, L, lam, tau, gap, b2)
    if verbose:
        print(f"smallest gap between the two largest log-marginals: {min(gaps):.3g}; largest 2 beta: {max(betas):.3g}")
    return min(gaps), max(betas)
