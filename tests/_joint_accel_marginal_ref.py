"""The float64 reference of the fusion along a video under the second-order motion model (zedo_joint_accel_marginal, include/zedo_hip.h),
stated directly in numpy: per joint the forward and the backward recurrence over PAIRS of hypotheses in the log domain, the pair
marginals, the marginals, the posterior mean, the covariance from centred differences and the arg-max in the statement order of the
header, one joint after the other, every sum ascending; a brute-force enumeration of all paths of a chain; and the error bound the GPU
test holds the kernels to.  The inputs, the camera frame, the motion terms and the chains are those of _joint_temporal_ref and
_joint_accel_ref.  Pinned on its own by tests/test_joint_accel_marginal_ref.py."""
import functools
import itertools

import numpy as np

from _joint_accel_ref import ALL_CASES, accel_term, chains
from _joint_marginal_ref import asc_sum, lse_ascending
from _joint_temporal_ref import camera_frame, case, joint_motion
from _temporal_ref import clips

# The kernels of csrc/zedo_joint_accel_marginal.hip take the pair dealing of csrc/zedo_joint_accel.hip, constant for constant (1, 2, 4, 7,
# 10, 13 or 16 pairs per lane: H = 16 | 17, 22 | 23, 32 | 33, 42 | 43, 50 | 51, 57 | 58, and 63 | 64 at the cap), and _joint_accel_ref.ALL_CASES
# holds both sides of each, J = 64 | 65 and clips of 1 to 300 frames.  The backward kernel stages no runs of frames (B2 stays in the LDS one
# frame at a time, A2 is fetched one frame ahead), so the long clips of that table (130, 230, 300 frames) are longer than any staging there is.
# What the table lacks is a clip of exactly two and of exactly three frames at more than one joint: (2, 11, 4, 3) has clips of 3, 3, 3 and 2.
BOUNDARY_CASES = [(2, 11, 4, 3)]
MARGINAL_CASES = ALL_CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}-L{L}" for J, N, H, L in MARGINAL_CASES]
WEIGHTS = ((0.0, 100.0, 1.0), (30.0, 100.0, 1.0), (100.0, 300.0, 0.25))     # (lambda_v, lambda_a, tau)
# the shapes the other weight sets run on, and the shapes of the tau -> 0 limit (GPU test and CPU test alike)
SMALL_CASES = [(5, 12, 3, 4), (1, 20, 17, 20), (3, 130, 7, 130), (2, 11, 4, 3)]
COLD_CASES = [(17, 70, 50, 35), (3, 40, 64, 9), (3, 130, 7, 130), (5, 12, 3, 4)]
COLD_TAU = 1e-9


def accel_term_back(X, n, j):
    """a'[n+1,j,h',h,h+] as [h', h, h+] float64: sqrt(e0^2 + e1^2 + e2^2), e_c = (X[h',n-1,j,c] - 2 X[h,n,j,c]) + X[h+,n+1,j,c] - the second
    difference of the frames n-1, n, n+1 in the association of the backward pass; the squares, then their sum ascending in c."""
    g = X[:, None, n - 1, j, :] - 2.0 * X[None, :, n, j, :]                                   # [h', h, c]: formed once per pair
    e0, e1, e2 = (g[:, :, None, c] + X[None, None, :, n + 1, j, c] for c in range(3))
    return np.sqrt(e0 * e0 + e1 * e1 + e2 * e2)


def joint_accel_marginal_ref(junary, x, T, seq_start, lam_v, lam_a, tau, N=None, descending=False):
    """-> dict(A2 [N,J,H,H] (NaN where a frame has no table), w [N,J,H], mean [N,J,3], cov [N,J,6], hmax [N,J] int32, wmax, logz [N,J],
    dead [N,J] bool, G): the definitions of the header, one joint after the other.  G = the largest magnitude a term is made of: the
    largest finite |l|, |A2|, |M| or |B2|, and 4 sqrt(3) max|X| (c_v + c_a) - the weights times the operands of the differences under the
    square roots.  descending: every sum over a hypothesis index (and over the pairs) in the other order."""
    lse = lambda t: lse_ascending(t, descending)
    asum = lambda a: asc_sum(a, descending)
    seq = [int(v) for v in seq_start]
    N = seq[-1] if N is None else int(N)
    H, J = x.shape[0] // N, x.shape[1]
    u = np.asarray(junary, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()       # u[n, j, h]
    ok = np.isfinite(u)
    with np.errstate(invalid="ignore"):
        l = np.where(ok, -u / tau, -np.inf)
    X = camera_frame(x, T, N)                                                                 # [H, N, J, 3]
    dead = ~ok.any(2)
    c_v, c_a = lam_v / tau, lam_a / tau
    A2 = np.full((N, J, H, H), np.nan)
    w, logz = np.zeros((N, J, H)), np.full((N, J), -np.inf)
    mean, cov = np.full((N, J, 3), np.nan), np.full((N, J, 6), np.nan)
    hmax, wmax = np.zeros((N, J), np.int32), np.zeros((N, J))
    G = 4.0 * np.sqrt(3.0) * float(np.abs(X).max()) * (c_v + c_a)

    def grow(t):
        nonlocal G
        t = np.abs(t[np.isfinite(t)])
        if t.size:
            G = max(G, float(t.max()))

    def moments(n, j):
        Xn = X[:, n, j, :]                                                                    # [H, 3]
        mu = asum(w[n, j][:, None] * Xn)
        d = Xn - mu
        mean[n, j] = mu
        cov[n, j] = [asum(w[n, j] * (d[:, p] * d[:, q])) for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        hmax[n, j] = int(np.argmax(w[n, j]))                                                  # the lowest h with the largest marginal
        wmax[n, j] = w[n, j, hmax[n, j]]

    grow(l)
    with np.errstate(invalid="ignore"):
        for j in range(J):
            for a, b in zip(seq[:-1], seq[1:]):
                for c0, c1 in chains(dead[:, j], max(0, min(a, N)), max(0, min(b, N))):
                    if c1 - c0 == 1:
                        lz = float(lse(l[c0, j]))
                        w[c0, j] = np.where(ok[c0, j], np.exp(l[c0, j] - lz), 0.0)
                        logz[c0, j] = lz
                        moments(c0, j)
                        continue
                    A2[c0 + 1, j] = l[c0, j][:, None] + (l[c0 + 1, j][None, :] - c_v * joint_motion(X, c0 + 1, j).T)       # [h', h]
                    for n in range(c0 + 2, c1):
                        inner = lse(np.moveaxis(A2[n - 1, j][:, :, None] - c_a * accel_term(X, n, j), 0, -1))   # [h', h], over h''
                        A2[n, j] = l[n, j][None, :] + (-c_v * joint_motion(X, n, j).T + inner)
                    grow(A2[c0 + 1:c1, j])
                    lz = float(lse(A2[c1 - 1, j].reshape(-1)))
                    logz[c0:c1, j] = lz
                    B2 = np.zeros((H, H))
                    for n in range(c1 - 1, c0, -1):
                        if n < c1 - 1:
                            M = (l[n + 1, j][:, None] - c_v * joint_motion(X, n + 1, j)) + B2.T        # [h+, h]; B2 is B2[n+1][h, h+]
                            B2 = lse(M.T[None, :, :] - c_a * accel_term_back(X, n, j))                # [h', h], over h+
                            grow(M)
                            grow(B2)
                        pi = np.exp((A2[n, j] + B2) - lz)                                         # exp(-inf) = 0: an excluded hypothesis
                        w[n, j] = asum(pi)                                                        # over h'
                        moments(n, j)
                        if n == c0 + 1:
                            w[c0, j] = asum(pi.T)                                                 # over h
                            moments(c0, j)
    return dict(A2=A2, w=w, mean=mean, cov=cov, hmax=hmax, wmax=wmax, logz=logz, dead=dead, G=G)


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam_v, lam_a, tau, with_T=True):
    x, T, u = case(J, N, H)
    return joint_accel_marginal_ref(u, x, T if with_T else None, clips(N, L), lam_v, lam_a, tau)


def brute_force_chain(u, X, lam_v, lam_a, tau):
    """One chain of one joint, every one of the H^L paths: u [L,H] (+inf: excluded), X [L,H,3] -> (w [L,H], logZ): a path's weight is
    exp(-(sum u + lam_v sum |X[n] - X[n-1]| + lam_a sum |X[n] - 2 X[n-1] + X[n-2]|) / tau), shifted by the smallest energy."""
    L, H = u.shape
    paths = list(itertools.product(range(H), repeat=L))
    E = np.empty(len(paths))
    for i, p in enumerate(paths):
        e = u[0, p[0]]
        for n in range(1, L):
            e = e + u[n, p[n]] + lam_v * float(np.sqrt(((X[n, p[n]] - X[n - 1, p[n - 1]]) ** 2).sum()))
            if n >= 2:
                e = e + lam_a * float(np.sqrt(((X[n, p[n]] - 2.0 * X[n - 1, p[n - 1]] + X[n - 2, p[n - 2]]) ** 2).sum()))
        E[i] = e
    Emin = E.min()
    pw = np.exp(-(E - Emin) / tau)
    Z = pw.sum()
    w = np.zeros((L, H))
    for i, p in enumerate(paths):
        for n in range(L):
            w[n, p[n]] += pw[i] / Z
    return w, -Emin / tau + np.log(Z)


def accel_marg_bound(L, H, G):
    """The absolute bound on the difference between two float64 evaluations of a log-marginal log w (and on |sum_h w - 1| and on the
    difference of two logZ): (4 L (H + 8 + 16 G) + 2 (H^2 + H + 12 + 4 G)) 2^-53, for chains of at most L frames.

    With eps = 2^-53 and G the largest magnitude a term is made of (joint_accel_marginal_ref), one step of either recurrence is an
    assembly of the form l + (-c_v m + LSE_i (V[i] - c_a a[i])):
      - the second difference e_c = (p - 2 q) + r, in EITHER association (the forward pass takes (X[n] - 2 X[n-1]) + X[n-2], the backward
        pass (X[n-1] - 2 X[n]) + X[n+1]): 2 q is exact, the two additions round once each on operands of at most 3 max|X| and 4 max|X|, so
        |delta e_c| <= 7 max|X| eps whichever way it is bracketed; the norm a = sqrt(sum e_c^2) moves by at most sqrt(3) 7 max|X| eps for
        that and by 3 eps a <= 3 eps 4 sqrt(3) max|X| for its own squares, sums and root; the product c_a a is one rounding more:
        together under 20 sqrt(3) c_a max|X| eps = 5 G eps, since G >= 4 sqrt(3) c_a max|X|;
      - the subtraction V - c_a a is one rounding of a number of at most 2 G: 2 G eps.  An absolute error d in every term moves the LSE
        by at most d: 7 G eps for the terms;
      - c_v m: m is the norm of a once-rounded difference (2 max|X| eps per coordinate) with the same 3 eps of its own, times c_v, one
        rounding: under 3 G eps;
      - the assembly: three additions of numbers of at most 2 G: 6 G eps.  The backward pass assembles (l - c_v m) + B2 into M before the
        walk and subtracts c_a a' from M: the same count;
      - the exponentials: exp and log of the device library are good to 2 ulp each (OCML's documented figure), the shift t - max is one
        rounding of a number below 1 in the terms that matter: under 8 eps absolute on the log of the sum, as in marg_bound;
      - the sum of H non-negative terms in ANY order is within (H - 1) eps relative: H eps on its log.
    That is (H + 8 + 16 G) eps per step; the errors of the steps add along the chain: at most L steps forward for A2, L backward for B2:
    2 L (H + 8 + 16 G) eps on A2 + B2.  Then, once per marginal:
      - logZ is one LSE over the H^2 pairs of A2[c1-1], summed in any order (the kernel: a lane's pairs, a butterfly, the waves; the
        reference: ascending q): (H^2 + 8) eps;
      - the pair marginal exp((A2 + B2) - logZ): two roundings of numbers of at most 2 G, 4 G eps on the argument, and exp's 2 ulp with
        the rounding of the result: 4 eps relative;
      - the marginal is a sum of H non-negative pair marginals in any order: H eps relative.
    One evaluation is therefore within 2 L (H + 8 + 16 G) eps + (H^2 + H + 12 + 4 G) eps of the exact log-marginal, and two evaluations
    within twice that of each other.  sum_h w is the sum of all pair marginals, exactly 1 in exact arithmetic: the same budget.  Nothing
    here is fitted to the kernel: tests/test_joint_accel_marginal_gpu.py prints the share of the bound each case uses."""
    return (4.0 * L * (H + 8.0 + 16.0 * G) + 2.0 * (H * H + H + 12.0 + 4.0 * G)) * 2.0 ** -53


def check_inputs(verbose=True):
    """On the reference alone, what the exact comparisons of the GPU test assume.  (1) At the weights the full table runs at, at most 1 %
    of the live (frame, joint) of any case have a runner-up marginal within twice the bound of the largest: hmax is compared on the
    others.  (2) At tau = COLD_TAU every live (frame, joint) of COLD_CASES has wmax >= 0.99: the arg-max is then the path of
    zedo_joint_accel_select unless two paths lie within about 5 tau of each other.  -> (the largest share left out, the smallest cold wmax)."""
    worst, cold = 0.0, 1.0
    for J, N, H, L in MARGINAL_CASES:
        sets = WEIGHTS if (J, N, H, L) in SMALL_CASES else WEIGHTS[1:2]
        for lam_v, lam_a, tau in sets:
            r = reference(J, N, H, L, lam_v, lam_a, tau)
            live = ~r["dead"]
            assert live.all() and np.isfinite(r["logz"]).all() and (np.abs(r["w"].sum(2) - 1.0) <= accel_marg_bound(L, H, r["G"])).all()
            if H > 1:
                top2 = np.sort(r["w"], axis=2)[:, :, -2:]
                with np.errstate(divide="ignore"):
                    close = np.log(top2[:, :, 1]) - np.log(top2[:, :, 0]) <= 2 * accel_marg_bound(min(L, N), H, r["G"])
                worst = max(worst, float(close[live].mean()))
                assert close[live].mean() <= 0.01, (J, N, H, L, lam_v, lam_a, tau)
    for J, N, H, L in COLD_CASES:
        r = reference(J, N, H, L, 30.0, 100.0, COLD_TAU)
        cold = min(cold, float(r["wmax"].min()))
        if verbose:
            print(f"tau = {COLD_TAU:g}, J={J} N={N} H={H} L={L}: smallest largest marginal {r['wmax'].min():.6f}")
        assert r["wmax"].min() >= 0.99, (J, N, H, L)
    if verbose:
        print(f"largest share of (frame, joint) whose arg-max is within twice the bound of its runner-up: {100 * worst:.2f} %")
    return worst, cold
