"""The float64 reference of the joint-wise fusion along a video (zedo_joint_marginal, include/zedo_hip.h), stated directly in numpy: the
forward and the backward recurrence in the log domain, the marginals, the posterior mean, the covariance from centred differences and
the arg-max exactly as the header words them, every sum ascending in h; a brute-force enumeration of all paths of a chain; and the error
bounds the GPU test holds the kernels to.  The inputs are those of _joint_temporal_ref.  Pinned on its own by
tests/test_joint_marginal_ref.py."""
import functools
import itertools

import numpy as np

from _joint_temporal_ref import ALL_CASES, camera_frame, case, joint_motion
from _temporal_ref import clips

# The kernels of csrc/zedo_joint_marginal.hip take the dispatch of the scan kernel of csrc/zedo_joint_temporal.hip, constant for constant:
# the h' split over 4 parts of the workgroup up to H = 64, over 2 up to H = 128, above that a lane owns 1, 2 or 4 hypotheses (up to 256,
# 512, 1024).  _joint_temporal_ref.ALL_CASES holds the smallest shapes on both sides of each of them - 64 | 65, 128 | 129, 256 | 257,
# 512 | 513, and 1024, the largest - and chains of several frames on each branch; the backward kernel stages no runs of frames (B stays
# in the LDS one frame at a time), so there is no run length to cross.  Splits with an empty last part are there as well (H = 3 and 5 over
# 4 parts).  What the table lacks is more than one joint, and a partly filled last group of 256, where a lane owns four hypotheses:
# H = 1000 = 3 x 256 + 232, two chains of four frames.
BOUNDARY_CASES = [(2, 4, 1000, 4)]
MARGINAL_CASES = ALL_CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}-L{L}" for J, N, H, L in MARGINAL_CASES]


def lse_ascending(t, descending=False):
    """log sum_k exp(t[..., k]) over the last axis: shifted by the true maximum of the terms, the sum ascending in k (descending: the
    other order, for the evidence that the order is free).  A row without a term above -inf gives -inf."""
    mx = t.max(axis=-1)
    sh = np.where(np.isfinite(mx), mx, 0.0)
    s = np.zeros(mx.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in (range(t.shape[-1] - 1, -1, -1) if descending else range(t.shape[-1])):
            s = s + np.exp(t[..., k] - sh)
    with np.errstate(divide="ignore"):
        return mx + np.log(s)


def asc_sum(a, descending=False):
    """sum over the first axis, ascending (or descending)."""
    s = np.zeros(a.shape[1:])
    for k in (range(a.shape[0] - 1, -1, -1) if descending else range(a.shape[0])):
        s = s + a[k]
    return s


def joint_marginal_ref(junary, x, T, seq_start, lam, tau, N=None, descending=False):
    """-> dict(A, B, w [N,J,H], mean [N,J,3], cov [N,J,6], hmax [N,J] int32, wmax, logz [N,J], dead [N,J] bool, G): the definitions of the
    header, one joint after the other.  G = the largest finite |A|.  descending: every sum over the hypotheses in the other order."""
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
    c = lam / tau
    A, B = np.full((N, J, H), -np.inf), np.zeros((N, J, H))
    w, logz = np.zeros((N, J, H)), np.full((N, J), -np.inf)
    mean, cov = np.full((N, J, 3), np.nan), np.full((N, J, 6), np.nan)
    hmax, wmax = np.zeros((N, J), np.int32), np.zeros((N, J))
    for j in range(J):
        for a, b in zip(seq[:-1], seq[1:]):
            for n in range(a, b):
                if dead[n, j]:
                    continue
                if n == a or dead[n - 1, j]:
                    A[n, j] = l[n, j]
                else:
                    A[n, j] = l[n, j] + lse(A[n - 1, j][None, :] - c * joint_motion(X, n, j))          # [h, h']
            lz = -np.inf
            for n in range(b - 1, a - 1, -1):
                if dead[n, j]:
                    continue
                if n == b - 1 or dead[n + 1, j]:
                    lz = float(lse(A[n, j]))
                else:
                    B[n, j] = lse((l[n + 1, j] + B[n + 1, j])[None, :] - c * joint_motion(X, n + 1, j).T)  # [h, h']
                logz[n, j] = lz
                with np.errstate(invalid="ignore"):
                    w[n, j] = np.where(ok[n, j], np.exp(A[n, j] + B[n, j] - lz), 0.0)
                Xn = X[:, n, j, :]                                                            # [H, 3]
                mu = asum(w[n, j][:, None] * Xn)
                d = Xn - mu
                mean[n, j] = mu
                cov[n, j] = [asum(w[n, j] * (d[:, p] * d[:, q])) for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
                hmax[n, j] = int(np.argmax(w[n, j]))                                          # the lowest h with the largest marginal
                wmax[n, j] = w[n, j, hmax[n, j]]
    fin = np.isfinite(A)
    return dict(A=A, B=B, w=w, mean=mean, cov=cov, hmax=hmax, wmax=wmax, logz=logz, dead=dead, G=float(np.abs(A[fin]).max()) if fin.any() else 0.0)


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam, tau, with_T=True):
    x, T, u = case(J, N, H)
    return joint_marginal_ref(u, x, T if with_T else None, clips(N, L), lam, tau)


def softmax_ref(junary, N, tau):
    """[N,J,H]: per (frame, joint) the softmax of -u / tau over the hypotheses with a finite unary (0 for the others) - the marginals of
    chains of one frame, and of any chain at lambda = 0.  Closed form, shifted by the smallest unary."""
    H, J = junary.shape[0] // N, junary.shape[1]
    u = np.asarray(junary, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()
    u[~np.isfinite(u)] = np.inf
    e = np.exp(-(u - u.min(axis=2, keepdims=True)) / tau)
    return e / e.sum(axis=2, keepdims=True)


def brute_force_chain(u, X, lam, tau):
    """One chain of one joint, every one of the H^L paths: u [L,H] (+inf: excluded), X [L,H,3] -> (w [L,H], logZ): a path's weight is
    exp(-(sum_n u[n,p_n] + lam sum_{n>=1} |X[n,p_n] - X[n-1,p_{n-1}]|) / tau), shifted by the smallest energy."""
    L, H = u.shape
    paths = list(itertools.product(range(H), repeat=L))
    E = np.empty(len(paths))
    for i, p in enumerate(paths):
        e = u[0, p[0]]
        for n in range(1, L):
            e = e + u[n, p[n]] + lam * float(np.sqrt(((X[n, p[n]] - X[n - 1, p[n - 1]]) ** 2).sum()))
        E[i] = e
    Emin = E.min()
    pw = np.exp(-(E - Emin) / tau)
    Z = pw.sum()
    w = np.zeros((L, H))
    for i, p in enumerate(paths):
        for n in range(L):
            w[n, p[n]] += pw[i] / Z
    return w, -Emin / tau + np.log(Z)


def marg_bound(L, H, G):
    """The absolute bound on the difference between two float64 evaluations of a log-marginal A + B - logZ (and on |sum_h w - 1|):
    4 L (H + 8 + 8 G) 2^-53.

    One step of a recurrence is l + LSE_h'(t_h'), t = V[h'] - c m.  With eps = 2^-53:
      - the terms: m is a square root of a three-term sum of squares of exact differences (about 3 eps relative), c m one product more,
        the subtraction one rounding of t; the term's absolute error is at most about 4 eps (|V| + |t|) <= 8 eps G, G the largest finite
        |A| (|t| <= G where the term carries weight: a term far below the maximum contributes its error times its vanishing weight).  An
        absolute error d in every term moves the LSE by at most d: 8 G eps;
      - the exponentials: exp and log of the device library are good to 2 ulp each (OCML's documented figure), the shift t - max is one
        rounding of a number below 1 in the terms that matter, the combination of the parts of a split is one exp and one product more:
        together under 8 eps relative on the sum, i.e. 8 eps absolute on its log;
      - the sum of H positive terms in ANY order is within (H - 1) eps relative: H eps on the log.
    That is (H + 8 + 8 G) eps per step and the errors of the steps add along the chain: L steps forward for A, L backward for B; logZ is
    one more LSE over A, inside the forward budget of its chain end.  A + B - logZ therefore differs from the exact value by at most
    2 L (H + 8 + 8 G) eps in each evaluation, and two evaluations from each other by twice that."""
    return 4.0 * L * (H + 8.0 + 8.0 * G) * 2.0 ** -53


def softmax_bound(L, H, G, log_sm):
    """The bound on |log w - log softmax_ref| where the marginals are a softmax (chains of one frame; lambda = 0): marg_bound(L, H, G) - the
    closed form's exponentials and its sum of H terms are the second of the two evaluations that bound speaks of - plus the two steps the
    closed form takes that a log-domain evaluation does not: softmax_ref divides e by sum(e) (one rounding of the quotient, 2^-53 relative:
    2^-53 absolute on its logarithm) and the test takes numpy's log of the quotient (one rounding of the result, 2^-53 |log softmax|).
    Together at most 2^-52 max(1, |log softmax|), with the largest |log softmax| of the case."""
    return marg_bound(L, H, G) + 2.0 ** -52 * max(1.0, float(np.abs(log_sm).max()))


def mean_bound(beta, xmax):
    """|mean - mean_ref| per coordinate, given that every log-marginal is within beta: w = w_ref exp(d), |d| <= beta, so
    sum_h |w - w_ref| <= (e^beta - 1) sum_h w_ref, and |sum_h (w - w_ref) X_h| <= (e^beta - 1)(1 + beta) max|X|; the sum of H products in
    any order adds (H + 1) 2^-53 max|X| (1 + beta), which is below beta max|X| because beta >= 4 (H + 8) 2^-53.  -> 2 (e^beta - 1)(1 + beta)
    max|X| (weights that sum to 1 within beta)."""
    return 2.0 * np.expm1(beta) * (1.0 + beta) * xmax


def cov_bound(beta, spread, xmax):
    """|cov - cov_ref| per entry.  With d = X - mean_ref (|d| <= spread, the largest coordinate range of the hypotheses of that (frame,
    joint): the mean lies in their hull) and delta = mean - mean_ref (|delta| <= mean_bound):
      sum_h w (d_p - delta_p)(d_q - delta_q) = sum_h w d_p d_q - delta_p sum_h w d_q - delta_q sum_h w d_p + delta_p delta_q sum_h w.
    The first sum differs from cov_ref by sum_h (w - w_ref) d_p d_q <= (e^beta - 1) spread^2; sum_h w_ref d = 0, so sum_h w d =
    sum_h (w - w_ref) d <= (e^beta - 1) spread and the middle terms are of second order; each difference X - mean is one correctly
    rounded subtraction, the products and the sum of H terms add (H + 6) 2^-53 spread^2 < beta spread^2.
    -> 2 (e^beta - 1) spread^2 + 2 delta (e^beta - 1) spread + delta^2 (1 + beta)."""
    delta = mean_bound(beta, xmax)
    e = np.expm1(beta)
    return 2.0 * e * spread ** 2 + 2.0 * delta * e * spread + delta ** 2 * (1.0 + beta)


def spread_of(x, T, N):
    """-> (spread [N,J]: per (frame, joint) the largest coordinate range of X over the hypotheses, xmax: the largest |X|)."""
    X = camera_frame(x, T, N)
    return (X.max(axis=0) - X.min(axis=0)).max(axis=-1), float(np.abs(X).max())


def chain_reference(r):
    """The reference arrays of hold_marginals out of what joint_marginal_ref returns (or the streaming reference, which words its dict
    alike): log w = A + B - logZ."""
    with np.errstate(invalid="ignore"):                              # a dead (frame, joint): -inf - -inf, which nothing looks at
        log_w = r["A"] + r["B"] - r["logz"][:, :, None]
    return dict(log_w_ref=log_w, logz_ref=r["logz"], mean_ref=r["mean"], cov_ref=r["cov"], hmax_ref=r["hmax"], w_ref=r["w"], dead=r["dead"])


def hold_marginals(out, *, log_w_ref, logz_ref, mean_ref, cov_ref, hmax_ref, w_ref, dead, beta, x, T, N, left_out_cap=None):
    """The one place the marginal outputs of a fusion call are held to a reference: out = (mean, cov, hmax, wmax, logz, w) as numpy
    arrays [N,J,..] against the reference's arrays, given beta, the bound on a log-marginal (marg_bound of the caller's model).  Asserts:
    a dead (frame, joint) is NaN / hypothesis 0 / weight 0 / logz -inf with w == 0; w > 0 wherever the reference's is above 1e-300;
    |log w - log_w_ref| there, |sum_h w - 1| and |logz - ref| on the live ones are at most beta; the mean and the covariance are within
    mean_bound / cov_bound of it; hmax and wmax are the arg-max of w as written; hmax is the reference's wherever the reference's
    runner-up is clear of 2 beta in the logarithm - and, with left_out_cap, at most that share of the live (frame, joint) is not.
    -> what was observed (the callers print it; a failing assertion shows it)."""
    mean, cov, hmax, wmax, logz, w = out
    H, live = w.shape[2], ~dead
    top = lambda a: float(a.max()) if a.size else 0.0
    assert np.array_equal(np.isnan(mean[:, :, 0]), dead) and (w[dead] == 0.0).all()
    assert (hmax[dead] == 0).all() and (wmax[dead] == 0.0).all() and np.isneginf(logz[dead]).all()
    big = w_ref > 1e-300
    assert (w[big] > 0).all()
    spread, xmax = spread_of(x, T, N)
    mb, cb = mean_bound(beta, xmax), np.broadcast_to(cov_bound(beta, spread, xmax)[:, :, None], cov.shape)
    e_cov = np.abs(cov - cov_ref)
    clear = live.copy()
    if H > 1:
        top2 = np.sort(w_ref, axis=2)[:, :, -2:]
        with np.errstate(divide="ignore", invalid="ignore"):
            clear = live & (np.log(top2[:, :, 1]) - np.log(top2[:, :, 0]) > 2 * beta)
    seen = dict(e_lw=top(np.abs(np.log(w[big].astype(np.longdouble)) - log_w_ref[big])), e_sum=top(np.abs(w.sum(2)[live] - 1.0)),
                e_lz=top(np.abs(logz[live] - logz_ref[live])), beta=beta, e_mean=top(np.abs(mean - mean_ref)[live]), mean_bound=mb,
                e_cov=top(e_cov[live]), cov_bound=float(cb[live].min()) if live.any() else 0.0,
                hmax_differs=int((hmax != hmax_ref).sum()), not_clear=int(live.sum() - clear.sum()),
                left_out=1.0 - float(clear[live].mean()) if live.any() else 0.0)
    assert seen["e_lw"] <= beta and seen["e_sum"] <= beta and seen["e_lz"] <= beta, seen
    assert seen["e_mean"] <= mb and (e_cov[live] <= cb[live]).all(), seen
    assert np.array_equal(hmax[live], np.argmax(w, axis=2)[live]) and np.array_equal(wmax[live], w.max(axis=2)[live])
    assert left_out_cap is None or seen["left_out"] <= left_out_cap, seen
    assert np.array_equal(hmax[clear], hmax_ref[clear]), seen
    return seen
