"""The float64 reference of the fixed-lag streaming fusion (zedo_joint_stream_marginal_push, include/zedo_hip.h), stated directly in numpy:
A is the forward table of _joint_marginal_ref.joint_marginal_ref on the whole clips - a prefix quantity, which does not depend on how the
frames were cut into pushes; per live (n, j) the horizon e = min(n + lag, the last frame of n's chain on the clip) is found as
_joint_stream_ref.fixed_lag finds it, B is walked from B[e] = 0 down to n with lse_ascending, logZ = LSE_h A[e,j,h], and w, the mean,
the covariance (centred, asc_sum), hmax, wmax and logz follow as the offline reference words them.  Also the comparison the GPU tests
hold the kernels to (_joint_marginal_ref.hold_marginals: the same derived bounds, with L the clip's length, and EVERY arg-max) and the
check of the inputs that lets every arg-max be compared.  Pinned on its own by tests/test_joint_stream_marginal_ref.py."""
import functools

import numpy as np

from _joint_marginal_ref import asc_sum, chain_reference, hold_marginals, joint_marginal_ref, lse_ascending, marg_bound
from _joint_marginal_ref import reference as offline_reference
from _joint_temporal_ref import camera_frame, case
from _temporal_ref import clips

LAGS = (0, 1, 3, 8)
WEIGHTS = ((100.0, 1.0), (30.0, 0.25))                             # (lambda, tau) of the comparisons
FINITE_CASES = [(17, 70, 50, 35), (3, 130, 7, 130), (2, 30, 130, 13), (1, 9, 1024, 9), (1, 6, 300, 3), (2, 4, 1000, 4)]
INPUT_CASES = FINITE_CASES + [(5, 12, 3, 4)]


def horizons(dead, seq, lag):
    """[N,J] int: e = min(n + lag, c_j(n)) of every live (n, j), c_j(n) the first m >= n of the clip whose successor is dead or absent;
    -1 where (n, j) is dead."""
    N, J = dead.shape
    e = np.full((N, J), -1, np.int64)
    for a, b in zip(seq[:-1], seq[1:]):
        for j in range(J):
            c = b - 1
            for n in range(b - 1, a - 1, -1):
                if dead[n, j]:
                    c = n - 1
                else:
                    e[n, j] = min(n + lag, c)
    return e


def fixed_lag_marginal(u, x, T, seq, lam, tau, lag, N=None, full=None):
    """-> dict(A, B, w [N,J,H], mean [N,J,3], cov [N,J,6], hmax [N,J] int32, wmax, logz [N,J], dead [N,J] bool, G, e [N,J]) of every clip
    of `seq` streamed with this lag and flushed at its end: row n is joint_marginal_ref on the clip cut after frame e[n,j].  B[n,j] is
    B of frame n under its own horizon.  All (n, j) walk together, one frame per step: the operations on each are those of
    joint_marginal_ref, element for element.  full: joint_marginal_ref of the same arguments, if the caller has it."""
    seq = [int(v) for v in seq]
    N = seq[-1] if N is None else int(N)
    full = joint_marginal_ref(u, x, T, seq, lam, tau, N) if full is None else full
    A, dead = full["A"], full["dead"]
    H, J = A.shape[2], A.shape[1]
    uu = np.asarray(u, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()
    ok = np.isfinite(uu)
    with np.errstate(invalid="ignore"):
        l = np.where(ok, -uu / tau, -np.inf)
    X = camera_frame(x, T, N)                                      # [H, N, J, 3]
    c = lam / tau
    e = horizons(dead, seq, lag)
    depth = np.where(e >= 0, e - np.arange(N)[:, None], -1)
    B = np.zeros((N, J, H))
    for d in range(int(depth.max()) - 1, -1, -1):                  # the walker of (n, j) steps from frame n + d + 1 to frame n + d
        nn, jj = np.nonzero(depth > d)
        m = nn + d
        d0, d1, d2 = (X[:, None, m + 1, jj, k] - X[None, :, m, jj, k] for k in range(3))        # [h' (frame m+1), h (frame m), walkers]
        mot = np.sqrt(d0 * d0 + d1 * d1 + d2 * d2).transpose(2, 1, 0)                              # [walkers, h, h']
        B[nn, jj] = lse_ascending((l[m + 1, jj] + B[nn, jj])[:, None, :] - c * mot)
    w, logz = np.zeros((N, J, H)), np.full((N, J), -np.inf)
    mean, cov = np.full((N, J, 3), np.nan), np.full((N, J, 6), np.nan)
    hmax, wmax = np.zeros((N, J), np.int32), np.zeros((N, J))
    for n, j in zip(*np.nonzero(~dead)):
        lz = float(lse_ascending(A[e[n, j], j]))
        logz[n, j] = lz
        with np.errstate(invalid="ignore"):
            w[n, j] = np.where(ok[n, j], np.exp(A[n, j] + B[n, j] - lz), 0.0)
        Xn = X[:, n, j, :]
        mu = asc_sum(w[n, j][:, None] * Xn)
        dd = Xn - mu
        mean[n, j] = mu
        cov[n, j] = [asc_sum(w[n, j] * (dd[:, p] * dd[:, q])) for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        hmax[n, j] = int(np.argmax(w[n, j]))
        wmax[n, j] = w[n, j, hmax[n, j]]
    B[dead] = 0.0
    return dict(A=A, B=B, w=w, mean=mean, cov=cov, hmax=hmax, wmax=wmax, logz=logz, dead=dead, G=full["G"], e=e)


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam, tau, lag, with_T=True):
    x, T, u = case(J, N, H)
    return fixed_lag_marginal(u, x, T if with_T else None, clips(N, L), lam, tau, lag, full=offline_reference(J, N, H, L, lam, tau, with_T))


def hold_to(out, r, x, T, N, L, tag):
    """Every output (mean, cov, hmax, wmax, logz, w as numpy arrays [N, ..]) against the reference r within the derived bounds of
    _joint_marginal_ref, L the clip's length; prints observed against bound.  -> the largest log-marginal error."""
    s = hold_marginals(out, beta=marg_bound(min(L, N), out[5].shape[2], r["G"]), x=x, T=T, N=N, **chain_reference(r))
    print(f"joint-stream-marginal {tag}: G = {r['G']:.3g}; max |log w - ref| = {s['e_lw']:.3e}, |sum w - 1| = {s['e_sum']:.3e}, |logz - ref| = "
          f"{s['e_lz']:.3e} (bound {s['beta']:.3e}); |mean - ref| = {s['e_mean']:.3e} m (bound {s['mean_bound']:.3e}); |cov - ref| = "
          f"{s['e_cov']:.3e} m^2 (smallest bound {s['cov_bound']:.3e}); hmax differs on {s['hmax_differs']} of {out[2].size}")
    # the reference's arg-max - check_inputs: EVERY one is clear of the bound
    assert s["not_clear"] == 0 and np.array_equal(out[2][~r["dead"]], r["hmax"][~r["dead"]])
    return s["e_lw"]


def smallest_log_gap(w, dead):
    """The smallest log-gap between the two largest marginals over the live (n, j) (inf if H = 1 or nothing is live)."""
    if w.shape[2] < 2 or dead.all():
        return np.inf
    top2 = np.sort(w, axis=2)[:, :, -2:][~dead]
    with np.errstate(divide="ignore"):
        return float((np.log(top2[:, 1]) - np.log(top2[:, 0])).min())


def check_inputs(verbose=True):
    """On the reference alone: at every lag of LAGS and both weights of WEIGHTS the log-gap between the two largest marginals of every
    live (n, j) of INPUT_CASES is above 1e-6 - orders above twice the largest marg_bound, which is asserted too - so NO arg-max is left
    out of a comparison.  -> (the smallest gap, the largest 2 beta)."""
    gaps, betas = [], []
    for J, N, H, L in INPUT_CASES:
        for lam, tau in WEIGHTS:
            for lag in LAGS:
                r = reference(J, N, H, L, lam, tau, lag)
                g = smallest_log_gap(r["w"], r["dead"])
                assert g > 1e-6, (J, N, H, L, lam, tau, lag, g)
                gaps.append(g)
                betas.append(2 * marg_bound(min(L, N), H, r["G"]))
    assert max(betas) * 100 < min(gaps)
    if verbose:
        print(f"smallest log-gap between the two largest marginals: {min(gaps):.3g}; largest 2 marg_bound: {max(betas):.3g}")
    return min(gaps), max(betas)


def distance_table(J=17, N=70, H=50, L=35, lam=100.0, tau=1.0, lags=(0, 1, 3, 8, 34)):
    """Per lag: (median |mean - whole-clip mean| in metres, median total variation of the marginals, share of (n, j) whose arg-max
    differs) against the whole-clip marginals (the reference at lag = L - 1)."""
    whole = reference(J, N, H, L, lam, tau, L - 1)
    rows = []
    for lag in lags:
        r = reference(J, N, H, L, lam, tau, lag)
        rows.append((lag, float(np.median(np.linalg.norm(r["mean"] - whole["mean"], axis=2))),
                     float(np.median(0.5 * np.abs(r["w"] - whole["w"]).sum(2))), float((r["hmax"] != whole["hmax"]).mean())))
    return rows
