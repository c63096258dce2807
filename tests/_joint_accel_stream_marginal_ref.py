"""The float64 reference of the fixed-lag streaming fusion under the second-order motion model (zedo_joint_accel_stream_marginal_push,
include/zedo_hip.h), stated directly in numpy: A2 is the forward table of _joint_accel_marginal_ref.joint_accel_marginal_ref on the whole
clips - a prefix quantity, which does not depend on how the frames were cut into pushes; per live (n, j) the horizon e = min(n + lag,
the last frame of n's chain on the clip) is _joint_stream_marginal_ref.horizons', B2 is walked from B2[e] = 0 down to max(n, c0 + 1) with
the statements of the offline reference, logZ is the LSE over the pairs of A2[e] (over l[e] where e is the chain's first frame), and w,
the mean, the covariance, hmax, wmax and logz follow as the offline reference words them.  Frames of a chain that share a horizon share
one walk: the same operations on the same operands.  Also the comparison the GPU tests hold the kernels to (hold_marginals with
accel_marg_bound, and EVERY arg-max) and the check of the inputs that lets every arg-max be compared.  Pinned on its own by
tests/test_joint_accel_stream_marginal_ref.py."""
import functools

import numpy as np

from _joint_accel_marginal_ref import WEIGHTS, accel_marg_bound, accel_term_back, joint_accel_marginal_ref
from _joint_accel_marginal_ref import reference as offline_reference
from _joint_accel_ref import chains
from _joint_marginal_ref import asc_sum, hold_marginals, lse_ascending
from _joint_stream_marginal_ref import horizons, smallest_log_gap
from _joint_temporal_ref import camera_frame, case, joint_motion
from _temporal_ref import clips

LAGS = (0, 1, 2, 3, 8)
# the shapes the finite lags are held to this reference on: clips of 4 and of 3, 3, 3 and 2 frames, both sides of the dealings of 1 | 2
# and of 4 | 7 pairs per lane (H = 17, 33), and one clip of 130 frames that wraps a short ring many times
SMALL = [(5, 12, 3, 4), (1, 20, 17, 20), (2, 11, 4, 3), (3, 130, 7, 130), (1, 6, 33, 6)]


def fixed_lag_accel_marginal(u, x, T, seq, lam_v, lam_a, tau, lag, N=None, full=None):
    """-> dict(A2, w [N,J,H], mean [N,J,3], cov [N,J,6], hmax [N,J] int32, wmax, logz [N,J], dead [N,J] bool, G, e [N,J]) of every clip of
    `seq` streamed with this lag and flushed at its end: row n is joint_accel_marginal_ref on the clip cut after frame e[n,j].  G: that
    of the whole clips, grown by every M and B2 of the walks.  full: joint_accel_marginal_ref of the same arguments, if the caller has
    it."""
    seq = [int(v) for v in seq]
    N = seq[-1] if N is None else int(N)
    full = joint_accel_marginal_ref(u, x, T, seq, lam_v, lam_a, tau, N) if full is None else full
    A2, dead, G = full["A2"], full["dead"], full["G"]
    H, J = A2.shape[2], A2.shape[1]
    uu = np.asarray(u, dtype=np.float64).reshape(H, N, J).transpose(1, 2, 0).copy()
    ok = np.isfinite(uu)
    with np.errstate(invalid="ignore"):
        l = np.where(ok, -uu / tau, -np.inf)
    X = camera_frame(x, T, N)                                      # [H, N, J, 3]
    c_v, c_a = lam_v / tau, lam_a / tau
    e = horizons(dead, seq, lag)
    w, logz = np.zeros((N, J, H)), np.full((N, J), -np.inf)
    mean, cov = np.full((N, J, 3), np.nan), np.full((N, J, 6), np.nan)
    hmax, wmax = np.zeros((N, J), np.int32), np.zeros((N, J))

    def grow(t):
        nonlocal G
        t = np.abs(t[np.isfinite(t)])
        if t.size:
            G = max(G, float(t.max()))

    def moments(n, j, lz):
        Xn = X[:, n, j, :]
        mu = asc_sum(w[n, j][:, None] * Xn)
        d = Xn - mu
        logz[n, j] = lz
        mean[n, j] = mu
        cov[n, j] = [asc_sum(w[n, j] * (d[:, p] * d[:, q])) for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        hmax[n, j] = int(np.argmax(w[n, j]))
        wmax[n, j] = w[n, j, hmax[n, j]]

    with np.errstate(invalid="ignore"):
        for j in range(J):
            for a, b in zip(seq[:-1], seq[1:]):
                for c0, c1 in chains(dead[:, j], max(0, min(a, N)), max(0, min(b, N))):
                    for eh in sorted(set(int(v) for v in e[c0:c1, j])):
                        served = [n for n in range(c0, c1) if e[n, j] == eh]       # the frames whose horizon is eh: one walk
                        if eh == c0:
                            lz = float(lse_ascending(l[c0, j]))
                            w[c0, j] = np.where(ok[c0, j], np.exp(l[c0, j] - lz), 0.0)
                            moments(c0, j, lz)
                            continue
                        lz = float(lse_ascending(A2[eh, j].reshape(-1)))
                        B2 = np.zeros((H, H))
                        for m in range(eh, max(served[0], c0 + 1) - 1, -1):
                            if m < eh:
                                M = (l[m + 1, j][:, None] - c_v * joint_motion(X, m + 1, j)) + B2.T        # [h+, h]; B2 is B2[m+1][h, h+]
                                B2 = lse_ascending(M.T[None, :, :] - c_a * accel_term_back(X, m, j))      # [h', h], over h+
                                grow(M)
                                grow(B2)
                            pi = np.exp((A2[m, j] + B2) - lz)
                            if m in served:
                                w[m, j] = asc_sum(pi)                                                     # over h'
                                moments(m, j, lz)
                            if m == c0 + 1 and c0 in served:
                                w[c0, j] = asc_sum(pi.T)                                                  # over h
                                moments(c0, j, lz)
    return dict(A2=A2, w=w, mean=mean, cov=cov, hmax=hmax, wmax=wmax, logz=logz, dead=dead, G=G, e=e)


@functools.lru_cache(maxsize=None)
def reference(J, N, H, L, lam_v, lam_a, tau, lag, with_T=True):
    x, T, u = case(J, N, H)
    return fixed_lag_accel_marginal(u, x, T if with_T else None, clips(N, L), lam_v, lam_a, tau, lag,
                                    full=offline_reference(J, N, H, L, lam_v, lam_a, tau, with_T))


def hold_to(out, r, x, T, N, L, tag):
    """Every output (mean, cov, hmax, wmax, logz, w as numpy arrays [N, ..]) against the reference r within accel_marg_bound and the mean
    and covariance bounds that follow from it, L the clip's length; prints observed against bound; hmax on EVERY live entry.  -> the
    largest log-marginal error."""
    with np.errstate(divide="ignore"):
        log_w = np.log(r["w"].astype(np.longdouble))
    s = hold_marginals(out, log_w_ref=log_w, logz_ref=r["logz"], mean_ref=r["mean"], cov_ref=r["cov"], hmax_ref=r["hmax"], w_ref=r["w"],
                       dead=r["dead"], beta=accel_marg_bound(min(L, N), out[5].shape[2], r["G"]), x=x, T=T, N=N)
    print(f"joint-accel-stream-marginal {tag}: G = {r['G']:.3g}; max |log w - ref| = {s['e_lw']:.3e}, |sum w - 1| = {s['e_sum']:.3e}, |logz - "
          f"ref| = {s['e_lz']:.3e} (bound {s['beta']:.3e}); |mean - ref| = {s['e_mean']:.3e} m (bound {s['mean_bound']:.3e}); |cov - ref| = "
          f"{s['e_cov']:.3e} m^2 (smallest bound {s['cov_bound']:.3e}); hmax differs on {s['hmax_differs']} of {out[2].size}")
    # the reference's arg-max - check_inputs: EVERY one is clear of the bound
    assert s["not_clear"] == 0 and np.array_equal(out[2][~r["dead"]], r["hmax"][~r["dead"]])
    return s["e_lw"]


def check_inputs(verbose=True):
    """On the reference alone: at every lag of LAGS and every weight set of WEIGHTS the log-gap between the two largest marginals of
    every live (n, j) of SMALL is above 1e-6 and above 100 x twice the largest accel_marg_bound, so NO arg-max is left out of a
    comparison.  -> (the smallest gap, the largest 2 bound)."""
    gaps, betas = [], []
    for J, N, H, L in SMALL:
        for lam_v, lam_a, tau in WEIGHTS:
            for lag in LAGS:
                r = reference(J, N, H, L, lam_v, lam_a, tau, lag)
                g = smallest_log_gap(r["w"], r["dead"])
                assert g > 1e-6, (J, N, H, L, lam_v, lam_a, tau, lag, g)
                gaps.append(g)
                betas.append(2 * accel_marg_bound(min(L, N), H, r["G"]))
    assert max(betas) * 100 < min(gaps), (max(betas), min(gaps))
    if verbose:
        print(f"smallest log-gap between the two largest marginals: {min(gaps):.3g}; largest 2 accel_marg_bound: {max(betas):.3g}")
    return min(gaps), max(betas)


def distance_table(J=5, N=40, H=8, L=20, lam_v=30.0, lam_a=100.0, tau=1.0, lags=(0, 1, 3, 8, 19)):
    """Per lag: (median |mean - whole-clip mean| in metres, median total variation of the marginals, share of (n, j) whose arg-max is
    the whole-clip arg-max) against the whole-clip marginals (the reference at lag = L - 1)."""
    whole = reference(J, N, H, L, lam_v, lam_a, tau, L - 1)
    rows = []
    for lag in lags:
        r = reference(J, N, H, L, lam_v, lam_a, tau, lag)
        rows.append((lag, float(np.median(np.linalg.norm(r["mean"] - whole["mean"], axis=2))),
                     float(np.median(0.5 * np.abs(r["w"] - whole["w"]).sum(2))), float((r["hmax"] == whole["hmax"]).mean())))
    return rows
