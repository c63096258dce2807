"""The float64 reference of the skeleton-coupled fusion per pose (zedo_joint_tree_marginal, include/zedo_hip.h), stated directly in numpy:
the upward and the downward pass over the bone tree in the log domain, the marginals, the posterior mean, the covariance from centred
differences, the arg-max, the log-partition value of every component and every bone's expected mismatch exactly as the header words
them - E_g by the SUM over the other children, where the kernel takes S[p] - M_g - every sum ascending; the enumeration of all H^J
assignments; and the error bounds the GPU test holds the kernel to.  Built on _joint_tree_ref (the trees, the unaries, the bone table,
the inputs) by import.  Pinned on its own by tests/test_joint_tree_marginal_ref.py."""
import functools
import itertools

import numpy as np

import _joint_tree_ref as R
from _joint_marginal_ref import asc_sum, cov_bound, lse_ascending, mean_bound, spread_of  # noqa: F401  (re-exported to the tests)
from _joint_tree_ref import (bone_table, camera_frame, case, confidences, dead_joint_case, default_tree, energy, five_roots,  # noqa: F401
                             post_order, reversed_chain, two_roots, unaries)

TREES = {"default": default_tree, "chain": reversed_chain, "forest": two_roots, "forest5": five_roots}
MUS = (0.0, 30.0, 100.0, 300.0)
TAUS = (1.0, 0.05)
WEIGHTS = [(mu, tau) for tau in TAUS for mu in MUS]
# The LDS of csrc/zedo_joint_tree_marginal.hip: 48 J H + 16 H + 8192 <= 163840 bytes, H <= 1024 (zedo_joint_tree_marginal_max_h)
MAX_H = {1: 1024, 2: 1024, 3: 972, 17: 187, 64: 50}
# (J, N, H): _joint_tree_ref.CASES thinned to the smallest shapes on both sides of the kernel's constants, few poses each: the inner
# index of a bone is split over 4 parts of the workgroup up to H = 64 and over 2 up to H = 128, above that a lane owns the outer indices
# t, t + 256, ..: 64 | 65, 128 | 129, 256 | 257 (J small enough that the LDS admits them); splits with an empty last part (H = 3 and 2 over
# 4 parts); a wave serves joints w, w + 4, .. with hypotheses 64 at a time: J = 64; the largest H at J = 64, J = 17 and J = 2.
CASES = [(1, 1, 1), (2, 3, 2), (5, 12, 3), (17, 6, 50), (3, 4, 64), (3, 4, 65), (17, 2, 128), (17, 2, 129), (3, 2, 256), (2, 2, 257),
         (64, 2, MAX_H[64]), (17, 2, MAX_H[17]), (2, 1, MAX_H[2])]
IDS = [f"J{J}-N{N}-H{H}" for J, N, H in CASES]


def joint_tree_marginal_ref(junary, x, T, parent, mu, tau, N, weight=None, descending=False):
    """-> dict(w, lw [N,J,H] (lw = S + Dn - logZ, -inf where excluded), mean [N,J,3], cov [N,J,6], hmax [N,J] int32, wmax, logz, bone [N,J],
    live [N,J] bool, G, bmax, lmax): the definitions of the header, one pose after the other.  G = the largest finite magnitude any term
    of any log-sum-exp is made of (|S|, |M|, |Dn|, |E|, |logZ|, and c times the lengths the bone term is a difference of); bmax = the largest
    b, lmax = the largest mix + own of any pair of any bone.  descending: every sum over the hypotheses in the other order."""
    lse = lambda t: lse_ascending(t, descending)
    asum = lambda a: asc_sum(a, descending)
    parent = [int(v) for v in parent]
    J = len(parent)
    H = x.shape[0] // N
    u = unaries(junary, N, weight)                                 # [N,J,H], +inf where excluded
    ok = np.isfinite(u)
    with np.errstate(invalid="ignore"):
        l_all = np.where(ok, -u / tau, -np.inf)
    X = camera_frame(x, T, N)                                      # [H,N,J,3]
    order = post_order(parent)
    c = mu / tau
    w, lw = np.zeros((N, J, H)), np.full((N, J, H), -np.inf)
    mean, cov = np.full((N, J, 3), np.nan), np.full((N, J, 6), np.nan)
    hmax, wmax = np.zeros((N, J), np.int32), np.zeros((N, J))
    logz, bone = np.full((N, J), -np.inf), np.zeros((N, J))
    live_all = ok.any(2)
    G, bmax, lmax = 0.0, 0.0, 0.0

    def mag(a):
        nonlocal G
        a = np.abs(a[np.isfinite(a)])
        if a.size:
            G = max(G, float(a.max()))

    for n in range(N):
        Xn, l, live = X[:, n], l_all[n], live_all[n]
        S, M, Dn = l.copy(), {}, np.zeros((J, H))
        coupled = [g for g in order if parent[g] >= 0 and live[g] and live[parent[g]]]
        tabs = {}
        for g in coupled:                                          # upwards: children before parents, siblings ascending
            p = parent[g]
            b, mix, own = bone_table(Xn, g, p)                     # [hp, hc]
            tabs[g] = b
            bmax, lmax = max(bmax, float(b.max())), max(lmax, float((mix + 0.5 * (own[None, :] + own[:, None])).max()))
            M[g] = lse(S[g][None, :] - c * b)
            S[p] = S[p] + M[g]
            mag(M[g])
        mag(S)
        G = max(G, c * lmax)
        lz = np.full(J, -np.inf)
        for j in range(J):
            if live[j] and not (parent[j] >= 0 and live[parent[j]]):
                lz[j] = lse(S[j])
        for g in reversed(coupled):                                # downwards: parents before children
            p = parent[g]
            E = l[p]
            for k in sorted(k for k in coupled if parent[k] == p and k != g):
                E = E + M[k]
            E = E + Dn[p]
            b = tabs[g]
            Dn[g] = lse((E[:, None] - c * b).T)                    # [hc, hp]
            lz[g] = lz[p]
            mag(E)
            with np.errstate(invalid="ignore", over="ignore"):
                pi = np.exp(E[:, None] - c * b + S[g][None, :] - lz[g])                     # [hp, hc]
            pi[~np.isfinite(pi)] = 0.0
            bone[n, g] = asum(asum(pi * b))                        # over hp for every hc, then over hc
        mag(Dn)
        mag(lz)
        for j in range(J):
            if not live[j]:
                continue
            logz[n, j] = lz[j]
            with np.errstate(invalid="ignore"):
                lw[n, j] = np.where(ok[n, j], S[j] + Dn[j] - lz[j], -np.inf)
                w[n, j] = np.where(ok[n, j], np.exp(S[j] + Dn[j] - lz[j]), 0.0)
            Xj = Xn[:, j, :]
            m = asum(w[n, j][:, None] * Xj)
            d = Xj - m
            mean[n, j] = m
            cov[n, j] = [asum(w[n, j] * (d[:, a] * d[:, b_])) for a, b_ in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
            hmax[n, j] = int(np.argmax(w[n, j]))                   # the lowest h with the largest marginal
            wmax[n, j] = w[n, j, hmax[n, j]]
    return dict(w=w, lw=lw, mean=mean, cov=cov, hmax=hmax, wmax=wmax, logz=logz, bone=bone, live=live_all, G=G, bmax=bmax, lmax=lmax)


@functools.lru_cache(maxsize=None)
def reference(J, N, H, mu, tau, tree="default", with_T=True, with_weight=False):
    x, T, u = case(J, N, H)
    return joint_tree_marginal_ref(u, x, T if with_T else None, TREES[tree](J), mu, tau, N, confidences(N, J) if with_weight else None)


def enumerate_marginals(junary, x, T, parent, mu, tau, N, weight=None):
    """(w [N,J,H], logZ [N], bone [N,J]) by summing exp(-energy / tau) over all H^J assignments of every pose (_joint_tree_ref.energy;
    small cases only), shifted by the smallest energy.  A dead joint takes part in no term of the energy, so its H choices multiply Z by
    H: logZ has that factor taken out again and is the SUM of the log-partition values of the pose's components; w of a dead joint is 0."""
    J = len(parent)
    H = x.shape[0] // N
    live = np.isfinite(unaries(junary, N, weight)).any(2)
    X = camera_frame(x, T, N)
    assigns = np.array(list(itertools.product(range(H), repeat=J)), np.int64)                # [A, J]
    E = np.stack([energy(junary, x, T, parent, mu, N, np.repeat(a[None, :], N, 0), weight) for a in assigns])   # [A, N]
    Emin = E.min(axis=0)
    pw = np.exp(-(E - Emin) / tau)
    Z = pw.sum(axis=0)
    w, bone = np.zeros((N, J, H)), np.zeros((N, J))
    for n in range(N):
        p_a = pw[:, n] / Z[n]
        for j in range(J):
            if live[n, j]:
                w[n, j] = np.bincount(assigns[:, j], weights=p_a, minlength=H)
        for g in range(J):
            p = parent[g]
            if p >= 0 and live[n, g] and live[n, p]:
                bone[n, g] = float((p_a * bone_table(X[:, n], g, p)[0][assigns[:, p], assigns[:, g]]).sum())
    return w, -Emin / tau + np.log(Z) - (~live).sum(1) * np.log(H), bone


def marg_bound(J, H, G):
    """The absolute bound on the difference between two float64 evaluations of a log-marginal S + Dn - logZ, of logZ and of |sum_h w - 1|:
    4 J (H + 8 + 28 G) 2^-53, the form of _joint_marginal_ref.marg_bound with the tree's J in the place of the chain's L.

    One message is LSE_q (V[q] - c b).  With eps = 2^-53 and G the largest magnitude any such term is made of (the reference's `G`):
      - the terms: b = |mix - 0.5 (own_c + own_p)| is a difference of lengths that nearly cancel; by _joint_tree_ref.cost_bound's count a
        length goes through 9 roundings, the three lengths and the sum and the difference through 20 in units of the operands, so c b is
        within 21 eps c (mix + own) <= 21 eps G, the product by c and the subtraction from V one rounding each of numbers below G: 24 G eps
        on every term that carries weight (a term far below the maximum contributes its error times its vanishing weight), and an
        absolute error d in every term moves the LSE by at most d;
      - the exponentials: exp and log of the device library are good to 2 ulp each, the shift by the maximum is one rounding of a number
        below 1 where it matters, the combination of the parts of a split one exp and one product more: under 8 eps on the log;
      - the sum of H positive terms in ANY order: within H eps on the log.
    The messages meet in sums: S[p] takes each child's message in one addition (1 eps G); E_g is S[p] - M_g + Dn[p] in the kernel - the
    M_g that is subtracted is the very number that was added, so what remains of it is the rounding of the subtraction - and a sum over
    the other children in the reference: at most 3 roundings of numbers below G per bone either way; that is the 24 + 4 = 28.
    S[j] + Dn[j] is made of the J - 1 messages of the tree, each directed towards j and each formed once: its error is at most
    J (H + 8 + 28 G) eps.  logZ is one more LSE over the root's S, whose error is that of the messages below it: J (H + 8 + 28 G) eps again.
    The log-marginal therefore differs from the exact value by at most 2 J (H + 8 + 28 G) eps in each evaluation, and two evaluations
    from each other by twice that."""
    return 4.0 * J * (H + 8.0 + 28.0 * G) * 2.0 ** -53


def bone_bound(beta, bmax, lmax):
    """|bone - bone_ref| in metres, given that every log pair marginal is within beta (pi is made of the same messages as w, one LSE
    less): sum (pi - pi_ref) b <= (e^beta - 1)(1 + beta) bmax for pair marginals that sum to 1 within beta; b itself is within 20 2^-53
    lmax (see marg_bound) in either evaluation; the sums of H^2 products add 2 (H + 1) 2^-53 bmax, below beta bmax because beta >=
    4 (H + 8) 2^-53.  -> 2 (e^beta - 1)(1 + beta) bmax + 40 2^-53 lmax."""
    return 2.0 * np.expm1(beta) * (1.0 + beta) * bmax + 40.0 * 2.0 ** -53 * lmax


def concentrated_mean_bound(w, h, X):
    """[N,J]: what |mean - X[h]| stays under per coordinate when the weights w [N,J,H] sit on the hypothesis h [N,J], from the weights
    THEMSELVES and not from marg_bound (which scales with G and says nothing at a temperature where G is 1e11): with X [H,N,J,3],
      sum_k w_k X_k - X_h = (sum_k w_k - 1) X_h + sum_{k != h} w_k (X_k - X_h),
    so |mean - X_h| <= |sum w - 1| max|X_h| + (sum_{k != h} w_k) spread, and the fp64 sum of H products adds (H + 2) 2^-53 max|X|."""
    H = w.shape[2]
    wh = np.take_along_axis(w, h[:, :, None].astype(np.int64), 2)[:, :, 0]
    rest = np.where(np.arange(H)[None, None, :] == h[:, :, None], 0.0, w).sum(2)
    Xh = np.take_along_axis(X.transpose(1, 2, 0, 3), h[:, :, None, None].astype(np.int64), 2)[:, :, 0]          # [N,J,3]
    spread = (X.max(axis=0) - X.min(axis=0)).max(axis=-1)
    return np.abs(wh + rest - 1.0) * np.abs(Xh).max(-1) + rest * spread + (H + 2) * 2.0 ** -53 * np.abs(X).max()


def concentrated_bone_bound(w, h, parent, b_sel, beta, G, bmax, lmax):
    """[N,J]: what |bone - b_sel| stays under when the weights sit on the assignment h, b_sel [N,J] = b of every bone at that assignment
    (zedo_joint_tree_select's bone), again from the weights themselves.  bone = sum pi b over the pairs; with * the kept pair,
      bone - b* = (pi* - 1) b* + sum_{pairs != *} pi b.
    Exactly, pi* <= w_g[h_g] and the other pairs hold at most rest_g + rest_p of the mass (rest_j = sum_{k != h_j} w[j,k]); the weights
    that small are good to a factor e^beta.  The computed pi* and the computed w_g[h_g] are exp of the same three numbers below G added
    in another order: they differ by at most 4 2^-53 G relative.  b is within 20 2^-53 lmax in either evaluation.
    pi* falls short of w_g[h_g] by the pairs (hp != h_p, h_g): at most rest_p more.
      -> (|w_g[h_g] - 1| + 4 2^-53 G) b* + e^beta (rest_g + 2 rest_p) bmax + 40 2^-53 lmax;  0 for a joint without a parent."""
    H = w.shape[2]
    wh = np.take_along_axis(w, h[:, :, None].astype(np.int64), 2)[:, :, 0]
    rest = np.where(np.arange(H)[None, None, :] == h[:, :, None], 0.0, w).sum(2)
    out = np.zeros(wh.shape)
    for g, p in enumerate(parent):
        if p >= 0:
            out[:, g] = (np.abs(wh[:, g] - 1.0) + 4 * 2.0 ** -53 * G) * b_sel[:, g] + np.exp(beta) * (rest[:, g] + 2.0 * rest[:, p]) * bmax + 40 * 2.0 ** -53 * lmax
    return out


def clear_argmax(r, beta):
    """[N,J] bool: the live (pose, joint) whose two largest reference marginals differ by more than 2 beta in the logarithm - where two
    evaluations within beta of the exact value must agree on the arg-max."""
    H = r["w"].shape[2]
    if H == 1:
        return r["live"].copy()
    top2 = np.sort(r["lw"], axis=2)[:, :, -2:]
    with np.errstate(invalid="ignore"):
        return r["live"] & (top2[:, :, 1] - top2[:, :, 0] > 2 * beta)
