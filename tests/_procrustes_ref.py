"""The 50-digit reference of the two row errors of zedo_min_mpjpe (include/zedo_hip.h) and the bound a float64 implementation is
held to against it.  tools/gen_procrustes_reference.py writes tests/golden/procrustes_hp.npz with hp_row; tests/test_procrustes_ref.py
pins the fixture, the bound and the float64 numpy oracle's place inside it; tests/test_procrustes_gpu.py holds the kernels to it.

P1 (MPJPE): e = mean_j |p_j - g_j|.  P2 (PA-MPJPE): the same after procrustes(A = gt, B = pred, scaling, reflection = 'best'):
M = A0^T B0 / (|A0| |B0|) = U diag(sigma) V^T, R = V U^T, s = |A0| (sigma1 + sigma2 + sigma3) / |B0|, Z = s B0 R + mean(A).

The bound, with u = 2^-53, J joints, C = max|gt| + s max|pred| (the magnitude the differences are formed from):

  P1:  c1 u (C + J e)            each difference carries u C, each of the J terms of the mean and the sum itself u e.
  P2, resolved rows (sigma3 / sigma1 >= 1e-12):
       c2 J u (C + e) / max(sigma2 + sigma3, u)
                                 M is a sum of J products (J u relative to its norm); 1 / (sigma2 + sigma3) is the condition number of
                                 the orthogonal polar factor of M when a reflection is allowed; the rotation error moves the
                                 aligned joints (size <= C) and the J-term mean adds u e per term.
  P2, unresolved rows (sigma3 / sigma1 < 1e-12, exact rank deficiency included): the smaller of
       plane:  the resolved bound with sigma3 = 0, plus 2 t,  t = sqrt(lambda_3(A0^T A0)) + s sqrt(lambda_3(B0^T B0)):
                                 no float64 algorithm can fix the sign of the thinnest direction there, and flipping that sign
                                 moves each aligned joint by at most twice its distance from the plane (both sets': the thickness t).
       line:   c2 J u (C + e) / max(sigma1 - sigma2, u), plus 2 t1,  t1 = sqrt((lambda_2 + lambda_3)(A0^T A0)) + s sqrt((same)(B0^T B0)):
                                 towards rank 1 sigma2 + sigma3 goes to zero with the product of the two thicknesses and the plane
                                 form grows without limit (metres at f = 1e-8 on the needle ladder), although only the first
                                 pair of singular vectors matters then: its gap to the rest is sigma1 - sigma2, and ANY orthogonal
                                 completion moves each aligned joint by at most twice its distance from the line.  Never larger
                                 than the plane form where it applies: a stricter bound, needed for the needle ladder's arg-min.

c1, c2 are 8 x the largest ratio the float64 numpy oracle (zedo_oracle.hypothesis_errors, the LAPACK route) needs on the fixture
(profiles/procrustes_accuracy.txt has the ratios per family): the 8 allows for a different but equally backward-stable SVD and
another summation order.  They are never fitted to a kernel."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "procrustes_hp.npz")

U53 = 2.0 ** -53
RESOLVED = 1e-12                      # sigma3 / sigma1 at and above which the sign of the third direction counts as known
ORACLE_RATIO_P1 = 0.374               # the oracle's largest |error| / (u (C + J e)) on the fixture, rounded up (measured: see the profile)
ORACLE_RATIO_P2 = 0.145               # the oracle's largest (|error| - 2 t [unresolved rows]) / (J u (C + e) / max(sigma2 + sigma3, u))
C1 = 8 * ORACLE_RATIO_P1
C2 = 8 * ORACLE_RATIO_P2
H = 4                                 # hypotheses per pose of the fixture
FAMILIES = {1: "ordinary", 2: "mirrored", 3: "similar", 4: "units and offset", 5: "equal singular values", 6: "flatness ladder",
            7: "needle ladder", 8: "uncorrelated"}


def bound_p1(C, J, e, c1=None):
    return (C1 if c1 is None else c1) * U53 * (np.asarray(C) + np.asarray(J) * np.asarray(e))


def resolved(sigma):
    sigma = np.asarray(sigma)
    return sigma[..., 2] >= RESOLVED * sigma[..., 0]


def bound_p2_parts(C, J, e, sigma, t, t1, c2=None):
    """-> (the conditioning term, the thickness term: zero on resolved rows) of the form that gives the smaller sum."""
    sigma = np.asarray(sigma)
    res = resolved(sigma)
    num = (C2 if c2 is None else c2) * np.asarray(J) * U53 * (np.asarray(C) + np.asarray(e))
    plane = num / np.maximum(sigma[..., 1] + np.where(res, sigma[..., 2], 0.0), U53)
    line = num / np.maximum(sigma[..., 0] - sigma[..., 1], U53)
    flip, flip1 = np.where(res, 0.0, 2.0 * np.asarray(t)), 2.0 * np.asarray(t1)
    use_line = ~res & (line + flip1 < plane + flip)
    return np.where(use_line, line, plane), np.where(use_line, flip1, flip)


def bound_p2(C, J, e, sigma, t, t1, c2=None):
    base, flip = bound_p2_parts(C, J, e, sigma, t, t1, c2)
    return base + flip


def stats64(pred, gt):
    """What the bound needs, in float64 from the inputs themselves (for tests whose inputs are not in the fixture): pred [..., J, 3],
    gt [..., J, 3] -> dict(e1, e2, sigma [..., 3], s, C, t, t1).  The quantities enter the bound to first order only.  One joint has no
    alignment (0 / 0): s counts as 1 there, which leaves the P1 bound defined."""
    import zedo_oracle as O
    A, B = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    A0, B0 = A - A.mean(-2, keepdims=True), B - B.mean(-2, keepdims=True)
    An, Bn = np.sqrt((A0 ** 2).sum((-1, -2))), np.sqrt((B0 ** 2).sum((-1, -2)))
    if A.shape[-2] == 1:
        sigma, s, Z = np.zeros(A.shape[:-2] + (3,)), np.ones(A.shape[:-2]), A
        return dict(e1=np.sqrt(((B - A) ** 2).sum(-1)).mean(-1), e2=np.full(A.shape[:-2], np.nan), sigma=sigma, s=s,
                    C=np.abs(A).max((-1, -2)) + np.abs(B).max((-1, -2)), t=np.zeros(A.shape[:-2]), t1=np.zeros(A.shape[:-2]))
    sigma = np.linalg.svd(np.swapaxes(A0, -1, -2) @ B0 / (An * Bn)[..., None, None], compute_uv=False)
    s = An * sigma.sum(-1) / Bn
    def thin(X, k=1):                                                  # sqrt of the k smallest eigenvalues of X^T X, from X's own singular
        sv = np.linalg.svd(X, compute_uv=False)                         # values (the Gram matrix would floor them at 1e-8 of the largest)
        sv = np.concatenate([sv, np.zeros(sv.shape[:-1] + (max(0, 3 - sv.shape[-1]),))], -1)
        return np.sqrt((np.sort(sv, -1)[..., :k] ** 2).sum(-1))
    Z = O.procrustes_align(A, B)
    return dict(e1=np.sqrt(((B - A) ** 2).sum(-1)).mean(-1), e2=np.sqrt(((Z - A) ** 2).sum(-1)).mean(-1), sigma=sigma, s=s,
                C=np.abs(A).max((-1, -2)) + s * np.abs(B).max((-1, -2)), t=thin(A0) + s * thin(B0), t1=thin(A0, 2) + s * thin(B0, 2))


def bounds64(pred, gt):
    """-> (P1 bound, P2 bound) of every row, from stats64."""
    st = stats64(pred, gt)
    J = np.asarray(gt).shape[-2]
    return bound_p1(st["C"], J, st["e1"]), bound_p2(st["C"], J, st["e2"], st["sigma"], st["t"], st["t1"])


def hp_row(pred, gt, dps=50):
    """One row in mpmath at `dps` digits: pred [J,3] float32, gt [J,3] float64 (both taken exactly) ->
    dict(e1, e2, sigma (3), s, C, t, t1), every value rounded once to float64."""
    import mpmath as mp
    with mp.workdps(dps):
        J = len(gt)
        A = mp.matrix([[mp.mpf(float(v)) for v in r] for r in np.asarray(gt, np.float64)])
        B = mp.matrix([[mp.mpf(float(v)) for v in r] for r in np.asarray(pred, np.float32)])
        dist = lambda X, Y: sum(mp.sqrt(sum((X[j, c] - Y[j, c]) ** 2 for c in range(3))) for j in range(J)) / J
        e1 = dist(B, A)
        ones = mp.matrix([[1]] * J)
        Ab, Bb = (ones.T * A) / J, (ones.T * B) / J
        A0, B0 = A - ones * Ab, B - ones * Bb
        An, Bn = mp.sqrt(sum(x * x for x in A0)), mp.sqrt(sum(x * x for x in B0))
        Uu, S, Vt = mp.svd_r(A0.T * B0 / (An * Bn))
        S = sorted((S[i] for i in range(3)), reverse=True)
        s = An * sum(S) / Bn
        e2 = dist(s * (B0 * (Vt.T * Uu.T)) + ones * Ab, A)
        thin = lambda X, k: mp.sqrt(max(mp.mpf(0), sum(sorted(mp.eigsy(X.T * X, eigvals_only=True))[:k])))
        t, t1 = thin(A0, 1) + s * thin(B0, 1), thin(A0, 2) + s * thin(B0, 2)
        C = max(abs(x) for x in A) + s * max(abs(x) for x in B)
        return dict(e1=float(e1), e2=float(e2), sigma=np.array([float(x) for x in S]), s=float(s), C=float(C), t=float(t), t1=float(t1))


def load():
    """The fixture as a dict of arrays (rows in pose-major order: row = 4 pose + hypothesis)."""
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def groups(fx):
    """The fixture per joint count, in the layout of zedo_min_mpjpe: {J: (rows [H N] fixture rows in (h, n) order, pred [H N,J,3] fp32,
    gt [N,J,3] fp64)} - local row h N + n is hypothesis h of the n-th pose of that joint count."""
    out = {}
    for J in sorted(set(int(j) for j in fx["J"])):
        poses = np.flatnonzero(fx["pose_J"] == J)
        rows = np.array([np.flatnonzero((fx["pose"] == p) & (fx["hyp"] == h))[0] for h in range(H) for p in poses])
        out[J] = (rows, np.ascontiguousarray(fx["pred"][rows][:, :J]), np.ascontiguousarray(fx["gt"][poses][:, :J]))
    return out


def row_bounds(fx):
    """-> (P1 bound, P2 bound) of every fixture row, from the stored 50-digit quantities."""
    return (bound_p1(fx["C"], fx["J"], fx["err_p1_hp"]), bound_p2(fx["C"], fx["J"], fx["err_p2_hp"], fx["sigma"], fx["t"], fx["t1"]))


def oracle_rows(fx):
    """zedo_oracle.hypothesis_errors on every fixture row -> (P1 [R], P2 [R])."""
    import zedo_oracle as O
    e1, e2 = np.empty(len(fx["J"])), np.empty(len(fx["J"]))
    for J, (rows, pred, gt) in groups(fx).items():
        N = len(gt)
        p = np.swapaxes(pred.reshape(H, N, J, 3), 0, 1)
        e1[rows] = O.hypothesis_errors(p, gt, False).T.reshape(-1)
        e2[rows] = O.hypothesis_errors(p, gt, True).T.reshape(-1)
    return e1, e2


def needed_ratios(fx, e1, e2):
    """What c1 and c2 would have to be for the values e1, e2 to sit exactly on the bound, per row (0 where the 2 t term alone covers a
    P2 deviation)."""
    r1 = np.abs(e1 - fx["err_p1_hp"]) / bound_p1(fx["C"], fx["J"], fx["err_p1_hp"], c1=1.0)
    base, flip = bound_p2_parts(fx["C"], fx["J"], fx["err_p2_hp"], fx["sigma"], fx["t"], fx["t1"], c2=1.0)
    return r1, np.maximum(np.abs(e2 - fx["err_p2_hp"]) - flip, 0.0) / base


def separation(fx):
    """Per pose and protocol: (runner-up - minimum) of the 50-digit errors over the largest bound among the pose's rows -> [P, 2]."""
    b1, b2 = row_bounds(fx)
    out = []
    for p in range(len(fx["pose_J"])):
        r = np.flatnonzero(fx["pose"] == p)
        out.append([(np.sort(e[r])[1] - np.sort(e[r])[0]) / b[r].max() for e, b in ((fx["err_p1_hp"], b1), (fx["err_p2_hp"], b2))])
    return np.array(out)
