"""The float64 reference of zedo_min_reproj (include/zedo_hip.h), stated directly in numpy: the confidence-weighted mean reprojection
distance of x + T in pixels per row, and the per-pose minimum over the hypotheses of a row shard.  Pinned on its own by
tests/test_select_reproj_ref.py; the GPU tests hold the kernels to it."""
import numpy as np


def reproj_ref(x, T, uv, K, conf=None, row_offset=0):
    """x [B,J,3], T [B,3], uv [N,J,2], K [N,3,3], conf [N,J] or None (fp32 inputs; fp64 ones are taken as they are) -> err [B] float64.
    Local row b belongs to pose (row_offset + b) % N.  A row with a joint at q.z <= 0 is +inf; NaN falls through that test."""
    x, T, uv, K = (np.asarray(a, dtype=np.float64) for a in (x, T, uv, K))
    n = (int(row_offset) + np.arange(x.shape[0])) % uv.shape[0]
    X = x + T[:, None, :]
    k = K[n][:, None, :, :]                                       # [B,1,3,3]
    q = k[..., 0] * X[..., 0:1] + k[..., 1] * X[..., 1:2] + k[..., 2] * X[..., 2:3]          # the full 3x3 product, [B,J,3]
    with np.errstate(all="ignore"):
        p = q[..., :2] / q[..., 2:]
        d = np.sqrt(((p - uv[n]) ** 2).sum(-1))
        w = np.ones(d.shape)
        if conf is not None:                                      # the clamp of gradient_field_gen, in fp32, first power
            c = np.array(conf, dtype=np.float32)
            c[c > 1] = 1
            c[c < np.float32(1e-4)] = np.float32(1e-4)
            w = c.astype(np.float64)[n]
        err = (w * d).sum(1) / w.sum(1)
    err[(q[..., 2] <= 0).any(1)] = np.inf
    return err


def select_ref(err, N, row_offset=0):
    """np.amin / np.argmin per pose over the local rows: NaN wins (lowest NaN hypothesis), ties to the lower hypothesis, a pose
    without a local row reports (+inf, -1).  -> (best [N] float64, idx [N] int32)."""
    best, idx = np.full(N, np.inf), np.full(N, -1, np.int32)
    g = int(row_offset) + np.arange(len(err))
    for n in range(N):
        loc = np.flatnonzero(g % N == n)
        if loc.size:
            k = loc[np.argmin(err[loc])]                          # np.argmin: the first NaN if there is one, else the first minimum
            best[n], idx[n] = err[k], g[k] // N
    return best, idx
