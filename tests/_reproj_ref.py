"""The float64 reference of the closed-form reprojection correction (reproj_row<17>, csrc/zedo_internal.h), the bound an fp32
implementation of it is held to, and the input families of tests/test_reproj_ref.py (CPU: reference, bound and families pinned) and
tests/test_reproj_accuracy_gpu.py / tests/test_reproj_fused_gpu.py (every launch form of the kernel held to them).  numpy only.

The operation, per row (pose n of the row, joints j, geom[n][j] = {r_x, r_y, W, 0, rhat_x, rhat_y, rhat_z, 0} taken as EXACT input:
the rounding of zedo_reproj_prepare is pinned to 1 ulp elsewhere and is not counted twice when the array is read back from the device):

  b_j = x_xy,j - x_z,j r_j,   rbar = sum W r / sum W,   bbar = sum W b / sum W,   d_j = r_j - rbar
  T_z = sum W [d_x (b_x - bbar_x) + d_y (b_y - bbar_y)] / den,   den = sum W (d_x^2 + d_y^2)
  T_xy = rbar T_z - bbar;   T <- -T if T_z < 0;   g_j = ((x_j + T) . rhat_j) rhat_j - (x_j + T)

The bound, with u = 2^-24 (every quantity below in float64, from solve()):

  bound_Tz  = C_T u (A / den + |T_z|),   A = sum W (|d_x| (|b_x| + |bbar_x|) + |d_y| (|b_y| + |bbar_y|))
              every term of the numerator is formed from d (u relative) and b - bbar (u (|b| + |bbar|) absolute: b is rounded at its
              own size and so is the mean), A is the sum of the terms' magnitudes before anything cancels, and the quotient and the
              denominator add u |T_z| each.  A / den is the condition number that grows when the rays of the joints that carry the
              weight draw together or the pose sits far from the origin.
  bound_Txy = C_T u (max(sum W |b_x|, sum W |b_y|) / sum W + max(sum W |r_x|, sum W |r_y|) / sum W |T_z|) + max(|rbar_x|, |rbar_y|) bound_Tz
              the two weighted means at the size of their terms, then T_z's own error carried through rbar T_z.
  bound_g   = ||(bound_Txy, bound_Txy, bound_Tz)||_2 + C_g u ||x_j + T||_1
              T -> g is (rhat rhat^T - I), a contraction: the error of T passes through at most unchanged; the second term is the
              rounding of x + T, of the dot product and of the final difference, all at the size of the point.  With T given only the
              second term applies.

C_T and C_g are 4 x the largest share of the C = 1 bound that emulate_f32 - the fp32 numpy statement of the formula, sequential sums,
every product rounded - uses over all families at the shape the GPU tests run (FAMILY_N x FAMILY_H), rounded up to an integer.  The 4
allows for what the emulation does not model (another summation order or register allocation in a fused epilogue, a contraction the
compiler may introduce).  They are never fitted to a kernel; tests/test_reproj_ref.py re-measures the shares and holds them under 1/4."""
import numpy as np

U24 = 2.0 ** -24
EMUL_SHARE_T = 2.838         # emulate_f32's largest share of the C = 1 bounds on T over all families (T_z 2.838 on far/uniform, T_xy 2.71)
EMUL_SHARE_G = 2.397         # ... and of u ||x + T||_1 on g with T given (std/none); tests/test_reproj_ref.py re-measures both (-s prints them)
C_T = int(np.ceil(4 * EMUL_SHARE_T))
C_G = int(np.ceil(4 * EMUL_SHARE_G))
SIGN_MARGIN = 64             # |T_z| >= SIGN_MARGIN bound_Tz on every row of every family: the sign fix is never in doubt

J = 17
FAMILY_N, FAMILY_H = 67, 3   # B = 201: two workgroups of reproj_grad_kernel, a tail of 73 rows
DEPTH_F = dict(near=(2.0, 600.0), std=(5.0, 1100.0), far=(50.0, 1100.0), tele=(5.0, 12000.0))
FAMILIES = ([f"{d}/{c}" for d in DEPTH_F for c in ("none", "uniform", "two")]
            + ["std/two-adjacent", "offset/std", "offset/far", "mirrored", "general"])
UNCENTRED_MUST_FAIL = [f for f in FAMILIES if f.endswith("/two") or f.startswith("far/") or f.startswith("offset/") or f == "std/two-adjacent"]
OFFSET = np.array([1.0, -1.0, 2.0])


# ---- inputs --------------------------------------------------------------------------------------------------------------

def prepare(uv, K, conf=None):
    """zedo_reproj_prepare in numpy: geom [N,17,8] float32 (rays in float64, rounded once; W = (c c)(c c) in fp32 of the clamped c).
    For the CPU tests; the GPU tests read the device's array back."""
    uv, K = np.asarray(uv, np.float64), np.asarray(K, np.float64)
    N, Jn = uv.shape[:2]
    hom = np.concatenate([uv, np.ones((N, Jn, 1))], -1)
    ray = np.einsum("nij,nkj->nki", np.linalg.inv(K), hom)
    r = ray[..., :2] / ray[..., 2:]
    rn = 1.0 / np.sqrt((r * r).sum(-1) + 1.0)
    geom = np.zeros((N, Jn, 8), np.float32)
    geom[..., 0:2] = r
    geom[..., 2] = 1.0
    if conf is not None:
        c = np.asarray(conf, np.float32)
        c = np.where(c > 1, np.float32(1), c)
        c = np.where(c < np.float32(1e-4), np.float32(1e-4), c)
        w = c * c
        geom[..., 2] = w * w
    geom[..., 4:6] = r * rn[..., None]
    geom[..., 6] = rn
    return geom


def family(name, N=FAMILY_N, H=FAMILY_H):
    """-> dict(name, N, H, uv [N,17,2], K [N,3,3], conf [N,17] or None, x [H N,17,3] (row h N + n is hypothesis h of pose n),
    T_given [H N,3]), float32.  Stream: numpy Philox, key [61, index of the name in FAMILIES].

    N poses (0.25 m N(0,1) per coordinate, root at the origin) stand at depth (1 + 0.1 N(0,1)), anywhere within 0.4 depth to either
    side and up or down (a 22 degree half field: the mean ray is as large as the rays' spread or larger, as in any uncropped frame);
    detections = their projection + 2 px noise; x = the root-relative pose + 5 cm noise per hypothesis; T_given = the root + 5 cm.
    depth, focal length: DEPTH_F (the focal entries of _shared.cameras times f / 1145).  Confidences: none / uniform(-0.2, 1.2) (both
    clamps) / two (15 joints at 1e-4, two random ones at 1).  two-adjacent: the two confident joints are the pair of the pose that is
    farthest apart in x, y and the second one's detection lies 3 px from the first one's, in the direction the pose gives.
    offset/*: x shifted by (1, -1, 2) m.  mirrored: the detections reflected through the principal point.  general: std through
    _shared.general_cameras (focal lengths as it draws them)."""
    from _shared import cameras, general_cameras
    k = FAMILIES.index(name)
    g = np.random.Generator(np.random.Philox(key=[61, k]))
    head, _, tail = name.partition("/")
    depth_key = tail if head == "offset" else head if head in DEPTH_F else "std"
    conf_mode = tail if head in DEPTH_F else "uniform"
    depth, f = DEPTH_F[depth_key]
    if name == "general":
        K = general_cameras(g, N)
    else:
        K = cameras(g, N)
        K[:, 0, 0] *= np.float32(f / 1145.0)
        K[:, 1, 1] *= np.float32(f / 1145.0)
    pose = 0.25 * g.standard_normal((N, J, 3))
    pose[:, 0] = 0.0
    root = np.stack([depth * g.uniform(-0.4, 0.4, N), depth * g.uniform(-0.4, 0.4, N), depth * (1 + 0.1 * g.standard_normal(N))], -1)
    w = np.einsum("nij,nkj->nki", K.astype(np.float64), pose + root[:, None])
    uv = w[..., :2] / w[..., 2:] + 2.0 * g.standard_normal((N, J, 2))
    conf = None
    if conf_mode == "uniform":
        conf = g.uniform(-0.2, 1.2, (N, J))
    elif conf_mode in ("two", "two-adjacent"):
        conf = np.full((N, J), 1e-4)
        if conf_mode == "two":
            pair = np.argsort(g.random((N, J)), axis=1)[:, :2]
        else:
            d2 = ((pose[:, :, None, :2] - pose[:, None, :, :2]) ** 2).sum(-1).reshape(N, -1)
            pair = np.stack(np.unravel_index(d2.argmax(1), (J, J)), -1)
            n = np.arange(N)
            dirn = pose[n, pair[:, 1], :2] - pose[n, pair[:, 0], :2]
            uv[n, pair[:, 1]] = uv[n, pair[:, 0]] + 3.0 * dirn / np.linalg.norm(dirn, axis=1, keepdims=True)
        conf[np.arange(N)[:, None], pair] = 1.0
    if name == "mirrored":
        uv = 2.0 * K[:, None, :2, 2].astype(np.float64) - uv
    x = pose[None] + 0.05 * g.standard_normal((H, N, J, 3))
    if head == "offset":
        x = x + OFFSET
    T = root[None] + 0.05 * g.standard_normal((H, N, 3))
    return dict(name=name, N=N, H=H, uv=uv.astype(np.float32), K=K.astype(np.float32), conf=None if conf is None else conf.astype(np.float32),
                x=x.reshape(H * N, J, 3).astype(np.float32), T_given=T.reshape(H * N, 3).astype(np.float32))


def _rows(x, geom, row_offset):
    """geom rows of the poses of x's rows: pose of row b = (row_offset + b) mod N."""
    x = np.asarray(x)
    n = (int(row_offset) + np.arange(x.shape[0])) % geom.shape[0]
    return x, np.asarray(geom)[n]


# ---- float64 -------------------------------------------------------------------------------------------------------------

def solve(x, geom, T=None, row_offset=0, c_t=None, c_g=None):
    """float64 on fp32 inputs taken as exact.  T None: the least-squares T (sign fix included; T_unfixed: before it), else g for the given
    T.  -> dict(T [B,3], T_unfixed, g [B,17,3], den, A, bound_Tz [B], bound_Txy [B], bound_g [B,17])."""
    c_t, c_g = C_T if c_t is None else c_t, C_G if c_g is None else c_g
    x, gm = _rows(x, geom, row_offset)
    x, gm = x.astype(np.float64), gm.astype(np.float64)
    r, W, rh = gm[..., 0:2], gm[..., 2], gm[..., 4:7]
    out = {}
    if T is None:
        b = x[..., :2] - x[..., 2:] * r
        sw = W.sum(1)
        rbar = (W[..., None] * r).sum(1) / sw[:, None]
        bbar = (W[..., None] * b).sum(1) / sw[:, None]
        d = r - rbar[:, None]
        den = (W * (d * d).sum(-1)).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tz = (W * (d * (b - bbar[:, None])).sum(-1)).sum(1) / den
            A = (W * (np.abs(d) * (np.abs(b) + np.abs(bbar)[:, None])).sum(-1)).sum(1)
            Tu = np.concatenate([rbar * tz[:, None] - bbar, tz[:, None]], 1)
            T = np.where(tz[:, None] < 0, -Tu, Tu)
            bz = c_t * U24 * (A / den + np.abs(tz))
            bxy = (c_t * U24 * ((W[..., None] * np.abs(b)).sum(1).max(1) / sw + (W[..., None] * np.abs(r)).sum(1).max(1) / sw * np.abs(tz))
                   + np.abs(rbar).max(1) * bz)
        out.update(T_unfixed=Tu, den=den, A=A, bound_Tz=bz, bound_Txy=bxy)
        carried = np.sqrt(2 * bxy * bxy + bz * bz)
    else:
        T = np.asarray(T, np.float64)
        carried = np.zeros(len(x))
    p = x + T[:, None]
    out["T"] = T
    out["g"] = (p * rh).sum(-1, keepdims=True) * rh - p
    out["bound_g"] = carried[:, None] + c_g * U24 * np.abs(p).sum(-1)
    return out


def solve_normal_equations(x, geom, row_offset=0):
    """The same T by an independent float64 route: np.linalg.lstsq on the c^2-scaled A and b of oracle/zedo_oracle.py::gradient_field_gen
    (c^2 = sqrt(W)), one row at a time; sign fix included."""
    x, gm = _rows(x, geom, row_offset)
    x, gm = x.astype(np.float64), gm.astype(np.float64)
    B = len(x)
    T = np.zeros((B, 3))
    for i in range(B):
        r, c2 = gm[i, :, 0:2], np.sqrt(gm[i, :, 2])
        A = np.zeros((2 * J, 3))
        b = np.zeros(2 * J)
        b[0::2] = x[i, :, 0] - x[i, :, 2] * r[:, 0]
        b[1::2] = x[i, :, 1] - x[i, :, 2] * r[:, 1]
        A[0::2, 0], A[0::2, 2] = -1, r[:, 0]
        A[1::2, 1], A[1::2, 2] = -1, r[:, 1]
        s = np.repeat(c2, 2)
        t = np.linalg.lstsq(A * s[:, None], b * s, rcond=None)[0]
        T[i] = -t if t[2] < 0 else t
    return T


# ---- fp32 ----------------------------------------------------------------------------------------------------------------

def emulate_f32(x, geom, variant=None, T=None, row_offset=0):
    """The formula in fp32 numpy, rows in parallel, joints one after the other, every product and sum rounded: a reference
    implementation (what a faithful fp32 kernel is expected to reach), not the code under test.  variant "uncentred": the numerator
    without the centring of b, d_x b_x + d_y b_y - algebraically the same (sum W d = 0).  -> (T [B,3], g [B,17,3]) float32."""
    assert variant in (None, "uncentred")
    x, gm = _rows(x, geom, row_offset)
    x, gm = x.astype(np.float32), gm.astype(np.float32)
    B = len(x)
    z = np.zeros(B, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if T is None:
            sw, srx, sry, sbx, sby = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
            bx = x[:, :, 0] - x[:, :, 2] * gm[:, :, 0]
            by = x[:, :, 1] - x[:, :, 2] * gm[:, :, 1]
            for j in range(J):
                a0, a1, a2 = gm[:, j, 0], gm[:, j, 1], gm[:, j, 2]
                sw = sw + a2
                srx, sry = srx + a2 * a0, sry + a2 * a1
                sbx, sby = sbx + a2 * bx[:, j], sby + a2 * by[:, j]
            iw = np.float32(1) / sw
            mrx, mry, mbx, mby = srx * iw, sry * iw, sbx * iw, sby * iw
            num, den = z.copy(), z.copy()
            for j in range(J):
                a0, a1, a2 = gm[:, j, 0], gm[:, j, 1], gm[:, j, 2]
                dx, dy = a0 - mrx, a1 - mry
                if variant == "uncentred":
                    num = num + a2 * (dx * bx[:, j] + dy * by[:, j])
                else:
                    num = num + a2 * (dx * (bx[:, j] - mbx) + dy * (by[:, j] - mby))
                den = den + a2 * (dx * dx + dy * dy)
            tz = num / den
            tx, ty = mrx * tz - mbx, mry * tz - mby
            neg = tz < 0
            T = np.stack([np.where(neg, -tx, tx), np.where(neg, -ty, ty), np.where(neg, -tz, tz)], 1)
        T = np.asarray(T, np.float32)
        p = x + T[:, None]
        rh = gm[:, :, 4:7]
        d = (p[..., 0] * rh[..., 0] + p[..., 1] * rh[..., 1]) + p[..., 2] * rh[..., 2]
        g = d[..., None] * rh - p
    assert T.dtype == np.float32 and g.dtype == np.float32
    return T, g


def shares(T, g, ref, given=False):
    """Largest share of each bound that (T, g) uses against ref = solve(...): dict(tz, txy, g); every row and joint counted."""
    T, g = np.asarray(T, np.float64), np.asarray(g, np.float64)
    out = dict(g=float((np.abs(g - ref["g"]).max(-1) / ref["bound_g"]).max()))
    if not given:
        out["tz"] = float((np.abs(T[:, 2] - ref["T"][:, 2]) / ref["bound_Tz"]).max())
        out["txy"] = float((np.abs(T[:, :2] - ref["T"][:, :2]).max(1) / ref["bound_Txy"]).max())
    return out


def assert_within(T, g, ref, given=False):
    """Every row of (T, g) within the bounds of ref = solve(...), none left out (the sign of T_z beyond doubt); -> shares."""
    T, g = np.asarray(T, np.float64), np.asarray(g, np.float64)
    s = shares(T, g, ref, given)
    assert np.isfinite(T).all() and np.isfinite(g).all()
    if not given:
        assert (np.abs(ref["T_unfixed"][:, 2]) >= SIGN_MARGIN * ref["bound_Tz"]).all()
        assert (np.abs(T[:, 2] - ref["T"][:, 2]) <= ref["bound_Tz"]).all(), s
        assert (np.abs(T[:, :2] - ref["T"][:, :2]) <= ref["bound_Txy"][:, None]).all(), s
    assert (np.abs(g - ref["g"]) <= ref["bound_g"][..., None]).all(), s
    return s
