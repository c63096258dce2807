"""The float64 reference of the joint-wise aggregation (zedo_joint_reproj / zedo_joint_compose, include/zedo_hip.h), stated directly in
numpy: every row's per-joint reprojection distance of x + T in pixels, the per-(pose, joint) minimum over the hypotheses of a row shard
(select_ref of tests/_select_ref.py on the flattened vector) and the compose formula; plus the inputs the CPU and GPU tests share.
Pinned on its own by tests/test_joint_reproj_ref.py; the GPU tests hold the kernels to it."""
import functools

import numpy as np

from _select_ref import select_ref

CASES = [(1, 1, 1), (1, 3, 2), (5, 3, 5), (17, 1, 5), (17, 64, 5), (17, 70, 5), (21, 70, 3), (17, 300, 7)]
# what the table above stays below (csrc/zedo_metric.hip): the walking kernel has one lane per (pose, joint) - J = 64: a pose's lanes are
# exactly one wavefront, 65: they straddle two, 33 with N = 70: 2310 lanes, ten workgroups with a tail; the row route hands
# launch_pose_min N J "poses" - 17 x 483 = 8211 >= POSE_MIN_LANE_N = 8192: the lane-per-pose arg-min on the flattened distances
BOUNDARY_CASES = [(64, 5, 3), (65, 4, 4), (33, 70, 3), (17, 483, 3)]
CASES = CASES + BOUNDARY_CASES
IDS = [f"J{J}-N{N}-H{H}" for J, N, H in CASES]


@functools.lru_cache(maxsize=None)
def case(J, N, H):
    """The recipe of tests/test_select_reproj_gpu.py::case -> (x [H N,J,3], T [H N,3], uv [N,J,2], K [N,3,3] general, conf [N,J] in
    (-0.2, 1.3)), float32 numpy; rows (h, n).  Read-only."""
    from _shared import problem
    cl, uv, K = problem(J, N, H, general=True)
    g = np.random.Generator(np.random.Philox(key=[77, 1000 * J + N]))
    B = H * N
    x = (np.repeat(cl, N, axis=0) + 0.05 * g.standard_normal((B, J, 3))).astype(np.float32)
    T = np.stack([0.4 * g.standard_normal(B), 0.4 * g.standard_normal(B), 5 + 0.5 * g.standard_normal(B)], -1).astype(np.float32)
    conf = g.uniform(-0.2, 1.3, (N, J)).astype(np.float32)
    out = (x, T, np.ascontiguousarray(uv, dtype=np.float32), np.ascontiguousarray(K, dtype=np.float32), conf)
    for a in out:
        a.setflags(write=False)
    return out


def depth_ref(x, T, K, row_offset=0):
    """q.z [B,J] of the projection below."""
    x, T, K = (np.asarray(a, dtype=np.float64) for a in (x, T, K))
    n = (int(row_offset) + np.arange(x.shape[0])) % K.shape[0]
    X = x + T[:, None, :]
    k = K[n][:, None, :, :]
    return k[..., 2, 0] * X[..., 0] + k[..., 2, 1] * X[..., 1] + k[..., 2, 2] * X[..., 2]


def joint_reproj_ref(x, T, uv, K, row_offset=0):
    """x [B,J,3], T [B,3], uv [N,J,2], K [N,3,3] (fp32 inputs; fp64 ones are taken as they are) -> d [B,J] float64: the distance in pixels
    between the projection of x[b,j] + T[b] through K[n] (the full 3x3 product) and uv[n,j], n = (row_offset + b) % N.  A joint at
    q.z <= 0 is +inf - that joint only; NaN falls through that test."""
    x, T, uv, K = (np.asarray(a, dtype=np.float64) for a in (x, T, uv, K))
    n = (int(row_offset) + np.arange(x.shape[0])) % uv.shape[0]
    X = x + T[:, None, :]
    k = K[n][:, None, :, :]                                       # [B,1,3,3]
    q = k[..., 0] * X[..., 0:1] + k[..., 1] * X[..., 1:2] + k[..., 2] * X[..., 2:3]          # [B,J,3]
    with np.errstate(all="ignore"):
        p = q[..., :2] / q[..., 2:]
        d = np.sqrt(((p - uv[n]) ** 2).sum(-1))
    d[q[..., 2] <= 0] = np.inf
    return d


def joint_select_ref(d, N, row_offset=0):
    """[B,J] flattened is an error vector over B*J rows with N*J "poses": -> (best [N,J] float64, idx [N,J] int32), select_ref's rules."""
    J = d.shape[1]
    best, idx = select_ref(np.ascontiguousarray(d).reshape(-1), N * J, int(row_offset) * J)
    return best.reshape(N, J), idx.reshape(N, J)


def compose_ref(x_full, T_full, joint_h, ref_h=None):
    """pose[n,j] = fl32((x[g,j] + T[g]) - (T[ref_h[n] N + n] if ref_h is given else 0)), g = joint_h[n,j] N + n, in float64 on the inputs."""
    N, J = joint_h.shape
    H = x_full.shape[0] // N
    x = np.asarray(x_full, dtype=np.float64).reshape(H, N, J, 3)
    T = np.asarray(T_full, dtype=np.float64).reshape(H, N, 3)
    n = np.arange(N)[:, None]
    out = x[joint_h, n, np.arange(J)[None, :]] + T[joint_h, n]
    if ref_h is not None:
        out = out - T[ref_h, np.arange(N)][:, None, :]
    return out.astype(np.float32)


def check_inputs(verbose=True):
    """On the reference alone, for every case: every joint in front of the camera (q.z > 1), no (pose, joint) whose best and second-best
    hypotheses are closer than 1e-6 px - the arg-min comparison cannot hide a failure behind a near tie - and, for J = 17 and N >= 64,
    more than half the poses take their joints from more than one hypothesis: the joint-wise selection is not the pose-level one."""
    gaps = []
    for J, N, H in CASES:
        x, T, uv, K, _ = case(J, N, H)
        assert depth_ref(x, T, K).min() > 1.0
        d = joint_reproj_ref(x, T, uv, K)
        assert np.isfinite(d).all() and 0.1 < d.min() and d.max() < 2000
        if H > 1:
            s = np.sort(d.reshape(H, N * J), axis=0)
            gaps.append((s[1] - s[0]).min())
        _, idx = joint_select_ref(d, N)
        mixed = (idx.min(1) != idx.max(1)).mean()
        if verbose:
            print(f"J={J} N={N} H={H}: d in [{d.min():.3g}, {d.max():.3g}] px, poses with joints of several hypotheses: {100 * mixed:.0f} %")
        if J == 17 and N >= 64:
            assert mixed > 0.5
    if verbose:
        print(f"smallest best-to-second gap: {min(gaps):.3g} px")
    assert min(gaps) > 1e-6
