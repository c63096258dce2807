"""CPU: the float64 reference of the label-free selection (tests/_select_ref.py) pinned on facts that hold by construction, so that
the GPU tests compare the kernels with something that has been checked itself."""
import numpy as np

from _select_ref import reproj_ref, select_ref


def _scene(N=3, H=2, J=5):
    g = np.random.Generator(np.random.Philox(key=[78, 1]))
    K = np.zeros((N, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 1100, 1150, 500, 520, 1.2
    K[:, 0, 1], K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = 25, -15, 0.01, -0.02          # skew and a general homogeneous row
    x = 0.3 * g.standard_normal((H * N, J, 3))
    T = np.stack([0.3 * g.standard_normal(H * N), 0.3 * g.standard_normal(H * N), 5 + 0.3 * g.standard_normal(H * N)], -1)
    return x, T, K


def _project(x, T, K, N):
    X = x + T[:, None]
    q = np.einsum("bik,bjk->bji", K[np.arange(len(x)) % N], X)
    return q[..., :2] / q[..., 2:]


def test_exact_projection_has_no_error_and_a_shift_is_its_length():
    """Detections that are the float64 projection of x + T: below 1e-9 px; every detection moved by (3, 4) px: 5 within 1e-9."""
    x, T, K = _scene(N=3, H=1)
    uv = _project(x, T, K, 3)
    assert reproj_ref(x, T, uv, K).max() < 1e-9
    assert np.abs(reproj_ref(x, T, uv + np.array([3.0, 4.0]), K) - 5.0).max() < 1e-9
    conf = np.random.default_rng(0).uniform(0.1, 1.0, (3, 5)).astype(np.float32)
    assert np.abs(reproj_ref(x, T, uv + np.array([3.0, 4.0]), K, conf) - 5.0).max() < 1e-9      # a weighted mean of equal distances


def test_weights_are_the_clamped_confidences_at_the_first_power():
    """Two joints 0 and 10 px off with confidences 0.25 and 0.75: 7.5; confidences 5.0 and 0.0 act as 1 and 1e-4 (in fp32)."""
    x, T, K = _scene(N=1, H=1, J=2)
    uv = _project(x, T, K, 1)
    uv[0, 1] += np.array([6.0, 8.0])
    assert abs(reproj_ref(x, T, uv, K, np.array([[0.25, 0.75]], np.float32))[0] - 7.5) < 1e-9
    lo = float(np.float32(1e-4))
    assert abs(reproj_ref(x, T, uv, K, np.array([[5.0, 0.0]], np.float32))[0] - 10.0 * lo / (1.0 + lo)) < 1e-9
    assert reproj_ref(x, T, uv, K, np.array([[5.0, 0.0]], np.float32))[0] == reproj_ref(x, T, uv, K, np.array([[1.0, 1e-4]], np.float32))[0]


def test_rows_map_to_poses_through_the_row_offset_and_points_behind_the_camera_are_infinite():
    x, T, K = _scene(N=3, H=2)
    uv = _project(x[:3], T[:3], K, 3) + 1.0
    full = reproj_ref(x, T, uv, K)
    assert np.array_equal(reproj_ref(x[2:5], T[2:5], uv, K, row_offset=2), full[2:5])
    xb = x.copy()
    xb[4, 1, 2] = -1.0 - T[4, 2]
    e = reproj_ref(xb, T, uv, K)
    assert np.isposinf(e[4]) and np.array_equal(np.delete(e, 4), np.delete(full, 4))
    xb[4, 0, 0] = np.nan                                           # behind the camera is tested first: the row stays +inf
    assert np.isposinf(reproj_ref(xb, T, uv, K)[4])
    xn = x.copy()
    xn[1, 0, 0] = np.nan
    assert np.isnan(reproj_ref(xn, T, uv, K)[1])


def test_select_ref_is_amin_and_argmin_per_pose():
    err = np.array([3.0, 1.0, np.inf, 2.0, 1.0, np.inf, np.nan, 0.5, 7.0, np.nan, 0.1, 6.0])      # H = 4, N = 3, rows h * 3 + n
    best, idx = select_ref(err, 3)
    assert np.isnan(best[0]) and idx[0] == 2 and best[1] == 0.1 and idx[1] == 3 and best[2] == 6.0 and idx[2] == 3
    best, idx = select_ref(err[:6], 3)
    assert list(best) == [2.0, 1.0, np.inf] and list(idx) == [1, 0, 0]                             # a tie and an all-inf pose: the first
    best, idx = select_ref(err[4:6], 3, row_offset=4)
    assert list(best) == [np.inf, 1.0, np.inf] and list(idx) == [-1, 1, 1]                         # pose 0 holds no row of this shard


def test_the_inputs_of_the_gpu_cases_are_what_the_bounds_assume():
    """The conditions tests/test_select_reproj_gpu.py asserts on its case table before it compares anything - depth above 1 m, finite errors
    of tens to hundreds of pixels, no best-to-second gap under 1e-6 px - hold on the reference alone, without a GPU."""
    import test_select_reproj_gpu as gpu
    gpu.test_the_inputs_are_what_the_bounds_assume()
