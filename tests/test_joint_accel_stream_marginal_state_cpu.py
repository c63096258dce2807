"""CPU: the host arithmetic of zedo_joint_accel_stream_marginal_state_bytes, pinned to the layout include/zedo_hip.h documents, with
R = lag + max_frames + 2, SJ = S J and HH = H^2:
    zedo_joint_accel_stream_marginal_state_bytes = pad8(8 (SJ R (HH + 4 H) + S) + 4 SJ R)
        A2 f64 [SJ,R,HH] | X f64 [SJ,R,H,3] | l f64 [SJ,R,H] | t i64 [S] | dead i32 [SJ,R]
and 0 for a shape the calls refuse (no GPU call: the function is host arithmetic); and the StreamCall the GPU tests of the call drive
tests/_stream_harness.py with."""
import ctypes

import pytest
import torch

from _shared import host_fn  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def state_bytes():
    return host_fn("zedo_joint_accel_stream_marginal_state_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)


def pad(v, k):
    return (v + k - 1) // k * k


def formula(S, H, J, lag, max_frames):
    sj, R, HH = S * J, lag + max_frames + 2, H * H
    return pad(8 * (sj * R * (HH + 4 * H) + S) + 4 * sj * R, 8)


@pytest.mark.parametrize("S,H,J,lag,mf", [(1, 1, 1, 0, 1), (1, 3, 1, 0, 1), (3, 7, 5, 2, 3), (16, 50, 17, 30, 1), (16, 50, 17, 30, 8),
                                          (1, 50, 17, 126, 127), (2, 64, 1, 8, 9), (29, 50, 17, 34, 35), (1, 5, 3, 100, 1)])
def test_state_bytes_match_the_documented_layout(state_bytes, S, H, J, lag, mf):
    assert state_bytes(S, H, J, lag, mf) == formula(S, H, J, lag, mf)


def test_the_live_shape_of_the_header_is_194_megabytes(state_bytes):
    assert 193.5e6 < state_bytes(16, 50, 17, 30, 1) < 194.5e6


def test_state_bytes_are_zero_for_the_shapes_the_calls_refuse(state_bytes):
    ok = (3, 7, 5, 2, 3)
    assert state_bytes(*ok) > 0
    for i, v in ((0, 0), (0, -1), (1, 0), (1, -2), (1, 65), (1, 1024), (2, 0), (2, -1), (3, -1), (4, 0), (4, -5)):
        bad = list(ok)
        bad[i] = v
        assert state_bytes(*bad) == 0, bad
    assert state_bytes(1, 64, 1, 0, 1) == formula(1, 64, 1, 0, 1)
    # (lag + max_frames + 2) S J H^2 past INT_MAX: through S J, through the rows, through lag + max_frames itself; the largest inside answers
    assert state_bytes(65536, 1, 32768, 0, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, INT_MAX) == 0
    assert state_bytes(1, 64, 1, 0, INT_MAX // 4096 - 1) == 0
    assert state_bytes(1, 64, 1, 0, INT_MAX // 4096 - 2) == formula(1, 64, 1, 0, INT_MAX // 4096 - 2)
    assert state_bytes(1 << 10, 64, 1 << 5, 8, 6) == 0                # 2^15 chains x 16 rows x 2^12 pairs = 2^31
    assert state_bytes(1, 1, 1, INT_MAX - 3, 1) == formula(1, 1, 1, INT_MAX - 3, 1)
    assert state_bytes(1, 1, 1, INT_MAX - 2, 1) == 0                  # R = INT_MAX + 1


def test_the_stream_call_of_the_gpu_tests():
    import test_joint_accel_stream_marginal_gpu as soft2
    c = soft2.CALL
    assert (c.prefix, c.weights, c.index, c.max_h, c.optional) == ("zedo_joint_accel_stream_marginal", ("lam_v", "lam_a", "tau"), 2, 64,
                                                                    dict(with_w=5))
    f64, i32 = torch.float64, torch.int32
    assert tuple(c.outputs(2, 3, 5, 7)) == (((2, 3, 5, 3), f64), ((2, 3, 5, 6), f64), ((2, 3, 5), i32), ((2, 3, 5), f64), ((2, 3, 5), f64),
                                            ((2, 3, 5, 7), f64))
    assert c.required() == (0, 1, 4, 5, 6, 7, 8, 9, 11)
