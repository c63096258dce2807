"""CPU: the host arithmetic of zedo_joint_accel_stream_state_bytes, pinned to the layout include/zedo_hip.h documents, with R = lag +
max_frames, SJ = S J and HH = H^2:
    zedo_joint_accel_stream_state_bytes = pad8(8 (SJ R + SJ HH + 7 SJ H + S) + 4 (3 SJ R + 2 SJ) + SJ R HH)
        arg {f64 v, i32 q, i32 kind} [SJ,R] | last f64 [SJ, HH + 7 H + 1] (E, X, X of the frame before, u, two i32 dead flags) |
        t i64 [S] | dead i32 [SJ,R] | back2 u8 [SJ,R,HH]
and 0 for a shape the calls refuse (no GPU call: the function is host arithmetic)."""
import ctypes

import pytest

from _shared import host_fn  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def state_bytes():
    return host_fn("zedo_joint_accel_stream_state_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)


def pad(v, k):
    return (v + k - 1) // k * k


def formula(S, H, J, lag, max_frames):
    sj, R, HH = S * J, lag + max_frames, H * H
    return pad(8 * (sj * R + sj * HH + 7 * sj * H + S) + 4 * (3 * sj * R + 2 * sj) + sj * R * HH, 8)


@pytest.mark.parametrize("S,H,J,lag,mf", [(1, 1, 1, 0, 1), (1, 3, 1, 0, 1), (3, 7, 5, 2, 3), (16, 50, 17, 30, 1), (16, 50, 17, 30, 8),
                                          (1, 50, 17, 1014, 1015), (2, 64, 1, 8, 9), (29, 50, 17, 34, 35), (1, 5, 3, 100, 1)])
def test_state_bytes_match_the_documented_layout(state_bytes, S, H, J, lag, mf):
    assert state_bytes(S, H, J, lag, mf) == formula(S, H, J, lag, mf)


def test_the_live_shape_of_the_header_is_27_megabytes(state_bytes):
    assert 26.5e6 < state_bytes(16, 50, 17, 30, 1) < 27.5e6


def test_state_bytes_are_zero_for_the_shapes_the_calls_refuse(state_bytes):
    ok = (3, 7, 5, 2, 3)
    assert state_bytes(*ok) > 0
    for i, v in ((0, 0), (0, -1), (1, 0), (1, -2), (1, 65), (1, 1024), (2, 0), (2, -1), (3, -1), (4, 0), (4, -5)):
        bad = list(ok)
        bad[i] = v
        assert state_bytes(*bad) == 0, bad
    assert state_bytes(1, 64, 1, 0, 1) == formula(1, 64, 1, 0, 1)
    # (lag + max_frames) S J H^2 past INT_MAX: through S J, through the rows, through lag + max_frames itself; the largest inside answers
    assert state_bytes(65536, 1, 32768, 0, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, INT_MAX) == 0
    assert state_bytes(1, 64, 1, 0, INT_MAX // 4096 + 1) == 0
    assert state_bytes(1, 64, 1, 0, INT_MAX // 4096) == formula(1, 64, 1, 0, INT_MAX // 4096)
    assert state_bytes(1 << 10, 64, 1 << 5, 8, 8) == 0                # 2^15 chains x 16 rows x 2^12 pairs = 2^31
    assert state_bytes(1, 1, 1, INT_MAX - 1, 1) == formula(1, 1, 1, INT_MAX - 1, 1)
