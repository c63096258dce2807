"""CPU: the host arithmetic of zedo_temporal_stream_state_bytes, pinned to the layout include/zedo_hip.h documents, with R = lag +
max_frames:
    zedo_temporal_stream_state_bytes = 8 (S R H + S H + S + S max_frames H^2) + pad8(4 (S R H + S R + S + 3 S H J))
        D f64 [S,R,H] | lastD f64 [S,H] | t i64 [S] | M f64 [S,max_frames,H,H] | back i32 [S,R,H] | dead i32 [S,R] | lastdead i32 [S] |
        lastx f32 [S,H,J,3]
and 0 for a shape the calls refuse (no GPU call: the function is host arithmetic)."""
import ctypes

import pytest

from _shared import host_fn  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def state_bytes():
    return host_fn("zedo_temporal_stream_state_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)


def pad(v, k):
    return (v + k - 1) // k * k


def formula(S, H, J, lag, max_frames):
    R = lag + max_frames
    return 8 * (S * R * H + S * H + S + S * max_frames * H * H) + pad(4 * (S * R * H + S * R + S + 3 * S * H * J), 8)


@pytest.mark.parametrize("S,H,J,lag,mf", [(1, 1, 1, 0, 1), (1, 3, 1, 0, 1), (3, 7, 5, 2, 3), (16, 50, 17, 30, 1), (16, 50, 17, 30, 8),
                                          (1, 50, 17, 1014, 1015), (2, 1024, 1, 8, 9), (29, 50, 17, 34, 35), (1, 5, 3, 100, 1),
                                          (1, 300, 17, 12, 13)])
def test_state_bytes_match_the_documented_layout(state_bytes, S, H, J, lag, mf):
    assert state_bytes(S, H, J, lag, mf) == formula(S, H, J, lag, mf)
    assert formula(S, H, J, lag, mf) % 8 == 0


def test_the_live_shape_of_the_header_is_under_a_megabyte(state_bytes):
    assert state_bytes(16, 50, 17, 30, 1) == 789376


def test_state_bytes_are_zero_for_the_shapes_the_calls_refuse(state_bytes):
    ok = (3, 7, 5, 2, 3)
    assert state_bytes(*ok) > 0
    for i, v in ((0, 0), (0, -1), (1, 0), (1, -2), (1, 1025), (1, 1030), (2, 0), (2, -1), (3, -1), (4, 0), (4, -5)):
        bad = list(ok)
        bad[i] = v
        assert state_bytes(*bad) == 0, bad
    assert state_bytes(1, 1024, 1, 0, 1) == formula(1, 1024, 1, 0, 1)
    # (lag + max_frames) S H past INT_MAX: through S H, through the rows, through lag + max_frames itself
    assert state_bytes(INT_MAX, 2, 1, 0, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, INT_MAX) == 0
    assert state_bytes(1 << 10, 1 << 10, 1, 1 << 10, 1 << 10) == 0
    assert state_bytes(1, 1, 1, INT_MAX - 1, 1) == formula(1, 1, 1, INT_MAX - 1, 1)
    # S max_frames H^2 past INT_MAX, the rows within it; the largest inside answers
    assert state_bytes(1, 64, 1, 0, INT_MAX // 4096 + 1) == 0
    assert state_bytes(1, 64, 1, 0, INT_MAX // 4096) == formula(1, 64, 1, 0, INT_MAX // 4096)
    assert state_bytes(INT_MAX // 4096 + 1, 64, 1, 0, 1) == 0
    # 3 S H J past INT_MAX, the other two within it
    assert state_bytes(1, 1, INT_MAX // 3 + 1, 0, 1) == 0
    assert state_bytes(1, 1, INT_MAX // 3, 0, 1) == formula(1, 1, INT_MAX // 3, 0, 1)
    assert state_bytes(2, 4, INT_MAX // 24 + 1, 0, 1) == 0
