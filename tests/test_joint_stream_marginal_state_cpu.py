"""CPU: the state size of the fixed-lag streaming fusion, pinned to the formula include/zedo_hip.h documents (no GPU call: the function
is host arithmetic).  With R = lag + max_frames, SJ = S J and pad8 rounding up to 8 bytes:
    zedo_joint_stream_marginal_state_bytes = 8 (5 SJ R H + S) + pad8(4 (SJ R + SJ))
        A f64 [SJ,R,H] | X f64 [SJ,R,H,3] | l f64 [SJ,R,H] | t i64 [S] | dead i32 [SJ,R] | lastdead i32 [SJ]
and 0 for a shape outside the entry points' range."""
import ctypes

import pytest

from _shared import host_fn  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def fn():
    return host_fn("zedo_joint_stream_marginal_state_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)


def pad(v, k):
    return (v + k - 1) // k * k


def state_bytes(S, H, J, lag, max_frames):
    R, SJ = lag + max_frames, S * J
    return 8 * (5 * SJ * R * H + S) + pad(4 * (SJ * R + SJ), 8)


# (S, H, J, lag, max_frames): SJ R + SJ odd (the padding bites) and even, lag = 0, one frame per push, the live shape
SHAPES = [(1, 1, 1, 0, 1), (1, 1, 1, 1, 1), (3, 7, 5, 2, 1), (1, 3, 1, 0, 2), (2, 50, 17, 34, 35), (16, 50, 17, 30, 8), (3, 3, 5, 0, 4),
          (1, 50, 17, 1014, 1015)]


@pytest.mark.parametrize("S,H,J,lag,mf", SHAPES)
def test_state_bytes_match_the_documented_layout(fn, S, H, J, lag, mf):
    assert fn(S, H, J, lag, mf) == state_bytes(S, H, J, lag, mf)
    assert fn(S, H, J, lag, mf) % 8 == 0


def test_the_padding_bites_on_an_odd_flag_count(fn):
    assert (1 * 1 + 1) % 2 == 0 and fn(1, 1, 1, 0, 1) == 8 * 6 + 8
    assert (1 * 2 + 1) % 2 == 1 and fn(1, 3, 1, 0, 2) == 8 * (5 * 2 * 3 + 1) + 16


def test_state_bytes_at_the_hypothesis_cap(fn):
    for S, J, lag, mf in ((1, 1, 0, 1), (3, 5, 2, 1), (2, 17, 8, 4)):
        assert fn(S, 1024, J, lag, mf) == state_bytes(S, 1024, J, lag, mf)
        assert fn(S, 1025, J, lag, mf) == 0


def test_state_bytes_are_zero_outside_the_range(fn):
    for bad in ((0, 5, 5, 1, 1), (-1, 5, 5, 1, 1), (5, 0, 5, 1, 1), (5, 5, 0, 1, 1), (5, 5, 5, -1, 1), (5, 5, 5, 1, 0), (5, 5, 5, 1, -2)):
        assert fn(*bad) == 0, bad
    # (lag + max_frames) S J H at INT_MAX | INT_MAX + 1, in each factor's place
    assert fn(1, 1, 1, INT_MAX - 1, 1) == state_bytes(1, 1, 1, INT_MAX - 1, 1)
    assert fn(1, 1, 1, INT_MAX, 1) == 0
    assert fn(1, 1, 1, 0, INT_MAX) == state_bytes(1, 1, 1, 0, INT_MAX)
    assert fn(INT_MAX, 1, 1, 0, 1) == state_bytes(INT_MAX, 1, 1, 0, 1)
    assert fn(INT_MAX, 1, 1, 1, 1) == 0 and fn(INT_MAX, 1, 2, 0, 1) == 0 and fn(INT_MAX, 2, 1, 0, 1) == 0
    assert fn(1 << 10, 1 << 10, 1 << 10, 0, 2) == 0                # 2^31 = INT_MAX + 1
    assert fn(1 << 10, 1 << 10, 1 << 10, 0, 1) == state_bytes(1 << 10, 1 << 10, 1 << 10, 0, 1)
    assert fn((1 << 10) - 1, 1 << 10, 1 << 10, 1, 1) == state_bytes((1 << 10) - 1, 1 << 10, 1 << 10, 1, 1)
    assert fn(1 << 15, 1, 1 << 15, 1, 1) == 0 and fn(65536, 1, 32768, 0, 1) == 0
