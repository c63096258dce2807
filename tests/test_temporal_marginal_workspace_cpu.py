"""CPU: the workspace size of zedo_temporal_marginal, pinned to the layout include/zedo_hip.h documents (no GPU call: the function is
host arithmetic).  With pad8 rounding up to 8 bytes and C = min(chunk_frames, N), or for chunk_frames <= 0 the largest C whose
transition costs stay at or under 256 MB (at least one frame), capped at N:
    zedo_temporal_marginal_workspace_bytes = 16 N H + 8 N + pad8(4 N) + 8 C H^2      A, B f64 [N,H] | logZ f64 [N] | dead i32 [N] | M f64 [C,H,H]
and 0 for a shape outside the entry point's range (H above 1024, a non-positive size, H N past INT_MAX)."""
import ctypes

import pytest

from _shared import host_fn  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

INT_MAX = 2 ** 31 - 1
CAP = 1024
VARIABLE = 256 << 20


@pytest.fixture(scope="module")
def fn():
    return host_fn("zedo_temporal_marginal_workspace_bytes", ctypes.c_size_t, [ctypes.c_int] * 3)


def fixed(N, H):
    return 16 * N * H + 8 * N + (4 * N + 7) // 8 * 8


def formula(N, H, chunk):
    per = 8 * H * H
    C = chunk if chunk > 0 else max(1, VARIABLE // per)
    return fixed(N, H) + min(C, N) * per


@pytest.mark.parametrize("N,H", [(1, 1), (3, 7), (70, 50), (300, 7), (130, 130), (1015, 50), (3, 1024), (70880, 50)])
@pytest.mark.parametrize("chunk", [1, 2, 7, 35, 10 ** 6, 0, -1, -100])
def test_workspace_bytes_match_the_documented_layout(fn, N, H, chunk):
    assert fn(N, H, chunk) == formula(N, H, chunk)


def test_the_flags_are_padded_and_a_chunk_is_capped_at_the_clip(fn):
    assert fn(3, 3, 1) == 16 * 9 + 24 + 16 + 72                                              # 12 bytes of flags padded to 16
    assert fn(3, 3, 3) == fn(3, 3, 4) == fn(3, 3, 0) == 16 * 9 + 24 + 16 + 3 * 72
    assert fn(5, 2, 1) < fn(5, 2, 2) < fn(5, 2, 5) == fn(5, 2, 6)


def test_the_256_mb_rule(fn):
    """chunk_frames <= 0: the largest C with 8 C H^2 <= 256 MB - 13 421 frames at H = 50, 32 at H = 1024 (exactly 256 MB), and never
    fewer than one."""
    for chunk in (0, -1):
        assert fn(10 ** 6, 50, chunk) == fixed(10 ** 6, 50) + 13421 * 8 * 2500
        assert fn(100, 1024, chunk) == fixed(100, 1024) + 32 * 8 * CAP * CAP
        assert fn(10, 1024, chunk) == fixed(10, 1024) + 10 * 8 * CAP * CAP
    assert 13421 * 8 * 2500 <= VARIABLE < 13422 * 8 * 2500 and 32 * 8 * CAP * CAP == VARIABLE
    assert fn(10 ** 6, 50, 13422) == fn(10 ** 6, 50, 0) + 8 * 2500                            # an explicit chunk may exceed it


def test_workspace_bytes_are_zero_outside_the_range(fn):
    for bad in ((0, 5, 1), (-1, 5, 1), (5, 0, 1), (5, -3, 1), (0, 0, 0), (5, CAP + 1, 1), (5, CAP + 1, 0), (1, 4097, 1)):
        assert fn(*bad) == 0, bad
    assert fn(5, CAP, 1) == formula(5, CAP, 1)
    # H N past INT_MAX; the largest product inside it still answers
    assert fn(INT_MAX // 2 + 1, 2, 1) == 0
    assert fn(1 << 21, CAP, 1) == 0
    assert fn(INT_MAX, 1, 1) == formula(INT_MAX, 1, 1)
    assert fn((1 << 21) - 1, CAP, 1) == formula((1 << 21) - 1, CAP, 1) > 2 ** 34
