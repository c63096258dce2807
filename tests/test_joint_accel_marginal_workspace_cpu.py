"""CPU: the workspace size of zedo_joint_accel_marginal, pinned to the formula include/zedo_hip.h documents (no GPU call: the function
is host arithmetic).  With nj = N J and pad8 rounding up to 8 bytes:
    zedo_joint_accel_marginal_workspace_bytes = 8 nj H^2 + pad8(4 nj)       A2 f64 [J,N,H,H] | dead i32
and 0 for a shape outside the entry point's range (H above 64, a non-positive size, N J or N J H past INT_MAX)."""
import ctypes

import pytest

from _shared import host_fn  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

INT_MAX = 2 ** 31 - 1
CAP = 64

# the shapes of tests/test_joint_workspace_cpu.py: odd nj, where the padding bites; then shapes around the cap on J of the tree kernels
SHAPES = [(1, 1, 1), (3, 7, 5), (70, 50, 17), (2, 3, 64), (2, 3, 65), (1015, 50, 17)]


@pytest.fixture(scope="module")
def fn():
    return host_fn("zedo_joint_accel_marginal_workspace_bytes", ctypes.c_size_t, [ctypes.c_int] * 3)


def formula(N, H, J):
    nj = N * J
    return 8 * nj * H * H + (4 * nj + 7) // 8 * 8


@pytest.mark.parametrize("N,H,J", SHAPES)
def test_workspace_bytes_match_the_documented_layout(fn, N, H, J):
    assert fn(N, H, J) == formula(N, H, J)


def test_the_figure_the_header_quotes(fn):
    assert fn(1015, 50, 17) == 345_169_024 and round(fn(1015, 50, 17) / 1e6) == 345        # "345 MB at 1 015 frames x 17 joints x 50^2"
    assert fn(3, 3, 1) == 8 * 27 + 16                                                       # 12 bytes of flags padded to 16


def test_workspace_bytes_at_the_hypothesis_cap(fn):
    for N, J in ((1, 1), (3, 5), (7, 17)):
        assert fn(N, CAP, J) == formula(N, CAP, J)
        assert fn(N, CAP + 1, J) == 0
    assert fn(5, 1024, 5) == 0


def test_workspace_bytes_are_zero_outside_the_range(fn):
    for bad in ((0, 5, 5), (-1, 5, 5), (5, 0, 5), (5, -3, 5), (5, 5, 0), (5, 5, -2), (0, 0, 0)):
        assert fn(*bad) == 0
    # N J past INT_MAX, and N J H past INT_MAX with N J inside it; the largest products that are inside still answer - past 2^31 bytes
    assert fn(65536, 1, 32768) == 0
    assert fn(INT_MAX, 1, 2) == 0
    assert fn(INT_MAX // 64 + 1, 64, 1) == 0
    assert fn(1 << 20, 64, 32) == 0
    assert fn(INT_MAX, 1, 1) == formula(INT_MAX, 1, 1)
    assert fn(INT_MAX // 64, 64, 1) == formula(INT_MAX // 64, 64, 1) > 2 ** 40
