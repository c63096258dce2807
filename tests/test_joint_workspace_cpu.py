"""CPU: the workspace sizes of the joint-wise chain entry points and the hypothesis cap of the tree fusion, pinned to the formulas
include/zedo_hip.h documents (no GPU call: the functions are host arithmetic).  With nj = N J, njh = nj H and pad_k rounding up to k bytes:
    zedo_joint_temporal_workspace_bytes = 8 njh + pad8(4 (njh + 2 nj))      D f64 | back i32, dead i32, endh i32
    zedo_joint_marginal_workspace_bytes = 8 njh + pad8(4 nj)                A f64 | dead i32
    zedo_joint_accel_workspace_bytes    = pad4(nj H^2) + 8 nj               back2 u8 | dead i32, endq i32
    zedo_joint_tree_marginal_max_h(J)   = min(1024, (163840 - 8192) // (48 J + 16))
and 0 for a shape outside the entry point's range."""
import ctypes

import pytest

from _shared import host_lib  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    so = host_lib()
    for name in ("zedo_joint_temporal_workspace_bytes", "zedo_joint_marginal_workspace_bytes", "zedo_joint_accel_workspace_bytes"):
        getattr(so, name).restype = ctypes.c_size_t
        getattr(so, name).argtypes = [ctypes.c_int] * 3
    so.zedo_joint_tree_marginal_max_h.restype = ctypes.c_int
    so.zedo_joint_tree_marginal_max_h.argtypes = [ctypes.c_int]
    return so


def pad(v, k):
    return (v + k - 1) // k * k


def temporal_bytes(N, H, J):
    nj, njh = N * J, N * J * H
    return 8 * njh + pad(4 * (njh + 2 * nj), 8)


def marginal_bytes(N, H, J):
    nj = N * J
    return 8 * nj * H + pad(4 * nj, 8)


def accel_bytes(N, H, J):
    nj = N * J
    return pad(nj * H * H, 4) + 8 * nj


ENTRY = {"temporal": ("zedo_joint_temporal_workspace_bytes", temporal_bytes, 1024),
         "marginal": ("zedo_joint_marginal_workspace_bytes", marginal_bytes, 1024),
         "accel": ("zedo_joint_accel_workspace_bytes", accel_bytes, 64)}

# odd nj, where the padding bites; then shapes around each entry point's cap on H and the cap on J of the tree kernels (no cap here)
SHAPES = [(1, 1, 1), (3, 7, 5), (70, 50, 17), (2, 3, 64), (2, 3, 65), (1015, 50, 17)]


@pytest.mark.parametrize("entry", sorted(ENTRY))
@pytest.mark.parametrize("N,H,J", SHAPES)
def test_workspace_bytes_match_the_documented_layout(lib, entry, N, H, J):
    name, formula, _ = ENTRY[entry]
    assert getattr(lib, name)(N, H, J) == formula(N, H, J)


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_workspace_bytes_at_the_hypothesis_cap(lib, entry):
    name, formula, cap = ENTRY[entry]
    fn = getattr(lib, name)
    for N, J in ((1, 1), (3, 5), (7, 17)):
        assert fn(N, cap, J) == formula(N, cap, J)
        assert fn(N, cap + 1, J) == 0


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_workspace_bytes_are_zero_outside_the_range(lib, entry):
    name, formula, cap = ENTRY[entry]
    fn = getattr(lib, name)
    for bad in ((0, 5, 5), (-1, 5, 5), (5, 0, 5), (5, -3, 5), (5, 5, 0), (5, 5, -2), (0, 0, 0)):
        assert fn(*bad) == 0
    # N J past INT_MAX, and N J H past INT_MAX with N J inside it; the largest products that are inside still answer
    assert fn(65536, 1, 32768) == 0
    assert fn(INT_MAX, 1, 2) == 0
    assert fn(INT_MAX // 64 + 1, 64, 1) == 0
    assert fn(1 << 20, 64, 32) == 0
    assert fn(INT_MAX, 1, 1) == formula(INT_MAX, 1, 1)
    assert fn(INT_MAX // 64, 64, 1) == formula(INT_MAX // 64, 64, 1)


def test_tree_marginal_max_h(lib):
    fn = lib.zedo_joint_tree_marginal_max_h
    for J in range(1, 65):
        want = min(1024, (163840 - 8192) // (48 * J + 16))
        assert fn(J) == want
        assert 48 * J * want + 16 * want + 8192 <= 163840              # what the formula stands for: the LDS of one workgroup
    assert fn(1) == fn(2) == 1024 and fn(3) == 972 and fn(17) == 187 and fn(64) == 50      # by hand: 155648 // 160, // 832, // 3088
    for J in (0, -1, 65, 1000, INT_MAX):
        assert fn(J) == 0
