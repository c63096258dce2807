"""The reference of the hypothesis pruning (zedo_prune_rank, zedo_prune_gather; include/zedo_hip.h), stated directly in numpy: the order of
a pose's slots (finite ascending, then +inf, then NaN, ties to the lower slot), the table of the K first slots in ascending slot order, and
the gather.  brute_order() states the same order with a Python comparator; tests/test_prune_ref.py holds the two together.  case() builds the
inputs the GPU tests share: float64 draws with duplicates, signed zeros, infinities and NaNs planted."""
import functools

import numpy as np

# H on both sides of every tile size of prune_rank_kernel (csrc/zedo_prune.hip): the small instantiation ends at H = 56, then tiles of
# P = 64 poses up to H = 256, P = 32 up to 512, P = 16 up to 1024 - 56 | 57, 256 | 257 and 512 | 513 - beside one, two and three slots and
# the wavefront (64 | 65).  N on both sides of the tiles: 33 is one pose more than a tile of 32, 64 | 65 and 130 the tiles of 64; 1 and 7
# leave most of a tile empty.  The largest H keeps to N <= 65 (four tiles of 16 and a tail): the reference sorts every column.
RANK_H = (1, 2, 3, 50, 56, 57, 64, 65, 256, 257, 512, 513, 1024)
RANK_N = (1, 7, 33, 64, 65, 130)
RANK_CASES = [(H, N) for H in RANK_H for N in RANK_N if H < 1024 or N <= 65]
# J of the gather tests: a row is 3 J + 4 words and the 64 lanes of its wavefront copy them 64 at a time - part of one trip (1, 5, 17),
# exactly one (20: 64 words), a second (21: 67), a third that two lanes take (42: 130), a fourth (64: 196)
GATHER_J = (1, 5, 17, 20, 21, 42, 64)


def rank_ks(H):
    """K in {1, H/2, H-1, H} where those are valid: the ends and one K in the middle."""
    return sorted({k for k in (1, H // 2, H - 1, H) if 1 <= k <= H})


def order_ref(err, N):
    """err [H*N] float64, rows (h, n) h-major -> [H,N] int: column n lists the slots of pose n from first to last."""
    e = np.asarray(err, np.float64).reshape(-1, N)
    H = e.shape[0]
    isnan = np.isnan(e)
    value = np.where(isnan, 0.0, e) + 0.0                       # -0.0 + 0.0 = +0.0: the two zeros are one value
    slot = np.broadcast_to(np.arange(H)[:, None], e.shape)
    return np.lexsort((slot, value, isnan), axis=0)             # the last key is the primary one


def keep_ref(err, N, K):
    """-> keep [K,N] int32: the K first slots of every pose's order, in ascending slot order."""
    return np.sort(order_ref(err, N)[:K], axis=0).astype(np.int32)


def gather_ref(keep, x, T, hyp=None):
    """keep [K,N], x [H*N,J,3], T [H*N,3], hyp [H,N] or None -> (x_out [K*N,J,3], T_out [K*N,3], hyp_out [K,N] int32); an entry of keep
    outside 0 .. H-1 gives a NaN row with id -1."""
    keep = np.asarray(keep)
    K, N = keep.shape
    H = x.shape[0] // N
    ok = (keep >= 0) & (keep < H)
    g = (np.where(ok, keep, 0).astype(np.int64) * N + np.arange(N)[None, :]).reshape(-1)
    okr = ok.reshape(-1)
    x_out = np.where(okr[:, None, None], x[g], np.float32(np.nan)).astype(np.float32)
    T_out = np.where(okr[:, None], T[g], np.float32(np.nan)).astype(np.float32)
    ids = keep if hyp is None else np.asarray(hyp).reshape(-1)[g].reshape(K, N)
    return x_out, T_out, np.where(ok, ids, -1).astype(np.int32)


def precedes(va, a, vb, b):
    """The three clauses of the contract, word for word."""
    if not np.isnan(va) and np.isnan(vb):
        return True
    if not np.isnan(va) and not np.isnan(vb) and va < vb:
        return True
    separated = (not np.isnan(vb) and np.isnan(va)) or (not np.isnan(va) and not np.isnan(vb) and vb < va)
    return not separated and a < b


def brute_order(err, N):
    e = np.asarray(err, np.float64).reshape(-1, N)
    H = e.shape[0]
    out = np.empty((H, N), np.int64)
    for n in range(N):
        cmp = lambda a, b: -1 if precedes(e[a, n], a, e[b, n], b) else (1 if precedes(e[b, n], b, e[a, n], a) else 0)
        out[:, n] = sorted(range(H), key=functools.cmp_to_key(cmp))
    return out


def case(H, N, seed=0):
    """err [H*N] float64 for the rank tests (numpy Philox, key [77, 1000 H + N + seed]): positive draws; per pose a few exact duplicates, a
    0.0 beside a -0.0 (the smallest values of the pose), +inf and NaN entries; pose 0 all NaN, pose 1 all +inf, pose 2 with one finite
    entry only (fewer than K finite ones for every K > 1), from N = 7 up."""
    g = np.random.Generator(np.random.Philox(key=[77, 1000 * H + N + seed]))
    e = np.abs(g.standard_normal((H, N))) * 30.0 + 0.5
    for n in range(N):
        k = int(g.integers(0, 4))
        if H >= 2 and k:
            src = g.integers(0, H, size=k)
            dst = g.integers(0, H, size=k)
            e[dst, n] = e[src, n]                                # exact duplicates
        if H >= 2 and n % 3 == 0:
            a, b = g.choice(H, size=2, replace=False)
            e[a, n], e[b, n] = 0.0, -0.0
        if H >= 3 and n % 4 == 1:
            e[g.integers(0, H, size=max(1, H // 8)), n] = np.inf
        if H >= 3 and n % 5 == 2:
            e[g.integers(0, H, size=max(1, H // 8)), n] = np.nan
    if N >= 7:                                                   # (N = 1 keeps its one pose general)
        e[:, 0] = np.nan
        e[:, 1] = np.inf
        e[:, 2] = np.where(np.arange(H) == H // 2, 3.25, np.where(np.arange(H) % 2 == 0, np.nan, np.inf))
    return e.reshape(-1)
