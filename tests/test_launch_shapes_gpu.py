"""Every row of every launch shape of the dense layers carries the bits of one tile.

csrc/zedo_gemm.hip ("bit-identical either way: every tile shape issues the same products in the same order") and
csrc/zedo_gemm16.hip ("two launches of the same rows agree bit for bit") pick a tile shape, a pair kernel and a post_dense form from
the row count; pruning, sharding and chunking rest on a row's bits not depending on the batch it is in.  Here that promise is held on
EVERY row of EVERY padded row count up to 36 864 (three rounds of the exact-fp32 tiles on 256 compute units, two and a quarter of
the split-fp16 ones), without any knowledge of the dispatch: the batch is periodic, x[b] = base[(b + r) % 67], so the result of a
launch of B rows must be the result of ONE launch of the 67 base rows (128 padded rows: one round of 64x64 tiles and the split
post_dense), tiled - and that base result is held to the float64 oracle on every row.  67 is odd and prime: within 128 * 67 = 8 576
rows every base row visits every position of a 128-row tile.  All comparisons are equalities of the int32 views on the device (-0
and NaN payloads count); nothing but the 67 base rows is evaluated in numpy.

Measured figures and the kernels this file launches: profiles/launch_shapes.txt; the three one-tile mutants it turns red, with the
tile named in the message: profiles/mutation_launch_shapes.txt."""
from types import SimpleNamespace

import numpy as np
import pytest

from _shared import LS_P, LS_TS, W, dev, launch_shape_base, launch_shape_reference64, report_env, zh  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K_MAX = 576                                   # 64 * 576 = 36 864 rows
ROWS = 64 * K_MAX + LS_P                      # the periodic buffers: any shift r < 67 of any B <= 36 864 is a slice
RAGGED = 37                                   # the ragged twin of 64 k rows: 64 k - 37 (the same padded row count, 37 rows of padding)
CHUNK = 64                                    # row counts per test case of the sweep
SHIFTS = {9: (5, 66), 150: (1, 33), 290: (13, 40), 430: (2, 64), 576: (31, 50)}      # k -> r of the 64 k launch, r of its ragged twin
# the row counts at which post_dense and its tail change form: up to POST_SPLIT_ROWS = 2 048 and a little beyond, 8 192 +- 64, one
# exact-fp32 round +- 64 on 256 compute units, and larger ones
EPI_K = list(range(1, 41)) + [127, 128, 129, 191, 192, 193, 300, 448, 576]
OIL_S = 5
PC_LABEL, PC_NS = np.float32(0.37) * np.float32(999), np.float32(-2.75)


def tiled(block, rows=ROWS):
    """block [67, ...] on the device -> [rows, ...], row b = block[b % 67]."""
    return block.repeat(-(-rows // LS_P), *([1] * (block.dim() - 1)))[:rows].contiguous()


def differing(got, want, what, keep=None):
    """None when the int32 views of got and want agree on every row (keep: on the rows of this mask), else the failure message."""
    B = got.shape[0]
    g, w = got.contiguous().view(torch.int32).reshape(B, -1), want.contiguous().view(torch.int32).reshape(B, -1)
    if keep is None and torch.equal(g, w):
        return None
    bad = (g != w).any(1)
    if keep is not None:
        bad &= keep
    n = int(bad.sum())
    if n == 0:
        return None
    first = int(torch.nonzero(bad)[0])
    return (f"{what}, B = {B}: {n} rows differ from the tiled one-tile reference; the first is row {first} "
            f"(mod 64: {first % 64}, mod 128: {first % 128}, mod 256: {first % 256})")


def verdict(fails, launches):
    assert not fails, f"{len(fails)} of {launches} launches differ:\n" + "\n".join(fails[:16])


@pytest.fixture(scope="module")
def periodic(zh, W):
    """The periodic batch and the one-tile references of the score network, on the device."""
    base = launch_shape_base()
    sched = zh.Schedule(W, LS_TS)
    xb = dev(base)
    eps67 = [zh.score_eps(W, sched, i, xb) for i in range(len(LS_TS))]
    x67 = xb.clone()
    zh.sde_step(W, sched, 0, x67)
    assert torch.equal(xb, dev(base))
    return SimpleNamespace(base=base, sched=sched, eps67=eps67, x=tiled(xb), eps=tiled(eps67[0]), sde=tiled(x67))


@pytest.fixture(scope="module")
def oil(zh, W):
    """67 poses, their centred rows + noise and their roots; the 5-step loop (switch at step 1) at B = 67 as reference."""
    import zedo_oracle as O
    from lib.dataset import synthetic as syn
    d = syn.make_poses(LS_P, seed=67, conf_mode="uniform")
    g = np.random.Generator(np.random.Philox(key=[67, 5]))
    x0 = ((d["db_3d"] - d["db_3d"][:, 0:1]) + 0.05 * g.standard_normal((LS_P, 17, 3))).astype(np.float32)
    T0 = d["db_3d"][:, 0, :].astype(np.float32)
    sched = zh.Schedule(W, O.oil_timestamps(OIL_S))
    geom = zh.reproj_prepare(dev(d["db_2d"][:, :, :2]), dev(d["camera_param"]), dev(d["db_2d"][:, :, 2]))
    x, T = dev(x0), dev(T0)
    zh.oil_run(W, sched, x, geom, T, 0, OIL_S, OIL_S // 5)
    return SimpleNamespace(d=d, x0=x0, T0=T0, sched=sched, geom=geom, x67=x, T67=T, xin=tiled(dev(x0)), Tin=tiled(dev(T0)),
                           x=tiled(x), T=tiled(T))


def run_oil(zh, W, oil, B, r, poison=None):
    x, T = oil.xin[r:r + B].clone(), oil.Tin[r:r + B].clone()
    if poison is not None:
        poison(x)
    zh.oil_run(W, oil.sched, x, oil.geom, T, 0, OIL_S, OIL_S // 5, row_offset=r)
    return x, T


# ---- the base block against float64 --------------------------------------------------------------------------------------

def test_the_one_tile_reference_against_the_float64_oracle(zh, W, weights0, periodic, math_mode):
    """zedo_score_eps at B = 67, every row and every noise level, by the rule of the parity tests: max |error| <= 2e-6 max(1, max |ref|).
    tests/test_launch_shapes_ref.py holds the fp32 numpy oracle to half of that on the same rows.  The achieved maxima go to the
    parity report (profiles/launch_shapes.txt)."""
    ref = launch_shape_reference64(weights0, periodic.base)
    rows = []
    for i, t in enumerate(LS_TS):
        eps = periodic.eps67[i].cpu().numpy()
        assert np.isfinite(eps).all()
        d = np.abs(eps.astype(np.float64) - ref[i]).reshape(LS_P, -1).max(1)
        rows.append(dict(test="launch_shapes_base_vs_float64", mode=math_mode, t=float(t), max_abs=float(d.max()), row=int(d.argmax()),
                         bound=2e-6 * max(1.0, float(np.abs(ref[i]).max()))))
        report_env(rows[-1])
    for r in rows:
        assert r["max_abs"] <= r["bound"], r


def test_the_one_tile_loop_against_the_float64_oracle(zh, W, weights0, oil):
    """The B = 67 zedo_oil_run result by the criterion of test_oil_loop_vs_oracle_ragged: 1.5 x the fp32 oracle's own gap to its
    float64 run + 2e-6 on x, + 2e-5 on T."""
    import zedo_oracle as O
    d = oil.d
    args = (d["db_2d"][:, :, :2], d["camera_param"], d["db_2d"][:, :, 2], oil.T0[:, None, :], OIL_S)
    x32, T32 = O.oil_loop(weights0, oil.x0, *args)
    x64, T64 = O.oil_loop(O.cast_weights(weights0, np.float64), oil.x0, *args, dtype=np.float64)
    gap, gapT = float(np.abs(x32 - x64).max()), float(np.abs(T32 - T64).max())
    dx = float(np.abs(oil.x67.cpu().numpy() - x64).max())
    dT = float(np.abs(oil.T67.cpu().numpy() - T64[:, 0, :]).max())
    report_env(dict(test="launch_shapes_oil_vs_float64", mode=W.math, dx=dx, gap=gap, dT=dT, gapT=gapT))
    assert dx <= 1.5 * gap + 2e-6, (dx, gap)
    assert dT <= 1.5 * gapT + 2e-5, (dT, gapT)


# ---- every padded row count, every row: zedo_score_eps --------------------------------------------------------------------

@pytest.mark.parametrize("k0", range(1, K_MAX + 1, CHUNK))
def test_score_eps_every_padded_row_count(zh, W, periodic, k0):
    """B = 64 k and the ragged B = 64 k - 37 for every k of the chunk, at t = 0.1: all B rows carry the bits of the tiled reference.
    Exhaustive instead of aimed: every branch below one round, every remainder length behind a whole round in both pair kernels,
    the exact multiples - whatever the cost model and the compute-unit count make of them.  At five k two more launches start the
    period at r != 0."""
    p, fails, n = periodic, [], 0
    for k in range(k0, k0 + CHUNK):
        for B, r in [(64 * k, 0), (64 * k - RAGGED, 0)] + list(zip((64 * k, 64 * k - RAGGED), SHIFTS.get(k, ()))):
            x = p.x[r:r + B].clone() if r else p.x[:B]
            m = differing(zh.score_eps(W, p.sched, 0, x), p.eps[r:r + B], f"zedo_score_eps, k = {k}, r = {r}")
            n += 1
            if m:
                fails.append(m)
    verdict(fails, n)


# ---- the other epilogues of the same layers -------------------------------------------------------------------------------

def epi_rows():
    return [B for k in EPI_K for B in (64 * k, 64 * k - RAGGED)]


def test_sde_step_at_the_row_counts_where_post_dense_changes_form(zh, W, periodic):
    """zedo_sde_step (EPI_SDE: x' = a x + c eps in the post_dense epilogue) on the updated x."""
    p, fails = periodic, []
    for B in epi_rows():
        x = p.x[:B].clone()
        zh.sde_step(W, p.sched, 0, x)
        m = differing(x, p.sde[:B], "zedo_sde_step")
        if m:
            fails.append(m)
    verdict(fails, len(epi_rows()))


@pytest.mark.parametrize("r", [0, 5])
def test_oil_run_at_the_row_counts_where_post_dense_changes_form(zh, W, oil, r):
    """zedo_oil_run, S = 5, steps 0 to 5, switch_step = 1: step 0 with the given T, steps 1 - 4 with the fused least-squares tail of
    post_dense in each of its launch forms.  x and T, with row_offset = 0 and with row_offset = 5 and the batch shifted to match
    (pose of row b: (row_offset + b) % 67; zedo_oil_run puts no constraint between B and N)."""
    fails = []
    for B in epi_rows():
        x, T = run_oil(zh, W, oil, B, r)
        for m in (differing(x, oil.x[r:r + B], f"zedo_oil_run x, row_offset = {r}"), differing(T, oil.T[r:r + B], f"zedo_oil_run T, row_offset = {r}")):
            if m:
                fails.append(m)
    verdict(fails, len(epi_rows()))


@pytest.mark.parametrize("kind", ["predictor", "ald"])
def test_pc_step_at_the_row_counts_where_post_dense_changes_form(zh, W, periodic, kind):
    """zedo_pc_step on x and x_mean: a predictor-only plan and an ALD plan of two corrector steps, with periodic noise draws (the
    Langevin corrector is left out: its step size is a mean over the batch, which a periodic batch of B rows does not keep)."""
    f1 = lambda v: np.array([v], np.float32)
    if kind == "predictor":
        plan = zh.PcPlan(W, SimpleNamespace(label=f1(PC_LABEL), net_scale=f1(PC_NS), has_predictor=True, pA=f1(1.0123), pB=f1(0.0371), pC=f1(0.0816),
                                            corrector=0, n_corr=0, corr=None))
    else:
        plan = zh.PcPlan(W, SimpleNamespace(label=f1(PC_LABEL), net_scale=f1(PC_NS), has_predictor=False, pA=None, pB=None, pC=None,
                                            corrector=2, n_corr=2, corr=f1(3e-4)))
    g = np.random.Generator(np.random.Philox(key=[67, 6]))
    z67 = [dev(g.standard_normal((LS_P, 17, 3)).astype(np.float32)) for _ in range(plan.n_draws)]
    z = [tiled(a) for a in z67]
    x67 = dev(periodic.base)
    m67 = torch.empty_like(x67)
    zh.pc_step(W, plan, 0, x67, z67, m67)
    assert not torch.equal(x67, dev(periodic.base))
    want_x, want_m = tiled(x67), tiled(m67)
    fails = []
    for B in epi_rows():
        x = periodic.x[:B].clone()
        xm = torch.empty_like(x)
        zh.pc_step(W, plan, 0, x, [a[:B] for a in z], xm)
        for m in (differing(x, want_x[:B], f"zedo_pc_step ({kind}) x"), differing(xm, want_m[:B], f"zedo_pc_step ({kind}) x_mean")):
            if m:
                fails.append(m)
    verdict(fails, len(epi_rows()))


# ---- a diverged row stays alone -------------------------------------------------------------------------------------------

# B, seam: a multiple of every power-of-two tile height in use at that B, so rows seam - 1 and seam lie in two tiles whatever the shape
DIVERGED = [(67, 64), (2112, 1024), (8256, 4096), (12352 + 64 * 24, 12288)]


def diverged_rows(B, seam):
    """row -> value: NaN and +inf on either side of the seam, 1e30 in the last tile."""
    return {seam - 1: float("nan"), seam: float("inf"), B - 2: 1e30}


@pytest.mark.parametrize("B,seam", DIVERGED)
def test_a_diverged_row_leaves_its_tile_neighbours_alone(zh, W, periodic, oil, B, seam):
    """Pruning exists because rows diverge; a NaN, a +inf and a 1e30 row must change no other row of their tiles: every other row of
    zedo_score_eps and of the 5-step zedo_oil_run (x and T) keeps the reference bits, and the NaN and inf rows come back non-finite."""
    bad = diverged_rows(B, seam)
    assert len(bad) == 3 and all(0 <= b < B for b in bad)
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[list(bad)] = False

    def poison(x):
        for b, v in bad.items():
            x[b] = v
    x = periodic.x[:B].clone()
    poison(x)
    eps = zh.score_eps(W, periodic.sched, 0, x)
    fails = [differing(eps, periodic.eps[:B], "zedo_score_eps beside diverged rows", keep)]
    for b in (seam - 1, seam):
        assert not bool(torch.isfinite(eps[b]).any()), (b, eps[b])
    xo, To = run_oil(zh, W, oil, B, 0, poison)
    fails += [differing(xo, oil.x[:B], "zedo_oil_run x beside diverged rows", keep), differing(To, oil.T[:B], "zedo_oil_run T beside diverged rows", keep)]
    verdict([m for m in fails if m], 3)
