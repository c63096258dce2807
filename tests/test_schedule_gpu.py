"""The time-bias table of zedo_schedule_create, tbias[S][5][1024], held to float64 and to one tile's bits at every length.

The table is the time-conditioning row that every GroupNorm layer of every step of every sampler reads (zedo_pc_plan_create builds its
own through the same call with label_scale = 1).  It comes from posemb_kernel and six launch_layer calls on round_up(S, 256) rows: one
EPI_BIAS_SILU layer of 512 columns and five EPI_BIAS layers of 1024 columns with a strided output - two epilogues that no other call
uses at these widths - and which tile shape they run on depends on S alone.  Here (a) the table of 67 labels (one round of 64x64
tiles) is held to the float64 criterion of tests/_schedule_ref.py on every label, from 0 and an fp32 denormal to 2000 and negative
ones; (b) every row of schedules of 1 to 24 832 periodic labels, ts[i] = LABELS[i % 67], must carry the bits of that table - without
any knowledge of the dispatch, as tests/test_launch_shapes_gpu.py does for the pose rows; (c) - (g) position, route, arithmetic mode,
step index, non-finite labels, the a / c tables at other SDE parameters and two host threads on the borrowed scratch.  All comparisons
of tables are equalities of int32 views (-0 and NaN payloads count), read through zedo_schedule_read.

The schedule's layers always run the exact-fp32 tiles: the file runs in the f32 session only, and one test proves that the mode of the
handle does not matter.  Measured figures: profiles/schedule_accuracy.txt.  The one-tile mutant behind 1 024 rows that (b) turns red with the tile named, and the
fast-form sin / cos that (a) does NOT turn red: profiles/mutation_schedule.txt."""
import threading

import numpy as np
import pytest

import _schedule_ref as R
from _schedule_ref import LABELS
from _shared import W, dev, launch_shape_base, one_arithmetic_mode, report_env, zh  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P = R.P
RAGGED = 37                                   # the ragged twin of a multiple of 256: 37 rows fewer, the same padded count
SLICE = 16 * P                                # rows per compared slice of a long table


def with_twins(lo, hi):
    return [S for m in range(lo, hi + 1, 256) for S in (m, m - RAGGED)]


SWEEP = {"1_to_257": [1, 66, 67, 255, 256, 257], "512_to_1536": with_twins(512, 1536), "1792_to_2816": with_twins(1792, 2816),
         "3072_to_3840": with_twins(3072, 3840), "4096_to_4608": with_twins(4096, 4608), "8192_8448": [8192, 8448],
         "12288_12544": [12288, 12544], "24576_24832": [24576, 24832]}
assert sorted(S for v in SWEEP.values() for S in v if S >= 512 - RAGGED and S <= 4608) == sorted(with_twins(512, 4608))


def periodic_labels(S):
    return LABELS[np.arange(S) % P]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def differing(tb, base, what):
    """None when every row s of tb [S,5,1024] carries the bits of base[s % 67] (compared in slices of 16 periods), else the failure
    message: the number of differing rows, the first of them with its position in a 64-, 128- and 256-row tile, and the layer and
    the columns of that row that differ."""
    S = tb.shape[0]
    g, w = bits(tb).reshape(S, -1), np.tile(bits(base).reshape(P, -1), (SLICE // P, 1))
    bad = np.zeros(S, bool)
    for r0 in range(0, S, SLICE):
        blk = g[r0:r0 + SLICE]
        if not np.array_equal(blk, w[:blk.shape[0]]):
            bad[r0:r0 + blk.shape[0]] = (blk != w[:blk.shape[0]]).any(1)
    if not bad.any():
        return None
    first = int(np.flatnonzero(bad)[0])
    cols = np.flatnonzero(g[first] != bits(base).reshape(P, -1)[first % P])
    layers = sorted(set((cols // 1024).tolist()))
    c = cols[cols // 1024 == layers[0]] % 1024
    return (f"{what}, S = {S}: {int(bad.sum())} rows differ from the tiled one-tile table; the first is row {first} (mod 64: {first % 64}, "
            f"mod 128: {first % 128}, mod 256: {first % 256}), label {LABELS[first % P]!r}: {cols.size} entries in layer(s) {layers}, in layer "
            f"{layers[0]} columns {int(c.min())} .. {int(c.max())}")


def verdict(fails, n):
    assert not fails, f"{len(fails)} of {n} schedules differ:\n" + "\n".join(fails[:16])


@pytest.fixture(scope="module")
def table(zh, W):
    """The one-tile table: Schedule(W, LABELS, label_scale = 1), 67 timestamps on 256 padded rows of 64x64 tiles."""
    tb, a, c = zh.Schedule(W, LABELS, label_scale=1.0).read()
    assert tb.shape == (P, 5, 1024) and tb.dtype == np.float32
    tb.setflags(write=False)
    return tb


# ---- (a) the one-tile table against float64 ----------------------------------------------------------------------------------

def test_the_one_tile_table_against_float64(weights0, table, math_mode):
    """The criterion of tests/_schedule_ref.py on every label: max |tbias[s] - table64_at32[s]| <= 2e-6 max(1, max |ref[s]|) + 2 x what
    forming the argument in fp32 costs between two float64 evaluations.  The achieved maxima and the share of the criterion used go
    to the parity report per label group (profiles/schedule_accuracy.txt): 0.33 / 0.25 / 0.42 / 0.44 of the criterion.  With __sinf / __cosf
    in posemb_kernel the shares are 0.33 / 0.31 / 0.48 / 0.68: one more rounding of the argument is inside the second term, and this test
    stays green under that mutant (profiles/mutation_schedule.txt)."""
    ref, bound, arg_cost = R.criterion(weights0, LABELS)
    assert np.isfinite(table).all()
    err = R.per_label(table.astype(np.float64) - ref)
    for row in R.group_report(err, bound, LABELS):
        report_env(dict(test="schedule_table_vs_float64", mode=math_mode, **row))
    parity_only = err / (R.PARITY * np.maximum(1.0, R.per_label(ref)))
    report_env(dict(test="schedule_table_vs_float64", mode=math_mode, group="all 67 labels", max_abs=float(err.max()), share=float((err / bound).max()),
                    share_of_the_parity_term_alone=float(parity_only.max()), at_label=float(LABELS[parity_only.argmax()])))
    over = err > bound
    assert not over.any(), [(float(v), float(e), float(b)) for v, e, b in zip(LABELS[over], err[over], bound[over])]


# ---- (b) every row of every length ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lengths", list(SWEEP))
def test_every_row_of_every_length_carries_the_bits_of_the_one_tile_table(zh, W, table, lengths):
    """S periodic labels for every S of the case (for the multiples of 256 also S - 37, the same padded count with 37 rows of
    padding): all S rows carry the bits of the tiled 67-row table, whatever tile shape, ring depth or pair kernel the row count and
    the compute-unit count select.  One table is held at a time (0.5 GB at 24 832 rows)."""
    fails = []
    for S in SWEEP[lengths]:
        sched = zh.Schedule(W, periodic_labels(S), label_scale=1.0)
        tb = sched.read()[0]
        del sched
        assert tb.shape == (S, 5, 1024)
        m = differing(tb, table, "zedo_schedule_create")
        del tb
        if m:
            fails.append(m)
    verdict(fails, len(SWEEP[lengths]))


# ---- (c) position and route --------------------------------------------------------------------------------------------------

def test_a_one_entry_schedule_gives_the_row_of_the_table(zh, W, table):
    """S = 1 borrows the scratch of the weights handle and computes its label in row 0 of the pad; the table has it in row k."""
    bad = [k for k in range(P) if not np.array_equal(bits(zh.Schedule(W, LABELS[k:k + 1], label_scale=1.0).read()[0][0]), bits(table[k]))]
    assert not bad, (bad, LABELS[bad])


def test_label_scale_and_premultiplied_labels_give_the_same_bits(zh, W):
    """Schedule(W, ts, label_scale = 999) against Schedule(W, fl32(ts * 999), label_scale = 1), the route of zedo_pc_plan_create."""
    ts = (LABELS / np.float32(999)).astype(np.float32)
    lab = (ts * np.float32(999)).astype(np.float32)
    a = zh.Schedule(W, ts, label_scale=999.0).read()[0]
    b = zh.Schedule(W, lab, label_scale=1.0).read()[0]
    assert np.array_equal(bits(a), bits(b)), differing(a, b, "label_scale = 999")


def test_the_arithmetic_mode_of_the_handle_does_not_matter(zh, W, table):
    """The schedule's layers run the exact-fp32 tiles in either mode: the same bits with the handle in f16x3 and back in f32."""
    assert W.math == "f32"
    try:
        W.set_math("f16x3")
        m16 = differing(zh.Schedule(W, periodic_labels(300), label_scale=1.0).read()[0], table, "handle in f16x3")
    finally:
        W.set_math("f32")
    m32 = differing(zh.Schedule(W, periodic_labels(300), label_scale=1.0).read()[0], table, "handle back in f32")
    verdict([m for m in (m16, m32) if m], 2)


# ---- (d) the step index ------------------------------------------------------------------------------------------------------

def test_the_step_index_reaches_the_right_row_of_a_long_schedule(zh, W):
    """zedo_score_eps at steps 0, 1023, 1024, 4097 and S - 1 of a 12 544-entry schedule against a one-entry schedule of that step's
    label, on the 67 base rows of the launch-shapes test, bit for bit."""
    S = 12544
    ts = periodic_labels(S)
    sched = zh.Schedule(W, ts, label_scale=1.0)
    x = dev(launch_shape_base())
    bad = []
    for step in (0, 1023, 1024, 4097, S - 1):
        one = zh.Schedule(W, ts[step:step + 1], label_scale=1.0)
        got, want = zh.score_eps(W, sched, step, x), zh.score_eps(W, one, 0, x)
        if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
            bad.append((step, float(ts[step]), int((got.view(torch.int32) != want.view(torch.int32)).reshape(P, -1).any(1).sum())))
    assert not bad, f"(step, label, differing rows of 67): {bad}"


# ---- (e) a non-finite label ----------------------------------------------------------------------------------------------------

def test_a_non_finite_label_stays_inside_its_row(zh, W, table):
    """S = 300 with NaN at row 70 and +inf at row 200: those two rows come back non-finite in every entry, every other row keeps the
    bits of the table; a is finite at every finite t, and c wherever the float64 closed form is (at t below 1e-16 it is 0 / 0 there
    too)."""
    import zedo_oracle as O
    S, rows = 300, {70: np.float32("nan"), 200: np.float32("inf")}
    ts = periodic_labels(S).copy()
    for r, v in rows.items():
        ts[r] = v
    tb, a, c = zh.Schedule(W, ts, label_scale=1.0).read()
    for r in rows:
        assert not np.isfinite(tb[r]).any(), (r, tb[r])
    patched = tb.copy()
    for r in rows:
        patched[r] = table[r % P]
    m = differing(patched, table, "beside a NaN and an inf label")
    assert m is None, m
    finite = np.isfinite(ts)
    assert finite.sum() == S - 2
    with np.errstate(invalid="ignore", divide="ignore"):
        c64 = O.step_coeffs(ts[finite].astype(np.float64) / 999.0)[1]
    assert np.isfinite(a[finite]).all()
    assert np.array_equal(np.isfinite(c[finite]), np.isfinite(c64)), (ts[finite][np.isfinite(c[finite]) != np.isfinite(c64)])
    assert np.isfinite(c64).sum() >= S - 2 - 2 * (S // P + 1)         # all but the rows of label 0 and of the denormal one


# ---- (f) the a / c tables ----------------------------------------------------------------------------------------------------

AC_T = np.array([1e-5, 1e-3, 0.01, 0.1, 0.5, 1.0], np.float32)


@pytest.mark.parametrize("beta_min,beta_max,n_sde,label_scale", [(0.1, 20.0, 1000, 999.0), (0.1, 20.0, 2000, 999.0), (0.01, 5.0, 500, 999.0),
                                                                  (0.1, 20.0, 1000, 1.0)])
def test_step_coefficients_at_other_sde_parameters(zh, W, beta_min, beta_max, n_sde, label_scale):
    """a and c against O.step_coeffs in float64 by the rule of test_schedule_tables, rtol = 2e-7; label_scale = 1 takes labels 999 t."""
    import zedo_oracle as O
    ts = AC_T if label_scale == 999.0 else (AC_T * np.float32(999)).astype(np.float32)
    _, a, c = zh.Schedule(W, ts, beta_min=beta_min, beta_max=beta_max, n_sde=n_sde, label_scale=label_scale).read()
    a64, c64 = O.step_coeffs(ts.astype(np.float64) * (label_scale / 999.0), n_sde=n_sde, beta_0=beta_min, beta_1=beta_max)
    report_env(dict(test="schedule_step_coeffs", params=[beta_min, beta_max, n_sde, label_scale], a_rel=float(np.abs(a / a64 - 1).max()),
                    c_rel=float(np.abs(c / c64 - 1).max())))
    np.testing.assert_allclose(a, a64.astype(np.float32), rtol=2e-7, atol=0)
    np.testing.assert_allclose(c, c64.astype(np.float32), rtol=2e-7, atol=0)


# ---- (g) two host threads ------------------------------------------------------------------------------------------------------

def test_two_threads_build_one_entry_schedules_on_one_handle(zh, W, table):
    """Two host threads, each on its own stream, build 40 one-entry schedules of different labels on the same weights handle - the
    borrowed scratch and its mutex - and obtain the rows the serial run obtains (which are the rows of the table)."""
    ks = [list(range(0, 40)), list(range(P - 1, P - 41, -1))]
    one = lambda k: zh.Schedule(W, LABELS[k:k + 1], label_scale=1.0).read()[0][0]
    serial = [[one(k) for k in kk] for kk in ks]
    assert all(np.array_equal(bits(r), bits(table[k])) for kk, rr in zip(ks, serial) for k, r in zip(kk, rr))
    gate = threading.Barrier(2, timeout=120)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    mismatches, errs = [], []

    def worker(j):
        def body():
            try:
                for i, k in enumerate(ks[j]):
                    gate.wait()                                  # both threads enter every build together
                    with torch.cuda.stream(streams[j]):
                        got = one(k)
                    if not np.array_equal(bits(got), bits(serial[j][i])):
                        mismatches.append((j, k))
            except BaseException as e:  # noqa: BLE001
                gate.abort()
                errs.append(e)
        return body

    th = [threading.Thread(target=worker(j)) for j in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not any(t.is_alive() for t in th), "a worker thread hung"
    if errs:
        raise errs[0]
    assert not mismatches, f"(thread, label index) whose row differs from the serial run: {mismatches[:8]}"
