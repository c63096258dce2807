"""CPU: the 50-digit Procrustes fixture (tests/golden/procrustes_hp.npz), the bound of tests/_procrustes_ref.py, and the float64
numpy oracle's place inside it.  The GPU half is tests/test_procrustes_gpu.py; the figures are in profiles/procrustes_accuracy.txt."""
import os

import numpy as np
import pytest

import _procrustes_ref as PR


@pytest.fixture(scope="module")
def fx():
    return PR.load()


@pytest.fixture(scope="module")
def oracle(fx):
    return PR.oracle_rows(fx)


def test_fixture_shape_and_size(fx):
    R, P = len(fx["J"]), len(fx["pose_J"])
    assert R == PR.H * P <= 320 and os.path.getsize(PR.FIXTURE) < 256 * 1024
    assert fx["pred"].dtype == np.float32 and fx["gt"].dtype == np.float64 and fx["pred"].shape == (R, 64, 3) and fx["gt"].shape == (P, 64, 3)
    assert np.array_equal(fx["pose"], np.repeat(np.arange(P), PR.H)) and np.array_equal(fx["hyp"], np.tile(np.arange(PR.H), P))
    assert np.array_equal(fx["J"], fx["pose_J"][fx["pose"]]) and np.array_equal(fx["family"], fx["pose_family"][fx["pose"]])
    for i in range(R):                                                  # the padding is zero, the rows are distinct
        assert not fx["pred"][i, fx["J"][i]:].any() and not fx["gt"][fx["pose"][i], fx["J"][i]:].any()
    assert len({fx["pred"][i].tobytes() + fx["gt"][fx["pose"][i]].tobytes() for i in range(R)}) == R
    want = {1: {3, 4, 5, 16, 17, 21, 64}, 2: {4, 17}, 3: {4, 17, 64}, 4: {17}, 5: {6, 8}, 6: {4, 17}, 7: {4, 17}, 8: {17}}
    assert {f: set(int(j) for j in fx["J"][fx["family"] == f]) for f in want} == want
    for k in ("err_p1_hp", "err_p2_hp", "sigma", "s", "C", "t", "t1"):
        assert np.isfinite(fx[k]).all() and (fx[k] >= 0).all(), k
    assert (np.diff(fx["sigma"], axis=1) <= 0).all() and (fx["t"] <= fx["t1"]).all()


def test_every_fifth_row_recomputed_at_50_digits(fx):
    pytest.importorskip("mpmath")
    for i in range(0, len(fx["J"]), 5):
        J = int(fx["J"][i])
        r = PR.hp_row(fx["pred"][i, :J], fx["gt"][fx["pose"][i], :J])
        assert r["e1"] == fx["err_p1_hp"][i] and r["e2"] == fx["err_p2_hp"][i] and np.array_equal(r["sigma"], fx["sigma"][i])
        assert (r["s"], r["C"], r["t"], r["t1"]) == (fx["s"][i], fx["C"][i], fx["t"][i], fx["t1"][i])


def test_the_numpy_oracle_stays_inside_the_bound_on_every_row(fx, oracle):
    """And needs at most an eighth of c1 and c2: the constants are 8 x the oracle's own largest ratio, rounded up in the third decimal."""
    b1, b2 = PR.row_bounds(fx)
    d1, d2 = np.abs(oracle[0] - fx["err_p1_hp"]), np.abs(oracle[1] - fx["err_p2_hp"])
    assert d1.shape == d2.shape == (len(fx["J"]),) and np.isfinite(d1).all() and np.isfinite(d2).all()
    assert (d1 <= b1).all() and (d2 <= b2).all()
    r1, r2 = PR.needed_ratios(fx, *oracle)
    assert r1.max() <= PR.ORACLE_RATIO_P1 <= r1.max() + 1e-3 and r2.max() <= PR.ORACLE_RATIO_P2 <= r2.max() + 1e-3
    assert PR.C1 == 8 * PR.ORACLE_RATIO_P1 < 64 and PR.C2 == 8 * PR.ORACLE_RATIO_P2 < 64          # the oracle's own ratio is below 8


def test_the_bound_is_tight_where_the_problem_is_well_posed(fx):
    b1, b2 = PR.row_bounds(fx)
    fam = fx["family"]
    assert (b2[np.isin(fam, (1, 2, 3, 4, 5, 8))] < 1e-10).all()
    assert (b2 < 1e-12).mean() >= 0.6
    base, thick = PR.bound_p2_parts(fx["C"], fx["J"], fx["err_p2_hp"], fx["sigma"], fx["t"], fx["t1"])
    res = PR.resolved(fx["sigma"])
    assert (thick[res] == 0).all() and np.array_equal(base + thick, b2)
    assert (fx["sigma"][~res, 2] < PR.RESOLVED * fx["sigma"][~res, 0]).all() and (~res).sum() >= 40 and res.sum() >= 200
    # the rank-1 form only ever lowers the bound of the issue's plane form
    plane = PR.C2 * fx["J"] * PR.U53 * (fx["C"] + fx["err_p2_hp"]) / np.maximum(fx["sigma"][:, 1] + np.where(res, fx["sigma"][:, 2], 0), PR.U53) + \
        np.where(res, 0, 2 * fx["t"])
    assert (b2 <= plane).all() and (b2[fam != 7] == plane[fam != 7]).all() and (b2[fam == 7] < plane[fam == 7]).any()
    assert (b1 < 1e-12 * np.maximum(1.0, fx["err_p1_hp"])).all()


def test_runner_up_is_a_hundred_bounds_above_the_minimum(fx):
    sep = PR.separation(fx)
    assert sep.shape == (len(fx["pose_J"]), 2) and (sep >= 100).all(), sep.min(0)


def test_the_ladders_stand_on_both_sides_of_the_rank_test(fx):
    """polar_from_svd treats a column with s[c] <= 1e-14 smax as missing: rows above, below and within a factor 100 of that, in both
    ladders; exactly rank-deficient rows (sigma3 == 0) as well."""
    ratio = fx["sigma"][:, 2] / fx["sigma"][:, 0]
    for fam in (6, 7):
        r = ratio[fx["family"] == fam]
        assert (r > 1e-14).any() and (r < 1e-14).any() and ((r > 1e-16) & (r < 1e-14)).any() and ((r >= 1e-14) & (r < 1e-12)).any()
        assert (r == 0).any()
    needle = fx["sigma"][fx["family"] == 7]
    r2 = needle[:, 1] / needle[:, 0]
    assert (r2 > 1e-14).any() and (r2 < 1e-14).any()                    # the second column crosses it too: rank 2 -> rank 1


def test_bounds_from_float64_inputs_agree_with_the_fixture(fx):
    """bounds64 (what tests use on inputs of their own) against the bounds from the stored 50-digit quantities, on resolved rows."""
    b1, b2 = PR.row_bounds(fx)
    for J, (rows, pred, gt) in PR.groups(fx).items():
        N = len(gt)
        g1, g2 = PR.bounds64(pred, np.tile(gt, (PR.H, 1, 1)))
        res = PR.resolved(fx["sigma"][rows])
        np.testing.assert_allclose(g1, b1[rows], rtol=1e-6)
        np.testing.assert_allclose(g2[res], b2[rows][res], rtol=1e-3)
        assert N * PR.H == len(rows)
