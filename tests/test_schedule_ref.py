"""The criterion of tests/_schedule_ref.py on the CPU: the fp32 numpy oracle, which forms the argument of sin / cos with the bits the
kernel states, meets it WITHOUT the argument term; that term is what it is said to be (small in the OIL range, growing with the
label); and the label list is what tests/test_schedule_gpu.py assumes."""
import numpy as np
import pytest

import _schedule_ref as R
from _schedule_ref import LABELS


@pytest.fixture(scope="module")
def crit(weights0):
    ref, bound, arg_cost = R.criterion(weights0, LABELS, arg_term=False)
    return ref, bound, arg_cost


def test_the_fp32_oracle_meets_the_criterion_without_the_argument_term(weights0, crit):
    """max |O.time_bias_table (fp32) - table64_at32| <= 2e-6 max(1, max |ref|) per label: the oracle shares the argument, so only the
    parity rule applies."""
    import zedo_oracle as O
    ref, bound, _ = crit
    tb32 = O.time_bias_table(weights0, LABELS)
    assert tb32.dtype == np.float32 and tb32.shape == (R.P, 5, 1024)
    err = R.per_label(tb32.astype(np.float64) - ref)
    for row in R.group_report(err, bound, LABELS):
        print(row)
    assert (err <= bound).all(), (LABELS[err > bound], err[err > bound])
    # the arithmetic of the two dense layers, about the same at every label: at most 2.8e-7 at the labels it was first measured at;
    # over all 67 the maximum is 3.6e-7 (label 156.3), a fifth of the bound
    first = np.isin(LABELS, np.array([0.0, 99.9, 300.0, 999.0, 2000.0], np.float32))
    assert first.sum() == 5 and err[first].max() <= 2.8e-7, err[first]
    assert err.max() <= 4e-7, (float(err.max()), float(LABELS[err.argmax()]))


def test_the_oracle_forms_the_argument_the_kernel_states():
    """arg32 is the argument of O.timestep_embedding in fp32, bit for bit: sin / cos of it in fp32 is the oracle's embedding."""
    import zedo_oracle as O
    a = R.arg32(LABELS)
    assert a.dtype == np.float32 and a.shape == (R.P, 256)
    pe = O.timestep_embedding(LABELS, 512)
    assert np.array_equal(pe.view(np.int32), np.concatenate([np.sin(a), np.cos(a)], axis=1).view(np.int32))
    # label_scale is applied to the label first, in fp32
    t = (LABELS / np.float32(999)).astype(np.float32)
    assert np.array_equal(R.arg32(t, 999.0), R.arg32((t * np.float32(999)).astype(np.float32)))


def test_the_argument_term_is_small_in_the_oil_range_and_grows_with_the_label(crit):
    _, bound, arg_cost = crit
    small = np.abs(LABELS) <= 100
    assert small.sum() >= 30 and (arg_cost[small] < 1e-6).all(), arg_cost[small].max()
    at = lambda v: float(arg_cost[np.flatnonzero(LABELS == np.float32(v))[0]])
    assert at(999.0) > at(99.9) > 0
    assert at(2000.0) > at(99.9)
    assert at(0.0) < 1e-12                                 # sin 0 and cos 0 are exact either way
    assert R.PARITY == 2e-6 and R.ARG_FACTOR == 2.0
    assert np.array_equal(bound, np.full(R.P, R.PARITY))   # max |tbias| is about 0.5: the floor of 1 holds at every label


def test_the_label_list_is_what_the_gpu_test_assumes():
    assert LABELS.dtype == np.float32 and LABELS.shape == (67,) and R.P == 67
    assert np.isfinite(LABELS).all()
    assert np.unique(LABELS).size == 67                    # no two labels equal: a row permutation cannot hide
    for v in R.NAMED:
        assert (LABELS == np.float32(v)).sum() == 1, v
    den = LABELS[1]
    assert den != 0 and abs(den) < np.finfo(np.float32).tiny
    assert ((LABELS >= np.float32(9.99)) & (LABELS <= np.float32(99.9))).sum() >= 8
    assert (LABELS < 0).sum() == 2
    drawn = LABELS[len(R.NAMED):]
    assert drawn.size == 47 and (drawn >= np.float32(1e-3)).all() and (drawn <= np.float32(999)).all()
    # every group of the report is populated
    assert [sum(R.group_of(v) == i for v in LABELS) > 0 for i in range(len(R.GROUPS))] == [True] * 4
    assert R.group_of(2000.0) == 3 and R.group_of(-999.0) == 2 and R.group_of(-99.9) == 1 and R.group_of(0.0) == 0
