"""CPU: what tests/test_ipo_key_lists_gpu.py assumes about its key lists and about its arbiter, from the float64 oracle alone.  The
lists are what they are called (length, distinct entries or the stated repeats, the largest index, the root in some and not in
others); with the lists the suite had they cover every length 1 .. 17 the ABI accepts, so that a later edit that drops one fails
here; the share of ambiguous pose-iterations stays under the 1 % the GPU test grants itself, so that it cannot go vacuous; and the
order of a key list is a statement about rounding only."""
import os

import numpy as np
import pytest

from _shared import (GOLDEN, IPO_FORM_IDS, IPO_FORM_KEYS, IPO_KEYS, IPO_LENGTH_KEYS, IPO_NEW_LENGTHS, KEYS, ipo_ambiguous, ipo_oracle_trace)

LENGTH_IDS = [f"k{len(kl)}" for _, kl in IPO_LENGTH_KEYS]


def test_the_length_lists_are_what_they_are_called():
    assert [len(kl) for _, kl in IPO_LENGTH_KEYS] == [6, 7, 9, 10, 11, 13, 14, 15, 16] == list(IPO_NEW_LENGTHS)
    rooted = []
    for J, kl in IPO_LENGTH_KEYS:
        k = len(kl)
        assert J == 21 and kl == [(5 * i + k) % 21 for i in range(k)]
        assert len(set(kl)) == k and min(kl) >= 0 and max(kl) <= 20, kl      # distinct (5 is coprime to 21) and inside the skeleton
        assert kl != sorted(kl) and kl != sorted(kl)[::-1], kl               # neither ascending nor descending
        rooted.append(0 in kl)
    # index 20 = J - 1 is reached by the lists of 10, 11, 15 and 16; all but the list of 6 index past the 17 joints of the shipped skeleton
    assert [max(kl) for _, kl in IPO_LENGTH_KEYS] == [16, 17, 19, 20, 20, 18, 19, 20, 20]
    # some hold the root (no gradient from it: the sums take an exact zero from a live slot), some do not
    assert [len(kl) for (_, kl), r in zip(IPO_LENGTH_KEYS, rooted) if r] == [6, 11, 13, 16]


def test_the_form_lists_are_what_they_are_called():
    k11 = dict((len(kl), kl) for _, kl in IPO_LENGTH_KEYS)[11]
    (Ja, asc), (Jb, rev), (Jc, rep) = IPO_FORM_KEYS
    assert Ja == Jb == Jc == 21 and len(IPO_FORM_IDS) == 3
    assert asc == sorted(k11) and asc != k11 and rev == k11[::-1] and rev != asc[::-1]
    assert sorted(rev) == asc and len(set(asc)) == 11 and max(asc) == 20 and 0 in asc
    assert rep == [0, 4, 4, 9, 20, 9, 13] and len(rep) == 7 and len(set(rep)) == 5             # two indices twice, not adjacent alike
    assert sorted(i for i in set(rep) if rep.count(i) == 2) == [4, 9] and max(rep) == 20 and 0 in rep


def test_the_suite_launches_every_key_list_length_the_abi_accepts():
    """The union over IPO_KEYS, KEYS, the keylist_* entries of tests/golden/ipo_custom.npz, IPO_LENGTH_KEYS and IPO_FORM_KEYS is
    exactly 1 .. 17 (IPO_KMAX of csrc/zedo_geom.hip: one ipo_row_kernel instantiation per length); without IPO_LENGTH_KEYS it is the
    eight lengths the suite had, and the nine new lists alone close the gap, each the only one of its length."""
    g = np.load(os.path.join(GOLDEN, "ipo_custom.npz"))
    custom = {len(g[f]) for f in g.files if f.startswith("keylist_")}
    old = {len(kl) for _, kl in IPO_KEYS} | {len(kl) for _, kl in KEYS} | custom
    assert old == {1, 2, 3, 4, 5, 8, 12, 17}, sorted(old)
    forms = {len(kl) for _, kl in IPO_FORM_KEYS}
    assert forms == {7, 11}
    new = [len(kl) for _, kl in IPO_LENGTH_KEYS]
    assert old | forms | set(new) == set(range(1, 18))
    # the form lists repeat the lengths 7 and 11; the length lists alone must close the gap, so that dropping ANY of the nine fails here
    assert old | set(new) == set(range(1, 18)) and not old & set(new) and len(new) == len(set(new)) == 9


@pytest.mark.parametrize("J,kl", IPO_LENGTH_KEYS + IPO_FORM_KEYS, ids=LENGTH_IDS + IPO_FORM_IDS)
def test_ambiguous_pose_iterations_stay_under_one_percent(J, kl):
    """A pose-iteration is ambiguous when some residual of a moving key joint is below 1e-3 px.  Over the first 50 iterations at
    N = 8 and 64 and axes "z" and "xyz" (3 200 + 400 pose-iterations per axes) the share is at most 1 % in every cell's own count AND
    over the list - the cap tests/test_ipo_key_lists_gpu.py asserts per cell.  A condition on the problems, not a measurement of a kernel."""
    total = 0
    for N in (8, 64):
        for axes in ("z", "xyz"):
            n = ipo_ambiguous(J, kl, N, axes)
            assert n <= 0.01 * 50 * N, (N, axes, n)
            total += n
    print(f"ambiguous pose-iterations k={len(kl)} {kl}: {total} of 7200")


def test_the_order_of_a_key_list_is_a_statement_about_rounding_only():
    """The oracle's 50 packed float64 states for the k = 11 list, its sorted form and its reversed form agree to 1e-12 at both N and
    both axes: the loss is a mean over the key joints.  So what test_ipo_key_lists_gpu.py finds between these lists on the GPU is the
    pairing tree's rounding - each list is held to the oracle run on ITS order."""
    k11 = dict((len(kl), kl) for _, kl in IPO_LENGTH_KEYS)[11]
    worst = 0.0
    for N in (8, 64):
        for axes in ("z", "xyz"):
            base = np.stack(ipo_oracle_trace(21, tuple(k11), N, axes)[3])
            assert base.shape == (51, N, 15) and np.isfinite(base).all()
            for _, kl in IPO_FORM_KEYS[:2]:
                other = np.stack(ipo_oracle_trace(21, tuple(kl), N, axes)[3])
                d = float(np.abs(other - base).max())
                worst = max(worst, d)
                assert d <= 1e-12, (N, axes, kl, d)
    print(f"largest difference between the three orders: {worst:.2e}")
    assert worst > 0                                                         # the three runs did sum in different orders
