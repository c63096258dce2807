"""GPU tests of the IPO fit at every key-list length the ABI accepts (zedo_ipo_fit, zedo_ipo_fit_resume: 1 .. 17 joint indices).
launch_ipo_fit (csrc/zedo_geom.hip) turns the length into code three times - a 17-way switch over ipo_row_kernel<1> .. <17>, the LDS
arrays s_cu[KJ][128] / s_cv[KJ][128] of each instantiation, and the crossover between the two kernels, B >= CUs x (4 k + 4) - and the
suite launched eight of the lengths: 1, 2, 3, 4, 5, 8, 12, 17.  Here the other nine (_shared.IPO_LENGTH_KEYS: unsorted lists, with and
without the root) and three lists in other forms (_shared.IPO_FORM_KEYS: a list sorted, reversed, and one with repeated indices):
  a. single iterations from the float64 oracle's state, the method and criteria of test_ipo_single_iterations_from_the_oracle_state
     (one copy: _shared.ipo_single_iterations_from_the_oracle) - unpinned, i.e. the half-wave kernel at these row counts;
  b. both kernels bit for bit over 500 iterations, one child process per pin of ZEDO_IPO_KERNEL - with (a) this holds each of the nine
     lane-per-row instantiations, whose pairing tree has another mix of live and exact-zero slots at every length, to the oracle;
  c. the dispatch seam unpinned: calls of B rows on both sides of each length's crossover return the rows of one large call.
What the lists are, that all lengths are covered, and that the oracle leaves at most 1 % of the pose-iterations ambiguous:
tests/test_ipo_key_lists_ref.py.  One arithmetic mode: the IPO does not touch the dense layers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _ipo_state as S
from _shared import (IPO_FORM_IDS, IPO_FORM_KEYS, IPO_LENGTH_KEYS, IPO_MAX, IPO_MIN, IPO_T, dev, ipo_single_iterations_from_the_oracle,
                     make_ipo_problem, one_arithmetic_mode, report_env as _report, zh)  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTS = IPO_LENGTH_KEYS + IPO_FORM_KEYS
LIST_IDS = [f"k{len(kl)}" for _, kl in IPO_LENGTH_KEYS] + IPO_FORM_IDS


# ---- a. single iterations from the oracle's float64 state -----------------------------------------------------------------------------

@pytest.mark.parametrize("axes", ["z", "xyz"])
@pytest.mark.parametrize("N", [8, 64])
@pytest.mark.parametrize("J,kl", LISTS, ids=LIST_IDS)
def test_ipo_single_iterations_at_every_key_list_length(zh, J, kl, N, axes):
    """test_ipo_single_iterations_from_the_oracle_state (tests/test_joint_counts_gpu.py) on the new lists: each of the first 50 Adam
    iterations on its own through zedo_ipo_fit_resume from the oracle's float64 state, |delta parameter| <= 1e-6 on the clear poses
    (asserted per iteration in the shared method), the second moments by _shared.MomentRule.  Nothing passes vacuously: at most 1 % of
    the pose-iterations are ambiguous (the oracle alone stays under that: tests/test_ipo_key_lists_ref.py), the largest parameter
    delta and the largest second moment are nonzero.  The list with repeated indices has the normaliser N 7 2: a joint named twice
    counts twice, as in the reference's gather x[:, keylist]."""
    worst, n_amb, rule_v = ipo_single_iterations_from_the_oracle(zh, J, kl, N, axes)
    _report(dict(test="ipo_key_lists_single", J=J, k=len(kl), keylist=kl, N=N, axes=axes, ambiguous_pose_iterations=n_amb,
                 max_param_delta=worst, max_v_delta=rule_v.delta, fp32_oracle_v_delta=rule_v.delta32, v_bound=rule_v.bound, v_ratio=rule_v.ratio))
    assert n_amb <= 0.01 * 50 * N, n_amb
    assert worst > 0 and rule_v.largest > 0
    assert rule_v.holds(), (rule_v.delta, rule_v.bound)


# ---- b. both kernels, bit for bit ------------------------------------------------------------------------------------------------------

CHILD = r"""
import os, sys
root = %r
sys.path[:0] = [os.path.join(root, "zedo-release_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")]
import _ipo_state
_ipo_state.key_lists_child_main()
"""


def test_both_kernels_agree_bit_for_bit_at_every_key_list_length():
    """One child process per pin (ZEDO_IPO_KERNEL=half, then row: read once per process; the second is not started if the first
    failed).  Each runs every list at N = 8 and 64 with H = 2 and axes "z" and "xyz", 500 iterations through zedo_ipo_fit_resume from
    it_begin = 0 with a state buffer (tests/_ipo_state.py::key_lists_child_main), asserts that every output is finite, and returns
    a SHA-256 per case over R, T, q, scale and all 15 state columns.  The two dictionaries are equal and no two cases share a
    digest - the k = 11 list, its sorted and its reversed form included: their sums differ in rounding."""
    res = {}
    for pin in ("half", "row"):
        e = dict(os.environ)
        e["ZEDO_IPO_KERNEL"] = pin
        r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (pin, r.stdout[-1000:] + r.stderr[-3000:])
        res[pin] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert len(res["half"]) == len(LISTS) * 4 == len(S.key_list_cases())
    assert res["half"] == res["row"], {k: (v, res["row"].get(k)) for k, v in res["half"].items() if v != res["row"].get(k)}
    assert len(set(res["half"].values())) == len(res["half"])


# ---- c. the dispatch seam, unpinned -------------------------------------------------------------------------------------------------------

SEAM_N, SEAM_H, SEAM_ITERS = 64, 320, 20
SEAM_B = [1, 2, 127, 129, 4096, 7167, 7168, 7169, 12287, 12288, 12289, 17407, 17408, 17409]
SEAM_SHARD = (7000, 6000)                                   # row_offset, B
SEAM_LISTS = [(J, kl) for J, kl in IPO_LENGTH_KEYS if len(kl) in (6, 11, 16)]


@pytest.mark.parametrize("J,kl", SEAM_LISTS, ids=[f"k{len(kl)}" for _, kl in SEAM_LISTS])
def test_a_call_of_any_size_returns_the_rows_of_the_whole_batch(zh, J, kl):
    """N = 64 poses x H = 320 hypotheses = 20 480 rows, axes "xyz", 20 iterations, nothing pinned: one call of all rows, then calls of
    the first B rows for every B of SEAM_B and one shard of 6 000 rows at row_offset 7 000; R, T, q and scale of every call are bit
    for bit the same rows of the whole batch.  launch_ipo_fit picks the lane-per-row kernel from B >= CUs x (4 k + 4) rows: on a
    256-CU device that is 7 168, 12 288 and 17 408 rows for k = 6, 11 and 16, and SEAM_B brackets each of the three by one row; the
    20 480-row call runs the lane-per-row kernel at all three lengths.  The shard starts and ends inside a hypothesis (7000 = 109 x 64
    + 24) and with its 6 000 rows lies below the k = 6 and k = 11 crossovers although it covers the global rows around them.  On
    another CU count the seam lies elsewhere and the test is still valid: it asserts a property of the entry point (a row's result
    does not depend on B, row_offset or the kernel that ran it: include/zedo_hip.h), not a dispatch."""
    cl, uvn, Kn = make_ipo_problem(J, SEAM_N, H=SEAM_H)
    x0, uv, K = dev(cl), dev(uvn), dev(Kn)
    norm, rows = SEAM_N * len(kl) * 2, SEAM_N * SEAM_H
    fit = lambda B, off=0: zh.ipo_fit(x0, uv, K, kl, "xyz", IPO_T, IPO_MIN, IPO_MAX, SEAM_ITERS, norm, B, row_offset=off, return_params=True)
    full = fit(rows)
    assert all(bool(torch.isfinite(t).all()) for t in full) and full[0].shape == (rows, 3, 3)
    assert not torch.equal(full[0][0:SEAM_N], full[0][SEAM_N:2 * SEAM_N])          # the hypotheses differ: h does select x0[h]
    assert not S.same_bits(full[2][0], full[2][SEAM_N])                            # hypothesis 0 and hypothesis 1 of pose 0
    for B in SEAM_B:
        for name, a, b in zip(("R", "T", "q", "scale"), full, fit(B)):
            assert b.shape[0] == B and S.same_bits(a[:B], b), (B, name, int((a[:B] != b).reshape(B, -1).any(1).sum()))
    off, B = SEAM_SHARD
    for name, a, b in zip(("R", "T", "q", "scale"), full, fit(B, off)):
        assert S.same_bits(a[off:off + B], b), ("shard", name, int((a[off:off + B] != b).reshape(B, -1).any(1).sum()))
