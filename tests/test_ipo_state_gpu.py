"""GPU tests of the resumable IPO state (zedo_ipo_fit_resume): the instrument every single-iteration test of the IPO kernels rests on.

What those tests leave open, closed here (the second moments against float64 are asserted in the single-iteration tests themselves):
  - the scale on, beside and beyond the clamp - in the trajectories of every fixture it leaves the clamp only above IPO_MAX, so the lower
    side of the clamp backward and of fmaxf(scale, min) never decided anything;
  - a fit split into resumed calls against the fit in one call, bit for bit in R, T, q, scale and all 15 state columns: with a state
    buffer that arrives dirty and is larger than the batch, an odd row count, a row shard, iters = 0, and across the end of the
    constant table of Adam's bias corrections;
  - all of it in the lane-per-row kernel, which no test had ever resumed: one child process per pin of ZEDO_IPO_KERNEL, digests over
    outputs AND state equal between the two kernels.
This process runs unpinned - the half-wave kernel at these row counts on any device of 8 compute units or more - and holds the values
to the float64 oracle; the equality of the digests carries that to ipo_row_kernel.  The cases, the launches and what the arbiter is
held to: tests/_ipo_state.py, tests/test_ipo_state_ref.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _ipo_state as S
from _shared import IPO_MAX, IPO_MIN, KEYS, MomentRule, dev, one_arithmetic_mode, report_env as _report, zh  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the scale on, beside and beyond the clamp ------------------------------------------------------------------------------------

@pytest.mark.parametrize("J,kl,axes", [(J, kl, axes) for J, kl in S.CLAMP_KEYS for axes in S.CLAMP_AXES],
                         ids=[f"J{J}-k{len(kl)}-{axes or 'none'}" for J, kl in S.CLAMP_KEYS for axes in S.CLAMP_AXES])
def test_scale_on_beside_and_beyond_the_clamp(zh, J, kl, axes):
    """The oracle's float64 state after 0, 10 and 30 iterations (N = 8, general K) with the scale of all poses set to 0.3, the fp32
    number below 0.5, 0.5, 2.0, the fp32 number above 2.0 and 2.4; one iteration and four iterations in one call with it_begin = the
    state's iteration count, against O.ipo_fit(init=, it0=) in float64:
      parameters within 1e-6 on the poses whose residuals are >= 1e-3 px in every iteration of the call;
      both moment rows by the rule of the single-iteration tests (_shared.MomentRule: 2 x the fp32 oracle's own distance + 1 ulp),
      its three maxima taken over all clear pose-iterations of the test, as there;
      the returned T within 1e-6 of T0 clip(scale), T0 from the oracle in float64 and the scale the one this call returned, read as
      float64 - the statement of ipo_store, fmaxf(scale, min) included;
      q and scale returned are the state's parameters - the scale UNCLAMPED;
      with "" the three axis slots keep the bits that went in.
    At most 5 % of the pose-iterations are left out (tests/test_ipo_state_ref.py asserts that share from the oracle alone).
    After 0 iterations the state is handed in with it_begin = 0, where zedo_ipo_fit_resume does not read it: all six values must
    give the fit from RotOpt's initial values.

    Why T is not held to T0 clip(scale) of the ORACLE's end state at 1e-6: |T0| = IPO_T = 5, so a scale that is within its own
    1e-6 moves T by up to 5e-6.  The fp32 oracle itself is up to 2.0e-6 from that product (21 of these 216 calls above 1e-6), and
    within 7.9e-7 of the product with its own scale; the kernel's distance to the oracle's product is reported as T_delta_oracle."""
    prob = S.Problem(J, kl, S.N8)
    left_out, total, rule_m, rule_v = 0, 0, MomentRule(), MomentRule()
    for it_state in S.CLAMP_STATES:
        for tag, value in S.CLAMP_SCALES:
            worst, worst_T, worst_To, case_m, case_v = 0.0, 0.0, 0.0, MomentRule(), MomentRule()
            for iters in S.CLAMP_ITERS:
                handed, want, o32, clear, T0 = S.clamp_reference(J, tuple(kl), axes, it_state, value, iters)
                s_in = handed.astype(np.float32)
                st = dev(s_in)
                R, T, q, sc = prob.fit(zh, axes, iters, S.N8, state=st, it_begin=it_state)
                out32 = st.cpu().numpy()
                out = out32.astype(np.float64)
                left_out, total = left_out + iters * int((~clear).sum()), total + iters * S.N8
                assert np.array_equal(q.cpu().numpy(), out32[:, 0:4]) and np.array_equal(sc.cpu().numpy(), out32[:, 4])
                if axes == "" and it_state > 0:
                    cols = [1, 2, 3, 6, 7, 8, 11, 12, 13]
                    assert np.array_equal(out32[:, cols].view(np.uint32), s_in[:, cols].view(np.uint32)), (it_state, tag, iters)
                d = float(np.abs(out - want)[clear][:, :5].max())
                T_got = T.cpu().numpy().astype(np.float64)
                dT = float(np.abs(T_got - T0 * np.clip(out[:, 4], IPO_MIN, IPO_MAX)[:, None])[clear].max())
                dTo = float(np.abs(T_got - T0 * np.clip(want[:, 4], IPO_MIN, IPO_MAX)[:, None])[clear].max())
                worst, worst_T, worst_To = max(worst, d), max(worst_T, dT), max(worst_To, dTo)
                for rule in (rule_m, case_m):
                    rule.add(out[clear][:, 5:10], o32[clear][:, 5:10], want[clear][:, 5:10])
                for rule in (rule_v, case_v):
                    rule.add(out[clear][:, 10:15], o32[clear][:, 10:15], want[clear][:, 10:15])
                assert d <= 1e-6, (it_state, tag, iters, d)
                assert dT <= 1e-6, (it_state, tag, iters, dT)
                if it_state > 0 and iters == 1 and tag in ("0.3", "2.4"):          # one step is at most ~lr = 0.1: still beyond the clamp
                    assert bool(((sc < IPO_MIN) | (sc > IPO_MAX)).all()), (it_state, tag)
            _report(dict(test="ipo_state_clamp", J=J, k=len(kl), axes=axes, state_after=it_state, scale=tag, max_param_delta=worst,
                         param_bound=1e-6, max_T_delta=worst_T, T_bound=1e-6, T_delta_oracle=worst_To, max_moment_delta=case_m.delta,
                         fp32_oracle_moment_delta=case_m.delta32, max_v_delta=case_v.delta, fp32_oracle_v_delta=case_v.delta32))
    _report(dict(test="ipo_state_clamp_moments", J=J, k=len(kl), axes=axes, left_out_pose_iterations=left_out, pose_iterations=total,
                 max_moment_delta=rule_m.delta, moment_bound=rule_m.bound, moment_ratio=rule_m.ratio, max_v_delta=rule_v.delta,
                 v_bound=rule_v.bound, v_ratio=rule_v.ratio))
    assert rule_m.holds(), (rule_m.delta, rule_m.bound)
    assert rule_v.holds() and rule_v.largest > 0, (rule_v.delta, rule_v.bound)
    assert left_out <= 0.05 * total, (left_out, total)


# ---- two calls equal one ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axes", S.SPLIT_AXES, ids=[a or "none" for a in S.SPLIT_AXES])
@pytest.mark.parametrize("J,kl", KEYS, ids=[f"J{J}-k{len(kl)}" for J, kl in KEYS])
def test_a_fit_split_into_resumed_calls_is_the_unsplit_fit(zh, J, kl, axes):
    """60 iterations in one call against 1 + 59, 25 + 35, 59 + 1 and 20 + 20 + 20 (general K, H = 2, N = 8): R, T, q, scale and all 15
    state columns bit for bit, for B = 16, B = 7 (odd: the half-wave without a row shadows row 6 and must store nothing), B = 14 at
    row_offset 5 (of H = 3: H = 2 has no row 16 .. 18), and B = 131 (N = 131, H = 1).  Every chain starts with it_begin = 0 on a state
    buffer of B + 2 rows whose bytes are all 0xFF: the first call gives the bits of the call without a state, overwrites rows
    [0, B) and leaves the two rows behind them alone.  iters = 0 with it_begin = 60 returns the state unchanged and R, T, q, scale of its parameters
    (tests/_ipo_state.py::round_trip).  Equality is what the design promises: parameters and moments are stored as the fp32
    registers, and below iteration 2048 every call reads the same table."""
    digests = {}
    for row in S.ROWS + [S.ROWS_FULL_BLOCK]:
        tag, N, H, B, off = row
        digests[tag] = S.round_trip(zh, S.Problem(J, kl, N, H), axes, B, off, S.split_id(J, kl, axes, row))
    assert len(set(digests.values())) == len(digests)


def test_a_split_fit_across_the_end_of_the_table(zh):
    """The float64 state after 20 iterations ((17, [0, 1, 4]), N = 8, "xyz") declared to be the state after 2040: 16 iterations in one
    call (the seam at 2048 is crossed inside the kernel's loop) against 8 + 8 (the second call starts ON the seam, with beta^2048
    formed by the host) and 5 + 11, bit for bit.  The host loop and the kernel form the same double products, and division and
    square root are correctly rounded on both sides."""
    S.round_trip_across_the_table_end(zh, S.seam_state())


# ---- the same in the lane-per-row kernel ---------------------------------------------------------------------------------------------

CHILD = r"""
import os, sys
root = %r
sys.path[:0] = [os.path.join(root, "zedo-release_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")]
import _ipo_state
_ipo_state.child_main(%r)
"""


def test_both_kernels_resume_to_the_same_bits(tmp_path):
    """One child process per pin (ZEDO_IPO_KERNEL=half, then row; read once per process; the second is not started if the first
    failed).  Each runs the clamp cases, the round trips (asserted inside the child as well: that is the split fit inside the
    lane-per-row kernel, B = 131 filling one 128-lane workgroup and a tail of 3) and the 50 single iterations of
    test_ipo_single_iterations_on_general_intrinsics at N = 8 for all eight axis subsets, from fp32 states this process writes to an
    .npz, and returns a SHA-256 per case over R, T, q, scale and the state.  The two dictionaries are equal, and no two cases share
    a digest - except the six scale values of a state handed in with it_begin = 0, which is not read: those six are one digest."""
    path = str(tmp_path / "ipo_states.npz")
    S.write_child_inputs(path)
    res = {}
    for pin in ("half", "row"):
        e = dict(os.environ)
        e["ZEDO_IPO_KERNEL"] = pin
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, path)], env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (pin, r.stdout[-1000:] + r.stderr[-3000:])
        res[pin] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    n_clamp = len(S.CLAMP_KEYS) * len(S.CLAMP_AXES) * len(S.CLAMP_STATES) * len(S.CLAMP_SCALES) * len(S.CLAMP_ITERS)
    assert len(res["half"]) == len(KEYS) * len(S.AXES8) + n_clamp + len(S.split_cases()) + 1
    assert res["half"] == res["row"], {k: (v, res["row"].get(k)) for k, v in res["half"].items() if v != res["row"].get(k)}
    unread = [k for k in res["half"] if k.startswith("clamp_") and "_s0_" in k]
    groups = {}
    for k in unread:
        groups.setdefault(k.split("_s0_")[0] + k[-3:], set()).add(res["half"][k])
    assert all(len(v) == 1 for v in groups.values()) and len(groups) == len(unread) // len(S.CLAMP_SCALES)
    cases = {}
    for k, v in res["half"].items():
        cases.setdefault(v, []).append(k if k not in unread else k.split("_s0_")[0] + "_s0_*" + k[-3:])
    shared = [sorted(set(ks)) for ks in cases.values() if len(set(ks)) > 1]
    assert not shared, shared
