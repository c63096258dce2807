"""CPU: the numpy reference of the fixed-lag pose-level streaming selection (tests/_temporal_stream_ref.py) on its own.  fixed_lag is held to
what defines it: path and cost at frame n are those of the OFFLINE reference (_temporal_ref.temporal_ref, run again on the truncated
inputs) on the clip cut after frame min(n + lag, last) - paths exactly, costs bit for bit; a lag of the clip's length - 1 gives the offline
arrays; lag 0 is the arg-min of D; the inputs keep every arg-min apart; and the lag matters on these inputs, in the order of the table the
README prints."""
import numpy as np
import pytest

from _joint_stream_ref import chunkings, emitted
from _temporal_ref import case, clips, dead_frame_case, reference, switch_rate, temporal_ref
from _temporal_stream_ref import LAGS, REFUSED, STREAM_CASES, check_inputs, fixed_lag, lag_table

SMALL = [c for c in STREAM_CASES if c[3] <= 64 and c[2] <= 65]     # every truncation of every clip is an offline run of its own


def truncated(x, u, N, a, e):
    """The frames a .. e of a case as a problem of their own: rows (h, n) h-major."""
    H = x.shape[0] // N
    rows = (np.arange(H)[:, None] * N + np.arange(a, e + 1)[None, :]).reshape(-1)
    return x[rows], u[rows]


def hold_to_truncated_clips(x, u, N, seq, lam, tables, lags):
    cut = {}                                                       # the offline reference on the frames a .. e, by e
    for lag in lags:
        path, cost = fixed_lag(tables, seq, lag)
        for a, b in zip(seq[:-1], seq[1:]):
            for n in range(a, b):
                e = min(n + lag, b - 1)
                if e not in cut:
                    xt, ut = truncated(x, u, N, a, e)
                    cut[e] = temporal_ref(ut, xt, [0, e + 1 - a], lam)
                assert path[n] == cut[e]["path"][n - a], (lag, n)
                assert cost[n:n + 1].view(np.int64)[0] == cut[e]["cost"][n - a:n - a + 1].view(np.int64)[0], (lag, n)


def test_the_small_cases_are_the_ones_meant():
    assert [c[2] for c in SMALL] == [1, 2, 3, 5, 50, 64, 65, 5, 17, 3] and REFUSED[2] > 1024 and all(c[2] <= 1024 for c in STREAM_CASES)


@pytest.mark.parametrize("J,N,H,L", SMALL, ids=lambda v: str(v))
def test_every_frame_is_the_offline_reference_on_the_truncated_clip(J, N, H, L):
    x, u = case(J, N, H)
    hold_to_truncated_clips(x, u, N, clips(N, L), 100.0, reference(J, N, H, L, 100.0), LAGS)


def test_dead_frame_case_on_truncated_clips_and_its_pinned_paths():
    """A dead frame inside the lag window and a chain end before the horizon: [0,0,0,1,0,1,0,0,0] at lag 0, the offline path
    [0,0,0,1,0,0,0,0,0] from lag 1 on."""
    x, u = dead_frame_case()
    for lam in (0.0, 100.0):
        hold_to_truncated_clips(x, u, 9, [0, 9], lam, temporal_ref(u, x, [0, 9], lam), (0, 1, 2, 8))
    r = temporal_ref(u, x, [0, 9], 100.0)
    for lag in (0, 1, 2, 8):
        p, c = fixed_lag(r, [0, 9], lag)
        assert p[4] == 0 and np.isposinf(c[4]) and np.isfinite(np.delete(c, 4)).all()
        assert p.tolist() == ([0, 0, 0, 1, 0, 1, 0, 0, 0] if lag == 0 else [0, 0, 0, 1, 0, 0, 0, 0, 0]), lag
    assert r["path"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (17, 300, 7, 300), (5, 12, 3, 4), (17, 40, 300, 13)], ids=lambda v: str(v))
def test_a_lag_of_the_clip_length_is_the_offline_reference(J, N, H, L):
    for lam in (30.0, 100.0):
        r = reference(J, N, H, L, lam)
        for lag in (L - 1, L, 10 * L):
            p, c = fixed_lag(r, clips(N, L), lag)
            assert np.array_equal(p, r["path"]) and np.array_equal(c.view(np.int64), r["cost"].view(np.int64))


def test_lag_zero_is_the_arg_min_of_D():
    r = reference(17, 70, 50, 35, 100.0)
    p, c = fixed_lag(r, clips(70, 35), 0)
    assert np.array_equal(p, np.argmin(r["D"], axis=1)) and np.array_equal(c, r["D"].min(axis=1))


def test_the_inputs_are_what_the_exact_comparison_assumes():
    """Measured on these cases at lambda = 30 / 100 / 300: at least 4.1e-4 between the two best entries of D, 3.8e-6 between the two best
    candidates of a minimum."""
    dgap, mgap = check_inputs()
    assert dgap > 1e-8 and mgap > 1e-8


def test_the_lag_matters_on_these_inputs_in_the_order_of_the_readme_table():
    """(17, 70, 50) in clips of 35 at lambda = 100: the per-frame arg-min of the unaries switches hypothesis more often than any
    fixed-lag path, and the share of frames that differ from the whole-clip path and the switch rate both fall as the lag grows - to 0
    and to the whole-clip path's rate at lag 34.  Only the ORDER is asserted; the figures are printed."""
    J, N, H, L, lam = 17, 70, 50, 35, 100.0
    lags = (0, 1, 3, 8, 34)
    tab = lag_table(J, N, H, L, lam, lags)
    per_frame = np.argmin(case(J, N, H)[1].reshape(H, N), axis=0)
    whole = switch_rate(reference(J, N, H, L, lam)["path"], clips(N, L))
    print(f"per-frame arg-min: switch rate {100 * switch_rate(per_frame, clips(N, L)):.1f} %; whole clip: {100 * whole:.1f} %; "
          + "; ".join(f"lag {k}: differs {100 * d:.1f} %, switches {100 * s:.1f} %" for k, (d, s) in tab.items()))
    differ, sw = [tab[k][0] for k in lags], [tab[k][1] for k in lags]
    assert all(a > b for a, b in zip(differ[:-1], differ[1:])) and differ[-1] == 0
    assert all(a > b for a, b in zip(sw[:-1], sw[1:])) and sw[-1] == whole
    assert switch_rate(per_frame, clips(N, L)) > sw[0]


def test_the_counts_of_the_header_formula_add_up():
    """The formula is zedo_joint_stream_push's (tests/_joint_stream_ref.py::emitted): over any chunking of a clip with a flush at the
    end the pushes emit the frames 0 .. L-1 once each, in order."""
    for L in (1, 4, 9, 35):
        for lag in (0, 1, 3, 8, L - 1, L + 5):
            for name, cut in chunkings(L).items():
                t = nxt = 0
                for i, F in enumerate(cut):
                    first, count = emitted(t, F, lag, i == len(cut) - 1)
                    assert first == nxt == max(0, t - lag) and 0 <= count <= F + lag
                    nxt, t = first + count, t + F
                assert nxt == L == t, (L, lag, name)
