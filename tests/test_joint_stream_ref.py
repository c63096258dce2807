"""CPU: the numpy reference of the fixed-lag streaming selection (tests/_joint_stream_ref.py) on its own, and the host arithmetic of
zedo_joint_stream_state_bytes.  fixed_lag is held to what defines it: path and cost at frame n are those of the OFFLINE reference
(_joint_temporal_ref.joint_temporal_ref, run again on the truncated inputs) on the clip cut after frame min(n + lag, last); a lag of the
clip's length - 1 gives the offline arrays; and the lag matters on these inputs.  The state size is pinned to the layout the header
documents, with R = lag + max_frames and SJ = S J:
    zedo_joint_stream_state_bytes = 8 (SJ R H + 4 SJ H + S) + pad8(4 (SJ R H + SJ R + SJ))
        D f64 [SJ,R,H] | lastX f64 [SJ,H,3] | lastD f64 [SJ,H] | t i64 [S] | back i32 [SJ,R,H] | dead i32 [SJ,R] | lastdead i32 [SJ]
and 0 for a shape the calls refuse (no GPU call: the function is host arithmetic)."""
import ctypes

import numpy as np
import pytest

from _joint_stream_ref import LAGS, check_inputs, chunkings, differ_share, emitted, fixed_lag
from _joint_temporal_ref import case, dead_joint_case, joint_temporal_ref, reference
from _shared import host_fn  # (imports torch first: it must precede the dlopen of libzedo_hip.so, torch bundles its own HIP runtime)
from _temporal_ref import clips

INT_MAX = 2 ** 31 - 1


def truncated(x, T, u, N, a, e):
    """The frames a .. e of a case as a problem of their own: rows (h, n) h-major."""
    H = x.shape[0] // N
    rows = (np.arange(H)[:, None] * N + np.arange(a, e + 1)[None, :]).reshape(-1)
    return x[rows], T[rows], u[rows]


def hold_to_truncated_clips(x, T, u, N, seq, lam, tables):
    for lag in LAGS:
        path, cost = fixed_lag(tables, seq, lag)
        for a, b in zip(seq[:-1], seq[1:]):
            cut = {}
            for n in range(a, b):
                e = min(n + lag, b - 1)
                if e not in cut:
                    xt, Tt, ut = truncated(x, T, u, N, a, e)
                    cut[e] = joint_temporal_ref(ut, xt, Tt, [0, e + 1 - a], lam)
                assert np.array_equal(path[n], cut[e]["path"][n - a]), (lag, n)
                assert np.array_equal(cost[n].view(np.int64), cut[e]["cost"][n - a].view(np.int64)), (lag, n)


@pytest.mark.parametrize("J,N,H,L", [(3, 130, 7, 130), (5, 12, 3, 4)], ids=lambda v: str(v))
def test_every_frame_is_the_offline_reference_on_the_truncated_clip(J, N, H, L):
    x, T, u = case(J, N, H)
    hold_to_truncated_clips(x, T, u, N, clips(N, L), 100.0, reference(J, N, H, L, 100.0))


def test_dead_joint_case_on_truncated_clips_and_its_pinned_paths():
    """A dead (frame, joint) inside the lag window and a chain end before the horizon.  Joint 2's fixed-lag path at lambda = 100 is
    pinned at lag 0 and at lag 8 (= the offline path); the other joints are those of the untouched unaries."""
    x, T, u, j = dead_joint_case()
    for lam in (0.0, 100.0):
        hold_to_truncated_clips(x, T, u, 9, [0, 9], lam, joint_temporal_ref(u, x, T, [0, 9], lam))
    r = joint_temporal_ref(u, x, T, [0, 9], 100.0)
    clean = joint_temporal_ref(case(5, 9, 3)[2], x, T, [0, 9], 100.0)
    others = [i for i in range(5) if i != j]
    for lag in (0, 1, 2, 8):
        p, c = fixed_lag(r, [0, 9], lag)
        p0, c0 = fixed_lag(clean, [0, 9], lag)
        assert np.array_equal(p[:, others], p0[:, others]) and np.array_equal(c[:, others], c0[:, others])
        assert p[4, j] == 0 and np.isposinf(c[4, j]) and np.isfinite(np.delete(c[:, j], 4)).all()
    assert fixed_lag(r, [0, 9], 0)[0][:, j].tolist() == [0, 0, 0, 1, 0, 2, 0, 0, 0]
    assert fixed_lag(r, [0, 9], 8)[0][:, j].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0] == r["path"][:, j].tolist()


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (3, 130, 7, 130), (5, 12, 3, 4), (2, 30, 130, 13)], ids=lambda v: str(v))
def test_a_lag_of_the_clip_length_is_the_offline_reference(J, N, H, L):
    for lam in (30.0, 100.0):
        r = reference(J, N, H, L, lam)
        for lag in (L - 1, L, 10 * L):
            p, c = fixed_lag(r, clips(N, L), lag)
            assert np.array_equal(p, r["path"]) and np.array_equal(c.view(np.int64), r["cost"].view(np.int64))


def test_lag_zero_is_the_arg_min_of_D():
    r = reference(17, 70, 50, 35, 100.0)
    p, c = fixed_lag(r, clips(70, 35), 0)
    assert np.array_equal(p, np.argmin(r["D"], axis=2)) and np.array_equal(c, r["D"].min(axis=2))


def test_the_lag_matters_on_these_inputs():
    """The shares of (frame, joint) at which the fixed-lag decision differs from the whole-clip path: no test at a finite lag is vacuous."""
    shares = {lag: differ_share(17, 70, 50, 35, 100.0, lag) for lag in LAGS + (34,)}
    one = {lag: differ_share(3, 130, 7, 130, 100.0, lag) for lag in LAGS + (129,)}
    print("differs from the whole-clip path, (17,70,50,35): " + ", ".join(f"lag {k}: {100 * v:.1f} %" for k, v in shares.items())
          + "; (3,130,7,130): " + ", ".join(f"lag {k}: {100 * v:.1f} %" for k, v in one.items()))
    assert shares[1] > 0.25 and shares[8] > 0 and shares[34] == 0
    assert shares[0] > shares[1] > shares[3] > shares[8]
    assert one[1] > 0.25 and one[8] > 0 and one[129] == 0


def test_the_inputs_are_what_the_exact_comparison_assumes():
    assert check_inputs() > 1e-6


def test_the_counts_of_the_header_formula_add_up():
    """Over any chunking of a clip of L frames with a flush at the end, the pushes emit the frames 0 .. L-1 once each, in order, and no
    push more than F + lag."""
    for L in (1, 4, 9, 35):
        for lag in (0, 1, 3, 8, L - 1, L + 5):
            for name, cut in chunkings(L).items():
                t = nxt = 0
                for i, F in enumerate(cut):
                    first, count = emitted(t, F, lag, i == len(cut) - 1)
                    assert first == nxt == max(0, t - lag) and 0 <= count <= F + lag
                    nxt, t = first + count, t + F
                assert nxt == L == t, (L, lag, name)
    assert chunkings(7) == {"whole": [7], "single": [1] * 7, "growing": [1, 2, 3, 1]}


# ---- zedo_joint_stream_state_bytes: host arithmetic ----
@pytest.fixture(scope="module")
def state_bytes():
    return host_fn("zedo_joint_stream_state_bytes", ctypes.c_size_t, [ctypes.c_int] * 5)


def pad(v, k):
    return (v + k - 1) // k * k


def formula(S, H, J, lag, max_frames):
    sj, R = S * J, lag + max_frames
    return 8 * (sj * R * H + 4 * sj * H + S) + pad(4 * (sj * R * H + sj * R + sj), 8)


@pytest.mark.parametrize("S,H,J,lag,mf", [(1, 1, 1, 0, 1), (1, 3, 1, 0, 1), (3, 7, 5, 2, 3), (16, 50, 17, 30, 8), (1, 50, 17, 1014, 1015),
                                          (2, 1024, 1, 8, 9), (29, 50, 17, 34, 35), (1, 5, 3, 100, 1)])
def test_state_bytes_match_the_documented_layout(state_bytes, S, H, J, lag, mf):
    assert state_bytes(S, H, J, lag, mf) == formula(S, H, J, lag, mf)
    assert formula(S, H, J, lag, mf) % 8 == 0


def test_state_bytes_are_zero_for_the_shapes_the_calls_refuse(state_bytes):
    ok = (3, 7, 5, 2, 3)
    assert state_bytes(*ok) > 0
    for i, v in ((0, 0), (0, -1), (1, 0), (1, -2), (1, 1025), (2, 0), (2, -1), (3, -1), (4, 0), (4, -5)):
        bad = list(ok)
        bad[i] = v
        assert state_bytes(*bad) == 0, bad
    assert state_bytes(1, 1024, 1, 0, 1) == formula(1, 1024, 1, 0, 1)
    # (lag + max_frames) S J H past INT_MAX: through S J, through the rows, through lag + max_frames itself; the largest inside answers
    assert state_bytes(65536, 1, 32768, 0, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, 1) == 0
    assert state_bytes(1, 1, 1, INT_MAX, INT_MAX) == 0
    assert state_bytes(1, 64, 1, 0, INT_MAX // 64 + 1) == 0
    assert state_bytes(1 << 10, 1 << 10, 1 << 5, 32, 32) == 0
    assert state_bytes(1, 64, 1, 0, INT_MAX // 64) == formula(1, 64, 1, 0, INT_MAX // 64)
    assert state_bytes(1, 1, 1, INT_MAX - 1, 1) == formula(1, 1, 1, INT_MAX - 1, 1)
