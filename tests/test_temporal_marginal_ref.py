"""CPU: the numpy reference of zedo_temporal_marginal (tests/_temporal_marginal_ref.py) on its own - against the enumeration of all H^L
paths of one clip; its limits: at a temperature far below the gap between the best and the second-best path the arg-max of the marginals
is the Viterbi path of _temporal_ref, at lambda = 0 and on clips of one frame the marginals are a softmax; the order of the sums is free
within beta; the condition on the inputs under which NO arg-max is left out of a comparison; and the figures that motivate the call, as
ORDER only.  They are properties of these synthetic inputs: whether the fused pose is closer to ground truth on real video is not
measured here or anywhere."""
import numpy as np
import pytest

from _temporal_marginal_ref import (brute_force_clip, case, check_inputs, clips, marg_bound, reference, softmax_ref, temporal_marginal_ref,
                                    translation)
from _temporal_ref import reference as viterbi_reference

LIMIT_CASES = [(17, 70, 50, 35), (17, 300, 7, 300), (17, 40, 300, 13)]


@pytest.mark.parametrize("H,L", [(3, 4), (2, 7)])
@pytest.mark.parametrize("lam,tau", [(100.0, 1.0), (30.0, 0.25), (0.0, 2.0)])
def test_reference_is_the_enumeration_of_all_paths(H, L, lam, tau):
    """One clip of L frames; with H = 3 one hypothesis of frame 1 is excluded (NaN: +inf in the enumeration, weight 0 exactly)."""
    J = 5
    x, u = case(J, L, H)
    u = u.copy()
    if H == 3:
        u.reshape(H, L)[2, 1] = np.nan
    T = translation(L, H)
    r = temporal_marginal_ref(u, x, T, [0, L], lam, tau)
    ub = u.copy()
    ub[~np.isfinite(ub)] = np.inf
    w, lz = brute_force_clip(ub, x, L, lam, tau)
    assert np.abs(r["w"] - w).max() < 1e-13 and np.abs(r["logz"] - lz).max() < 1e-12
    X = (x.astype(np.float64) + T.astype(np.float64)[:, None, :]).reshape(H, L, J, 3)
    for n in range(L):
        mu = (w[n][:, None, None] * X[:, n]).sum(0)                                           # [J, 3]
        d = X[:, n] - mu
        full = (w[n][:, None, None, None] * d[:, :, :, None] * d[:, :, None, :]).sum(0)       # [J, 3, 3]
        assert np.abs(r["mean"][n] - mu).max() < 1e-12
        assert np.abs(r["cov"][n] - full[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]).max() < 1e-14
        assert r["hmax"][n] == int(np.argmax(w[n])) and abs(r["wmax"][n] - w[n].max()) < 1e-13
    if H == 3:
        assert r["w"][1, 2] == 0.0
    assert np.abs(r["w"].sum(1) - 1.0).max() < marg_bound(L, H, J, r["G"])
    # T moves the moments and nothing else
    r0 = temporal_marginal_ref(u, x, None, [0, L], lam, tau)
    assert np.array_equal(r0["w"], r["w"]) and np.array_equal(r0["logz"], r["logz"]) and not np.array_equal(r0["mean"], r["mean"])


@pytest.mark.parametrize("J,N,H,L", LIMIT_CASES, ids=lambda v: str(v))
def test_cold_marginals_are_the_viterbi_path(J, N, H, L):
    """tau = 1e-9 at lambda = 100: any other path costs at least the 1e-6 gap of _temporal_ref.check_inputs more, >= 1000 tau, so the
    most probable hypothesis of every frame is the Viterbi path's and holds more than 0.99 of the mass."""
    cold, path = reference(J, N, H, L, 100.0, 1e-9), viterbi_reference(J, N, H, L, 100.0)["path"]
    print(f"J={J} N={N} H={H} L={L}: tau = 1e-9: the smallest largest marginal is {cold['wmax'].min():.6f}")
    assert np.array_equal(cold["hmax"], path) and cold["wmax"].min() > 0.99


def test_chains_of_one_frame_and_lambda_zero_are_the_softmax():
    J, N, H, L = 5, 12, 3, 4
    x, u = case(J, N, H)
    for tau in (1.0, 0.3):
        sm = softmax_ref(u[:, None], N, tau)[:, 0]                                            # [N, H]
        assert np.abs(temporal_marginal_ref(u, x, None, list(range(N + 1)), 100.0, tau)["w"] - sm).max() < 1e-14
        assert np.abs(temporal_marginal_ref(u, x, None, clips(N, L), 0.0, tau)["w"] - sm).max() < 1e-13


def test_the_order_of_the_sums_is_free_within_the_bound():
    """The ascending and the descending evaluation of every sum over the hypotheses differ by far less than beta: a kernel may add in
    any fixed order."""
    J, N, H, L = 17, 70, 50, 35
    x, u = case(J, N, H)
    up = reference(J, N, H, L, 100.0, 1.0)
    down = temporal_marginal_ref(u, x, translation(N, H), clips(N, L), 100.0, 1.0, descending=True)
    d = float(np.abs(((up["A"] + up["B"]) - up["logz"][:, None]) - ((down["A"] + down["B"]) - down["logz"][:, None])).max())
    beta = marg_bound(L, H, J, up["G"])
    print(f"ascending against descending sums at J={J} N={N} H={H} L={L}: max |log w - log w'| = {d:.3e} (bound {beta:.3e})")
    assert 0.0 < d <= beta and np.abs(up["mean"] - down["mean"]).max() <= 1e-12


def test_no_arg_max_has_to_be_left_out_of_a_comparison():
    gap, beta2 = check_inputs()
    assert gap > 1e-4 and beta2 < 1e-5


def test_the_hard_answer_discards_mass_and_the_fused_pose_moves_less():
    """On (17, 70, 50) in clips of 35 at lambda = 100, tau = 1: the most probable hypothesis of a frame holds less than half of the
    posterior mass (median), and the posterior-mean pose moves less between consecutive frames than the selected one - per joint, in
    the median and at most.  ORDER only; the figures are printed."""
    J, N, H, L = 17, 70, 50, 35
    x, _ = case(J, N, H)
    r = reference(J, N, H, L, 100.0, 1.0, False)
    path = viterbi_reference(J, N, H, L, 100.0)["path"]
    X = x.astype(np.float64).reshape(H, N, J, 3)
    sel = X[path, np.arange(N)]                                                               # [N, J, 3]
    inside = np.ones(N - 1, bool)
    inside[np.array(clips(N, L)[1:-1]) - 1] = False                                           # no jump across a clip boundary
    jump = lambda p: np.linalg.norm(np.diff(p, axis=0), axis=2)[inside]
    js, jf = jump(sel), jump(r["mean"])
    print(f"largest marginal: median {np.median(r['wmax']):.3f}, minimum {r['wmax'].min():.3f}; arg-max differs from the Viterbi path on "
          f"{100 * (r['hmax'] != path).mean():.1f} % of frames; jump per joint, selected: median {1e3 * np.median(js):.1f} mm, max "
          f"{1e3 * js.max():.1f} mm; fused: median {1e3 * np.median(jf):.1f} mm, max {1e3 * jf.max():.1f} mm; median sqrt trace cov "
          f"{1e3 * np.median(np.sqrt(r['cov'][:, :, [0, 3, 5]].sum(-1))):.0f} mm")
    assert np.median(r["wmax"]) < 0.5
    assert np.median(jf) < np.median(js) and jf.max() < js.max()
