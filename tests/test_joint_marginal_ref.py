"""CPU: the numpy reference of zedo_joint_marginal (tests/_joint_marginal_ref.py) on its own - against the enumeration of all H^L paths of
every chain of a hand-built case (two joints, one excluded entry, one dead (frame, joint) that splits one joint's chain); its limits: at a
temperature far below the gap between the best and the second-best path the marginals are the Viterbi path of _joint_temporal_ref, at
tau = 1 they are soft; and the driver's argument checks that need no GPU."""
import numpy as np
import pytest

from _joint_marginal_ref import brute_force_chain, joint_marginal_ref, marg_bound, reference, softmax_ref
from _joint_temporal_ref import camera_frame, case
from _joint_temporal_ref import reference as viterbi_reference

LIMIT_CASES = [(17, 70, 50, 35), (2, 30, 130, 13), (3, 130, 7, 130)]


def hand_built():
    """H = 3, one clip of 5 frames, joints 0 and 1 of case(2, 5, 3): (frame 1, joint 0, hypothesis 2) is excluded (NaN); (frame 2, joint 1) is
    dead (NaN, +inf, -inf) - joint 1 has the chains [0, 1] and [3, 4], joint 0 the chain [0 .. 4]."""
    x, T, u = case(2, 5, 3)
    u = u.reshape(3, 5, 2).copy()
    u[2, 1, 0] = np.nan
    u[:, 2, 1] = [np.nan, np.inf, -np.inf]
    return x, T, u.reshape(15, 2)


@pytest.mark.parametrize("lam,tau", [(100.0, 1.0), (30.0, 0.25), (0.0, 2.0)])
def test_reference_is_the_enumeration_of_all_paths(lam, tau):
    x, T, u = hand_built()
    N, H, J = 5, 3, 2
    r = joint_marginal_ref(u, x, T, [0, N], lam, tau)
    X = camera_frame(x, T, N).transpose(1, 2, 0, 3)                                           # [N, J, H, 3]
    un = u.reshape(H, N, J).transpose(1, 2, 0).copy()
    un[~np.isfinite(un)] = np.inf
    assert r["dead"].sum() == 1 and r["dead"][2, 1]
    for j, frames in ((0, [0, 1, 2, 3, 4]), (1, [0, 1]), (1, [3, 4])):
        w, lz = brute_force_chain(un[frames, j], X[frames, j], lam, tau)
        assert np.abs(r["w"][frames, j] - w).max() < 1e-13
        assert np.abs(r["logz"][frames, j] - lz).max() < 1e-12
        for i, n in enumerate(frames):
            mu = (w[i][:, None] * X[n, j]).sum(0)
            d = X[n, j] - mu
            full = (w[i][:, None, None] * d[:, :, None] * d[:, None, :]).sum(0)
            assert np.abs(r["mean"][n, j] - mu).max() < 1e-12
            assert np.abs(r["cov"][n, j] - full[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]).max() < 1e-14
            assert r["hmax"][n, j] == int(np.argmax(w[i])) and abs(r["wmax"][n, j] - w[i].max()) < 1e-13
    assert r["w"][1, 0, 2] == 0.0                                                             # the excluded entry, exactly
    assert np.isnan(r["mean"][2, 1]).all() and np.isnan(r["cov"][2, 1]).all() and r["hmax"][2, 1] == 0 and r["wmax"][2, 1] == 0.0
    assert np.isneginf(r["logz"][2, 1]) and (r["w"][2, 1] == 0.0).all()
    assert r["logz"][0, 1] == r["logz"][1, 1] and r["logz"][3, 1] == r["logz"][4, 1] and r["logz"][1, 1] != r["logz"][3, 1]
    live = ~r["dead"]
    assert np.abs(r["w"].sum(2)[live] - 1.0).max() < marg_bound(N, H, r["G"])


@pytest.mark.parametrize("J,N,H,L", LIMIT_CASES, ids=lambda v: str(v))
def test_cold_marginals_are_the_viterbi_path_and_warm_ones_are_soft(J, N, H, L):
    """tau = 1e-9 at lambda = 100: any other path costs at least the 1e-6 gap of _joint_temporal_ref.check_inputs more, >= 1000 tau, so
    the most probable hypothesis of every (frame, joint) is the Viterbi path's and holds more than 0.99 of the mass.  tau = 1: the median
    largest marginal is under 0.9 - the Viterbi path discards a real share of the probability."""
    cold, path = reference(J, N, H, L, 100.0, 1e-9), viterbi_reference(J, N, H, L, 100.0)["path"]
    assert np.array_equal(cold["hmax"], path) and cold["wmax"].min() > 0.99
    warm = reference(J, N, H, L, 100.0, 1.0)
    print(f"J={J} N={N} H={H} L={L}: tau = 1: the largest marginal has median {np.median(warm['wmax']):.2f}, minimum {warm['wmax'].min():.2f}; "
          f"G = {warm['G']:.1f}; tau = 1e-9: minimum {cold['wmax'].min():.6f}")
    assert np.median(warm["wmax"]) < 0.9
    assert np.abs(warm["w"].sum(2) - 1.0).max() < marg_bound(L, H, warm["G"])


def test_the_order_of_the_sums_is_free_within_the_bound():
    """The ascending and the descending evaluation of every sum over the hypotheses differ by far less than marg_bound: a kernel may add in
    any fixed order."""
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    up, down = reference(J, N, H, L, 100.0, 1.0), joint_marginal_ref(u, x, T, [0, 35, 70], 100.0, 1.0, descending=True)
    d = float(np.abs((up["A"] + up["B"] - up["logz"][:, :, None]) - (down["A"] + down["B"] - down["logz"][:, :, None])).max())
    beta = marg_bound(L, H, up["G"])
    print(f"ascending against descending sums at J={J} N={N} H={H} L={L}: max |log w - log w'| = {d:.3e} (bound {beta:.3e})")
    assert 0.0 < d <= beta and np.abs(up["mean"] - down["mean"]).max() <= 1e-12


def test_chains_of_one_frame_and_lambda_zero_are_the_softmax():
    J, N, H, L = 5, 12, 3, 4
    x, T, u = case(J, N, H)
    for tau in (1.0, 0.3):
        sm = softmax_ref(u, N, tau)
        assert np.abs(joint_marginal_ref(u, x, T, list(range(N + 1)), 100.0, tau)["w"] - sm).max() < 1e-14
        assert np.abs(joint_marginal_ref(u, x, T, [0, 4, 8, N], 0.0, tau)["w"] - sm).max() < 1e-13


def test_driver_accepts_joints_fused_with_its_switches():
    """Argument checks that need no GPU: --select joints-fused takes --smooth / --seq_len / --temperature (defaults 100 and 1), refuses bad
    values; the other choices refuse --temperature and keep refusing the two other switches in the words they used."""
    from run._driver import build_parser, check_select_args
    p = build_parser("t", inference=True)
    base = ["--config", "c.py", "--select", "joints-fused"]
    a = p.parse_args(base)
    check_select_args(a)
    assert a.select == "joints-fused" and a.smooth == 100.0 and a.temperature == 1.0 and a.seq_len is None
    a = p.parse_args(base + ["--smooth", "0", "--seq_len", "7", "--temperature", "1e-9"])
    check_select_args(a)
    assert a.smooth == 0.0 and a.seq_len == 7 and a.temperature == 1e-9
    for extra in (["--smooth", "-1"], ["--seq_len", "0"], ["--temperature", "0"], ["--temperature", "-1"], ["--temperature", "nan"],
                  ["--temperature", "inf"]):
        with pytest.raises(SystemExit):
            check_select_args(p.parse_args(base + extra))
    for sel in ("none", "reproj", "joints", "temporal", "joints-temporal"):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(["--config", "c.py", "--select", sel, "--temperature", "2"]))
        assert "--temperature is a switch of --select joints-fused" in str(e.value)
    with pytest.raises(SystemExit) as e:
        check_select_args(p.parse_args(["--config", "c.py", "--select", "joints", "--seq_len", "4"]))
    assert str(e.value) == "--smooth and --seq_len are switches of --select temporal and --select joints-temporal"
