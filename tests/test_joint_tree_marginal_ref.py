"""CPU: the numpy reference of zedo_joint_tree_marginal (tests/_joint_tree_marginal_ref.py) on its own - against the enumeration of all
H^J assignments on the three small trees _joint_tree_ref enumerates (with and without confidences) and on its dead-joint case; its
limits: without the bone term every joint is a softmax on its own, one hypothesis is certain; the marginals of a spanning tree do not
depend on the joint it is rooted at; the order of the sums is free within the bound the GPU test uses; the share of (pose, joint) whose
arg-max is too close to call stays under 1 % on every case the GPU test runs; and the driver's argument checks that need no GPU."""
import numpy as np
import pytest

import _joint_tree_marginal_ref as M
import _joint_tree_ref as R
from _joint_tree_marginal_ref import case, joint_tree_marginal_ref


def full_cov(w, X):
    m = (w[:, None] * X).sum(0)
    d = X - m
    return m, (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(0)[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def against_enumeration(u, x, T, parent, mu, tau, N, weight=None):
    J = len(parent)
    r = joint_tree_marginal_ref(u, x, T, parent, mu, tau, N, weight)
    w, lz, bone = M.enumerate_marginals(u, x, T, parent, mu, tau, N, weight)
    assert np.abs(r["w"] - w).max() < 1e-12
    assert np.abs(r["bone"] - bone).max() < 1e-12
    X = M.camera_frame(x, T, N)
    for n in range(N):
        live = r["live"][n]
        roots = [j for j in range(J) if live[j] and not (parent[j] >= 0 and live[parent[j]])]
        assert abs(sum(r["logz"][n, j] for j in roots) - lz[n]) < 1e-10 * max(1.0, abs(lz[n]))
        for j in range(J):
            if not live[j]:
                continue
            p = j
            while parent[p] >= 0 and live[parent[p]]:              # logz is repeated on every joint of the component
                p = parent[p]
            assert r["logz"][n, j] == r["logz"][n, p]
            m, c6 = full_cov(w[n, j], X[:, n, j])
            assert np.abs(r["mean"][n, j] - m).max() < 1e-11 and np.abs(r["cov"][n, j] - c6).max() < 1e-12
            assert abs(r["wmax"][n, j] - w[n, j].max()) < 1e-12
            top = np.sort(w[n, j])
            if top.size == 1 or top[-1] - top[-2] > 1e-9:
                assert r["hmax"][n, j] == int(np.argmax(w[n, j]))
    return r


@pytest.mark.parametrize("J,H,tree", [(5, 4, "heap"), (6, 3, "chain"), (4, 5, "forest")], ids=lambda v: str(v))
@pytest.mark.parametrize("with_weight", [False, True], ids=["plain", "weights"])
def test_reference_is_the_enumeration_of_all_assignments(J, H, tree, with_weight):
    N = 3
    x, T, u = case(J, N, H)
    parent = {"heap": R.heap_tree, "chain": R.reversed_chain, "forest": R.two_roots}[tree](J)
    wgt = M.confidences(N, J) if with_weight else None
    for mu, tau in ((100.0, 1.0), (30.0, 0.25)):
        r = against_enumeration(u, x, T, parent, mu, tau, N, wgt)
        assert np.abs(r["w"].sum(2) - 1.0).max() < M.marg_bound(J, H, r["G"])


def test_reference_is_the_enumeration_with_a_dead_joint_and_excluded_entries():
    x, T, u, parent, j = M.dead_joint_case()
    N, H, J = 9, 3, 5
    r = against_enumeration(u, x, T, parent, 100.0, 1.0, N)
    assert not r["live"][4, j] and r["live"].sum() == N * J - 1
    assert np.isnan(r["mean"][4, j]).all() and np.isnan(r["cov"][4, j]).all() and r["hmax"][4, j] == 0 and r["wmax"][4, j] == 0.0
    assert np.isneginf(r["logz"][4, j]) and r["bone"][4, j] == 0.0 and (r["w"][4, j] == 0.0).all()
    assert (r["bone"][4, [3, 4]] == 0.0).all()                      # roots now: three components in that pose
    assert len({r["logz"][4, 0], r["logz"][4, 3], r["logz"][4, 4]}) == 3 and r["logz"][4, 2] == r["logz"][4, 0]
    excluded = ~np.isfinite(R.unaries(u, N))
    assert (r["w"][excluded] == 0.0).all() and (r["w"][~excluded] > 0.0).all()


@pytest.mark.parametrize("J,N,H", [(5, 12, 3), (17, 6, 50)], ids=lambda v: str(v))
def test_without_the_bone_term_every_joint_is_a_softmax_on_its_own(J, N, H):
    x, T, u = case(J, N, H)
    parent = M.default_tree(J)
    for tau in (1.0, 0.3):
        r = joint_tree_marginal_ref(u, x, T, parent, 0.0, tau, N)
        un = R.unaries(u, N)
        e = np.exp(-(un - un.min(axis=2, keepdims=True)) / tau)
        assert np.abs(r["w"] - e / e.sum(axis=2, keepdims=True)).max() < 1e-13
        per_joint = M.lse_ascending(-un / tau)                      # [N,J]: one root here, so logz is the sum over all joints
        assert np.abs(r["logz"] - per_joint.sum(1, keepdims=True)).max() < 1e-9 * np.abs(per_joint.sum(1)).max()


def test_one_hypothesis_is_certain():
    J, N, H = 5, 4, 1
    x, T, u = case(J, N, H)
    parent = R.heap_tree(J)
    r = joint_tree_marginal_ref(u, x, T, parent, 100.0, 0.5, N)
    e = R.energy(u, x, T, parent, 100.0, N, np.zeros((N, J), np.int64))
    beta = M.marg_bound(J, H, r["G"])                                # S + Dn and logZ are the same sum in two orders: w = 1 within beta
    assert np.abs(r["w"] - 1.0).max() <= beta and np.abs(r["cov"]).max() <= beta ** 2 * 100.0 and (r["bone"] == 0.0).all() and (r["hmax"] == 0).all()
    assert np.abs(r["logz"] - (-e / 0.5)[:, None]).max() < 1e-12 * np.abs(e / 0.5).max()
    assert np.abs(r["mean"] - M.camera_frame(x, T, N)[0]).max() <= beta * 10.0


def test_the_marginals_of_a_spanning_tree_do_not_depend_on_the_root():
    import zedo_hip
    J, N, H = 17, 6, 50
    x, T, u = case(J, N, H)
    a = joint_tree_marginal_ref(u, x, T, zedo_hip.skeleton_parents(R.H36M_EDGES, 17, root=0), 100.0, 1.0, N)
    b = joint_tree_marginal_ref(u, x, T, zedo_hip.skeleton_parents(R.H36M_EDGES, 17, root=5), 100.0, 1.0, N)
    beta = M.marg_bound(J, H, max(a["G"], b["G"]))
    d = float(np.abs(a["lw"] - b["lw"]).max())
    print(f"root 0 against root 5 at J={J} N={N} H={H}: max |log w - log w'| = {d:.3e} (bound {beta:.3e})")
    assert d <= beta and np.abs(a["logz"] - b["logz"]).max() <= beta and np.abs(a["w"] - b["w"]).max() < 1e-12


def test_the_order_of_the_sums_is_free_within_the_bound():
    """The ascending and the descending evaluation of every sum over the hypotheses at (17, 70, 50): the size of the round-off the GPU
    bound is set beside."""
    J, N, H = 17, 70, 50
    x, T, u = case(J, N, H)
    up = M.reference(J, N, H, 100.0, 1.0)
    down = joint_tree_marginal_ref(u, x, T, M.default_tree(J), 100.0, 1.0, N, descending=True)
    d = float(np.abs(up["lw"] - down["lw"]).max())
    beta = M.marg_bound(J, H, up["G"])
    print(f"ascending against descending sums at J={J} N={N} H={H}: max |log w - log w'| = {d:.3e}, |logz - logz'| = "
          f"{np.abs(up['logz'] - down['logz']).max():.3e} (bound {beta:.3e}); |bone - bone'| = {np.abs(up['bone'] - down['bone']).max():.3e} m; "
          f"the largest marginal has median {np.median(up['wmax']):.2f}")
    assert 0.0 < d <= beta and np.abs(up["mean"] - down["mean"]).max() <= 1e-12


def test_the_arg_max_is_clear_of_the_bound_on_every_gpu_case():
    """On the reference alone: at most 1 % of the (pose, joint) of a case the GPU test runs have a runner-up within 2 beta of the
    largest log-marginal (those are left out of the arg-max comparison there); the share is printed."""
    worst = 0.0
    for J, N, H in M.CASES:
        for mu, tau in M.WEIGHTS:
            r = M.reference(J, N, H, mu, tau)
            out = 1.0 - M.clear_argmax(r, M.marg_bound(J, H, r["G"])).sum() / max(r["live"].sum(), 1)
            worst = max(worst, out)
            assert out <= 0.01, (J, N, H, mu, tau, out)
    print(f"largest share of (pose, joint) left out of the arg-max comparison: {worst:.4f}")


def test_driver_accepts_joints_tree_fused_with_its_switches():
    """Argument checks that need no GPU: joints-tree-fused is a --select choice that takes --bone (default 100, finite >= 0) and
    --temperature (default 1, finite > 0) and refuses the switches of the video choices in the words joints-tree gets; the other choices
    keep their words."""
    from run._driver import build_parser, check_select_args
    p = build_parser("t", inference=True)
    base = ["--config", "c.py", "--select", "joints-tree-fused"]
    a = p.parse_args(base)
    check_select_args(a)
    assert a.select == "joints-tree-fused" and a.bone == 100.0 and a.temperature == 1.0 and a.smooth is None and a.seq_len is None and a.accel is None
    a = p.parse_args(base + ["--bone", "0", "--temperature", "1e-9"])
    check_select_args(a)
    assert a.bone == 0.0 and a.temperature == 1e-9
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(base + ["--bone", bad]))
        assert "a finite weight >= 0 expected" in str(e.value)
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(base + ["--temperature", bad]))
        assert "a finite temperature > 0 expected" in str(e.value)
    for switch, words in ((["--smooth", "10"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal"),
                          (["--seq_len", "5"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal"),
                          (["--accel", "10"], "--accel is a switch of --select joints-temporal")):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(base + switch))
        assert words in str(e.value)
    with pytest.raises(SystemExit) as e:
        check_select_args(p.parse_args(["--config", "c.py", "--select", "joints-tree", "--temperature", "2"]))
    assert str(e.value) == "--temperature is a switch of --select joints-fused"
    with pytest.raises(SystemExit) as e:
        check_select_args(p.parse_args(["--config", "c.py", "--select", "joints-fused", "--bone", "3"]))
    assert str(e.value) == "--bone is a switch of --select joints-tree"
