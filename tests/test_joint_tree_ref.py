"""CPU: the numpy reference of the skeleton-coupled joint-wise aggregation (tests/_joint_tree_ref.py) pinned on its own - against the
enumeration of every assignment, the two limits of the bone weight, the rules for excluded entries and a dead joint, the condition on
the shared inputs that makes an exact comparison of assignments honest, the property the model is built for - the assembled bones agree
with the hypotheses that supply them - and the argument checks of the driver and of skeleton_parents.  Whether the coupled pose is closer
to ground truth is not measured here or anywhere: these tests hold the arithmetic."""
import numpy as np
import pytest

import _joint_tree_ref as R
from _joint_tree_ref import case, per_frame_argmin


@pytest.mark.parametrize("J,H,tree", [(5, 4, "heap"), (6, 3, "chain"), (4, 5, "forest")], ids=lambda v: str(v))
def test_the_dynamic_programme_finds_the_best_of_all_assignments(J, H, tree):
    """Every pose against the enumeration of its H^J assignments: the same assignment, and the cost is the assignment's energy up to the
    rounding of another order of the same additions."""
    N = 3
    x, T, u = case(J, N, H)
    parent = {"heap": R.heap_tree, "chain": R.reversed_chain, "forest": R.two_roots}[tree](J)
    for mu in R.MUS:
        r = R.joint_tree_ref(u, x, T, parent, mu, N)
        assert r["gap"] > R.GAP_MIN
        a, e = R.enumerate_best(u, x, T, parent, mu, N)
        assert np.array_equal(r["joint_h"], a), mu
        assert np.all(np.abs(r["cost"] - e) <= R.cost_bound(J, r["scale"]))
        assert np.all(np.abs(R.energy(u, x, T, parent, mu, N, r["joint_h"]) - e) <= R.cost_bound(J, r["scale"]))


@pytest.mark.parametrize("J,N,H", [(5, 12, 3), (17, 70, 50), (21, 20, 65)], ids=lambda v: str(v))
def test_without_the_bone_term_every_joint_is_on_its_own(J, N, H):
    x, T, u = case(J, N, H)
    r = R.reference(J, N, H, 0.0)
    assert np.array_equal(r["joint_h"], per_frame_argmin(u, N))
    assert np.all(r["bone"][:, [j for j, p in enumerate(R.default_tree(J)) if p < 0]] == 0.0)


@pytest.mark.parametrize("J,N,H", [(5, 12, 3), (17, 70, 50), (21, 20, 65), (64, 6, 5)], ids=lambda v: str(v))
def test_a_large_bone_weight_keeps_one_whole_hypothesis(J, N, H):
    x, T, u = case(J, N, H)
    r = R.reference(J, N, H, 1e9)
    whole = np.argmin(R.unaries(u, N).sum(1), axis=1)
    assert np.array_equal(r["joint_h"], np.repeat(whole[:, None], J, axis=1))
    assert np.all(r["bone"] == 0.0)


def test_a_dead_joint_cuts_the_tree_there_and_nowhere_else():
    """Joint 1 of pose 4 has no finite unary: it reports hypothesis 0 and bone 0, its children 3 and 4 become roots, and the pose's other
    joints are the run on the tree with that joint removed; a NaN or +inf entry elsewhere excludes that hypothesis for that joint only."""
    x, T, u, parent, j = R.dead_joint_case()
    N, H, J = 9, 3, 5
    for mu in R.MUS:
        r = R.joint_tree_ref(u, x, T, parent, mu, N)
        assert not r["live"][4, j] and r["live"].sum() == N * J - 1
        assert r["joint_h"][4, j] == 0 and r["bone"][4, j] == 0.0
        assert np.all(r["bone"][4, [3, 4]] == 0.0)                 # roots now
        # the tree with joint 1 removed: joints 0, 2, 3, 4 -> 0, 1, 2, 3; 2 hangs under 0, the former children of 1 are roots
        keep = [0, 2, 3, 4]
        r2 = R.joint_tree_ref(np.ascontiguousarray(u[:, keep]), np.ascontiguousarray(x[:, keep]), T, [-1, 0, -1, -1], mu, N)
        assert np.array_equal(r["joint_h"][4, keep], r2["joint_h"][4])
        assert np.array_equal(r["bone"][4, keep], r2["bone"][4])
        assert r["cost"][4] == r2["cost"][4]
        # an excluded entry is never chosen, and the poses it sits in stay whole trees
        u3 = u.reshape(H, N, J)
        for n in (2, 6):
            assert np.isfinite(u3[r["joint_h"][n, j], n, j]) and r["live"][n].all()
        # the untouched poses equal the run on the untouched unaries
        r0 = R.joint_tree_ref(case(J, N, H)[2], x, T, parent, mu, N)
        for n in (0, 1, 3, 5, 7, 8):
            assert np.array_equal(r["joint_h"][n], r0["joint_h"][n]) and r["cost"][n] == r0["cost"][n]
    allnan = np.full_like(u, np.nan)
    r = R.joint_tree_ref(allnan, x, T, parent, 100.0, N)
    assert np.all(r["cost"] == np.inf) and np.all(r["joint_h"] == 0) and np.all(r["bone"] == 0.0)


def test_the_shared_inputs_allow_an_exact_comparison():
    assert R.check_inputs(verbose=True) > R.GAP_MIN


def test_the_bone_term_makes_the_assembled_bones_agree_with_their_hypotheses():
    """(17, 70, 50) on the H36M tree: at mu = 100 the mean bone mismatch is below a tenth of the per-joint arg-min's, and the pose is still
    assembled from more than one hypothesis."""
    J, N, H = 17, 70, 50
    x, T, u = case(J, N, H)
    r0, r100 = R.reference(J, N, H, 0.0), R.reference(J, N, H, 100.0)
    m0, m100 = (R.mismatch(x, T, R.H36M_PARENTS, N, r["joint_h"]) for r in (r0, r100))
    used = lambda r: float(np.mean([len(set(row)) for row in r["joint_h"]]))
    print(f"mean bone mismatch: {1e3 * m0:.1f} mm at mu = 0 ({used(r0):.1f} hypotheses per pose), {1e3 * m100:.1f} mm at mu = 100 "
          f"({used(r100):.1f} hypotheses per pose)")
    assert m100 < 0.1 * m0
    assert used(r100) > 1.0
    assert np.isclose(m100, r100["bone"][:, [j for j, p in enumerate(R.H36M_PARENTS) if p >= 0]].mean(), rtol=1e-12)


def test_driver_accepts_bone_with_joints_tree_only():
    """Argument checks that need no GPU: joints-tree is a --select choice, --bone is its switch, defaults to 100 there and refuses a
    negative or non-finite value; every other --select refuses --bone; joints-tree refuses the switches of the video choices in the words
    those switches already use."""
    from run._driver import build_parser, check_select_args
    p = build_parser("t", inference=True)
    base = ["--config", "c.py", "--select", "joints-tree"]
    a = p.parse_args(base)
    check_select_args(a)
    assert a.bone == 100.0 and a.smooth is None and a.seq_len is None and a.temperature is None and a.accel is None
    a = p.parse_args(base + ["--bone", "0"])
    check_select_args(a)
    assert a.bone == 0.0
    a = p.parse_args(base + ["--bone", "1e9"])
    check_select_args(a)
    assert a.bone == 1e9
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(base + ["--bone", bad]))
        assert "--bone" in str(e.value) and "a finite weight >= 0 expected" in str(e.value)
    for sel in ("none", "reproj", "joints", "temporal", "joints-temporal", "joints-fused"):
        a = p.parse_args(["--config", "c.py", "--select", sel])
        check_select_args(a)
        assert a.bone is None
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(["--config", "c.py", "--select", sel, "--bone", "100"]))
        assert "--bone is a switch of --select joints-tree" in str(e.value)
    for switch, words in ((["--smooth", "10"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal"),
                          (["--seq_len", "5"], "--smooth and --seq_len are switches of --select temporal and --select joints-temporal"),
                          (["--temperature", "2"], "--temperature is a switch of --select joints-fused"),
                          (["--accel", "10"], "--accel is a switch of --select joints-temporal")):
        with pytest.raises(SystemExit) as e:
            check_select_args(p.parse_args(base + switch))
        assert words in str(e.value)
    with pytest.raises(SystemExit) as e:                                # run.opt_main has the switch in its parser and refuses it too
        check_select_args(build_parser("t").parse_args(["--config", "c.py", "--bone", "100"]))
    assert "--bone" in str(e.value)


def test_skeleton_parents():
    import zedo_hip
    assert zedo_hip.skeleton_parents(R.H36M_EDGES, 17) == R.H36M_PARENTS
    assert list(zedo_hip.H36M_EDGES) == [tuple(e) for e in R.H36M_EDGES]
    assert zedo_hip.skeleton_parents([(1, 0), (2, 1)], 3, root=2) == [1, 2, -1]
    assert zedo_hip.skeleton_parents([], 1) == [-1]
    cyc = [e for e in R.H36M_EDGES if e != [15, 16]] + [[14, 8]]        # a doubled bone: 16 bones, joint 16 left out
    with pytest.raises(ValueError):
        zedo_hip.skeleton_parents(cyc, 17)
    with pytest.raises(ValueError):
        zedo_hip.skeleton_parents([[0, 1], [1, 2], [2, 0], [3, 4]], 5)   # a cycle and a disconnected part
    with pytest.raises(ValueError):
        zedo_hip.skeleton_parents(R.H36M_EDGES[:-1], 17)                 # disconnected: a bone short
    with pytest.raises(ValueError):
        zedo_hip.skeleton_parents([[0, 0]], 2)
    with pytest.raises(ValueError):
        zedo_hip.skeleton_parents([[0, 5]], 2)


def test_post_order_puts_children_first_and_siblings_ascending():
    assert R.post_order(R.H36M_PARENTS) == [3, 2, 1, 6, 5, 4, 10, 9, 13, 12, 11, 16, 15, 14, 8, 7, 0]
    assert R.post_order(R.reversed_chain(4)) == [0, 1, 2, 3]
    assert R.post_order(R.two_roots(5)) == [4, 2, 0, 3, 1]
