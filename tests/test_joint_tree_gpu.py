"""GPU: zedo_joint_tree_select - per pose the assignment of a hypothesis to every joint that minimises the joints' unaries plus mu times,
over the bones, the mismatch between the assembled bone's length and the length its two hypotheses give that bone: exact min-sum over
the bone tree in fp64, one workgroup per pose with everything in the LDS (csrc/zedo_joint_tree.hip).  Held to the float64 reference of
tests/_joint_tree_ref.py (pinned on its own in tests/test_joint_tree_ref.py): the ASSIGNMENT exactly, cost and bone within
_joint_tree_ref.cost_bound = 23 J 2^-53 (sum u + mu sum (mix + own)) at mu = 30 / 100 / 300 (asserted; the difference each case shows is
printed; the recorded run is profiles/joint_tree_accuracy.txt); check_inputs() asserts on the reference alone that no minimum the
recurrence takes has a runner-up closer than 1e-8.  The case table crosses every split of the kernel and both sides of its LDS cap.
With and without T, with confidences on both sides of the clamp, a reversed chain and forests; mu = 0 against zedo_joint_reproj's bits;
the dead joint; a side stream, stream capture and replay, bit identity; the refusals of the raw ABI.
Whether the coupled pose is closer to ground truth than the per-joint arg-min is not measured here or anywhere: these tests hold the
arithmetic.  The selection does not depend on the arithmetic mode of the dense layers: one session runs it."""
import ctypes

import numpy as np
import pytest

from _invariance import all_same, launch_invariant, ptr as P, refusal_sweep, same, sentinels
import _joint_tree_ref as R
from _joint_ref import case as reproj_case
from _joint_tree_ref import case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def held(out, r, J, mu, what):
    """The assignment exactly; cost and mu * bone within cost_bound of the reference."""
    joint_h, cost, bone = (t.cpu().numpy() for t in out)
    bound = R.cost_bound(J, r["scale"])
    dc, db = np.abs(cost - r["cost"]), np.abs(bone - r["bone"])
    print(f"joint-tree {what} mu={mu:g}: max |cost - ref| = {dc.max():.3e}, mu max |bone - ref| = {mu * db.max():.3e} (smallest bound "
          f"{bound.min():.3e}); assignment differs on {int((joint_h != r['joint_h']).sum())} of {joint_h.size}; gap {r['gap']:.3e}")
    assert np.array_equal(joint_h, r["joint_h"]), (what, mu)
    assert (dc <= bound).all() and (mu * db <= bound[:, None]).all(), (what, mu)


def test_the_inputs_are_what_the_exact_comparison_assumes():
    R.check_inputs()


@pytest.mark.parametrize("J,N,H", R.ALL_CASES, ids=R.IDS)
def test_assignment_cost_and_bone_match_the_float64_reference(zh, J, N, H):
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    parent = R.default_tree(J)
    for mu in R.MUS:
        out = zh.joint_tree_select(ud, xd, Td, parent, N, mu)
        assert out[0].shape == (N, J) and out[0].dtype == torch.int32 and out[1].shape == (N,) and out[1].dtype == torch.float64
        assert out[2].shape == (N, J) and out[2].dtype == torch.float64
        held(out, R.reference(J, N, H, mu), J, mu, f"J={J} N={N} H={H}")
    joint_h = zh.joint_tree_select(ud, xd, Td, parent, N, 1e9)[0]          # one whole hypothesis per pose: the assignment only
    assert np.array_equal(joint_h.cpu().numpy(), R.reference(J, N, H, 1e9)["joint_h"])
    assert bool((joint_h == joint_h[:, :1]).all())


@pytest.mark.parametrize("J,N,H", [(5, 12, 3), (17, 70, 50), (21, 20, 65), (17, 4, 129), (2, 4, 257)], ids=lambda v: str(v))
@pytest.mark.parametrize("variant", ["no_T", "weight", "chain", "forest", "forest5"])
def test_without_T_with_confidences_and_on_other_trees(zh, J, N, H, variant):
    x, T, u = case(J, N, H)
    with_T, with_w = variant != "no_T", variant == "weight"
    tree = variant if variant in ("chain", "forest", "forest5") else "default"
    parent = {"default": R.default_tree, "chain": R.reversed_chain, "forest": R.two_roots, "forest5": R.five_roots}[tree](J)
    w = dev(R.confidences(N, J)) if with_w else None
    for mu in R.MUS:
        r = R.reference(J, N, H, mu, tree, with_T, with_w)
        assert r["gap"] > R.GAP_MIN
        out = zh.joint_tree_select(dev(u, torch.float64), dev(x), dev(T) if with_T else None, parent, N, mu, w)
        held(out, r, J, mu, f"J={J} N={N} H={H} {variant}")


@pytest.mark.parametrize("J,N,H", [(17, 70, 5), (17, 70, 50), (21, 6, 130), (5, 12, 3)], ids=lambda v: str(v))
def test_without_the_bone_term_the_call_is_joint_reproj(zh, J, N, H):
    """mu = 0 and no weights: joint_h is the bits of zedo_joint_reproj's best_h on the same rows, fed that call's own distances; and
    those distances drive the coupled call to the reference's assignment (the reference is fed the kernel's distances themselves)."""
    x, T, uv, K, _ = reproj_case(J, N, H)
    xd, Td = dev(x), dev(T)
    _, idx, jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)
    parent = R.default_tree(J)
    joint_h, cost, bone = zh.joint_tree_select(jerr, xd, Td, parent, N, 0.0)
    assert same(joint_h, idx)
    assert bool((bone[:, [j for j, p in enumerate(parent) if p < 0]] == 0).all())
    u = jerr.cpu().numpy()
    r = R.joint_tree_ref(u, x, T, parent, 100.0, N)
    assert r["gap"] > R.GAP_MIN
    held(zh.joint_tree_select(jerr, xd, Td, parent, N, 100.0), r, J, 100.0, f"unaries of zedo_joint_reproj J={J} N={N} H={H}")


def test_a_dead_joint(zh):
    """The hand-built case of tests/test_joint_tree_ref.py: joint 1 of pose 4 has no finite unary - hypothesis 0, bone 0, its children
    roots; the other poses return the bits of the run on the untouched unaries; a pose without a live joint costs +inf."""
    x, T, u, parent, j = R.dead_joint_case()
    N, H, J = 9, 3, 5
    clean = case(J, N, H)[2]
    for mu in R.MUS:
        r = R.joint_tree_ref(u, x, T, parent, mu, N)
        out = zh.joint_tree_select(dev(u, torch.float64), dev(x), dev(T), parent, N, mu)
        held(out, r, J, mu, "dead joint")
        assert out[0][4, j].item() == 0 and out[2][4, j].item() == 0.0 and bool((out[2][4, 3:] == 0).all())
        o0 = zh.joint_tree_select(dev(clean, torch.float64), dev(x), dev(T), parent, N, mu)
        keep = [0, 1, 3, 5, 7, 8]
        assert all(same(a[keep], b[keep]) for a, b in zip(out, o0))
    u2 = u.copy().reshape(H, N, J)
    u2[:, 7, :] = np.nan
    out = zh.joint_tree_select(dev(u2.reshape(H * N, J), torch.float64), dev(x), dev(T), parent, N, 100.0)
    assert np.isposinf(out[1][7].item()) and bool((out[0][7] == 0).all()) and bool((out[2][7] == 0).all())
    assert np.array_equal(out[0].cpu().numpy(), R.joint_tree_ref(u2.reshape(H * N, J), x, T, parent, 100.0, N)["joint_h"])
    # a weight that is NaN kills its joint, whatever the unaries
    w = np.ones((N, J), np.float32)
    w[3, 2] = np.nan
    out = zh.joint_tree_select(dev(clean, torch.float64), dev(x), dev(T), parent, N, 100.0, dev(w))
    held(out, R.joint_tree_ref(clean, x, T, parent, 100.0, N, w), J, 100.0, "NaN weight")
    assert out[0][3, 2].item() == 0


@pytest.mark.parametrize("J,N,H", [(17, 70, 50), (21, 20, 65), (17, 4, 129), (2, 4, 257)], ids=lambda v: str(v))
def test_the_bits_do_not_depend_on_the_run_the_stream_or_the_alignment(zh, J, N, H):
    """Two runs; a side stream; one call captured into a graph and replayed twice; d_x at a 12-byte offset."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    parent, mu = R.default_tree(J), 100.0
    ref = zh.joint_tree_select(ud, xd, Td, parent, N, mu)
    assert np.array_equal(ref[0].cpu().numpy(), R.reference(J, N, H, mu)["joint_h"])
    assert all_same(zh.joint_tree_select(ud, xd, Td, parent, N, mu), ref)                        # two runs
    launch_invariant(ref, lambda x=xd, seq_on_device=False: zh.joint_tree_select(ud, x, Td, parent, N, mu), xd)


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer other than d_T / d_weight, a non-positive size, a size above the caps, H N J above INT_MAX, a parent array that
    is no forest, a negative / NaN / infinite mu: ZEDO_E_BADARG and the sentinel-filled outputs untouched.  The same call with valid
    arguments is accepted, with and without d_T and d_weight."""
    lib = zh._lib
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud, wd = dev(x), dev(T), dev(u, torch.float64), dev(R.confidences(N, J))
    par = lambda v: np.ascontiguousarray(np.asarray(v, np.int32))
    good = par(R.heap_tree(J))
    joint_h, cost, bone = sentinels((((N, J), torch.int32), ((N,), torch.float64), ((N, J), torch.float64)))
    ptrs = [P(ud), P(xd), P(Td), P(wd), None, P(joint_h), P(cost), P(bone)]

    def call(p=ptrs, parent=good, h=H, n=N, j=J, mu=100.0):
        pp = None if parent is None else parent.ctypes.data_as(ctypes.c_void_p)
        return lib.zedo_joint_tree_select(p[0], p[1], p[2], p[3], pp, h, n, j, mu, p[5], p[6], p[7], None)

    big = par([-1] + list(range(64)))
    sizes = [dict(parent=None), dict(h=0), dict(n=0), dict(j=0), dict(h=-1), dict(n=-3), dict(j=-1)]
    sizes += [dict(parent=big, h=hh, n=1, j=jj) for jj, hh in R.TOO_LARGE]                # sizes above the caps (the pointers are never followed)
    sizes += [dict(parent=big, h=2 ** 10, n=2 ** 20, j=4)]                                 # H N J above INT_MAX
    # a parent array that is no forest: self, out of range (twice), two cycles beside a root, no root
    sizes += [dict(parent=par(bad)) for bad in ([0, 0, 0, 1, 1], [-1, 0, 0, 1, 5], [-1, 0, 0, 1, -2], [1, 0, -1, 2, 2], [-1, 0, 0, 4, 3], [1, 2, 3, 4, 0])]
    refusal_sweep(call, ptrs, (0, 1, 5, 6, 7), sizes=sizes, weights=("mu",), untouched=((joint_h, -7), (cost, -7.0), (bone, -7.0)))
    w = R.confidences(N, J)
    assert np.array_equal(joint_h.cpu().numpy(), R.joint_tree_ref(u, x, T, list(good), 100.0, N, w)["joint_h"])
    assert call([None if i in (2, 3) else p for i, p in enumerate(ptrs)]) == 0           # d_T and d_weight may be NULL
    torch.cuda.synchronize()
    assert np.array_equal(joint_h.cpu().numpy(), R.joint_tree_ref(u, x, None, list(good), 100.0, N)["joint_h"])
    with pytest.raises(ValueError):
        zh.joint_tree_select(ud[:-1], xd, Td, list(good), N)
    with pytest.raises(ValueError):
        zh.joint_tree_select(ud, xd, Td[:-1], list(good), N)
    with pytest.raises(ValueError):
        zh.joint_tree_select(ud, xd, Td, list(good)[:-1], N)
    with pytest.raises(ValueError):
        zh.joint_tree_select(ud, xd, Td, list(good), N, weight=wd[:-1])
    with pytest.raises(zh.ZedoError):
        zh.joint_tree_select(ud, xd, Td, [0, 0, 0, 1, 1], N)


def test_pipeline_aggregate_tree(zh, weights0):
    """Pipeline.aggregate_tree on the problem of load() is joint_reproj's per-(row, joint) distances fed to joint_tree_select with the
    pipeline's confidences and the H36M tree; compose() assembles the pose from the assignment."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)[2]
    for mu in (100.0, 0.0):
        want = zh.joint_tree_select(jerr, xd, Td, R.H36M_PARENTS, N, mu, pipe.conf)
        got = pipe.aggregate_tree(xd, Td, mu=mu)
        assert all_same(got[:3], want) and same(got[3], jerr)
    got = pipe.aggregate_tree(xd, Td, mu=30.0, parent=R.reversed_chain(17))
    assert all_same(got[:3], zh.joint_tree_select(jerr, xd, Td, R.reversed_chain(17), N, 30.0, pipe.conf))
    assert same(pipe.compose(xd, Td, want[0]), zh.joint_compose(xd, Td, want[0]))
    with pytest.raises(ValueError):
        pipe.aggregate_tree(xd[:N], Td[:N])
