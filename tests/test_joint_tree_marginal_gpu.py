"""GPU: zedo_joint_tree_marginal - per pose the exact posterior marginals of every joint's hypotheses under the energy
zedo_joint_tree_select minimises, at a temperature tau (sum-product over the bone tree in the log domain, fp64, one workgroup per pose
with everything in the LDS: csrc/zedo_joint_tree_marginal.hip), the posterior mean, its covariance, the most probable hypothesis, the
log-partition value of every component and every bone's expected mismatch.  Held to the float64 reference of
tests/_joint_tree_marginal_ref.py (pinned on its own in tests/test_joint_tree_marginal_ref.py): the log-marginals, logz and |sum_h w - 1|
within marg_bound = 4 J (H + 8 + 28 G) 2^-53, the mean, the covariance and the bone within the bounds that follow from it (derived in the
reference file); asserted, and the difference each case shows is printed beside its bound (the recorded run is
profiles/joint_tree_marginal_accuracy.txt).  The case table crosses every split of the kernel and reaches its LDS cap.  With and without
T, with confidences, a reversed chain and forests; the limits tie it to shipped code: tau -> 0 is zedo_joint_tree_select's assignment and
bone, mu = 0 is a softmax whose arg-max is zedo_joint_reproj's; the dead joint; bit identity across runs, d_w NULL or dirty, a side
stream and stream capture; the refusals of the raw ABI.
Whether the fused pose is closer to ground truth than a selected one is not measured here or anywhere: these tests hold the arithmetic.
The fusion does not depend on the arithmetic mode of the dense layers: one session runs it."""
import ctypes

import numpy as np
import pytest

from _invariance import all_same, cur_stream, launch_invariant, ptr as P, refusal_sweep, same, sentinels
from _joint_marginal_ref import hold_marginals
import _joint_tree_marginal_ref as M
import _joint_tree_ref as R
from _joint_ref import case as reproj_case
from _joint_tree_marginal_ref import case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MU, TAU = 100.0, 1.0
SHAPES = (((3,), torch.float64), ((6,), torch.float64), ((), torch.int32), ((), torch.float64), ((), torch.float64), ((), torch.float64))
OUT_SPECS = lambda N, J, H: [((N, J) + tail, dt) for tail, dt in SHAPES + (((H,), torch.float64),)]


def run(zh, x, T, u, parent, N, mu=MU, tau=TAU, weight=None):
    out = zh.joint_tree_marginal(dev(u, torch.float64), dev(x), None if T is None else dev(T), parent, N, mu, tau,
                                 None if weight is None else dev(weight), return_weights=True)
    return [t.cpu().numpy() for t in out]


def hold_to(out, r, x, T, N, tag):
    """Every output against the reference r within the derived bounds; prints observed against bound."""
    mean, cov, hmax, wmax, logz, bone, w = out
    dead = ~r["live"]
    beta = M.marg_bound(w.shape[1], w.shape[2], r["G"])
    s = hold_marginals((mean, cov, hmax, wmax, logz, w), log_w_ref=r["lw"], logz_ref=r["logz"], mean_ref=r["mean"], cov_ref=r["cov"],
                       hmax_ref=r["hmax"], w_ref=r["w"], dead=dead, beta=beta, x=x, T=T, N=N, left_out_cap=0.01)
    # what only the tree has: the covariance of a dead joint, the bone output, and excluded entries that are exactly 0
    assert np.array_equal(np.isnan(cov).any(2), dead) and (bone[dead] == 0.0).all() and (w[np.isneginf(r["lw"])] == 0.0).all()
    bb = M.bone_bound(beta, r["bmax"], r["lmax"])
    e_bone = float(np.abs(bone - r["bone"]).max())
    print(f"joint-tree-marginal {tag}: G = {r['G']:.3g}; max |log w - ref| = {s['e_lw']:.3e}, |sum w - 1| = {s['e_sum']:.3e}, |logz - ref| = "
          f"{s['e_lz']:.3e} (bound {beta:.3e}); |mean - ref| = {s['e_mean']:.3e} m (bound {s['mean_bound']:.3e}); |cov - ref| = {s['e_cov']:.3e} m^2 "
          f"(smallest bound {s['cov_bound']:.3e}); |bone - ref| = {e_bone:.3e} m (bound {bb:.3e}); hmax differs on {s['hmax_differs']} of "
          f"{hmax.size}, {s['not_clear']} left out")
    assert e_bone <= bb


@pytest.mark.parametrize("J,N,H", M.CASES, ids=M.IDS)
def test_marginals_mean_covariance_and_bone_match_the_float64_reference(zh, J, N, H):
    assert H <= zh.joint_tree_marginal_max_h(J)
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    parent = M.default_tree(J)
    for mu, tau in M.WEIGHTS:
        out = zh.joint_tree_marginal(ud, xd, Td, parent, N, mu, tau, return_weights=True)
        for t, (tail, dt) in zip(out, SHAPES + (((H,), torch.float64),)):
            assert tuple(t.shape) == (N, J) + tail and t.dtype == dt
        hold_to([t.cpu().numpy() for t in out], M.reference(J, N, H, mu, tau), x, T, N, f"J={J} N={N} H={H} mu={mu:g} tau={tau:g}")


@pytest.mark.parametrize("J,N,H", [(5, 12, 3), (17, 6, 50), (17, 2, 129), (2, 2, 257)], ids=lambda v: str(v))
@pytest.mark.parametrize("variant", ["no_T", "weight", "chain", "forest", "forest5"])
def test_without_T_with_confidences_and_on_other_trees(zh, J, N, H, variant):
    x, T, u = case(J, N, H)
    with_T, with_w = variant != "no_T", variant == "weight"
    tree = variant if variant in ("chain", "forest", "forest5") else "default"
    for mu, tau in ((100.0, 1.0), (300.0, 0.05)):
        r = M.reference(J, N, H, mu, tau, tree, with_T, with_w)
        out = run(zh, x, T if with_T else None, u, M.TREES[tree](J), N, mu, tau, M.confidences(N, J) if with_w else None)
        hold_to(out, r, x, T if with_T else None, N, f"J={J} N={N} H={H} {variant} mu={mu:g} tau={tau:g}")


def test_the_limits_of_max_h(zh):
    assert [zh.joint_tree_marginal_max_h(J) for J in (1, 2, 3, 17, 64)] == [M.MAX_H[J] for J in (1, 2, 3, 17, 64)]
    assert zh.joint_tree_marginal_max_h(0) == 0 and zh.joint_tree_marginal_max_h(65) == 0 and zh.joint_tree_marginal_max_h(-3) == 0
    for J in range(1, 65):
        h = zh.joint_tree_marginal_max_h(J)
        assert h == min(1024, (163840 - 8192) // (48 * J + 16))
    assert zh.joint_tree_marginal_max_h(17) >= 128 and zh.joint_tree_marginal_max_h(64) >= 32


@pytest.mark.parametrize("J,N,H", [(5, 12, 3), (17, 6, 50), (3, 4, 65), (17, 2, 129), (2, 2, 257)], ids=lambda v: str(v))
def test_a_cold_tree_is_the_min_sum_assignment(zh, J, N, H):
    """tau = 1e-9: any other assignment costs at least the 6.5e-7 gap of _joint_tree_ref.check_inputs more, >= 650 tau - hmax is
    zedo_joint_tree_select's joint_h exactly.  G is about 1e11 there, so marg_bound is wide (a weight is good to about 1e-2 only in the
    worst case): wmax = 1 is held to it as everywhere else and must stay above 0.99 - no term of any log-sum-exp has underflowed -,
    but the mean and the bone are held to what the weights THEMSELVES allow (concentrated_mean_bound, concentrated_bone_bound: the
    mass that is not on the kept assignment times the hypotheses' spread, and fp64 rounding), which is micrometres: the mean is the
    kept hypothesis' position and bone is zedo_joint_tree_select's bone."""
    x, T, u = case(J, N, H)
    parent = M.default_tree(J)
    X = M.camera_frame(x, T, N)
    for mu in R.MUS:
        mean, cov, hmax, wmax, logz, bone, w = run(zh, x, T, u, parent, N, mu, 1e-9)
        joint_h, _, tbone = (t.cpu().numpy() for t in zh.joint_tree_select(dev(u, torch.float64), dev(x), dev(T), parent, N, mu))
        assert R.reference(J, N, H, mu)["gap"] >= 6.5e-7
        r = M.reference(J, N, H, mu, 1e-9)
        beta = M.marg_bound(J, H, r["G"])
        assert np.array_equal(hmax, joint_h)
        Xsel = np.take_along_axis(X.transpose(1, 2, 0, 3), joint_h[:, :, None, None].astype(np.int64), 2)[:, :, 0]
        mb = M.concentrated_mean_bound(w, joint_h, X)
        bb = M.concentrated_bone_bound(w, joint_h, parent, tbone, beta, r["G"], r["bmax"], r["lmax"])
        e_mean, e_bone = np.abs(mean - Xsel).max(2), np.abs(bone - tbone)
        print(f"tau = 1e-9, J={J} N={N} H={H} mu={mu:g}: G = {r['G']:.3g}, smallest largest marginal {wmax.min():.9f} (|wmax - 1| bound "
              f"{np.expm1(beta):.3e}), max |mean - X[kept]| = {e_mean.max():.3e} m (largest bound {mb.max():.3e}), max |bone - min-sum bone| = "
              f"{e_bone.max():.3e} m (largest bound {bb.max():.3e})")
        assert np.isfinite(mean).all() and np.isfinite(logz).all()
        assert np.abs(wmax - 1.0).max() <= np.expm1(beta) and wmax.min() > 0.99
        assert (e_mean <= mb).all() and (e_bone <= bb).all()


@pytest.mark.parametrize("J,N,H", [(5, 12, 3), (17, 6, 50), (21, 3, 130)], ids=lambda v: str(v))
def test_without_the_bone_term_the_arg_max_is_joint_reproj(zh, J, N, H):
    """mu = 0 and no weights, fed zedo_joint_reproj's own distances: the marginals are the per-joint softmax of -u / tau, and hmax is
    d_best_h wherever the two smallest distances of a (pose, joint) are further apart than 2 beta tau."""
    x, T, uv, K, _ = reproj_case(J, N, H)
    xd, Td = dev(x), dev(T)
    _, idx, jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)
    parent = M.default_tree(J)
    out = zh.joint_tree_marginal(jerr, xd, Td, parent, N, 0.0, TAU, return_weights=True)
    u = jerr.cpu().numpy()
    r = M.joint_tree_marginal_ref(u, x, T, parent, 0.0, TAU, N)
    hold_to([t.cpu().numpy() for t in out], r, x, T, N, f"unaries of zedo_joint_reproj J={J} N={N} H={H} mu=0")
    clear = M.clear_argmax(r, M.marg_bound(J, H, r["G"]))
    assert clear.sum() >= 0.99 * clear.size
    assert np.array_equal(out[2].cpu().numpy()[clear], idx.cpu().numpy()[clear])
    un = R.unaries(u, N)
    e = np.exp(-(un - un.min(axis=2, keepdims=True)) / TAU)
    assert np.abs(out[6].cpu().numpy() - e / e.sum(axis=2, keepdims=True)).max() < 1e-12


def test_a_dead_joint(zh):
    """The hand-built case of _joint_tree_ref: joint 1 of pose 4 has no finite unary - NaN, hypothesis 0, weight 0, logz -inf, bone 0,
    its children roots (three values of logz in that pose); the other poses return the bits of the run on the untouched unaries; excluded
    entries are exactly 0; a NaN weight kills its joint."""
    x, T, u, parent, j = M.dead_joint_case()
    N, H, J = 9, 3, 5
    clean = case(J, N, H)[2]
    for mu, tau in ((100.0, 1.0), (30.0, 0.05)):
        r = M.joint_tree_marginal_ref(u, x, T, parent, mu, tau, N)
        out = run(zh, x, T, u, parent, N, mu, tau)
        hold_to(out, r, x, T, N, f"dead joint mu={mu:g} tau={tau:g}")
        mean, cov, hmax, wmax, logz, bone, w = out
        assert np.isnan(mean[4, j]).all() and hmax[4, j] == 0 and np.isneginf(logz[4, j]) and (bone[4, [j, 3, 4]] == 0).all()
        assert len({logz[4, 0], logz[4, 3], logz[4, 4]}) == 3 and logz[4, 2] == logz[4, 0]
        excluded = ~np.isfinite(R.unaries(u, N))
        assert (w[excluded] == 0.0).all() and (w[~excluded] > 0.0).all()
        o0 = run(zh, x, T, clean, parent, N, mu, tau)
        keep = [0, 1, 3, 5, 7, 8]
        assert all(a[keep].tobytes() == b[keep].tobytes() for a, b in zip(out, o0))
    u2 = u.copy().reshape(H, N, J)
    u2[:, 7, :] = np.nan                                              # a pose without a live joint
    out = run(zh, x, T, u2.reshape(H * N, J), parent, N)
    hold_to(out, M.joint_tree_marginal_ref(u2.reshape(H * N, J), x, T, parent, MU, TAU, N), x, T, N, "a dead pose")
    assert np.isnan(out[0][7]).all() and np.isneginf(out[4][7]).all()
    wgt = np.ones((N, J), np.float32)
    wgt[3, 2] = np.nan
    out = run(zh, x, T, clean, parent, N, weight=wgt)
    hold_to(out, M.joint_tree_marginal_ref(clean, x, T, parent, MU, TAU, N, wgt), x, T, N, "NaN weight")
    assert np.isnan(out[0][3, 2]).all() and out[2][3, 2] == 0


@pytest.mark.parametrize("J,N,H", [(17, 6, 50), (3, 4, 65), (17, 2, 129), (2, 2, 257)], ids=lambda v: str(v))
def test_the_bits_do_not_depend_on_the_run_d_w_the_stream_or_the_alignment(zh, J, N, H):
    """Two runs; d_w NULL, and d_w pre-filled at the raw ABI; a side stream; one call captured into a graph and replayed twice; d_x at a
    12-byte offset."""
    x, T, u = case(J, N, H)
    xd, Td, ud, wd = dev(x), dev(T), dev(u, torch.float64), dev(M.confidences(N, J))
    parent = M.default_tree(J)
    ref = zh.joint_tree_marginal(ud, xd, Td, parent, N, MU, TAU, wd, return_weights=True)
    assert all_same(zh.joint_tree_marginal(ud, xd, Td, parent, N, MU, TAU, wd, return_weights=True), ref)
    assert all_same(zh.joint_tree_marginal(ud, xd, Td, parent, N, MU, TAU, wd), ref[:6])           # d_w NULL (through the binding)
    par = np.ascontiguousarray(np.asarray(parent, np.int32))
    for with_w in (True, False):                                     # d_w pre-filled at the raw ABI, and NULL
        o = sentinels(OUT_SPECS(N, J, H))
        assert zh._lib.zedo_joint_tree_marginal(P(ud), P(xd), P(Td), P(wd), par.ctypes.data_as(ctypes.c_void_p), H, N, J, MU, TAU, P(o[0]), P(o[1]),
                                                P(o[2]), P(o[3]), P(o[4]), P(o[5]), P(o[6]) if with_w else None, cur_stream()) == 0
        torch.cuda.synchronize()
        assert all_same(o[:6], ref[:6]) and (same(o[6], ref[6]) if with_w else bool((o[6] == -7).all()))
    launch_invariant(ref, lambda x=xd, seq_on_device=False: zh.joint_tree_marginal(ud, x, Td, parent, N, MU, TAU, wd, return_weights=True), xd)


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer other than d_T / d_weight / d_w, a non-positive size, H = max_h(J) + 1 for J in (1, 17, 64), J = 65, H N J above
    INT_MAX, a parent array that is no forest, tau of 0, negative, NaN and inf, a negative / NaN / infinite mu: ZEDO_E_BADARG and the
    pattern-filled outputs untouched.  The same call with valid arguments is accepted, with and without d_T, d_weight and d_w."""
    lib = zh._lib
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud, wd = dev(x), dev(T), dev(u, torch.float64), dev(M.confidences(N, J))
    par = lambda v: np.ascontiguousarray(np.asarray(v, np.int32))
    good = par(R.heap_tree(J))
    outs = sentinels(OUT_SPECS(N, J, H))
    ptrs = [P(ud), P(xd), P(Td), P(wd)] + [P(t) for t in outs]

    def call(p=ptrs, parent=good, h=H, n=N, j=J, mu=MU, tau=TAU):
        pp = None if parent is None else parent.ctypes.data_as(ctypes.c_void_p)
        return lib.zedo_joint_tree_marginal(p[0], p[1], p[2], p[3], pp, h, n, j, mu, tau, p[4], p[5], p[6], p[7], p[8], p[9], p[10], None)

    big = par([-1] + list(range(64)))
    sizes = [dict(parent=None), dict(h=0), dict(n=0), dict(j=0), dict(h=-1), dict(n=-3), dict(j=-1)]
    sizes += [dict(parent=big, h=zh.joint_tree_marginal_max_h(jj) + 1, n=1, j=jj) for jj in (1, 17, 64)]     # sizes above the caps (the pointers are never followed)
    sizes += [dict(parent=big, h=2, n=1, j=65), dict(parent=big, h=2 ** 10, n=2 ** 20, j=2)]                # ... and H N J above INT_MAX
    # a parent array that is no forest: self, out of range (twice), two cycles beside a root, no root
    sizes += [dict(parent=par(bad)) for bad in ([0, 0, 0, 1, 1], [-1, 0, 0, 1, 5], [-1, 0, 0, 1, -2], [1, 0, -1, 2, 2], [-1, 0, 0, 4, 3], [1, 2, 3, 4, 0])]
    sizes += [dict(mu=1e300, tau=1e-300)]                            # mu / tau is not finite
    refusal_sweep(call, ptrs, (0, 1, 4, 5, 6, 7, 8, 9), sizes=sizes, weights=("mu",), taus=("tau",), untouched=[(t, -7) for t in outs])
    r = M.joint_tree_marginal_ref(u, x, T, list(good), MU, TAU, N, M.confidences(N, J))
    assert np.array_equal(outs[2].cpu().numpy(), r["hmax"]) and np.abs(outs[6].cpu().numpy() - r["w"]).max() < 1e-9
    for t in outs:
        t.fill_(-7)
    assert call([None if i in (2, 3, 10) else p for i, p in enumerate(ptrs)]) == 0       # d_T, d_weight and d_w may be NULL
    torch.cuda.synchronize()
    assert np.abs(outs[0].cpu().numpy() - M.joint_tree_marginal_ref(u, x, None, list(good), MU, TAU, N)["mean"]).max() < 1e-9
    assert bool((outs[6] == -7).all())
    with pytest.raises(ValueError):
        zh.joint_tree_marginal(ud[:-1], xd, Td, list(good), N)
    with pytest.raises(ValueError):
        zh.joint_tree_marginal(ud, xd, Td[:-1], list(good), N)
    with pytest.raises(ValueError):
        zh.joint_tree_marginal(ud, xd, Td, list(good)[:-1], N)
    with pytest.raises(ValueError):
        zh.joint_tree_marginal(ud, xd, Td, list(good), N, weight=wd[:-1])
    with pytest.raises(zh.ZedoError):
        zh.joint_tree_marginal(ud, xd, Td, [0, 0, 0, 1, 1], N)
    with pytest.raises(zh.ZedoError):
        zh.joint_tree_marginal(ud, xd, Td, list(good), N, tau=0.0)


def test_pipeline_fuse_tree(zh, weights0):
    """Pipeline.fuse_tree on the problem of load() is joint_reproj's per-(row, joint) distances fed to joint_tree_marginal with the
    pipeline's confidences and the H36M tree."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)[2]
    for mu, tau in ((100.0, 1.0), (30.0, 0.5)):
        want = zh.joint_tree_marginal(jerr, xd, Td, R.H36M_PARENTS, N, mu, tau, pipe.conf)
        got = pipe.fuse_tree(xd, Td, mu=mu, tau=tau)
        assert len(got) == 7 and all_same(got[:6], want) and same(got[6], jerr)
    got = pipe.fuse_tree(xd, Td, mu=30.0, parent=R.reversed_chain(17))
    assert all_same(got[:6], zh.joint_tree_marginal(jerr, xd, Td, R.reversed_chain(17), N, 30.0, 1.0, pipe.conf))
    with pytest.raises(ValueError):
        pipe.fuse_tree(xd[:N], Td[:N])
