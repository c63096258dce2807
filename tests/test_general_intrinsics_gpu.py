"""GPU tests of the geometry and IPO kernels on GENERAL camera matrices and on all eight subsets of rotation axes.

Every other test feeds a pure pinhole K (K01 = K10 = K20 = K21 = 0, K22 = 1) and RotAxes "z" or "xyz".  With such input the
products of ipo_joint_terms with K[1], K[3], K[6], K[7] vanish forward and backward, five of the nine cofactors of inv3x3 are exact
zeros, the homogeneous divide of reproj_prepare_kernel divides by 1, the third row of ipo_T0 is (0, 0, 1), and six of the eight axis
masks never reach the update predicates of the two IPO kernels: a wrong index, sign or transposition in any of these is invisible.
Here K has skew, a homogeneous row other than (0, 0, 1) and K22 != 1 (lib.dataset.synthetic.general_intrinsics; a user's
camera_param [N,3,3] reaches these kernels unchanged), the detections are re-projected through it, and every axis subset runs.  Adam's
bias corrections are also run across the end of the constant table (iteration 2048).  The arbiter is the numpy oracle in float64,
which tests/test_general_intrinsics_oracle.py pins to captures of the reference on such input; the bounds are the ones the suite
applies to pinhole input, except the bound on the two moment rows, which is computed from the fp32 oracle (see the test)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _reproj_ref as RR
from _shared import (IPO_MAX, IPO_MIN, IPO_T, KEYS, TWIN_AXES, MomentRule, dev, general_cameras, oracle_args, oracle_resume, oracle_run,
                     problem, report_env as _report, ulp32, zh)  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = ["", "x", "y", "z", "xy", "xz", "yz", "xyz"]
SLOT = {"x": 1, "y": 2, "z": 3}


# ---- a / b. single iterations from the float64 state: parameters, first moments, absent axes ---------------------------------

ITER_CASES = [(J, kl, N, axes, True) for J, kl in KEYS for N in (8, 64) for axes in AXES] + \
             [(17, [0, 1, 4], N, "z", False) for N in (8, 64)]
ITER_IDS = [f"J{J}-k{len(kl)}-N{N}-{axes or 'none'}-{'general' if gen else 'pinhole'}" for J, kl, N, axes, gen in ITER_CASES]


@pytest.mark.parametrize("J,kl,N,axes,general", ITER_CASES, ids=ITER_IDS)
def test_ipo_single_iterations_on_general_intrinsics(zh, J, kl, N, axes, general):
    """test_ipo_single_iterations_from_the_oracle_state on general K for all eight axis subsets (pinhole K with "z" as the control):
    each of the first 50 Adam iterations on its own through zedo_ipo_fit_resume from the oracle's float64 state.

    Parameters: |delta| <= 1e-6 on poses whose residuals are all >= 1e-3 px; at most 5 % of the pose-iterations may be left out.

    First moments (state[:, 5:10] = 0.9 m_old + 0.1 g: the gradient itself - Adam's first steps are +-lr whatever its size, so the
    parameters alone are blind to a scale error early on): |m - m64| on the same pose-iterations within
        2 x max |m32 - m64| + ulp32(max |m64|),
    m32 being the fp32 ORACLE's iteration from the same fp32 state - computed here, on the CPU, from the oracle alone.  The factor 2:
    the kernel sums the key joints in a pairing tree, the oracle in einsum order (the project's usual margin between two fp32
    evaluations of one formula).

    Second moments (state[:, 10:15] = 0.999 v_old + 0.001 g g): the same rule with v in the place of m (_shared.MomentRule).

    Axes absent from the mask: parameter and both moments bit for bit what went in, and the returned q an exact 0."""
    states, clear, m32 = oracle_run(J, tuple(kl), N, axes, general)
    cl, uvn, Kn = problem(J, N, 1, general)
    x0, uv, K = dev(cl), dev(uvn), dev(Kn)
    norm = N * len(kl) * 2
    absent = [SLOT[a] for a in "xyz" if a not in axes]
    present = [0] + [SLOT[a] for a in axes] + [4]
    worst, n_amb, rule_m, rule_v = 0.0, 0, MomentRule(), MomentRule()
    for it in range(50):
        s_in = states[it].astype(np.float32)
        st = dev(s_in)
        R, T, q, sc = zh.ipo_fit(x0, uv, K, kl, axes, IPO_T, IPO_MIN, IPO_MAX, 1, norm, N, state=st, it_begin=it, return_params=True)
        out32 = st.cpu().numpy()
        out = out32.astype(np.float64)
        for a in absent:
            cols = [a, 5 + a, 10 + a]
            assert np.array_equal(out32[:, cols].view(np.uint32), s_in[:, cols].view(np.uint32)), (it, a)
            assert (q.cpu().numpy()[:, a].view(np.uint32) == 0).all(), (it, a)
        assert np.array_equal(q.cpu().numpy(), out32[:, 0:4]) and np.array_equal(sc.cpu().numpy(), out32[:, 4])
        c = clear[it]
        n_amb += int((~c).sum())
        if c.any():
            d = float(np.abs(out - states[it + 1])[c][:, :5].max())
            worst = max(worst, d)
            assert d <= 1e-6, (it, d)
            rule_m.add(out[c][:, 5:10], m32[it][c][:, 0:5], states[it + 1][c][:, 5:10])
            rule_v.add(out[c][:, 10:15], m32[it][c][:, 5:10], states[it + 1][c][:, 10:15])
    _report(dict(test="general_k_ipo", J=J, k=len(kl), N=N, axes=axes, K="general" if general else "pinhole",
                 ambiguous_pose_iterations=n_amb, max_param_delta=worst, max_moment_delta=rule_m.delta, fp32_oracle_moment_delta=rule_m.delta32,
                 moment_bound=rule_m.bound, moment_ratio=rule_m.ratio, max_v_delta=rule_v.delta, fp32_oracle_v_delta=rule_v.delta32,
                 v_bound=rule_v.bound, v_ratio=rule_v.ratio))
    assert n_amb <= 0.05 * 50 * N, n_amb
    assert worst > 0
    assert rule_m.holds(), (rule_m.delta, rule_m.bound)
    assert rule_v.holds() and rule_v.largest > 0, (rule_v.delta, rule_v.bound)
    assert (np.abs(states[50][:, present]).min(0) > 0).all() and (states[50][:, absent] == 0).all()


# ---- c. Adam beyond the constant table ------------------------------------------------------------------------------------------

def test_adam_bias_corrections_across_the_end_of_the_table(zh):
    """ipo_adam_terms reads step size and sqrt(1 - beta2^t) from a constant table below iteration 2048 and forms them from running
    double products above; zedo_ipo_fit_resume forms beta^it_begin on the host.  The oracle's float64 state after 20 iterations
    ((17, [0, 1, 4]), N = 8, "xyz", general K) is DECLARED to be the state after it0 iterations: one iteration from it with
    it_begin = it0 on either side of the seam and far beyond it, and four iterations in one call from 2046 (the seam is crossed
    inside the kernel's loop), against O.ipo_fit(init=, it0=) in float64.  Bound: 1e-6 on the parameters of poses whose residuals are
    all >= 1e-3 px (in all four iterations for the second part); the second moments of the same poses by the rule of
    test_ipo_single_iterations_on_general_intrinsics, the fp32 oracle running the same call from the same fp32 state.  (Running
    thousands of iterations to get there would end in a converged L1 fit that sits on its sign changes.)"""
    J, kl, N, axes = 17, [0, 1, 4], 8, "xyz"
    states = oracle_run(J, tuple(kl), N, axes)[0]
    cl, uvn, Kn = problem(J, N)
    x0, uv, K = dev(cl), dev(uvn), dev(Kn)
    args = oracle_args(J, kl, N)
    norm = N * len(kl) * 2
    moving = np.abs(cl[0][kl]).max(-1) > 0
    s20 = states[20]

    def run(it0, iters):
        want, _, _, res = oracle_resume(args, axes, norm, s20, it0, iters)
        clear = (res[:, :, moving, :].reshape(iters, N, -1).min(2) >= 1e-3).all(0)
        st = dev(s20.astype(np.float32))
        zh.ipo_fit(x0, uv, K, kl, axes, IPO_T, IPO_MIN, IPO_MAX, iters, norm, N, state=st, it_begin=it0)
        return st.cpu().numpy().astype(np.float64), want, clear, oracle_resume(args, axes, norm, s20, it0, iters, np.float32)[0]

    def second_moments(got, want, clear, o32):
        rule = MomentRule()
        rule.add(got[clear][:, 10:15], o32[clear][:, 10:15], want[clear][:, 10:15])
        return rule

    n_amb, ends = 0, {}
    for it0 in (2046, 2047, 2048, 2049, 4095):
        got, want, clear, o32 = run(it0, 1)
        n_amb += int((~clear).sum())
        d = float(np.abs(got - want)[clear][:, :5].max())
        dm = float(np.abs(got - want)[clear][:, 5:10].max())
        rv = second_moments(got, want, clear, o32)
        _report(dict(test="general_k_adam_table", it_begin=it0, iters=1, clear_poses=int(clear.sum()), max_param_delta=d, max_moment_delta=dm,
                     max_v_delta=rv.delta, v_bound=rv.bound, v_ratio=rv.ratio))
        assert d <= 1e-6, (it0, d)
        assert rv.holds() and rv.largest > 0, (it0, rv.delta, rv.bound)
        ends[it0] = want
    assert n_amb <= 0.05 * 5 * N, n_amb
    # neighbouring iterations differ by far more than the bound (2.6e-5 on either side of the seam): an it_begin that is off by one,
    # in the table index or in the host's beta^it_begin, cannot pass
    assert min(np.abs(ends[a] - ends[a + 1])[:, :5].max() for a in (2046, 2047, 2048)) > 1e-5
    got, want, clear, o32 = run(2046, 4)
    d = float(np.abs(got - want)[clear][:, :5].max())
    rv = second_moments(got, want, clear, o32)
    _report(dict(test="general_k_adam_table", it_begin=2046, iters=4, clear_poses=int(clear.sum()), max_param_delta=d, max_v_delta=rv.delta,
                 v_bound=rv.bound, v_ratio=rv.ratio))
    assert clear.sum() >= N // 2 and d <= 1e-6, (int(clear.sum()), d)
    assert rv.holds() and rv.largest > 0, (rv.delta, rv.bound)


# ---- d. rays, T0, singular systems ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 5, 300])
@pytest.mark.parametrize("J", [1, 17, 21])
def test_reproj_prepare_on_general_intrinsics(zh, J, N):
    """test_reproj_prepare_at_other_joint_counts on general K: rays and unit rays within 1 fp32 ulp of the float64 oracle, the weight
    (c c)(c c) in fp32 and the clamped confidences exact.  Detections in [0, 1000) px keep the homogeneous coordinate of the ray
    (Kinv's third row applied to (u, v, 1): 1 / K22 -+ a few per cent) well away from 0 - asserted."""
    import zedo_oracle as O
    g = np.random.Generator(np.random.Philox(key=[45, 1000 * J + N]))
    K = general_cameras(g, N)
    uv = (1000 * g.random((N, J, 2))).astype(np.float32)
    conf = (1.4 * g.random((N, J)) - 0.2).astype(np.float32)
    conf.reshape(-1)[::7] = np.float32(3e-5)
    conf.reshape(-1)[1::7] = np.float32(1.3)
    Ki = np.linalg.inv(K.astype(np.float64))
    rz = np.einsum("nj,nkj->nk", Ki[:, 2], np.concatenate([uv.astype(np.float64), np.ones((N, J, 1))], -1))
    assert (np.abs(rz * K[:, 2, 2].astype(np.float64)[:, None]) > 0.5).all() and (N == 1 or np.median(np.abs(rz - 1)) > 0.05)
    ray = O.rays_from_keypoints(uv.astype(np.float64), K.astype(np.float64), dtype=np.float64)
    rhat = ray / np.linalg.norm(ray, axis=-1, keepdims=True)
    for c in (None, conf):
        cc = torch.full((N, J), -7.0, device="cuda")
        geom = zh.reproj_prepare(dev(uv), dev(K), None if c is None else dev(c), None if c is None else cc).cpu().numpy()
        assert geom.shape == (N, J, 8)
        for got, want in ((geom[..., 0:2], ray[..., 0:2]), (geom[..., 4:7], rhat)):
            w32 = want.astype(np.float32)
            assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= ulp32(w32)).all()
        assert (geom[..., 3] == 0).all() and (geom[..., 7] == 0).all()
        if c is None:
            assert (geom[..., 2] == 1).all() and (cc == -7.0).all()
        else:
            cl = np.clip(c, np.float32(1e-4), np.float32(1.0))
            assert np.array_equal(cc.cpu().numpy(), cl)
            assert np.array_equal(geom[..., 2], (cl * cl) * (cl * cl))


def test_reproj_grad_on_general_intrinsics_against_the_reference(zh, golden):
    """zedo_reproj_prepare + zedo_reproj_grad against the reference's gradient_field_gen on general K (tests/golden/ipo_general.npz),
    T given and T solved, with and without confidences: the tolerances of test_gradient_field_gen_golden, and the float64 solve beside them."""
    r = golden("ipo_general")
    for tag, conf in (("wild", r["rp_conf_wild"]), ("none", None)):
        cc = torch.empty(16, 17, device="cuda") if conf is not None else None
        geom = zh.reproj_prepare(dev(r["rp_uv"]), dev(r["rp_K"]), None if conf is None else dev(conf), cc)
        T = dev(r["rp_T_given"].reshape(16, 3))
        g = zh.reproj_grad(dev(r["rp_x"]), geom, T, False).cpu().numpy()
        _report(dict(test="general_k_reproj", conf=tag, g_given_max_abs=float(np.abs(g - r[f"rp_g_given_{tag}"]).max())))
        np.testing.assert_allclose(g, r[f"rp_g_given_{tag}"], atol=3e-6, rtol=0)
        assert np.array_equal(T.cpu().numpy(), r["rp_T_given"].reshape(16, 3))
        RR.assert_within(T.cpu().numpy(), g, RR.solve(r["rp_x"], geom.cpu().numpy(), T=r["rp_T_given"].reshape(16, 3)), given=True)
        T = torch.zeros(16, 3, device="cuda")
        g = zh.reproj_grad(dev(r["rp_x"]), geom, T, True).cpu().numpy()
        np.testing.assert_allclose(T.cpu().numpy(), r[f"rp_T_solve_{tag}"].reshape(16, 3), atol=2e-5, rtol=0)
        np.testing.assert_allclose(g, r[f"rp_g_solve_{tag}"], atol=5e-6, rtol=0)
        RR.assert_within(T.cpu().numpy(), g, RR.solve(r["rp_x"], geom.cpu().numpy()))         # float64 at the derived bound (tests/_reproj_ref.py)


def test_initial_translation_on_general_intrinsics(zh):
    """zedo_ipo_fit with iters = 0 returns T = T0 (scale 1) and R = I: against O.ipo_init_T in float64, atol 1e-6 (the bound of
    test_ipo_trajectory_golden on the same quantity).  The third row of Kinv is not (0, 0, 1) here."""
    import zedo_oracle as O
    for J, kl in KEYS:
        for N in (8, 64):
            cl, uvn, Kn = problem(J, N)
            R, T, q, sc = zh.ipo_fit(dev(cl), dev(uvn), dev(Kn), kl, "xy", IPO_T, IPO_MIN, IPO_MAX, 0, N * len(kl) * 2, N, return_params=True)
            want = O.ipo_init_T(uvn.astype(np.float64), Kn.astype(np.float64), IPO_T, dtype=np.float64).reshape(N, 3)
            np.testing.assert_allclose(T.cpu().numpy(), want, atol=1e-6, rtol=0)
            assert np.median(np.abs(want[:, :2])) > 1e-2 and np.median(np.abs(want[:, 2] - IPO_T)) > 1e-3
            assert np.array_equal(R.cpu().numpy(), np.tile(np.eye(3, dtype=np.float32), (N, 1, 1)))
            assert np.array_equal(q.cpu().numpy(), np.tile(np.array([1, 0, 0, 0], np.float32), (N, 1))) and bool((sc == 1).all())


def test_reproj_degenerate_on_general_intrinsics(zh):
    """Unit weights, general K: random detections of two or more joints are never singular, one joint always is."""
    g = np.random.Generator(np.random.Philox(key=[46, 0]))
    for N in (1, 5, 300):
        K = general_cameras(g, N)
        assert zh.reproj_degenerate(zh.reproj_prepare(dev((1000 * g.random((N, 1, 2))).astype(np.float32)), dev(K))) == N
        for J in (2, 17, 21):
            assert zh.reproj_degenerate(zh.reproj_prepare(dev((1000 * g.random((N, J, 2))).astype(np.float32)), dev(K))) == 0


# ---- e. shards ----------------------------------------------------------------------------------------------------------------------

def test_ipo_shard_equals_the_unsharded_rows_on_general_intrinsics(zh):
    """test_ipo_shard_equals_the_unsharded_rows (H = 3, N = 8, J = 21, 100 iterations) with general K and axes "xy": rows [5, 19)
    through row_offset against the same rows of the whole batch, bit for bit - K is indexed by pose (row_offset + b) mod N."""
    J, kl = 21, [0, 1, 4, 20]
    cl, uvn, Kn = problem(J, 8, 3)
    x0, uv, K = dev(cl), dev(uvn), dev(Kn)
    norm = 8 * len(kl) * 2
    full = zh.ipo_fit(x0, uv, K, kl, "xy", IPO_T, IPO_MIN, IPO_MAX, 100, norm, 24, return_params=True)
    part = zh.ipo_fit(x0, uv, K, kl, "xy", IPO_T, IPO_MIN, IPO_MAX, 100, norm, 14, row_offset=5, return_params=True)
    for a, b in zip(full, part):
        assert bool(torch.isfinite(a).all()) and torch.equal(a[5:19], b)
    assert not torch.equal(full[0][0:8], full[0][8:16])                        # the hypotheses differ
    assert not torch.equal(full[1][0:4], full[1][4:8])                         # and so do the poses' cameras
    assert bool((full[2][:, 3] == 0).all()) and bool((full[2][:, 1:3] != 0).all())


# ---- f. the two IPO kernels are twins here as well -------------------------------------------------------------------------------

IPO_TWINS_GENERAL = r"""
import hashlib, json, os, sys
import numpy as np
root = %r
sys.path[:0] = [os.path.join(root, "zedo-release_amd"), os.path.join(root, "tests")]
import torch
import zedo_hip as zh
from _shared import KEYS, TWIN_AXES, IPO_T, IPO_MIN, IPO_MAX, dev, problem
out = {}
for J, kl in KEYS:
    for N in (8, 64):
        cl, uv, K = problem(J, N, 2)
        for axes in TWIN_AXES:
            R, T, q, sc = zh.ipo_fit(dev(cl), dev(uv), dev(K), kl, axes, IPO_T, IPO_MIN, IPO_MAX, 500, N * len(kl) * 2, 2 * N, return_params=True)
            h = hashlib.sha256()
            for t in (R, T, q, sc):
                h.update(t.cpu().numpy().tobytes())
            out["J%%d_k%%d_N%%d_%%s" %% (J, len(kl), N, axes or "none")] = h.hexdigest()
            assert bool(torch.isfinite(R).all())
print("RESULT " + json.dumps(out))
"""


def test_ipo_kernels_are_bitwise_twins_on_general_intrinsics():
    """The half-wave kernel and the lane-per-row kernel (ZEDO_IPO_KERNEL=half|row, read once per process: one child each; the second
    is not started if the first failed) agree bit for bit in R, T, q and scale after 500 iterations on the general-K problems, for the
    six axis subsets the existing twin tests do not run."""
    res = {}
    for pin in ("half", "row"):
        e = dict(os.environ)
        e["ZEDO_IPO_KERNEL"] = pin
        r = subprocess.run([sys.executable, "-c", IPO_TWINS_GENERAL % ROOT], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        res[pin] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert len(res["half"]) == len(KEYS) * 2 * len(TWIN_AXES) and len(set(res["half"].values())) == len(res["half"])
    assert res["half"] == res["row"], {k: (v, res["row"][k]) for k, v in res["half"].items() if v != res["row"][k]}


# ---- g. the module surface -----------------------------------------------------------------------------------------------------------

def test_rotopt_fit_surface_on_general_intrinsics(zh, golden):
    """RotOpt(axis="xy").fit on general K (tests/golden/ipo_general.npz, N = 8, key list [0, 1, 4]) against the reference's captures,
    with the criterion of test_rotopt_fit_surface: the reference's float64 run is the arbiter, its own fp32 run the yardstick -
    after 10 iterations every pose within 2 gaps + 1e-7, after 50 the median pose within 2 median gaps + 1e-7 and every pose within
    0.1.  After 500 iterations (the reference's fp32 end state; Adam on an L1 loss is chaotic by then): the loss of the returned
    (R, T), evaluated by the oracle in float64, within 5 % + 1e-3 of the reference's, the bound of the oracle's own end-state test."""
    import zedo_oracle as O
    from lib.algorithms.advanced.simple_zeroshot_opt import RotOpt
    g = golden("ipo_general")
    N, kl, ai = 8, [0, 1, 4], AXES.index("xy")
    x0, uv, K = dev(g["cluster0"][None]), dev(g["uv_8"]), dev(g["K_8"])
    for i, it in enumerate((10, 50)):
        ro = RotOpt(N, axis="xy", minT=0.5, maxT=2).cuda()
        R, T = ro.fit(x0, uv, K, kl, 3.0, iters=it)
        p = np.concatenate([ro.quaternion().detach().cpu().numpy(), ro.scale.detach().cpu().numpy().reshape(-1, 1)], 1).astype(np.float64)
        p64, p32 = g[f"p64_it{it}_8_h36m"][ai], g["p32_8_h36m_xy"][i].astype(np.float64)
        dp, gp = np.abs(p - p64).max(1), np.abs(p32 - p64).max(1)
        _report(dict(test="general_k_surface", it=it, hip_vs_ref64=float(dp.max()), ref32_vs_ref64=float(gp.max()),
                     hip_vs_ref64_median=float(np.median(dp)), ref32_vs_ref64_median=float(np.median(gp))))
        if it <= 30:
            assert dp.max() <= 2.0 * gp.max() + 1e-7, (it, dp.max(), gp.max())
        else:
            assert np.median(dp) <= 2.0 * np.median(gp) + 1e-7 and dp.max() <= 0.1, (it, np.median(dp), np.median(gp))
        assert (p[:, 3] == 0).all() and R.shape == (N, 3, 3) and T.shape == (N, 1, 3)
    ro = RotOpt(N, axis="xy", minT=0.5, maxT=2).cuda()
    R, T = ro.fit(x0, uv, K, kl, 3.0, iters=500)
    R, T = R.cpu().numpy().astype(np.float64), T.cpu().numpy().astype(np.float64)
    K64, c64 = g["K_8"].astype(np.float64), g["uv_8"].astype(np.float64)[:, kl]
    w = np.einsum("nij,nkj->nki", K64, np.einsum("nij,kj->nki", R, g["cluster0"].astype(np.float64)[kl]) + T)
    loss = float(np.abs(w[..., :2] / w[..., 2:] - c64).mean())
    ref = float(g["loss32_8_h36m_xy"])
    _report(dict(test="general_k_surface", it=500, loss=loss, reference_loss=ref))
    assert abs(loss - ref) <= 0.05 * ref + 1e-3, (loss, ref)
