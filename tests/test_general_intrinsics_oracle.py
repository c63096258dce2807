"""Pins the numpy oracle to captures of the reference on GENERAL camera matrices and on all eight subsets of rotation axes
(tests/golden/ipo_general.npz, tools/gen_golden.py::gen_ipo_general).  CPU only.

Every other fixture feeds a pure pinhole K (K01 = K10 = K20 = K21 = 0, K22 = 1) and RotAxes "z" or "xyz": the products of the IPO's
forward and hand-derived backward with K01, K10, K20, K21, five of the nine cofactors of the inverse, the homogeneous divide of the
rays and the third row of T0 are multiplied by zero there, and six of the eight axis masks never run.  Here K has skew, a homogeneous
row other than (0, 0, 1) and K22 != 1 (lib.dataset.synthetic.general_intrinsics), and the detections are the same poses re-projected
through it.  This is what licenses the oracle as the arbiter of tests/test_general_intrinsics_gpu.py.

What the fixture holds of the reference's float64 IPO run (full traces of all cases would be 2.6 MB; the file stays below
joint_counts.npz): the loss of every one of the 50 iterations - a function of every pose's parameters at every iteration - and the
parameters of every pose after iteration 50 (N = 8: also after iteration 10).  The bounds are those of
test_ipo_custom_key_lists_follow_the_reference: 1e-8 on parameters, 1e-9 relative on the loss."""
import numpy as np
import pytest

import zedo_oracle as O

AXES = ["", "x", "y", "z", "xy", "xz", "yz", "xyz"]                               # the order the fixture stacks them in
KEYLISTS = dict(h36m=(3.0, 0.5), pw3d=(8.0, 0.2), k5=(3.0, 0.5))                  # name -> (IPO_T, IPO_minScaleT)
SNAPS = {8: (10, 50), 64: (50,)}
CASES = [(N, kname) for N in (8, 64) for kname in KEYLISTS if (N, kname) != (64, "pw3d")]


def test_the_fixture_is_general(golden):
    g = golden("ipo_general")
    for K in (g["K_8"], g["K_64"], g["rp_K"]):
        K = K.astype(np.float64)
        assert np.abs(K[:, 0, 1]).min() > 0.05 and np.abs(K[:, 1, 0]).min() > 0.05
        assert np.abs(K[:, 2, 0]).min() > 1e-5 and np.abs(K[:, 2, 1]).min() > 1e-5
        assert np.abs(K[:, 2, 2] - 1).min() > 1e-3
        assert np.median(np.abs(np.linalg.det(K) / (K[:, 0, 0] * K[:, 1, 1]) - 1)) > 0.05
        assert (np.abs(np.linalg.inv(K)) > 0).all()                                # no cofactor is an exact zero
    assert [int(k) for k in g["keylist_k5"]] == [0, 2, 5, 11, 14] and len(g["keylist_pw3d"]) == 17


@pytest.mark.parametrize("axes", AXES, ids=[a or "none" for a in AXES])
@pytest.mark.parametrize("N,kname", CASES)
def test_ipo_on_general_intrinsics_follows_the_reference(golden, N, kname, axes):
    g = golden("ipo_general")
    kl = [int(k) for k in g[f"keylist_{kname}"]]
    ipoT, minT = KEYLISTS[kname]
    a = AXES.index(axes)
    c64, K64 = g[f"uv_{N}"].astype(np.float64), g[f"K_{N}"].astype(np.float64)
    x64 = np.broadcast_to(g["cluster0"][None], (N, 17, 3)).astype(np.float64)
    T0 = O.ipo_init_T(c64, K64, ipoT, dtype=np.float64)
    np.testing.assert_allclose(T0, g[f"T0f64_{N}_{kname}"], atol=1e-10, rtol=0)
    np.testing.assert_allclose(O.ipo_init_T(g[f"uv_{N}"], g[f"K_{N}"], ipoT), g[f"T0_{N}_{kname}"], atol=1e-6, rtol=0)
    tr = []
    O.ipo_fit(x64[:, kl], T0, K64, c64[:, kl], axes, minT, 2.0, 50, dtype=np.float64, trace=tr)
    ref_loss = g[f"trace_loss64_{N}_{kname}"][a]
    for it in range(50):
        assert abs(tr[it][2] - ref_loss[it]) <= 1e-9 * max(1.0, ref_loss[it]), it
    absent = [1 + i for i, c in enumerate("xyz") if c not in axes]
    for it in SNAPS[N]:
        ref = g[f"p64_it{it}_{N}_{kname}"][a]
        assert np.abs(tr[it - 1][0] - ref[:, :4]).max() <= 1e-8, it
        assert np.abs(tr[it - 1][1] - ref[:, 4]).max() <= 1e-8, it
        assert (ref[:, absent] == 0).all() and (tr[it - 1][0][:, absent] == 0).all()
        present = [0] + [1 + i for i, c in enumerate("xyz") if c in axes] + [4]
        assert (np.abs(ref[:, present]).min(0) > 0).all()                          # every parameter of the mask did move
    if axes in ("", "xy"):
        # the fp32 oracle against the reference's fp32 run: the loss of the end state after 500 iterations, at the bound of
        # test_ipo_custom_key_lists_follow_the_reference (5 % + 1e-3; Adam on an L1 loss is chaotic by then)
        x32 = x64.astype(np.float32)
        loss = O.ipo_fit(x32[:, kl], O.ipo_init_T(g[f"uv_{N}"], g[f"K_{N}"], ipoT), g[f"K_{N}"], g[f"uv_{N}"][:, kl], axes, minT, 2.0, 500)[4]
        ref = float(g[f"loss32_{N}_{kname}_{axes or 'none'}"])
        assert abs(loss - ref) <= 0.05 * ref + 1e-3, (loss, ref)


def test_ipo_fit_continues_from_a_given_state(golden):
    """ipo_fit(init=, it0=): 20 + 30 iterations equal 50 in one call bit for bit (float64 and fp32), and the defaults are the fresh start."""
    g = golden("ipo_general")
    kl, N = [0, 1, 4], 8
    for dt in (np.float64, np.float32):
        c, K = g["uv_8"].astype(dt), g["K_8"].astype(dt)
        x = np.broadcast_to(g["cluster0"][None], (N, 17, 3)).astype(dt)
        T0 = O.ipo_init_T(c, K, 3.0, dtype=dt)
        one, two = [], []
        O.ipo_fit(x[:, kl], T0, K, c[:, kl], "xyz", 0.5, 2.0, 50, dtype=dt, trace=one)
        O.ipo_fit(x[:, kl], T0, K, c[:, kl], "xyz", 0.5, 2.0, 20, dtype=dt, trace=two)
        t = two[-1]
        init = (t[0], t[1], t[3], t[4], t[5], t[6])
        O.ipo_fit(x[:, kl], T0, K, c[:, kl], "xyz", 0.5, 2.0, 30, dtype=dt, trace=two, init=init, it0=20)
        assert len(two) == 50
        for a, b in zip(one, two):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        assert np.array_equal(init[0], two[19][0])                                 # the caller's state is not written to


RP_VARIANTS = [("wild", np.float64), ("wild", np.float32), ("none", np.float64), ("none", np.float32)]
RP_IDS = [f"{t}-{d.__name__}" for t, d in RP_VARIANTS]


@pytest.mark.parametrize("tag,dt", RP_VARIANTS, ids=RP_IDS)
def test_gradient_field_gen_with_the_least_squares_T_on_general_intrinsics(golden, tag, dt):
    """O.gradient_field_gen (T solved) in float64 and in fp32 against the reference's fp32 values, at the bounds test_gradient_field_gen
    applies to reproj.npz: 3e-6 on the gradient, 1e-5 on T."""
    r = golden("ipo_general")
    conf = r["rp_conf_wild"] if tag == "wild" else None
    g2, T2 = O.gradient_field_gen(r["rp_uv"], r["rp_x"], r["rp_K"], t=None, conf=conf, dtype=dt)
    np.testing.assert_allclose(g2, r[f"rp_g_solve_{tag}"], atol=3e-6, rtol=0)
    np.testing.assert_allclose(T2, r[f"rp_T_solve_{tag}"], atol=1e-5, rtol=0)
    assert np.abs(r[f"rp_g_solve_{tag}"]).max() > 1e-2 and (r[f"rp_T_solve_{tag}"][:, 0, 2] > 0).all()


def test_gradient_field_gen_with_a_given_T_on_general_intrinsics(golden):
    """O.gradient_field_gen in float64 (T given, 5 m in front of the camera) against the reference, bound 1e-6 (the bound
    test_gradient_field_gen applies to reproj.npz).

    The captured values it is held to are the reference's gradient_field_gen called with DOUBLE tensors (rp_g_given_f64: with T given
    every statement of that function is then evaluated in double).  The reference's fp32 output cannot serve a float64 oracle at this
    bound - it is itself farther than 1e-6 from the same function in double.  Figures (max |difference| over 16 x 17 x 3):
        float64 oracle - reference with double tensors                       3.6e-15
        reference fp32 - reference with double tensors                       1.271e-6   (7 of 816 above 1e-6)
        the same gap on the pinhole fixture (reproj.npz: g_given_none)       1.391e-6
        float64 oracle - reference fp32                                      1.271e-6
        fp32 oracle    - reference fp32                                      1.431e-6
    (one fp32 ulp of the 5 m operands is 4.8e-7; on reproj.npz the fp32 oracle meets 1e-6 because numpy and torch round a pinhole
    inverse - five exact zeros, K22 = 1 - alike, which they do not with a general K).  The fp32 capture stays in the fixture: the HIP
    kernels are compared with it (tests/test_general_intrinsics_gpu.py), and its distance from the double run is asserted here to be
    what one expects of an fp32 evaluation: above the oracle's bound, below the 3e-6 the kernels are allowed against it.
    The confidences do not enter with T given."""
    r = golden("ipo_general")
    ref = r["rp_g_given_f64"]
    assert ref.dtype == np.float64 and np.abs(ref).max() > 1e-2
    for conf in (r["rp_conf_wild"], None):
        g1, T1 = O.gradient_field_gen(r["rp_uv"], r["rp_x"], r["rp_K"], t=r["rp_T_given"], conf=conf, dtype=np.float64)
        assert np.array_equal(T1, r["rp_T_given"])
        d = float(np.abs(g1 - ref).max())
        print(f"gradient_field_gen, T given, float64: max |oracle - reference in double| = {d:.4e}")
        assert d <= 1e-6, d
    assert np.array_equal(r["rp_g_given_wild"], r["rp_g_given_none"])
    gap = float(np.abs(r["rp_g_given_none"] - ref).max())
    assert 1e-6 < gap < 3e-6, gap
