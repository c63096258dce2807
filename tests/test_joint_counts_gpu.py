"""GPU tests at every skeleton size the C ABI accepts, not only 17 joints x 3 coordinates (include/zedo_hip.h): the score
network for J3 = n_joints * joint_dim from 1 to 64 (padding to 64 columns, the other pre_dense instantiation above 56, pack /
unpack / noise / norm kernels indexed with J3, the chunk walk), the geometry, IPO and selection kernels for other joint counts,
and the refusals of the two entry points that are 17-joint only.  The arbiter is the numpy oracle in float64, which
tests/test_joint_counts_oracle.py pins to captures of the reference at these sizes; every bound is one the suite already applies
at 17 joints, except the Langevin step size, whose bound is derived below from the fixed summation order of its kernels.
(17, 3) rides along in every parametrisation as the control."""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _procrustes_ref as PR
from _shared import (IPO_KEYS, IPO_MAX, IPO_MIN, IPO_T, cameras, cfg_path, dev, ipo_single_iterations_from_the_oracle, make_ipo_problem,
                     report_env as _report, ulp32, zh)  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(1, 1), (1, 3), (16, 3), (14, 4), (19, 3), (21, 3), (16, 4)]          # J3 = 1, 3, 48, 56, 57, 63, 64 (the fixture's)
CONTROL = (17, 3)
BY_J3 = {nj * jd: (nj, jd) for nj, jd in SIZES + [CONTROL]}
TS = np.array([0.1, 0.05, 0.011], np.float32)


@functools.lru_cache(maxsize=None)
def weights_of(nj, jd, lifted=False):
    """make_weights(seed=0) at this size.  lifted: the rows of pre_dense.weight whose largest entry is below 2^-7.9 of the matrix
    maximum raised to that (sign kept) - see needs_lift."""
    from lib.dataset import synthetic as syn
    w = syn.make_weights(seed=0, n_joints=nj, joint_dim=jd)
    if lifted:
        a = w["pre_dense.weight"]
        lim = np.float32(np.abs(a).max() * 2.0 ** -7.9)
        low = np.abs(a).max(1) < lim
        assert low.any() and a.shape[1] == 1
        a[low] = np.where(a[low] < 0, -lim, lim)
    return w


def needs_lift(nj, jd, mode):
    """A limit of the split-fp16 mode, not of a size: each matrix carries one scale, and zedo_weights_set_math refuses a matrix with
    a row whose largest entry is below 2^-8 of the matrix maximum (include/zedo_hip.h).  With ONE input coordinate every row of
    pre_dense.weight is a single uniform draw, so a random-init J3 = 1 network always has such rows (J3 = 3 already does not):
    test_split_fp16_refuses_the_random_single_coordinate_network asserts the refusal, and the J3 = 1 cases run in that mode on the
    same draw with those rows lifted to 2^-7.9 of the maximum - the oracle evaluates the same weights."""
    return nj * jd == 1 and mode == "f16x3"


@functools.lru_cache(maxsize=None)
def weights64_of(nj, jd, lifted=False):
    import zedo_oracle as O
    return O.cast_weights(weights_of(nj, jd, lifted), np.float64)


_HANDLES = {}


def handle(zh, nj, jd, mode, lifted=False):
    """One zedo_hip.Weights per size, arithmetic mode and weight variant for the whole module."""
    k = (nj, jd, mode, lifted)
    if k not in _HANDLES:
        _HANDLES[k] = zh.Weights(weights_of(nj, jd, lifted), n_joints=nj, joint_dim=jd, math=mode)
    assert _HANDLES[k].math == mode
    return _HANDLES[k]


# ---- 1. the network, single calls ----------------------------------------------------------------------------------------

NET_CASES = [(nj, jd, B) for nj, jd in SIZES + [CONTROL] for B in (1, 70)] + \
            [(nj, jd, B) for nj, jd in ((1, 1), (19, 3), (16, 4), CONTROL) for B in (2100, 8500)]


def test_score_network_golden_at_other_sizes(zh, golden, math_mode):
    """The reference's own output (tests/golden/joint_counts.npz), as test_score_network_golden holds the 17-joint capture."""
    g = golden("joint_counts")
    for nj, jd in SIZES:
        if needs_lift(nj, jd, math_mode):                    # the capture is of the stock draw, which this mode refuses
            continue
        W = handle(zh, nj, jd, math_mode)
        s = zh.Schedule(W, g["ts"])
        for i in range(len(g["ts"])):
            eps = zh.score_eps(W, s, i, dev(g[f"x_{nj}x{jd}"])).cpu().numpy()
            assert eps.shape == (8, nj, jd)
            np.testing.assert_allclose(eps, g[f"eps_{nj}x{jd}"][i], atol=2e-6, rtol=0)


def test_split_fp16_refuses_the_random_single_coordinate_network(zh):
    """needs_lift: the stock J3 = 1 draw is accepted in exact fp32 and refused by zedo_weights_set_math (ZEDO_E_BADARG, the handle
    stays in exact fp32); the lifted draw is accepted."""
    W = zh.Weights(weights_of(1, 1), n_joints=1, joint_dim=1, math="f32")
    with pytest.raises(zh.ZedoError, match=r"code -1"):
        W.set_math("f16x3")
    assert W.math == "f32" and zh._lib.zedo_weights_get_math(W._h) == 0
    with pytest.raises(zh.ZedoError, match=r"code -1"):
        zh.Weights(weights_of(1, 1), n_joints=1, joint_dim=1, math="f16x3")
    assert zh.Weights(weights_of(1, 1, True), n_joints=1, joint_dim=1, math="f16x3").math == "f16x3"
    assert zh.Weights(weights_of(1, 3), n_joints=1, joint_dim=3, math="f16x3").math == "f16x3"


@pytest.mark.parametrize("nj,jd,B", NET_CASES, ids=[f"{a}x{b}-B{c}" for a, b, c in NET_CASES])
def test_score_eps_and_sde_step_against_the_float64_oracle(zh, math_mode, nj, jd, B):
    """zedo_score_eps and zedo_sde_step at three noise levels against the oracle in float64: max |error| <= 2e-6 x max(1, output
    scale) in both modes, the split-fp16 rms within 1.25 x the exact-fp32 rms + 1e-8
    (test_both_math_modes_are_fp32_accurate_against_the_fp64_oracle), x' against a x + c eps with atol 5e-7 (test_pc_step_golden).
    B = 1 / 70: every size; 2100 and 8500 rows (the other two post_dense shapes) for J3 = 1, 57, 64 and the control, the oracle on
    a sample of rows that includes the first and the last 40."""
    import zedo_oracle as O
    g = np.random.Generator(np.random.Philox(key=[31, 100000 * nj * jd + B]))
    # The rms of the two modes is compared on at least 400 rows (the sample the bound was checked on at these sizes): B rows alone
    # are 3 numbers at J3 = 1, B = 1, where the statistic is the final fp32 rounding of three outputs (half an ulp of 0.3 is 1.5e-8,
    # the size of either rms) and says nothing about the arithmetic.  Small batches are therefore repeated with fresh draws - every
    # call is one of B rows, the launch shape of the case - and every one of those calls is held to the max-abs bound as well.
    reps = -(-400 // B) if B < 400 else 1
    x = (0.3 * g.standard_normal((reps, B, nj, jd))).astype(np.float32)
    pick = np.arange(B) if B < 400 else np.unique(np.concatenate([np.arange(40), np.arange(B - 40, B), g.integers(0, B, 320)]))
    lift = needs_lift(nj, jd, math_mode)
    w64 = weights64_of(nj, jd, lift)
    W = handle(zh, nj, jd, math_mode, lift)
    s = zh.Schedule(W, TS)
    W32 = handle(zh, nj, jd, "f32", lift) if math_mode == "f16x3" else None
    s32 = zh.Schedule(W32, TS) if W32 is not None else None
    sq, sq32, n, worst, worst_step = 0.0, 0.0, 0, 0.0, 0.0
    for i, t in enumerate(TS):
        xp = x[:, pick].reshape(-1, nj, jd).astype(np.float64)
        ref = O.score_model_forward(w64, xp, np.float64(t) * 999.0, dtype=np.float64).reshape(reps, len(pick), nj, jd)
        scale = max(1.0, float(np.abs(ref).max()))
        for k in range(reps):
            eps = zh.score_eps(W, s, i, dev(x[k])).cpu().numpy()
            assert eps.shape == x[k].shape and np.isfinite(eps).all()
            d = np.abs(eps[pick].astype(np.float64) - ref[k])
            worst = max(worst, float(d.max()) / scale)
            assert d.max() <= 2e-6 * scale, (float(t), k, float(d.max()), scale)
            sq, n = sq + float((d * d).sum()), n + d.size
            if W32 is not None:
                d32 = np.abs(zh.score_eps(W32, s32, i, dev(x[k])).cpu().numpy()[pick].astype(np.float64) - ref[k])
                sq32 += float((d32 * d32).sum())
        xs = dev(x[0])
        assert zh.sde_step(W, s, i, xs) is xs
        want = O.pc_step(w64, x[0][pick].astype(np.float64), np.float64(t), dtype=np.float64)
        ds = float(np.abs(xs.cpu().numpy()[pick].astype(np.float64) - want).max())
        worst_step = max(worst_step, ds)
        assert ds <= 5e-7, (float(t), ds)
    rms = float(np.sqrt(sq / n))
    _report(dict(test="joint_counts_net", math=math_mode, J3=nj * jd, B=B, calls_per_label=reps, max_abs_over_scale=worst, rms=rms,
                 rms_f32=float(np.sqrt(sq32 / n)) if W32 is not None else None, sde_step_max_abs=worst_step))
    if W32 is not None:
        assert rms <= 1.25 * float(np.sqrt(sq32 / n)) + 1e-8, (rms, float(np.sqrt(sq32 / n)))


# ---- 2. padding is inert -------------------------------------------------------------------------------------------------

EMBED = [(48, 51), (51, 56), (51, 57), (57, 64), (1, 64)]


@pytest.mark.parametrize("d,D", EMBED, ids=[f"{a}in{b}" for a, b in EMBED])
def test_a_network_embedded_in_a_wider_one_gives_the_same_bits(zh, math_mode, d, D):
    """A J3 = d network inside a J3 = D > d one: the extra pre_dense columns, post_dense rows and biases are zero, the extra input
    coordinates arbitrary.  The first d outputs equal the small network's bit for bit and the extra outputs are exactly 0: the
    exact-fp32 layers are an fma chain per output and 0 * x terms do not change its value (51 -> 57 changes the pre_dense
    instantiation: k = 56..63 are then walked instead of skipped, the same products in the same order); the split-fp16 copies carry
    one scale per matrix, which depends on the matrix maximum only."""
    (nj, jd), (NJ, JD) = BY_J3[d], BY_J3[D]
    lift = needs_lift(nj, jd, math_mode)
    small = weights_of(nj, jd, lift)
    big = {k: v.copy() for k, v in small.items()}
    big["pre_dense.weight"] = np.zeros((1024, D), np.float32)
    big["pre_dense.weight"][:, :d] = small["pre_dense.weight"]
    big["post_dense.weight"] = np.zeros((D, 1024), np.float32)
    big["post_dense.weight"][:d] = small["post_dense.weight"]
    big["post_dense.bias"] = np.zeros(D, np.float32)
    big["post_dense.bias"][:d] = small["post_dense.bias"]
    Ws, Wb = handle(zh, nj, jd, math_mode, lift), zh.Weights(big, n_joints=NJ, joint_dim=JD, math=math_mode)
    ss, sb = zh.Schedule(Ws, TS), zh.Schedule(Wb, TS)
    for B in (70, 2100):
        g = np.random.Generator(np.random.Philox(key=[32, 1000000 * d + 10000 * D + B]))
        xs = (0.3 * g.standard_normal((B, d))).astype(np.float32)
        xb = np.concatenate([xs, (1.0 + g.random((B, D - d))).astype(np.float32)], axis=1)       # the extra coordinates: 1 .. 2
        for i in (0, 2):
            es = zh.score_eps(Ws, ss, i, dev(xs.reshape(B, nj, jd))).cpu().numpy().reshape(B, d)
            eb = zh.score_eps(Wb, sb, i, dev(xb.reshape(B, NJ, JD))).cpu().numpy().reshape(B, D)
            assert np.abs(es).max() > 1e-3
            assert np.array_equal(eb[:, :d], es), (B, i, int((eb[:, :d] != es).sum()), float(np.abs(eb[:, :d] - es).max()))
            assert (eb[:, d:] == 0).all()
            ys, yb = dev(xs.reshape(B, nj, jd)), dev(xb.reshape(B, NJ, JD))
            zh.sde_step(Ws, ss, i, ys)
            zh.sde_step(Wb, sb, i, yb)
            assert np.array_equal(yb.cpu().numpy().reshape(B, D)[:, :d], ys.cpu().numpy().reshape(B, d))


# ---- 3. zedo_pc_step at the ABI ------------------------------------------------------------------------------------------

PC_J3 = [1, 48, 51, 57, 64]
PC_B = [1, 63, 70, 886]
LABEL = np.float32(0.37) * np.float32(999)
NS = np.float32(-2.75)
f1 = lambda v: np.array([v], np.float32)


def _pc_inputs(zh, math_mode, J3, B, key):
    nj, jd = BY_J3[J3]
    W = handle(zh, nj, jd, math_mode, needs_lift(nj, jd, math_mode))
    g = np.random.Generator(np.random.Philox(key=[key, 100000 * J3 + B]))
    x = (0.3 * g.standard_normal((B, nj, jd))).astype(np.float32)
    z = [g.standard_normal((B, nj, jd)).astype(np.float32) for _ in range(2)]
    sched = zh.Schedule(W, [LABEL], label_scale=1.0)
    eps_of = lambda a: zh.score_eps(W, sched, 0, dev(a)).cpu().numpy().astype(np.float64)
    return W, x, z, eps_of


@pytest.mark.parametrize("B", PC_B)
@pytest.mark.parametrize("J3", PC_J3)
def test_predictor_step_is_the_epilogue_fma_and_the_noise_term(zh, math_mode, J3, B):
    """test_one_step_abi_is_the_epilogue_fma_and_the_noise_term (tests/test_pc_native_gpu.py) at other J3: x_mean =
    fma(A, x, fl32(c eps)) with eps = zedo_score_eps at the same label, to 1 fp32 ulp; x_new - x_mean = fl32(C z) to 1 ulp of x_new."""
    W, x, z, eps_of = _pc_inputs(zh, math_mode, J3, B, 91)
    A, Bc, C = np.float32(1.0123), np.float32(0.0371), np.float32(0.0816)
    eps = eps_of(x)
    p = zh.PcPlan(W, SimpleNamespace(label=f1(LABEL), net_scale=f1(NS), has_predictor=True, pA=f1(A), pB=f1(Bc), pC=f1(C),
                                     corrector=0, n_corr=0, corr=None))
    xn, xm = dev(x), torch.empty_like(dev(x))
    zh.pc_step(W, p, 0, xn, [dev(z[0])], xm)
    xn, xm = xn.cpu().numpy(), xm.cpu().numpy()
    c = np.float32(Bc * NS)
    ref = np.float64(A) * x.astype(np.float64) + (np.float64(c) * eps).astype(np.float32).astype(np.float64)
    d = np.abs(xm.astype(np.float64) - ref) / ulp32(ref)
    assert d.max() <= 1.0, float(d.max())
    want = (np.float64(C) * z[0].astype(np.float64)).astype(np.float32).astype(np.float64)
    dn = np.abs(xn.astype(np.float64) - xm.astype(np.float64) - want) / ulp32(xn)
    assert dn.max() <= 1.0, float(dn.max())
    k = dev(x)
    zh.pc_step(W, p, 0, k, [], None)                         # noise removal: x returns x_mean
    assert np.array_equal(k.cpu().numpy(), xm)
    assert zh.workspace_bytes(B) == int(zh._lib.zedo_pc_workspace_bytes(p._h, B))


@pytest.mark.parametrize("B", PC_B)
@pytest.mark.parametrize("J3", PC_J3)
def test_ald_corrector_steps(zh, math_mode, J3, B):
    """ALD, one and two corrector steps, no predictor: x_mean = fma(1, x, fl32(cc eps(x))) (the same epilogue with a = 1,
    cc = fl32(s net_scale)), x = x_mean + fl32(cz z), cz = fl32(sqrt(2 s)).  Composed in float64 from zedo_score_eps at the state the
    step starts from; each stage is held to its roundings: 1 ulp of x_mean (the bound of the predictor test), 1 ulp of the noise
    product and 1 ulp of the sum.  The second step starts from the first call's own output (one launch sequence: the same bits)."""
    W, x, z, eps_of = _pc_inputs(zh, math_mode, J3, B, 92)
    sv = np.float32(3e-4)
    cc, cz = np.float64(np.float32(sv * NS)), np.float64(np.float32(np.sqrt(2.0 * np.float64(sv))))
    plan = lambda n: zh.PcPlan(W, SimpleNamespace(label=f1(LABEL), net_scale=f1(NS), has_predictor=False, pA=None, pB=None, pC=None,
                                                  corrector=2, n_corr=n, corr=f1(sv)))

    def check(got, start, zz, what):
        xm = start.astype(np.float64) + (cc * eps_of(start)).astype(np.float32).astype(np.float64)
        nz = (cz * zz.astype(np.float64)).astype(np.float32).astype(np.float64)
        ref = xm + nz
        bound = ulp32(xm) + ulp32(nz) + ulp32(ref)
        r = float((np.abs(got.astype(np.float64) - ref) / bound).max())
        assert r <= 1.0, (what, r)
        assert np.abs(got - start).max() > 1e-4              # the step did move the state
    x1, m1 = dev(x), torch.empty_like(dev(x))
    zh.pc_step(W, plan(1), 0, x1, [dev(z[0])], m1)
    assert torch.equal(x1, m1)                               # no predictor: x_mean receives x_new
    x1 = x1.cpu().numpy()
    check(x1, x, z[0], "one step")
    x2 = dev(x)
    zh.pc_step(W, plan(2), 0, x2, [dev(z[0]), dev(z[1])], None)
    check(x2.cpu().numpy(), x1, z[1], "second of two steps")


@pytest.mark.parametrize("B", PC_B)
@pytest.mark.parametrize("J3", PC_J3)
def test_langevin_step_size_is_over_the_real_columns_and_rows(zh, math_mode, J3, B):
    """Langevin corrector: s = factor (mean_b ||z_b|| / (|net_scale| mean_b ||eps_b||))^2, x <- x + s net_scale eps + sqrt(2 s) z,
    recomputed in float64 from zedo_score_eps and the draw over exactly the J3 real columns and the B real rows.

    Bound (derived, not measured): every sum in the step size is a sum of non-negative fp32 terms along a chain of at most
    n = 4 + 4 + ceil(B / 256) + 8 additions (pc_norms_kernel: four columns per lane, a 16-lane tree; pc_lvn_scalars_kernel: rows
    t, t + 256, ... then a 256-wide tree), so each mean carries a relative error of at most n 2^-24 and s, a squared ratio of two
    means times a few roundings, at most r = 2 (2 n + 3) 2^-24 to first order.  Every element of the updated state must lie within
    r (|s net_scale eps| + |sqrt(2 s) z| / 2) + 2 ulp(x) of the float64 formula, for every J3 alike."""
    W, x, z, eps_of = _pc_inputs(zh, math_mode, J3, B, 93)
    factor = np.float32(2 * 0.16 ** 2)
    p = zh.PcPlan(W, SimpleNamespace(label=f1(LABEL), net_scale=f1(NS), has_predictor=False, pA=None, pB=None, pC=None,
                                     corrector=1, n_corr=1, corr=f1(factor)))
    eps = eps_of(x).reshape(B, J3)
    z64 = z[0].astype(np.float64).reshape(B, J3)
    me, mz = np.sqrt((eps ** 2).sum(1)).mean(), np.sqrt((z64 ** 2).sum(1)).mean()
    s = np.float64(factor) * (mz / (abs(np.float64(NS)) * me)) ** 2
    drift, noise = s * np.float64(NS) * eps, np.sqrt(2.0 * s) * z64
    ref = x.astype(np.float64).reshape(B, J3) + drift + noise
    n = 4 + 4 + -(-B // 256) + 8
    r = 2 * (2 * n + 3) * 2.0 ** -24
    bound = r * (np.abs(drift) + np.abs(noise) / 2) + 2 * ulp32(ref)
    xn = dev(x)
    zh.pc_step(W, p, 0, xn, [dev(z[0])], None)
    got = xn.cpu().numpy().astype(np.float64).reshape(B, J3)
    frac = float((np.abs(got - ref) / bound).max())
    _report(dict(test="joint_counts_langevin", math=math_mode, J3=J3, B=B, step_size=float(s), r=r, max_fraction_of_bound=frac))
    assert np.isfinite(got).all() and frac <= 1.0, frac
    assert np.abs(noise).max() > 0.1 and np.abs(drift).max() > 1e-3      # both terms are exercised, not rounded away


# ---- 4. the chunk walk ---------------------------------------------------------------------------------------------------

def test_row_chunks_advance_by_the_handles_own_row_width(tmp_path):
    """J3 = 57, B = 300: zedo_score_eps, zedo_sde_step and an ALD zedo_pc_step with ZEDO_CHUNK_ROWS=128 (rounded up to 256 rows:
    two chunks) against the unchunked run, bit for bit.  The chunk walk advances the caller's pointers by r0 * J3.  Child
    processes: the cap is read once."""
    code = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from types import SimpleNamespace as NS
import zedo_hip as zh
from lib.dataset import synthetic as syn
W = zh.Weights(syn.make_weights(0, n_joints=19, joint_dim=3), n_joints=19, joint_dim=3)
f = lambda *v: np.array(v, np.float32)
g = np.random.Generator(np.random.Philox(key=[33, 57]))
x = (0.3 * g.standard_normal((300, 19, 3))).astype(np.float32)
z = [torch.tensor(g.standard_normal((300, 19, 3)).astype(np.float32), device="cuda") for _ in range(3)]
s = zh.Schedule(W, f(0.1, 0.02))
out = {}
for i in (0, 1):
    out[f"eps_{i}"] = zh.score_eps(W, s, i, torch.tensor(x, device="cuda")).cpu().numpy()
    out[f"sde_{i}"] = zh.sde_step(W, s, i, torch.tensor(x, device="cuda")).cpu().numpy()
p = zh.PcPlan(W, NS(label=f(311.0), net_scale=f(-1.9), pA=f(1.004), pB=f(0.011), pC=f(0.09), has_predictor=True, corrector=2, n_corr=2,
                    corr=f(3e-4)))
xn, xm = torch.tensor(x, device="cuda"), torch.empty(300, 19, 3, device="cuda")
zh.pc_step(W, p, 0, xn, z, xm)
out["ald_x"], out["ald_m"] = xn.cpu().numpy(), xm.cpu().numpy()
out["ws"] = np.int64(zh.workspace_bytes(300))
np.savez(sys.argv[1], **out)
''' % (os.path.join(ROOT, "zedo-release_amd"), ROOT)
    outs = []
    for tag, env in (("full", {}), ("chunk", {"ZEDO_CHUNK_ROWS": "128"})):
        out = str(tmp_path / f"{tag}.npz")
        env_all = {k: v for k, v in os.environ.items() if k != "ZEDO_CHUNK_ROWS"}
        subprocess.run([sys.executable, "-c", code, out], check=True, env={**env_all, **env}, timeout=600)
        outs.append(np.load(out))
    keys = [k for k in outs[0].files if k != "ws"]
    assert len(keys) == 6
    for k in keys:
        assert outs[0][k].shape == (300, 19, 3) and np.isfinite(outs[0][k]).all()
        assert np.array_equal(outs[0][k], outs[1][k]), (k, int((outs[0][k] != outs[1][k]).sum()))
    assert not np.array_equal(outs[0]["ald_x"], outs[0]["ald_m"])
    assert int(outs[1]["ws"]) == 256 * (64 + 2048) * 4 < int(outs[0]["ws"])          # 300 rows did walk two chunks


# ---- 5. the model surface ------------------------------------------------------------------------------------------------

def test_model_surface_with_nineteen_joints(zh, math_mode):
    """ScoreModelFC_Adv(cfg, 19, 3, ...) hands its own n_joints to zedo_hip.Weights (lib/algorithms/advanced/model.py): forward on
    the GPU against the float64 oracle, the single-call bound."""
    import zedo_oracle as O
    from lib.algorithms.advanced.model import ScoreModelFC_Adv
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    cfg = load_config(cfg_path("h36m"))
    m = ScoreModelFC_Adv(cfg, 19, 3, 1024, 512, 3)
    sd = {k: torch.tensor(v) for k, v in weights_of(19, 3).items()}
    sd["sigmas"] = torch.tensor(syn.sigmas_buffer())
    m.load_state_dict(sd)
    m.eval()
    g = np.random.Generator(np.random.Philox(key=[34, 57]))
    x = (0.3 * g.standard_normal((70, 19, 3))).astype(np.float32)
    for t in TS:
        label = np.float32(t) * np.float32(999)
        eps = m(dev(x), torch.full((70,), float(label), device="cuda"))
        assert eps.shape == (70, 19, 3) and m.hip_weights().math == math_mode and m.hip_weights().n_joints == 19
        ref = O.score_model_forward(weights64_of(19, 3), x.astype(np.float64), np.float64(label), dtype=np.float64)
        d = float(np.abs(eps.cpu().numpy().astype(np.float64) - ref).max())
        assert d <= 2e-6 * max(1.0, float(np.abs(ref).max())), d


# ---- 6. geometry ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 5, 300])
@pytest.mark.parametrize("J", [1, 2, 16, 17, 21, 40])
def test_reproj_prepare_at_other_joint_counts(zh, J, N):
    """Rays against the oracle in float64 rounded to fp32, within 1 ulp (the kernel computes them in double); the weight equal to
    (c c)(c c) evaluated in fp32 with c = clamp(conf, 1e-4, 1), the clamped confidences equal, weight 1 without confidences."""
    import zedo_oracle as O
    g = np.random.Generator(np.random.Philox(key=[35, 1000 * J + N]))
    K = cameras(g, N)
    uv = (1000 * g.random((N, J, 2))).astype(np.float32)
    conf = (1.4 * g.random((N, J)) - 0.2).astype(np.float32)                   # -0.2 .. 1.2: both clamps are taken
    conf.reshape(-1)[::7] = np.float32(3e-5)
    conf.reshape(-1)[1::7] = np.float32(1.3)
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
            assert cl.min() == np.float32(1e-4) and (cl.size == 1 or cl.max() == 1.0)
            assert np.array_equal(cc.cpu().numpy(), cl)
            assert np.array_equal(geom[..., 2], (cl * cl) * (cl * cl))


def test_reproj_degenerate_at_other_joint_counts(zh):
    """Unit weights.  One joint: every pose is singular (one ray).  Random detections of two or more joints: none.  All J
    detections of a pose on one pixel: flagged when the ray is exactly representable (power-of-two K and pixel, as
    test_singular_least_squares_system_raises_like_torch_inverse builds it: sums of a ray that needs rounding do not cancel
    exactly, in the kernel as in the reference)."""
    g = np.random.Generator(np.random.Philox(key=[36, 0]))
    for N in (1, 5, 300):
        K = cameras(g, N)
        assert zh.reproj_degenerate(zh.reproj_prepare(dev((1000 * g.random((N, 1, 2))).astype(np.float32)), dev(K))) == N
        for J in (2, 16, 21, 40):
            assert zh.reproj_degenerate(zh.reproj_prepare(dev((1000 * g.random((N, J, 2))).astype(np.float32)), dev(K))) == 0
    for J in (2, 16, 21, 40):
        N = 5
        K = np.tile(np.array([[1024, 0, 512], [0, 1024, 512], [0, 0, 1]], np.float32), (N, 1, 1))
        uv = (1000 * g.random((N, J, 2))).astype(np.float32)
        uv[2] = np.array([768, 256], np.float32)                               # ray (0.25, -0.25, 1)
        uv[4] = np.array([512, 1024], np.float32)
        geom = zh.reproj_prepare(dev(uv), dev(K))
        assert np.array_equal(geom[2, :, :2].cpu().numpy(), np.tile(np.array([0.25, -0.25], np.float32), (J, 1)))
        assert zh.reproj_degenerate(geom) == 2


@pytest.mark.parametrize("J", [1, 5, 17, 21])
def test_rotate_init_at_other_joint_counts(zh, J):
    g = np.random.Generator(np.random.Philox(key=[37, J]))
    H, N = 3, 7
    x0 = g.standard_normal((H, J, 3)).astype(np.float32)
    R = g.standard_normal((H * N, 3, 3)).astype(np.float32)
    ref = np.einsum("bij,bkj->bki", R.astype(np.float64), np.repeat(x0, N, axis=0).astype(np.float64))
    x = zh.rotate_init(dev(x0), dev(R), N).cpu().numpy()
    assert x.shape == (H * N, J, 3)
    np.testing.assert_allclose(x, ref, atol=1e-6, rtol=0)
    lo, hi = 5, 18                                                             # a shard that starts and ends inside a hypothesis
    xs = zh.rotate_init(dev(x0), dev(R[lo:hi]), N, row_offset=lo).cpu().numpy()
    np.testing.assert_allclose(xs, ref[lo:hi], atol=1e-6, rtol=0)
    assert np.array_equal(xs, x[lo:hi])


# ---- 7. IPO --------------------------------------------------------------------------------------------------------------

IPO_IDS = [f"J{J}-k{len(kl)}" for J, kl in IPO_KEYS]


@pytest.mark.parametrize("axes", ["z", "xyz"])
@pytest.mark.parametrize("N", [8, 64])
@pytest.mark.parametrize("J,kl", IPO_KEYS, ids=IPO_IDS)
def test_ipo_single_iterations_from_the_oracle_state(zh, J, kl, N, axes):
    """The method of test_ipo_single_iterations_from_reference_state with the float64 oracle as the state source (the oracle's
    float64 run is pinned to the reference's to 1e-8 at 17 joints, key lists of 1 .. 17 joints): each of the first 50 Adam
    iterations on its own through zedo_ipo_fit_resume from the oracle's float64 state, |delta parameter| <= 1e-6 on poses whose
    residuals are all sign-unambiguous (|e| >= 1e-3 px; a key joint at the root contributes no gradient and is not counted); the
    second moments of the same pose-iterations by the rule of test_ipo_single_iterations_from_reference_state (_shared.MomentRule).
    uv is [N, J, 2] and x0 [1, J, 3] with J up to 33: key indices reach past 16, the strides are J."""
    worst, n_amb, rule_v = ipo_single_iterations_from_the_oracle(zh, J, kl, N, axes)          # the method, with its per-iteration assertion
    _report(dict(test="joint_counts_ipo", J=J, k=len(kl), N=N, axes=axes, ambiguous_pose_iterations=n_amb, max_param_delta=worst,
                 max_v_delta=rule_v.delta, fp32_oracle_v_delta=rule_v.delta32, v_bound=rule_v.bound, v_ratio=rule_v.ratio))
    assert n_amb <= 0.05 * 50 * N, n_amb
    assert worst > 0 or N * 50 == n_amb
    assert rule_v.holds() and (rule_v.largest > 0 or N * 50 == n_amb), (rule_v.delta, rule_v.bound)


def test_ipo_shard_equals_the_unsharded_rows(zh):
    """H = 3 hypotheses x N = 8 poses of 21 joints, 100 iterations: rows [5, 19) in a call of their own (row_offset) against the
    same rows of the whole batch, bit for bit - pose (row_offset + b) mod N and hypothesis (row_offset + b) / N index uv and x0
    with strides of J."""
    for J, kl in ((21, [0, 1, 4, 20]), (5, [0, 1, 2, 3, 4])):
        cl, uvn, Kn = make_ipo_problem(J, 8, H=3)
        x0, uv, K = dev(cl), dev(uvn), dev(Kn)
        norm = 8 * len(kl) * 2
        full = zh.ipo_fit(x0, uv, K, kl, "xyz", IPO_T, IPO_MIN, IPO_MAX, 100, norm, 24, return_params=True)
        part = zh.ipo_fit(x0, uv, K, kl, "xyz", IPO_T, IPO_MIN, IPO_MAX, 100, norm, 14, row_offset=5, return_params=True)
        for a, b in zip(full, part):
            assert bool(torch.isfinite(a).all()) and torch.equal(a[5:19], b)
        assert not torch.equal(full[0][0:8], full[0][8:16])                    # the hypotheses differ: h does select x0[h]


IPO_TWINS_J = r"""
import hashlib, json, os, sys
import numpy as np
root = %r
sys.path[:0] = [os.path.join(root, "zedo-release_amd"), os.path.join(root, "tests")]
import torch
import zedo_hip as zh
from _shared import IPO_KEYS, IPO_T, IPO_MIN, IPO_MAX, dev, make_ipo_problem
out = {}
for J, kl in IPO_KEYS:
    for N in (8, 64):
        cl, uv, K = make_ipo_problem(J, N, H=2)
        for axes in ("z", "xyz"):
            R, T, q, sc = zh.ipo_fit(dev(cl), dev(uv), dev(K), kl, axes, IPO_T, IPO_MIN, IPO_MAX, 500, N * len(kl) * 2, 2 * N, return_params=True)
            h = hashlib.sha256()
            for t in (R, T, q, sc):
                h.update(t.cpu().numpy().tobytes())
            out["J%%d_k%%d_N%%d_%%s" %% (J, len(kl), N, axes)] = h.hexdigest()
            assert bool(torch.isfinite(R).all())
print("RESULT " + json.dumps(out))
"""


def test_ipo_kernels_are_bitwise_twins_at_other_joint_counts():
    """test_ipo_kernels_are_bitwise_twins on the problems above at 500 iterations: the half-wave kernel and the lane-per-row kernel
    (ZEDO_IPO_KERNEL=half|row, read once per process; the row kernel is dispatched per key-list length) agree bit for bit in R, T, q
    and scale for 2 .. 33 joints."""
    res = {}
    for pin in ("half", "row"):
        e = dict(os.environ)
        e["ZEDO_IPO_KERNEL"] = pin
        r = subprocess.run([sys.executable, "-c", IPO_TWINS_J % ROOT], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        res[pin] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert len(res["half"]) == len(IPO_KEYS) * 4 and len(set(res["half"].values())) == len(res["half"])
    assert res["half"] == res["row"], {k: (v, res["row"][k]) for k, v in res["half"].items() if v != res["row"][k]}


# ---- 8. selection --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("J", [1, 2, 3, 5, 16, 17, 21])
def test_min_mpjpe_at_other_joint_counts(zh, J):
    """N = 23 poses x H = 11 hypotheses, a row shard with a ragged end and NaN rows: every row error against
    oracle.hypothesis_errors in float64, each row within the bound of tests/_procrustes_ref.py evaluated on these inputs (below
    1e-12 under both protocols, where P2 used to be held to 3e-7), the per-pose minimum and
    arg-min against numpy including the NaN rule.  Two joints are a rank-1 alignment, three a rank-2 one.  J = 1: P1 only (with
    alignment the reference raises: test_single_joint_alignment_is_nan)."""
    import zedo_oracle as O
    g = np.random.Generator(np.random.Philox(key=[38, J]))
    N, H, off = 23, 11, 17
    B = N * H - off - 5
    gt = 0.3 * g.standard_normal((N, J, 3))
    gt = gt - gt[:, 0:1]
    pose = (off + np.arange(B)) % N
    x = (gt[pose] + 0.05 * g.standard_normal((B, J, 3))).astype(np.float32)
    bad = np.zeros(B, bool)
    bad[[5, 100, 101, B - 1]] = True
    x[5, J // 2, 1] = np.nan
    x[[100, 101, B - 1]] = np.nan
    bounds = PR.bounds64(x[~bad], gt[pose[~bad]])
    for p2 in (False, True):
        if p2 and J == 1:
            continue
        err, best, best_h = zh.min_mpjpe(dev(x), dev(gt, torch.float64), N, procrustes=p2, row_offset=off)
        e = err.cpu().numpy()
        assert np.isnan(e[bad]).all() and np.isfinite(e[~bad]).all()
        ref = O.hypothesis_errors(x[~bad][:, None], gt[pose[~bad]], p2)[:, 0]
        d = np.abs(e[~bad] - ref)
        _report(dict(test="joint_counts_min_mpjpe", J=J, p2=p2, max_abs=float(d.max()), largest_share_of_bound=float((d / bounds[p2]).max()),
                     largest_bound=float(bounds[p2].max())))
        assert bounds[p2].max() < 1e-12 and (d <= bounds[p2]).all(), float((d / bounds[p2]).max())
        full = np.full(H * N, np.inf)
        full[off:off + B] = e
        held = np.zeros(H * N, bool)
        held[off:off + B] = True
        full, held = full.reshape(H, N), held.reshape(H, N)
        assert held.any(0).all()
        for n in range(N):
            col = np.where(held[:, n], full[:, n], np.inf)
            want_h = int(np.flatnonzero(np.isnan(col))[0]) if np.isnan(col).any() else int(np.argmin(col))
            assert int(best_h[n]) == want_h
            assert (np.isnan(col[want_h]) and np.isnan(float(best[n]))) or float(best[n]) == col[want_h]


@pytest.mark.parametrize("kernel", ["staged", "pose_major", "generic"])
def test_rank1_alignment_matches_the_reference_in_every_row_error_kernel(zh, golden, kernel):
    """The rank-1 captures (17 predicted joints on a coordinate axis, on a line in a random direction, both sets on lines:
    tests/golden/joint_counts.npz) through all three row-error kernels: row_error17_kernel (aligned rows, few poses),
    row_error17_pose_major_kernel (N >= 8192) and the generic kernel (a row pointer that is not 16-byte aligned).  P2 within 3e-7 of
    the reference's values (the capture's own distance from float64 - tests/test_hip_parity.py::test_min_mpjpe_golden - so that
    tolerance stays), and beside it within the bound of tests/_procrustes_ref.py of the float64 oracle on the same rows (its line
    form, 2 t1 the distance of BOTH sets' joints from their lines; where only one set is collinear it exceeds 3e-7, which then stays).  Before the rank-1 branch of polar_from_svd was written the exactly collinear cases came out with
    R = I: 0.456 / 0.407 / 0.392 against the reference's 0.432 / 0.393 / 0.389 (on an axis), 0.271 against 0.230 (both)."""
    g = golden("joint_counts")
    G = np.concatenate([g[f"r1_{t}_gt"] for t in ("axis", "dir", "both")])
    P = np.concatenate([g[f"r1_{t}_pred"] for t in ("axis", "dir", "both")]).astype(np.float32)
    ref = np.concatenate([g[f"r1_{t}_err_p2"] for t in ("axis", "dir", "both")])
    ref1 = np.concatenate([g[f"r1_{t}_err_p1"] for t in ("axis", "dir", "both")])
    reps = 920 if kernel == "pose_major" else 1                                # 9 x 920 = 8280 poses, one hypothesis
    G, P, ref, ref1 = np.tile(G, (reps, 1, 1)), np.tile(P, (reps, 1, 1)), np.tile(ref, reps), np.tile(ref1, reps)
    N = len(G)
    assert (N >= 8192) == (kernel == "pose_major")
    if kernel == "generic":
        buf = torch.empty(N * 51 + 1, dtype=torch.float32, device="cuda")
        x = buf[1:].view(N, 17, 3)
        x.copy_(dev(P))
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    else:
        x = dev(P)
        assert x.data_ptr() % 16 == 0
    err, best, best_h = zh.min_mpjpe(x, dev(G, torch.float64), N, procrustes=True)
    e = err.cpu().numpy()
    _report(dict(test="joint_counts_rank1", kernel=kernel, gpu=[float(v) for v in e[:9]], reference=[float(v) for v in ref[:9]]))
    np.testing.assert_allclose(e, ref, atol=3e-7, rtol=0)
    assert np.array_equal(best.cpu().numpy(), e) and (best_h.cpu().numpy() == 0).all()
    e1 = zh.min_mpjpe(x, dev(G, torch.float64), N, procrustes=False)[0].cpu().numpy()
    np.testing.assert_allclose(e1, ref1, atol=1e-12, rtol=0)
    import zedo_oracle as O
    b1, b2 = PR.bounds64(P[:9], G[:9])
    d1 = np.abs(e1 - np.tile(O.hypothesis_errors(P[:9, None], G[:9], False)[:, 0], reps))
    d2 = np.abs(e - np.tile(O.hypothesis_errors(P[:9, None], G[:9], True)[:, 0], reps))
    _report(dict(test="joint_counts_rank1_oracle", kernel=kernel, p2_max_abs=float(d2.max()), p2_largest_bound=float(b2.max())))
    b2 = np.minimum(b2, 3e-7)                                                  # (joints of one set on a line, the other thick: t1 is the thick set's)
    assert b2.min() < 1e-12 and b1.max() < 1e-12 and (d1 <= np.tile(b1, reps)).all() and (d2 <= np.tile(b2, reps)).all()


def test_single_joint_alignment_is_nan(zh, golden):
    """One joint with alignment: the reference's procrustes raises (numpy's SVD is handed 0 / 0; recorded in the fixture), so the
    call has no defined value there (include/zedo_hip.h).  The kernel returns without fault and writes NaN - the numpy-faithful
    reading of 0 / 0 - for every row, and NaN poisons each pose's minimum."""
    assert str(golden("joint_counts")["j1_p2_behaviour"]) == "raises LinAlgError"
    g = np.random.Generator(np.random.Philox(key=[39, 1]))
    N, H = 7, 3
    x = dev(g.standard_normal((N * H, 1, 3)).astype(np.float32))
    err, best, best_h = zh.min_mpjpe(x, dev(np.zeros((N, 1, 3)), torch.float64), N, procrustes=True)
    assert bool(torch.isnan(err).all()) and bool(torch.isnan(best).all()) and (best_h.cpu().numpy() == 0).all()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------

def test_sizes_an_entry_point_does_not_support_are_refused(zh, math_mode):
    """zedo_oil_run (J3 == 51) and zedo_reproj_grad (J == 17) return ZEDO_E_BADARG for other sizes and leave their outputs
    untouched; zedo_weights_create refuses J3 = 0 and 65; zedo_ipo_fit a key index == J and a key list of 18."""
    import ctypes
    import zedo_oracle as O
    lib = zh._lib
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    W = handle(zh, 19, 3, math_mode)
    s = zh.Schedule(W, O.oil_timestamps(10))
    x, T = torch.full((4, 19, 3), 0.25, device="cuda"), torch.full((4, 3), 5.0, device="cuda")
    geom, ws = torch.zeros(4, 19, 8, device="cuda"), zh.workspace(4)
    assert lib.zedo_oil_run(W._h, s._h, P(x), P(geom), P(T), 0, 5, 1, 4, 4, 0, P(ws), ws.numel(), None) == -1
    with pytest.raises(zh.ZedoError, match=r"code -1"):
        zh.oil_run(W, s, x, geom, T, 0, 5, 1)
    gout = torch.full((4, 19, 3), -7.0, device="cuda")
    assert lib.zedo_reproj_grad(P(x), P(geom), P(T), 1, P(gout), 4, 4, 19, 0, None) == -1
    with pytest.raises(zh.ZedoError, match=r"code -1"):
        zh.reproj_grad(x, geom, T, True)
    torch.cuda.synchronize()
    assert bool((x == 0.25).all()) and bool((T == 5.0).all()) and bool((gout == -7.0).all())
    # the control: the same calls are accepted at 17 x 3
    W17 = handle(zh, 17, 3, math_mode)
    assert lib.zedo_weights_get_math(W17._h) == zh.MATH_MODES[math_mode]
    for nj, jd in ((13, 5), (65, 1), (0, 3), (5, 0)):
        sd = {k: v for k, v in weights_of(17, 3).items()}
        sd["pre_dense.weight"] = np.zeros((1024, nj * jd), np.float32)
        sd["post_dense.weight"], sd["post_dense.bias"] = np.zeros((nj * jd, 1024), np.float32), np.zeros(nj * jd, np.float32)
        with pytest.raises(zh.ZedoError, match=r"code -1"):
            zh.Weights(sd, n_joints=nj, joint_dim=jd)
    cl, uv, K = make_ipo_problem(21, 8)
    args = (dev(cl), dev(uv), dev(K))
    zh.ipo_fit(*args, [0, 20], "z", IPO_T, IPO_MIN, IPO_MAX, 1, 32, 8)                      # index J - 1 is the last one accepted
    zh.ipo_fit(*args, list(range(17)), "z", IPO_T, IPO_MIN, IPO_MAX, 1, 272, 8)             # and seventeen keys the longest list
    for kl in ([0, 21], [-1, 3], list(range(18))):
        with pytest.raises(zh.ZedoError, match=r"code -1"):
            zh.ipo_fit(*args, kl, "z", IPO_T, IPO_MIN, IPO_MAX, 1, 16 * len(kl), 8)
