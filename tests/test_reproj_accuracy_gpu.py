"""GPU: zedo_reproj_grad (reproj_grad_kernel, csrc/zedo_geom.hip) against the float64 solve of tests/_reproj_ref.py on the geom array
the device itself prepared, every row within the bound derived there (its constants come from the fp32 numpy statement of the formula,
never from a kernel; tests/test_reproj_ref.py pins reference, bound and families on the CPU).  What no capture of the reference has:
weights that span 16 decades, subjects 50 m away, poses away from the origin, two confident detections 3 px apart, more than one
workgroup, a ragged last workgroup, row shards (row_offset != 0), a NaN confidence next to healthy poses.  The fused launch forms of the
same source: tests/test_reproj_fused_gpu.py.  The largest share of each bound per family is reported (profiles/reproj_accuracy.txt)."""
import numpy as np
import pytest

import _reproj_ref as RR
from _shared import dev, one_arithmetic_mode, report_env as _report, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def on_device(zh, f):
    """geom of a family as the device prepares it: the tensor and its exact copy on the host."""
    geom = zh.reproj_prepare(dev(f["uv"]), dev(f["K"]), None if f["conf"] is None else dev(f["conf"]))
    return geom, geom.cpu().numpy()


@pytest.fixture(scope="module")
def fams(zh):
    out = {}
    for name in RR.FAMILIES:
        f = RR.family(name)
        f["geom_d"], f["geom"] = on_device(zh, f)
        out[name] = f
    return out


def grad(zh, x, geom, T=None, row_offset=0):
    """zedo_reproj_grad -> (T, g) on the host; T None: solved (the buffer starts as NaN: every row must be written)."""
    Td = torch.full((len(x), 3), float("nan"), device="cuda") if T is None else dev(T)
    g = zh.reproj_grad(dev(x), geom, Td, T is None, row_offset)
    return Td.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("name", RR.FAMILIES)
def test_solved_T_and_g_within_the_bounds_of_float64(zh, fams, name):
    f = fams[name]
    assert len(f["x"]) == 201
    ref = RR.solve(f["x"], f["geom"])
    T, g = grad(zh, f["x"], f["geom_d"])
    s = RR.shares(T, g, ref)
    _report(dict(test="reproj_accuracy", form="reproj_grad_kernel solve", family=name, share_tz=s["tz"], share_txy=s["txy"], share_g=s["g"],
                 max_abs_dT=float(np.abs(T - ref["T"]).max()), max_abs_dg=float(np.abs(g - ref["g"]).max())))
    RR.assert_within(T, g, ref)                                                    # every row: the sign margin holds with the device's rays too


@pytest.mark.parametrize("name", RR.FAMILIES)
def test_given_T_comes_back_and_g_within_the_bound(zh, fams, name):
    f = fams[name]
    ref = RR.solve(f["x"], f["geom"], T=f["T_given"])
    T, g = grad(zh, f["x"], f["geom_d"], T=f["T_given"])
    assert np.array_equal(T, f["T_given"])
    bound = RR.C_G * RR.U24 * np.abs(f["x"].astype(np.float64) + f["T_given"].astype(np.float64)[:, None]).sum(-1)
    assert np.array_equal(bound, ref["bound_g"])
    s = RR.shares(T, g, ref, given=True)
    _report(dict(test="reproj_accuracy", form="reproj_grad_kernel T given", family=name, share_g=s["g"]))
    assert (np.abs(g - ref["g"]) <= bound[..., None]).all(), s


def test_sign_fix_on_mirrored_detections(zh, fams):
    f = fams["mirrored"]
    ref = RR.solve(f["x"], f["geom"])
    assert (ref["T_unfixed"][:, 2] < 0).all()
    T, _ = grad(zh, f["x"], f["geom_d"])
    assert (T[:, 2] > 0).all()
    d = np.abs(T + ref["T_unfixed"])
    assert (d[:, 2] <= ref["bound_Tz"]).all() and (d[:, :2] <= ref["bound_Txy"][:, None]).all()


@pytest.mark.parametrize("B", [1, 127, 128, 129, 300])
def test_every_row_of_a_launch_gives_the_bits_of_a_call_of_its_own(zh, B):
    """Rows 128 and above of a launch and the last partial workgroup: every row once more alone, as a B = 1 call at row_offset = b."""
    f = RR.family("std/uniform", N=50, H=6)
    geom, _ = on_device(zh, f)
    x = f["x"][:B]
    T, g = grad(zh, x, geom)
    assert np.isfinite(T).all() and np.isfinite(g).all()
    for b in range(B):
        T1, g1 = grad(zh, x[b:b + 1], geom, row_offset=b)
        assert np.array_equal(T1[0], T[b]) and np.array_equal(g1[0], g[b]), b


@pytest.mark.parametrize("solve", [True, False])
def test_row_shards_give_the_bits_of_the_whole_call_and_write_nothing_else(zh, solve):
    N, H = 50, 6
    f = RR.family("std/uniform", N=N, H=H)
    geom, _ = on_device(zh, f)
    full_T, full_g = grad(zh, f["x"], geom, None if solve else f["T_given"])
    for off in (0, 1, N - 1, N, 2 * N + 5):
        B = min(131, N * H - off)
        x = torch.full((B + 8, 17, 3), -7.0, device="cuda")
        T = torch.full((B + 8, 3), -7.0, device="cuda")
        x[:B] = dev(f["x"][off:off + B])
        if not solve:
            T[:B] = dev(f["T_given"][off:off + B])
        g = torch.full((B + 8, 17, 3), -7.0, device="cuda")
        # zh.reproj_grad allocates g itself: the C entry point, so that the caller's g has spare rows as well
        zh._check(zh._lib.zedo_reproj_grad(zh._p(x), zh._p(geom), zh._p(T), int(solve), zh._p(g), B, N, 17, off, zh._stream()))
        T, g = T.cpu().numpy(), g.cpu().numpy()
        assert np.array_equal(T[:B], full_T[off:off + B]) and np.array_equal(g[:B], full_g[off:off + B]), off
        assert (T[B:] == -7).all() and (g[B:] == -7).all() and bool((x[B:] == -7).all()), off
        if off % N:                                                                # the shard is not the whole call's first rows over again
            assert not np.array_equal(g[:B], full_g[:B])


def test_a_nan_confidence_stays_inside_its_pose(zh):
    f = RR.family("std/uniform")
    N, H = f["N"], f["H"]
    geom, _ = on_device(zh, f)
    clean_T, clean_g = grad(zh, f["x"], geom)
    conf = f["conf"].copy()
    bad = 41
    conf[bad, 5] = np.nan
    geom_bad = zh.reproj_prepare(dev(f["uv"]), dev(f["K"]), dev(conf))
    assert zh.reproj_degenerate(geom_bad) == 0                                     # NaN is not "singular": the count is of den == 0
    T, g = grad(zh, f["x"], geom_bad)
    rows = np.arange(N * H) % N == bad
    assert rows.sum() == H and np.isnan(T[rows]).all() and np.isnan(g[rows]).all()
    assert np.array_equal(T[~rows], clean_T[~rows]) and np.array_equal(g[~rows], clean_g[~rows])


def test_singular_count_is_the_number_of_poses_with_a_non_finite_T(zh):
    """Exactly singular poses (every detection on one pixel whose ray is exactly representable: power-of-two K and pixel), poses whose
    two confident detections are 3 px apart (nearly singular: finite T, not counted) and ordinary ones, in one call."""
    adj, std = RR.family("std/two-adjacent", N=20, H=1), RR.family("std/none", N=20, H=1)
    N = 45
    uv = np.concatenate([adj["uv"], std["uv"], np.zeros((5, 17, 2), np.float32)])
    K = np.concatenate([adj["K"], std["K"], np.tile(np.array([[1024, 0, 512], [0, 1024, 512], [0, 0, 1]], np.float32), (5, 1, 1))])
    conf = np.concatenate([adj["conf"], np.ones((25, 17), np.float32)])
    uv[40:] = np.array([[768, 256], [512, 1024], [512, 512], [0, 0], [1536, 768]], np.float32)[:, None]
    x = np.concatenate([adj["x"], std["x"], std["x"][:5]])
    order = np.random.Generator(np.random.Philox(key=[61, 100])).permutation(N)    # the singular poses are not the last ones
    uv, K, conf, x = uv[order], K[order], conf[order], x[order]
    singular = order >= 40
    geom = zh.reproj_prepare(dev(uv), dev(K), dev(conf))
    T, g = grad(zh, x, geom)
    assert np.array_equal(~np.isfinite(T).all(1), singular)
    assert zh.reproj_degenerate(geom) == int(singular.sum()) == 5
    ref = RR.solve(x[~singular], geom.cpu().numpy()[~singular])
    assert (np.abs(T[~singular][:, 2] - ref["T"][:, 2]) <= ref["bound_Tz"]).all()
    assert (np.abs(T[~singular][:, :2] - ref["T"][:, :2]) <= ref["bound_Txy"][:, None]).all()
