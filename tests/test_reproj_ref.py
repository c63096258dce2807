"""CPU: the float64 reference of the reprojection solve, its bound and its input families (tests/_reproj_ref.py) pinned without a GPU.
The two float64 routes agree; the fp32 statement of the kernel's formula uses at most a quarter of the bounds (which is where C_T and
C_g come from); the sign of T_z is never in doubt; and the bound tells the kernel's centred numerator from the algebraically equal
uncentred one, which every capture of the reference lets pass."""
import numpy as np
import pytest

import _reproj_ref as RR


@pytest.fixture(scope="module")
def fams():
    out = {}
    for name in RR.FAMILIES:
        f = RR.family(name)
        f["geom"] = RR.prepare(f["uv"], f["K"], f["conf"])
        f["ref"] = RR.solve(f["x"], f["geom"])
        out[name] = f
    return out


def test_families_are_what_they_claim(fams):
    assert len(set(RR.FAMILIES)) == len(RR.FAMILIES) == 17
    for name, f in fams.items():
        assert f["x"].shape == (RR.FAMILY_N * RR.FAMILY_H, 17, 3) and f["geom"].shape == (RR.FAMILY_N, 17, 8)
        assert all(np.isfinite(v).all() for v in (f["x"], f["geom"], f["ref"]["T"], f["ref"]["g"])), name
        W, lo = f["geom"][..., 2], (np.float32(1e-4) * np.float32(1e-4)) * (np.float32(1e-4) * np.float32(1e-4))
        if name.endswith("/none"):
            assert f["conf"] is None and (W == 1).all()
        elif "two" in name:
            assert ((W == 1).sum(1) == 2).all() and ((W == lo).sum(1) == 15).all(), name
        else:
            assert (f["conf"] > 1).any() and (f["conf"] < 1e-4).any() and W.max() == 1 and W.min() == lo, name
    two = fams["std/two-adjacent"]
    pair = np.argsort(-two["geom"][..., 2], axis=1)[:, :2]
    n = np.arange(RR.FAMILY_N)
    gap = np.linalg.norm(two["uv"][n, pair[:, 0]] - two["uv"][n, pair[:, 1]], axis=1)
    assert np.abs(gap - 3).max() < 1e-3
    assert np.abs(fams["offset/std"]["x"].mean((0, 1)) - RR.OFFSET).max() < 0.1


def test_two_float64_routes_agree(fams):
    for name, f in fams.items():
        ne = RR.solve_normal_equations(f["x"], f["geom"])
        T = f["ref"]["T"]
        assert (np.abs(ne - T) <= 1e-9 * (1 + np.abs(T))).all(), (name, float((np.abs(ne - T) / (1 + np.abs(T))).max()))


def test_emulation_within_a_quarter_of_the_bounds(fams):
    """... and the two constants are 4 x its largest share of the C = 1 bounds, rounded up: re-measured here."""
    worst_t = worst_g = 0.0
    for name, f in fams.items():
        Te, ge = RR.emulate_f32(f["x"], f["geom"])
        s = RR.shares(Te, ge, f["ref"])
        # g on its own: T given (the family's, and the emulation's own T), where only the C_g term of the bound applies
        sg = [s["g"]]
        for Tg in (f["T_given"], Te):
            Tb, gb = RR.emulate_f32(f["x"], f["geom"], T=Tg)
            assert np.array_equal(Tb, Tg)
            sg.append(RR.shares(Tb, gb, RR.solve(f["x"], f["geom"], T=Tg), given=True)["g"])
        print(f"{name:17s} emulate_f32 shares: T_z {s['tz']:.3f}  T_xy {s['txy']:.3f}  g {sg[0]:.3f}  g (T given) {sg[1]:.3f} {sg[2]:.3f}")
        assert max(s["tz"], s["txy"], *sg) <= 0.25, (name, s, sg)
        worst_t, worst_g = max(worst_t, s["tz"] * RR.C_T, s["txy"] * RR.C_T), max(worst_g, sg[1] * RR.C_G, sg[2] * RR.C_G)
    print(f"largest share of the C = 1 bounds: T {worst_t:.3f}, g {worst_g:.3f}; C_T = {RR.C_T}, C_g = {RR.C_G}")
    assert worst_t <= RR.EMUL_SHARE_T and worst_g <= RR.EMUL_SHARE_G               # the recorded figures are the measured ones, rounded up
    assert RR.C_T == int(np.ceil(4 * worst_t)) and RR.C_G == int(np.ceil(4 * worst_g))


def test_sign_of_tz_is_never_in_doubt(fams):
    for name, f in fams.items():
        ratio = np.abs(f["ref"]["T_unfixed"][:, 2]) / f["ref"]["bound_Tz"]
        assert ratio.min() >= RR.SIGN_MARGIN, (name, float(ratio.min()))
        assert (f["ref"]["T"][:, 2] > 0).all()
    assert (fams["mirrored"]["ref"]["T_unfixed"][:, 2] < 0).all()
    assert np.array_equal(fams["mirrored"]["ref"]["T"], -fams["mirrored"]["ref"]["T_unfixed"])


def test_bound_separates_the_uncentred_numerator(fams):
    """d_x b_x + d_y b_y instead of d_x (b_x - bbar_x) + d_y (b_y - bbar_y): equal in exact arithmetic, outside the bound in fp32 on
    every family with two confident joints, a far subject or a pose away from the origin."""
    assert len(RR.UNCENTRED_MUST_FAIL) == 9
    for name in RR.UNCENTRED_MUST_FAIL:
        f = fams[name]
        s = RR.shares(*RR.emulate_f32(f["x"], f["geom"], variant="uncentred"), f["ref"])
        print(f"{name:17s} uncentred shares: T_z {s['tz']:.2f}  T_xy {s['txy']:.2f}")
        assert max(s["tz"], s["txy"]) > 1.0, (name, s)
