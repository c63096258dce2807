"""GPU: the least-squares T that the FUSED reprojection epilogues of zedo_oil_run write - post_reduce_kernel, the EPI_SDE epilogue of the
32x64 and 64x64 fp32 post_dense tiles, the epilogue of layer16_post_kernel (f16x3 mode: all shapes) - against the float64 solve of
tests/_reproj_ref.py on the very state it was computed from, and against the standalone zedo_reproj_grad bit for bit.  Until now the fused
forms were compared with each other and with the unfused launch only; inside long loops they are held to a criterion 1e-5 to 1e-3 m wide.
Runs in both arithmetic modes of the dense layers (the launch form depends on it); the standalone kernel: tests/test_reproj_accuracy_gpu.py.

Two iterations of a 7-step schedule: zedo_oil_run(0, 2, switch_step) = [reproj_step_kernel on x0] -> step 0 -> [fused correction on x1,
writes T] -> step 1.  The same from surface calls: g0 = zedo_reproj_grad(x0), x1 = zedo_sde_step(0, x0 + g0), g1 = zedo_reproj_grad(x1),
x = zedo_sde_step(1, x1 + g1)."""
import numpy as np
import pytest

import _reproj_ref as RR
from _shared import W, dev, report_env as _report, zh  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (N, H) -> B = N H: post_reduce_kernel with one ragged tile / at its largest size (POST_SPLIT_ROWS), 32x64 fp32 tiles (Mp = 2112), 64x64
# fp32 tiles (Mp = 8320); in the f16x3 session layer16_post_kernel serves all four
SHAPES = [(70, 1), (128, 16), (70, 30), (83, 100)]
FORM = {70: "post_reduce_kernel (one tile)", 2048: "post_reduce_kernel (2048 rows)", 2100: "post_dense 32x64 tiles", 8300: "post_dense 64x64 tiles"}


def run_both_ways(zh, W, math_mode, name, N, H, row_offset=0, switch_step=0, tag=""):
    import zedo_oracle as O
    B = N * H
    f = RR.family(name, N=N, H=H + 1)                                             # one hypothesis more: a shard starts row_offset rows in
    x0, T0 = f["x"][row_offset:row_offset + B], f["T_given"][row_offset:row_offset + B]
    geom = zh.reproj_prepare(dev(f["uv"]), dev(f["K"]), dev(f["conf"]))
    sched = zh.Schedule(W, O.oil_timestamps(7))
    xbuf, Tbuf = torch.full((B + 8, 17, 3), -7.0, device="cuda"), torch.full((B + 8, 3), -7.0, device="cuda")
    x, T = xbuf[:B], Tbuf[:B]
    x.copy_(dev(x0))
    T.copy_(dev(T0))
    zh.oil_run(W, sched, x, geom, T, 0, 2, switch_step, row_offset)
    # the same from the surface calls
    xs, Ts = dev(x0), dev(T0)
    x1 = xs + zh.reproj_grad(xs, geom, Ts, switch_step <= 0, row_offset)
    zh.sde_step(W, sched, 0, x1)
    T1 = torch.full((B, 3), float("nan"), device="cuda")
    xe = x1 + zh.reproj_grad(x1, geom, T1, True, row_offset)
    zh.sde_step(W, sched, 1, xe)
    ref = RR.solve(x1.cpu().numpy(), geom.cpu().numpy(), row_offset=row_offset)
    Th = T.cpu().numpy()
    dz, dxy = np.abs(Th[:, 2] - ref["T"][:, 2]) / ref["bound_Tz"], np.abs(Th[:, :2] - ref["T"][:, :2]).max(1) / ref["bound_Txy"]
    _report(dict(test="reproj_accuracy", form=("layer16_post_kernel" if math_mode == "f16x3" else FORM[B]) + tag, B=B, family=name,
                 share_tz=float(dz.max()), share_txy=float(dxy.max()), bits_equal_standalone=bool(torch.equal(T, T1)),
                 min_sign_margin=float((np.abs(ref["T_unfixed"][:, 2]) / ref["bound_Tz"]).min())))
    assert torch.isfinite(x).all() and torch.isfinite(T).all()
    assert (np.abs(ref["T_unfixed"][:, 2]) >= RR.SIGN_MARGIN * ref["bound_Tz"]).all()      # the sign is not in doubt on x1 either: every row counts
    assert torch.equal(T, T1), "the fused epilogue and zedo_reproj_grad solve different T from the same state"
    assert (dz <= 1.0).all() and (dxy <= 1.0).all(), (float(dz.max()), float(dxy.max()))
    assert torch.equal(x, xe), "the state after the fused correction and step 1 differs from the rebuilt one"
    assert bool((xbuf[B:] == -7).all()) and bool((Tbuf[B:] == -7).all())
    if switch_step > 0:                                                           # the first correction used the given T, not a solved one
        assert not torch.equal(x1, dev(x0) + zh.reproj_grad(dev(x0), geom, dev(T0), True, row_offset))


@pytest.mark.parametrize("name", ["std/uniform", "std/two"])
@pytest.mark.parametrize("N,H", SHAPES)
def test_fused_T_is_the_standalone_T_and_within_the_bounds_of_float64(zh, W, math_mode, N, H, name):
    run_both_ways(zh, W, math_mode, name, N, H)


def test_fused_T_of_a_row_shard(zh, W, math_mode):
    run_both_ways(zh, W, math_mode, "std/two", 70, 30, row_offset=35, tag=", row_offset 35")


def test_fused_T_when_only_the_fused_correction_solves(zh, W, math_mode):
    run_both_ways(zh, W, math_mode, "std/uniform", 70, 30, switch_step=1, tag=", switch_step 1")
