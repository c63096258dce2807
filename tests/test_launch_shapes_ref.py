"""The inputs of tests/test_launch_shapes_gpu.py, validated without a device: on the base block of the periodic batch the oracle
run in fp32 is well inside the bound the GPU result is held to, so the bound measures the kernels and not the inputs."""
import numpy as np

from _shared import LS_EDGE_ROWS, LS_P, LS_TS, launch_shape_base, launch_shape_reference64


def test_the_fp32_oracle_uses_at_most_half_of_the_bound_on_the_base_block(weights0):
    """Bound of the GPU test (the rule of the parity tests): max |error| <= 2e-6 max(1, max |ref|) per noise level, every row.  The
    fp32 numpy oracle - the same layers with numpy's summation order - must be within HALF of it of the float64 oracle, the edge
    rows included (measured: 2.9e-7 at the worst, row 12 at t = 0.1; the edge rows are not the worst)."""
    import zedo_oracle as O
    base = launch_shape_base()
    assert base.shape == (LS_P, 17, 3) and base.dtype == np.float32 and len(LS_EDGE_ROWS) == 8
    assert not base[3].any() and (base[43] == 5.0).all() and np.array_equal(base[59], -base[53])
    ref = launch_shape_reference64(weights0, base)
    assert np.isfinite(ref).all()
    for i, t in enumerate(LS_TS):
        e32 = O.score_model_forward(weights0, base, np.float32(t) * np.float32(999))
        d = np.abs(e32.astype(np.float64) - ref[i]).reshape(LS_P, -1).max(1)
        bound = 2e-6 * max(1.0, float(np.abs(ref[i]).max()))
        print(f"t = {t}: fp32 oracle {d.max():.3e} from float64 (row {int(d.argmax())}), bound {bound:.3e}, max |ref| {np.abs(ref[i]).max():.3f}")
        assert d.max() <= 0.5 * bound, (float(t), int(d.argmax()), float(d.max()), bound)
