"""GPU: the row errors of zedo_min_mpjpe / zedo_min_mpjpe_both against the 50-digit fixture tests/golden/procrustes_hp.npz, every row
within the bound of tests/_procrustes_ref.py (derived there; its constants come from the float64 numpy oracle, never from a kernel),
through all three row-error kernels.  The fixture is what no other test has: singular values between comfortably full rank and
exactly deficient (ladders across the 1e-14 rank test of polar_from_svd), equal singular values, reflections, errors of 1e-8 m formed
from 0.3 m quantities, poses kilometres from the origin, millimetres against metres.  tests/test_procrustes_ref.py pins the fixture and
the bound on the CPU; the largest share of the bound each kernel uses per family is reported (profiles/procrustes_accuracy.txt)."""
import numpy as np
import pytest

import _procrustes_ref as PR
from _invariance import misaligned
from _shared import dev, one_arithmetic_mode, report_env as _report, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H = PR.H
POSE_MAJOR_N = 8192                                                  # POSE_MIN_LANE_N of zedo_metric.hip


@pytest.fixture(scope="module")
def hp():
    fx = PR.load()
    fx["b1"], fx["b2"] = PR.row_bounds(fx)
    fx["groups"] = PR.groups(fx)
    return fx


def unaligned(a):
    """a [B,J,3] fp32 on the device behind a pointer 4 bytes off 16-byte alignment: the generic kernel's dispatch condition."""
    return misaligned(dev(a), floats=1)


def operands(hp, kernel):
    """[(J, fixture rows in local order, x on the device, gt [N,J,3], N)] that reach `kernel` in launch_row_errors."""
    out = []
    for J, (rows, pred, gt) in hp["groups"].items():
        N = len(gt)
        if kernel == "generic" and J != 17:
            out.append((J, rows, dev(pred), gt, N))
        elif kernel == "generic_unaligned" and J == 17:
            out.append((J, rows, unaligned(pred), gt, N))
        elif kernel == "staged" and J == 17:
            out.append((J, rows, dev(pred), gt, N))
        elif kernel == "pose_major" and J == 17:
            reps = -(-POSE_MAJOR_N // N)                              # the 17-joint poses tiled: pose n of the call is pose n mod N here
            idx = np.tile(np.arange(H * N).reshape(H, 1, N), (1, reps, 1)).reshape(-1)
            out.append((J, rows[idx], dev(pred[idx]), np.tile(gt, (reps, 1, 1)), reps * N))
    for J, rows, x, gt, N in out:
        assert (N >= POSE_MAJOR_N) == (kernel == "pose_major") and N < 2 * POSE_MAJOR_N
        assert (x.data_ptr() % 16 == 0) == (kernel != "generic_unaligned") and len(rows) == H * N == x.shape[0]
    return out


KERNELS = ["generic", "generic_unaligned", "staged", "pose_major"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_row_errors_minimum_and_argmin_against_50_digits(zh, hp, kernel):
    """Every row's P1 and P2 within the bound of the 50-digit value; the per-pose minimum is the error of the reference's arg-min row
    (hence within that row's bound of the reference minimum), the arg-min exact - the runner-up is 100 bounds away
    (tests/test_procrustes_ref.py).  zedo_min_mpjpe_both gives the bits of the two single calls on the same rows."""
    ops = operands(hp, kernel)
    seen = np.zeros(len(hp["J"]), bool)
    share = {p: {} for p in ("p1", "p2")}
    for J, rows, x, gt, N in ops:
        g = dev(gt, torch.float64)
        both = [t.cpu().numpy() for t in zh.min_mpjpe_both(x, g, N)]
        for slot, (p, key, bkey) in enumerate((("p1", "err_p1_hp", "b1"), ("p2", "err_p2_hp", "b2"))):
            err, best, best_h = (t.cpu().numpy() for t in zh.min_mpjpe(x, g, N, procrustes=bool(slot)))
            ref, bound = hp[key][rows], hp[bkey][rows]
            used = np.abs(err - ref) / bound
            for fam in np.unique(hp["family"][rows]):
                m = hp["family"][rows] == fam
                share[p][int(fam)] = max(share[p].get(int(fam), 0.0), float(used[m].max()))
            print(f"{kernel} J={J} {p}: max |d| {np.abs(err - ref).max():.3e}, largest share of the bound {used.max():.3f}")
            assert np.isfinite(err).all() and (used <= 1.0).all(), (J, p, rows[np.argmax(used)], float(used.max()))
            want_h = ref.reshape(H, N).argmin(0)
            assert np.array_equal(best_h, want_h), (J, p, np.flatnonzero(best_h != want_h)[:8])
            win = want_h * N + np.arange(N)
            assert np.array_equal(best, err[win]) and (np.abs(best - ref.reshape(H, N).min(0)) <= bound[win]).all()
            assert np.array_equal(both[0][slot], err) and np.array_equal(both[1][slot], best) and np.array_equal(both[2][slot], best_h)
        seen[rows] = True
    want_rows = (hp["J"] != 17) if kernel == "generic" else (hp["J"] == 17)
    assert np.array_equal(seen, want_rows) and seen.any()             # no row of the fixture is left out of the comparison
    _report(dict(test="procrustes_hp", kernel=kernel, rows=int(sum(len(o[1]) for o in ops)),
                 p1_share_by_family=share["p1"], p2_share_by_family=share["p2"]))


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_shard_that_starts_inside_a_wave_gives_the_bits_of_the_full_call(zh, hp, kernel):
    """Local rows [off, off + B) of the calls above in a call of their own (row_offset = off, no multiple of 64, a ragged end): the same
    bits for the rows the shard holds, single calls and zedo_min_mpjpe_both alike."""
    for J, rows, x, gt, N in operands(hp, kernel):
        g = dev(gt, torch.float64)
        full = zh.min_mpjpe_both(x, g, N)[0].cpu().numpy()
        off, tail = (N + 100, 5) if N >= POSE_MAJOR_N else (40, 5) if len(rows) > 100 else (3, 1)
        B = len(rows) - off - tail
        assert off % 64 and B > N
        xs = unaligned(x[off:off + B].cpu().numpy()) if kernel == "generic_unaligned" else x[off:off + B].clone()
        assert (xs.data_ptr() % 16 == 0) == (kernel != "generic_unaligned")
        part = zh.min_mpjpe_both(xs, g, N, row_offset=off)[0].cpu().numpy()
        assert np.isfinite(part).all() and np.array_equal(part, full[:, off:off + B])
        for slot in (0, 1):
            one = zh.min_mpjpe(xs, g, N, procrustes=bool(slot), row_offset=off)[0].cpu().numpy()
            assert np.array_equal(one, full[slot, off:off + B])
