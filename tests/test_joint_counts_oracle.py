"""Pins the numpy oracle against captures of the reference on skeletons OTHER than 17 joints x 3 coordinates
(tests/golden/joint_counts.npz, tools/gen_golden.py::gen_joint_counts): the network for seven (n_joints, joint_dim) sizes up
to the 64 coordinates the C ABI accepts, MPJPE / Procrustes-aligned MPJPE for 2, 3, 5, 16 and 21 joints, and rank-1
alignments.  CPU only.  This is what licenses the oracle as the arbiter of tests/test_joint_counts_gpu.py; tolerances are
the ones tests/test_oracle_golden.py applies to the 17-joint captures."""
import numpy as np
import pytest

import zedo_oracle as O
from lib.dataset import synthetic as syn

SIZES = [(1, 1), (1, 3), (16, 3), (14, 4), (19, 3), (21, 3), (16, 4)]


@pytest.mark.parametrize("nj,jd", SIZES)
def test_score_network_forward_at_other_sizes(golden, nj, jd):
    g = golden("joint_counts")
    assert [tuple(s) for s in g["sizes"]] == SIZES
    tag = f"{nj}x{jd}"
    w = syn.make_weights(seed=0, n_joints=nj, joint_dim=jd)
    assert syn.weights_checksum(w) == str(g[f"sha_{tag}"])
    assert w["pre_dense.weight"].shape == (1024, nj * jd) and w["post_dense.weight"].shape == (nj * jd, 1024)
    x = g[f"x_{tag}"]
    assert x.shape == (8, nj, jd)
    w64 = O.cast_weights(w, np.float64)
    for i, t in enumerate(g["ts"]):
        eps = O.score_model_forward(w, x, np.float32(t) * np.float32(999))
        assert eps.shape == x.shape and eps.dtype == np.float32
        np.testing.assert_allclose(eps, g[f"eps_{tag}"][i], atol=1e-6, rtol=0)
        # the float64 oracle against the reference's .double() model (labels formed in fp32, as the capture forms them)
        e64 = O.score_model_forward(w64, x.astype(np.float64), np.float64(np.float32(t) * np.float32(999)), dtype=np.float64)
        np.testing.assert_allclose(e64, g[f"eps64_{tag}"][i], atol=1e-6, rtol=0)


@pytest.mark.parametrize("J", [2, 3, 5, 16, 21])
def test_hypothesis_errors_at_other_joint_counts(golden, J):
    g = golden("joint_counts")
    G, P = g[f"gt_j{J}"], g[f"pred_j{J}"]
    assert G.shape == (6, J, 3) and P.shape == (6, 4, J, 3) and P.dtype == np.float32
    np.testing.assert_allclose(O.hypothesis_errors(P, G, False), g[f"err_p1_j{J}"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(O.hypothesis_errors(P, G, True), g[f"err_p2_j{J}"], atol=2e-7, rtol=0)
    assert (g[f"err_p2_j{J}"][::3, 3] < 1e-6).all()          # the mirrored hypothesis was aligned with a reflection


@pytest.mark.parametrize("tag", ["axis", "dir", "both"])
def test_rank1_procrustes_error_is_pinned(golden, tag):
    """A0^T B0 with ONE non-zero singular value: 17 predicted joints on a line (exactly on a coordinate axis; in a random
    direction, collinear to fp32 rounding), and both sets on lines.  LAPACK completes the two null directions arbitrarily, but
    the error has one value: the aligned pose has no component along the null directions of the ground truth."""
    g = golden("joint_counts")
    G, P, ref = g[f"r1_{tag}_gt"], g[f"r1_{tag}_pred"], g[f"r1_{tag}_err_p2"]
    assert G.shape == P.shape == (3, 17, 3)
    for n in range(3):
        A0, B0 = G[n] - G[n].mean(0), P[n].astype(np.float64) - P[n].astype(np.float64).mean(0)
        s = np.linalg.svd((A0 / np.linalg.norm(A0)).T @ (B0 / np.linalg.norm(B0)), compute_uv=False)
        assert s[1] <= 1e-6 * s[0], (n, s)                    # rank 1 (exactly, or to fp32 rounding of the prediction)
    np.testing.assert_allclose(O.hypothesis_errors(P[:, None], G, False)[:, 0], g[f"r1_{tag}_err_p1"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(O.hypothesis_errors(P[:, None], G, True)[:, 0], ref, atol=2e-7, rtol=0)
    assert ref.min() > 1e-3                                   # a line cannot be aligned onto a pose: the error is not small


def test_single_joint_alignment_raises_in_the_reference_and_in_the_oracle(golden):
    """One joint: centring leaves nothing, both norms are zero and the SVD is handed 0 / 0.  The reference's procrustes raises
    there (recorded by the capture script); so does the oracle.  P1 is well defined."""
    g = golden("joint_counts")
    assert str(g["j1_p2_behaviour"]) == "raises LinAlgError" and "j1_err_p2" not in g.files
    G, P = np.zeros((1, 1, 3)), np.array([[[[0.1, -0.2, 0.05]]]], np.float32)
    assert abs(O.hypothesis_errors(P, G, False)[0, 0] - float(g["j1_err_p1"])) <= 1e-12
    with np.errstate(all="ignore"), pytest.raises(np.linalg.LinAlgError):
        O.hypothesis_errors(P, G, True)
