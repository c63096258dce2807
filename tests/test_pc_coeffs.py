"""CPU: the per-step scalars of the native predictor-corrector route (lib/algorithms/advanced/_pc_coeffs.py).

Every registered predictor is x_mean = A x + B score, x_new = x_mean + C z and every corrector step is
x_mean = x + s score, x = x_mean + sqrt(2 s) z; the module derives A, B, C, s (and the label / net_scale that turn the
network's output into the score) from the sde object's own methods, folds them in float64 and rounds once.  Applied in
fp32 to the inputs of tests/golden/samplers.npz (captured from the reference: tools/gen_golden.py::gen_samplers) they
must reproduce what the reference's update rules gave, under the rule the generic surface is held to
(tests/test_surface_gpu.py::test_pc_sampler_other_sdes_and_update_rules): max|d| < 1e-6 max(1, max|ref|)."""
import numpy as np
import pytest
import torch

from _shared import host_lib, make_sde, sampler_cases
from lib.algorithms.advanced import _pc_coeffs, sampling, sde_lib
from lib.algorithms.advanced import utils as mutils

SDES, PREDS, CORRS = sampler_cases()
SNR, N_CORR = 0.16, 2          # what gen_samplers ran the correctors with


def noise(k, shape):
    """draw k of the capture's DetNoise stream, as fp32"""
    return np.random.Generator(np.random.Philox(key=[555, k])).standard_normal(shape).astype(np.float32)


def analytic_score(x, cond, t):
    return (-(x - np.float32(0.3) * cond) / (np.float32(0.5) + t)[:, None, None]).astype(np.float32)


def coeffs(sde, pname, cname, pf, ts, continuous=True, snr=SNR, n_steps=N_CORR, sbs=False, sigmas=None):
    return _pc_coeffs.coefficients(sde, sampling.get_predictor(pname), sampling.get_corrector(cname), pf, continuous, snr,
                                   n_steps, sbs, sigmas, ts)


def check(tag, got, ref):
    scale = max(1.0, float(np.abs(ref).max()))
    d = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"pc_coeffs[{tag}]: max|d| {d:.2e} = {d / scale:.2e} of scale {scale:.3g}")
    assert d < 1e-6 * scale, (tag, d, scale)


def col(v):
    return v.astype(np.float32)[:, None, None]


@pytest.mark.parametrize("name", SDES)
@pytest.mark.parametrize("pname,pf", PREDS)
def test_predictor_coefficients_reproduce_the_reference(golden, name, pname, pf):
    g = golden("samplers")
    sde = make_sde(sde_lib, name)
    key = f"{name}_pred_{pname}_pf{int(pf)}"
    c = coeffs(sde, pname, "none", pf, g["t"])
    if key + "_raises" in g.files:
        assert c is None
        return
    assert c is not None and c.has_predictor and c.n_corr == 0 and c.corr is None
    for a in (c.label, c.net_scale, c.pA, c.pB, c.pC):
        assert a.dtype == np.float32 and a.shape == g["t"].shape
    x, score = g["x"], analytic_score(g["x"], g["cond"], g["t"])
    x_mean = col(c.pA) * x + col(c.pB) * score
    x_new = x_mean + col(c.pC) * noise(0, x.shape)
    check(key + "_mean", x_mean, g[key + "_mean"])
    check(key + "_x", x_new, g[key + "_x"])
    if pf:
        assert not c.pC.any()


@pytest.mark.parametrize("name", SDES)
@pytest.mark.parametrize("cname", CORRS)
def test_corrector_coefficients_reproduce_the_reference(golden, name, cname):
    g = golden("samplers")
    sde = make_sde(sde_lib, name)
    key = f"{name}_corr_{cname}"
    c = coeffs(sde, "none", cname, False, g["t"])
    if key + "_raises" in g.files:
        assert c is None
        return
    assert c is not None and not c.has_predictor and c.n_corr == N_CORR
    assert c.corrector == dict(langevin=_pc_coeffs.CORR_LANGEVIN, ald=_pc_coeffs.CORR_ALD)[cname]
    x = g["x"]
    for k in range(N_CORR):
        score, z = analytic_score(x, g["cond"], g["t"]), noise(k, x.shape)
        if cname == "ald":
            s = c.corr
        else:       # s = factor (mean ||z|| / mean ||score||)^2 with the means over the batch, in fp32
            gn = np.sqrt((score.reshape(len(x), -1) ** 2).sum(1, dtype=np.float32)).mean(dtype=np.float32)
            zn = np.sqrt((z.reshape(len(x), -1) ** 2).sum(1, dtype=np.float32)).mean(dtype=np.float32)
            s = c.corr * (zn / gn) ** 2
        x_mean = x + col(s) * score
        x = x_mean + col(np.sqrt(np.float32(2) * s.astype(np.float32))) * z
    check(key + "_mean", x_mean, g[key + "_mean"])
    check(key + "_x", x, g[key + "_x"])


class Recorder(torch.nn.Module):
    """Stands in for the score network: keeps the labels get_score_fn hands to model.forward."""

    def __init__(self):
        super().__init__()
        self.labels = []

    def forward(self, x, labels, condition, mask):
        self.labels.append(labels.reshape(-1).float().clone())        # model.forward reads labels as float32 (model.py of this tree)
        return torch.zeros_like(x)


@pytest.mark.parametrize("name,continuous", [("vpsde", True), ("vpsde", False), ("subvpsde", True), ("subvpsde", False),
                                             ("vesde", True), ("vesde", False)])
def test_labels_are_bit_identical_to_get_score_fn(name, continuous):
    sde = make_sde(sde_lib, name)
    ts = np.concatenate([torch.linspace(1.0, 0.01, 37).numpy(), np.float32([0.9, 0.5, 0.31, 0.1, 0.013, 0.0005])])
    rec = Recorder()
    score_fn = mutils.get_score_fn(sde, rec, train=False, continuous=continuous)
    for t in ts:
        vec_t = torch.ones(3) * float(t)                  # pc_sampler: vec_t = ones(B) * t
        score_fn(torch.zeros(3, 17, 3), vec_t, None, None)
    want = torch.stack([lab[0] for lab in rec.labels]).numpy()
    c = coeffs(sde, "euler_maruyama", "none", False, ts, continuous=continuous)
    assert c is not None and c.label.dtype == np.float32
    assert np.array_equal(c.label.view(np.uint32), want.view(np.uint32))
    # net_scale is what turns the stub's output into the score: -1/std for VP and sub-VP, 1 for VE
    if name == "vesde":
        assert np.array_equal(c.net_scale, np.ones_like(c.net_scale))
    else:
        assert (c.net_scale < 0).all()
    # scale_by_sigma divides by sigmas[int(label)] (model.py:294 of the reference)
    sig = np.exp(np.linspace(np.log(50.0), np.log(0.01), 1000))
    c2 = coeffs(sde, "euler_maruyama", "none", False, ts, continuous=continuous, sbs=True, sigmas=torch.tensor(sig))
    want2 = c.net_scale.astype(np.float64) / sig[c.label.astype(np.int64)].astype(np.float32)
    np.testing.assert_allclose(c2.net_scale, want2, rtol=2e-7, atol=0)
    assert np.array_equal(c2.label, c.label)


def test_only_the_registered_classes_are_native():
    vp = sde_lib.VPSDE()
    ts = np.float32([0.5])
    assert coeffs(vp, "reverse_diffusion", "langevin", False, ts) is not None

    class MyPredictor(sampling.ReverseDiffusionPredictor):
        pass

    class MyVP(sde_lib.VPSDE):
        pass

    @sampling.register_corrector(name="pc_coeffs_test_corrector")
    class MyCorrector(sampling.Corrector):
        def update_fn(self, x, t, condition, mask):
            return x, x
    try:
        args = (False, True, SNR, 1, False, None, ts)
        assert _pc_coeffs.coefficients(vp, MyPredictor, sampling.NoneCorrector, *args) is None
        assert _pc_coeffs.coefficients(MyVP(), sampling.ReverseDiffusionPredictor, sampling.NoneCorrector, *args) is None
        assert _pc_coeffs.coefficients(vp, sampling.ReverseDiffusionPredictor, sampling.get_corrector("pc_coeffs_test_corrector"), *args) is None
        assert not _pc_coeffs.is_native(vp, MyPredictor, sampling.NoneCorrector, False)
    finally:
        del sampling._CORRECTORS["pc_coeffs_test_corrector"]
    # what raises in the reference is not native either: it keeps raising on the torch route
    sub = sde_lib.subVPSDE()
    assert coeffs(sub, "ancestral_sampling", "none", False, ts) is None
    assert coeffs(sub, "euler_maruyama", "langevin", False, ts) is None and coeffs(sub, "euler_maruyama", "ald", False, ts) is None
    assert coeffs(vp, "ancestral_sampling", "none", True, ts) is None
    # the none / none pair is native and does nothing
    c = coeffs(vp, "none", "none", False, ts)
    assert c is not None and not c.has_predictor and c.n_corr == 0


def test_the_module_does_not_need_the_library():
    src = open(_pc_coeffs.__file__).read()
    assert "import zedo_hip" not in src


def test_library_exports_the_pc_entry_points():
    import zedo_hip
    lib = host_lib()
    for n in ("zedo_pc_plan_create", "zedo_pc_plan_destroy", "zedo_pc_workspace_bytes", "zedo_pc_step"):
        assert hasattr(lib, n) and n in zedo_hip.SIGNATURES, n
    assert lib.zedo_abi_version() == 5 and zedo_hip.abi_version() == 5
    assert callable(zedo_hip.pc_step) and isinstance(zedo_hip.PcPlan, type)
