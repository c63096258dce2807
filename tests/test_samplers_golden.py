"""VPSDE / VESDE / subVPSDE schedule methods, their reverse-time forms and every registered
predictor / corrector update rule against captures from the reference (tools/gen_golden.py::gen_samplers,
reference sde_lib.py:112-261, sampling.py:180-331).  The score function is analytic and torch.randn_like is
replaced by a numpy-Philox stream in both the capture and this test, so only the update arithmetic is compared.
Host-side torch code on [B]-sized tensors: runs on CPU, fp32 tolerance 2e-6 relative (most entries are bit-equal)."""
import numpy as np
import pytest
import torch

from _shared import DetNoise, analytic_score, make_sde, sampler_cases
from lib.algorithms.advanced import sampling, sde_lib

SDES, PREDS, CORRS = sampler_cases()
ERRORS = dict(NotImplementedError=NotImplementedError, AssertionError=AssertionError, AttributeError=AttributeError)


@pytest.fixture(autouse=True)
def _capture_sqrt(request, monkeypatch, golden):
    """torch's float32 sqrt on the CPU is only faithfully rounded, and which of the two neighbours of the exact root it returns
    depends on the host (on one host a fifth of random arguments get the other neighbour than the correctly rounded root, and the
    capture's host returned yet other ones).  Where the update rule
    cancels - VPSDE.discretize's sqrt(alpha) x - x, the reverse drift f - G^2 score - one ulp of a root is up to 9e-5 relative in
    the result, so the comparison would measure the host's sqrt instead of the update arithmetic.  Like the noise above, the
    primitive is therefore pinned: the correctly rounded root (float64 sqrt rounded once to float32 - exact for float32, since
    53 >= 2 * 24 + 2), or the other faithful neighbour where the capture recorded that one as a root of the SDE under test (its
    <sde>_diffusion and <sde>_disc_G entries are roots the capture's host returned)."""
    g = golden("samplers")
    name = getattr(request.node, "callspec", None) and request.node.callspec.params.get("name")
    keys = [f"{name}_diffusion", f"{name}_disc_G"] if name else []
    roots = torch.tensor(np.unique(np.concatenate([g[k].ravel() for k in keys] or [np.zeros(0, np.float32)])))
    sqrt = torch.sqrt

    def capture_sqrt(a, *args, **kw):
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.float32 and not args and not kw):
            return sqrt(a, *args, **kw)
        r64 = sqrt(a.double())
        r = r64.float()
        other = torch.nextafter(r, torch.where(r64 > r.double(), torch.inf, -torch.inf).float())
        return torch.where((r64 != r.double()) & torch.isin(other, roots), other, r)
    monkeypatch.setattr(torch, "sqrt", capture_sqrt)


def close(a, b):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    np.testing.assert_allclose(np.broadcast_to(a, b.shape) if a.shape != b.shape else a, b, rtol=2e-6, atol=1e-7)


@pytest.fixture()
def inputs(golden):
    g = golden("samplers")
    return g, torch.tensor(g["x"]), torch.tensor(g["cond"]), torch.tensor(g["t"])


@pytest.mark.parametrize("name", SDES)
def test_sde_schedule_methods(inputs, name):
    g, x, cond, t = inputs
    sde = make_sde(sde_lib, name)
    for got, key in zip(sde.sde(x, t), ("drift", "diffusion")):
        close(got, g[f"{name}_{key}"])
    for got, key in zip(sde.marginal_prob(x, t), ("mean", "std")):
        close(got, g[f"{name}_{key}"])
    for got, key in zip(sde.discretize(x, t), ("disc_f", "disc_G")):
        close(got, g[f"{name}_{key}"])
    mask = torch.zeros_like(x)
    for pf in (False, True):
        r = sde.reverse(analytic_score, pf)
        assert r.N == sde.N and r.T == sde.T
        for got, key in zip(r.sde(x, t, cond, mask), ("rsde_drift", "rsde_diffusion")):
            close(got, g[f"{name}_{key}_pf{int(pf)}"])
        for got, key in zip(r.discretize(x, t, cond, mask), ("rdisc_f", "rdisc_G")):
            close(got, g[f"{name}_{key}_pf{int(pf)}"])


@pytest.mark.parametrize("name", SDES)
@pytest.mark.parametrize("pname,pf", PREDS)
def test_predictor_update_rules(inputs, monkeypatch, name, pname, pf):
    g, x, cond, t = inputs
    sde = make_sde(sde_lib, name)
    key = f"{name}_pred_{pname}_pf{int(pf)}"
    monkeypatch.setattr(torch, "randn_like", DetNoise())
    if key + "_raises" in g.files:
        with pytest.raises(ERRORS[str(g[key + "_raises"])]):
            sampling.get_predictor(pname)(sde, analytic_score, pf).update_fn(x, t, cond, torch.zeros_like(x))
        return
    xn, xm = sampling.get_predictor(pname)(sde, analytic_score, pf).update_fn(x, t, cond, torch.zeros_like(x))
    close(xn, g[key + "_x"])
    close(xm, g[key + "_mean"])


@pytest.mark.parametrize("name", SDES)
@pytest.mark.parametrize("cname", CORRS)
def test_corrector_update_rules(inputs, monkeypatch, name, cname):
    g, x, cond, t = inputs
    sde = make_sde(sde_lib, name)
    key = f"{name}_corr_{cname}"
    monkeypatch.setattr(torch, "randn_like", DetNoise())
    if key + "_raises" in g.files:
        with pytest.raises(ERRORS[str(g[key + "_raises"])]):
            sampling.get_corrector(cname)(sde, analytic_score, 0.16, 2).update_fn(x, t, cond, torch.zeros_like(x))
        return
    xn, xm = sampling.get_corrector(cname)(sde, analytic_score, 0.16, 2).update_fn(x, t, cond, torch.zeros_like(x))
    close(xn, g[key + "_x"])
    close(xm, g[key + "_mean"])


def test_ancestral_sampling_rejects_probability_flow():
    with pytest.raises(AssertionError):
        sampling.get_predictor("ancestral_sampling")(sde_lib.VPSDE(), analytic_score, True)


def test_registries_hold_the_reference_names():
    assert sorted(sampling._PREDICTORS) == ["ancestral_sampling", "euler_maruyama", "none", "reverse_diffusion"]
    assert sorted(sampling._CORRECTORS) == ["ald", "langevin", "none"]
