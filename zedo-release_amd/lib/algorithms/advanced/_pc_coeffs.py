"""Per-step scalars of one predictor-corrector call, for the native route of `get_pc_sampler` (host only: torch on CPU).

Every registered predictor is   x_mean = A x + B score(x),   x_new = x_mean + C z      (reference advanced/sampling.py:180-248)
every corrector step is         x_mean = x + s score(x),     x     = x_mean + sqrt(2 s) z        (:259-331)
with score = net_scale * net(x, label) (advanced/utils.py:751-800, model.py:294).  The sampler always passes
vec_t = ones(B) * t (:497), so A, B, C, s, net_scale and label depend on the step alone.  `coefficients` evaluates them for
a vector of S times at once:

 * labels with the SAME fp32 torch expressions as `get_score_fn` (utils.py:37-54 of this tree) - the time embedding sees
   999 t, one ulp of the label is visible in eps;
 * everything else from the sde object's own methods and fp32 tables (sde.sde, sde.discretize, sde.marginal_prob,
   discrete_betas, alphas, discrete_sigmas) evaluated on the [S] time tensor with x = ones where a linear coefficient is
   wanted, products folded in float64 and rounded once to fp32.  Nothing is re-derived in closed form: the VE
   discretisation sigma_i^2 - sigma_{i-1}^2 cancels in fp32 in the reference and the fixtures hold what it computed.

`None` = not native: the caller keeps the torch route (and with it the exception a combination raises there).
This module never imports zedo_hip.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import sde_lib

CORR_NONE, CORR_LANGEVIN, CORR_ALD = 0, 1, 2       # ZEDO_PC_CORR_* of include/zedo_hip.h


def _f32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).astype(np.float32).reshape(-1))


def _d(t):
    return t.detach().reshape(-1).double().numpy()


def _labels_and_scale(sde, continuous, t):
    """-> (labels as model.forward sees them after .float(), labels as passed (for sigmas[labels.long()]), net_scale float64)."""
    x0 = torch.zeros(t.shape[0], 1, 1)
    if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
        if continuous or isinstance(sde, sde_lib.subVPSDE):
            labels = t * 999
            std = sde.marginal_prob(x0, t)[1]
        else:
            labels = t * (sde.N - 1)
            std = sde.sqrt_1m_alphas_cumprod[labels.long()]
        return labels.float(), labels, -1.0 / _d(std)
    if continuous:
        labels = sde.marginal_prob(x0, t)[1]
    else:
        labels = torch.round((sde.T - t) * (sde.N - 1)).long()
    return labels.float(), labels, np.ones(t.shape[0])


def _disc_step(sde, t):
    return (t * (sde.N - 1) / sde.T).long()


def _predictor(sde, name, probability_flow, t):
    """-> (A, B, C) float64 [S] in terms of the score."""
    ones = torch.ones(t.shape[0], 1, 1)
    if name == "euler_maruyama":
        dt = -1.0 / sde.N
        drift, g = sde.sde(ones, t)
        f1, g = _d(drift), _d(g)
        return 1.0 + f1 * dt, -(g * g) * dt, g * np.sqrt(-dt)
    if name == "reverse_diffusion":
        f, G = sde.discretize(ones, t)
        f1, G = _d(f), _d(G)
        return 1.0 - f1, G * G, G
    # ancestral sampling
    step = _disc_step(sde, t)
    if isinstance(sde, sde_lib.VESDE):
        sig = sde.discrete_sigmas
        s2 = sig[step] ** 2
        p2 = torch.where(step == 0, torch.zeros_like(t), sig[step - 1]) ** 2
        return np.ones(t.shape[0]), _d(s2 - p2), _d(torch.sqrt(p2 * (s2 - p2) / s2))
    beta = sde.discrete_betas[step]
    r = _d(torch.sqrt(1.0 - beta))
    return 1.0 / r, _d(beta) / r, _d(torch.sqrt(beta))


def _kinds(sde, predictor, corrector, probability_flow):
    """-> (predictor name, CORR_*) of a native combination, else None."""
    from . import sampling       # at call time: sampling imports this module
    if type(sde) not in (sde_lib.VPSDE, sde_lib.VESDE, sde_lib.subVPSDE):
        return None
    pname = {sampling.EulerMaruyamaPredictor: "euler_maruyama", sampling.ReverseDiffusionPredictor: "reverse_diffusion",
             sampling.AncestralSamplingPredictor: "ancestral_sampling", sampling.NonePredictor: "none"}.get(predictor)
    ckind = {sampling.NoneCorrector: CORR_NONE, sampling.LangevinCorrector: CORR_LANGEVIN,
             sampling.AnnealedLangevinDynamics: CORR_ALD}.get(corrector)
    if pname is None or ckind is None:      # a user-registered class or a subclass of a registered one
        return None
    sub = type(sde) is sde_lib.subVPSDE
    # what raises in the reference stays on the torch route and keeps raising there: ancestral sampling knows VP and VE only
    # and no probability flow (:212-216), the correctors read sde.alphas, which subVPSDE does not have (:272-274)
    if pname == "ancestral_sampling" and (sub or probability_flow):
        return None
    if ckind != CORR_NONE and sub:
        return None
    return pname, ckind


def is_native(sde, predictor, corrector, probability_flow):
    """Whether this combination of classes has a native step at all (the times may still rule a plan out)."""
    return _kinds(sde, predictor, corrector, probability_flow) is not None


def coefficients(sde, predictor, corrector, probability_flow, continuous, snr, n_steps, scale_by_sigma, sigmas, ts):
    """-> None (not native) or a namespace of per-step fp32 arrays of length S = len(ts):
    label, net_scale, has_predictor, pA, pB, pC (C = 0 under probability flow), corrector (CORR_*), n_corr and
    corr (ALD: step[S]; Langevin: factor[S] = 2 alpha snr^2; else None)."""
    kinds = _kinds(sde, predictor, corrector, probability_flow)
    if kinds is None:
        return None
    pname, ckind = kinds
    n_corr = int(n_steps) if ckind != CORR_NONE else 0
    if n_corr < 0:
        return None
    with torch.no_grad():
        t = torch.as_tensor(np.asarray(ts, dtype=np.float32).reshape(-1).copy())
        S = t.shape[0]
        try:
            label, label_raw, net_scale = _labels_and_scale(sde, bool(continuous), t)
            if scale_by_sigma:
                idx = label_raw.reshape(-1).long().numpy()
                sg = torch.as_tensor(sigmas).detach().cpu().reshape(-1)
                if idx.min() < 0 or idx.max() >= sg.shape[0]:
                    return None
                net_scale = net_scale / sg[torch.as_tensor(idx)].float().double().numpy()      # model.py:294, in the output's dtype
            out = SimpleNamespace(S=S, label=_f32(label.numpy()), net_scale=_f32(net_scale), has_predictor=pname != "none",
                                  pA=_f32(np.ones(S)), pB=_f32(np.zeros(S)), pC=_f32(np.zeros(S)),
                                  corrector=ckind, n_corr=n_corr, corr=None)
            if out.has_predictor:
                A, B, C = _predictor(sde, pname, probability_flow, t)
                out.pA, out.pB, out.pC = _f32(A), _f32(B), _f32(np.zeros(S) if probability_flow else C)
            if ckind != CORR_NONE:
                alpha = _d(sde.alphas[_disc_step(sde, t)]) if isinstance(sde, sde_lib.VPSDE) else np.ones(S)
                if ckind == CORR_ALD:
                    std = _d(sde.marginal_prob(torch.ones(S, 1, 1), t)[1])
                    out.corr = _f32((float(snr) * std) ** 2 * 2.0 * alpha)
                else:
                    out.corr = _f32(2.0 * alpha * float(snr) ** 2)
        except IndexError:         # a time outside the discrete tables: the torch route raises the same way
            return None
    arrays = [out.label, out.net_scale, out.pA, out.pB, out.pC] + ([out.corr] if out.corr is not None else [])
    if not all(np.isfinite(a).all() for a in arrays):
        return None
    return out
