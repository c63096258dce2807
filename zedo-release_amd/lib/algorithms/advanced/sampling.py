"""Samplers of the drop-in surface (reference lib/algorithms/advanced/sampling.py).

`get_sampling_fn(config, sde, shape, inverse_scaler, eps, device)` returns `pc_sampler` with the reference's
signature and return types: `(trajs np.ndarray[1,B,J,3], x_mean np.ndarray[B,J,3])` (:450-527).

Fast path = the shipped configuration (configs/optim/*.py: method 'pc', predictor 'euler_maruyama',
corrector 'none', probability_flow forced True at run/opt_main.py:157, sub-VP SDE): the whole call is one
`zedo_sde_step` - x' = a_t x + c_t eps(x, 999 t) - on the device.  Every other combination of the registered
predictors / correctors with VPSDE / VESDE / subVPSDE is one `zedo_pc_step` per call (scalars from _pc_coeffs.py, once per
loop; the noise draws stay here, in the caller's RNG stream).  What is left (user-registered classes, subclasses,
ZEDO_GENERIC_PC=torch) runs the update rules below as torch operators around the HIP score function.  The fused driver
(run/opt_main.py) does not go through this per-step surface at all; it exists so that callers of the
reference's sampling_fn keep working.
"""
import functools
import os

import numpy as np
import torch

from . import _pc_coeffs, sde_lib
from . import utils as mutils
from .utils import from_flattened_numpy, to_flattened_numpy, get_score_fn  # noqa: F401  (re-exported like the reference)

_PREDICTORS, _CORRECTORS = {}, {}


def _registrar(table, cls, name):
    def deco(c):
        key = name or c.__name__
        if key in table:
            raise ValueError(f"Already registered model with name: {key}")
        table[key] = c
        return c
    return deco if cls is None else deco(cls)


def register_predictor(cls=None, *, name=None):
    return _registrar(_PREDICTORS, cls, name)


def register_corrector(cls=None, *, name=None):
    return _registrar(_CORRECTORS, cls, name)


def get_predictor(name):
    return _PREDICTORS[name]


def get_corrector(name):
    return _CORRECTORS[name]


class Predictor:
    def __init__(self, sde, score_fn, probability_flow=False):
        self.sde, self.score_fn = sde, score_fn
        self.rsde = sde.reverse(score_fn, probability_flow)

    def update_fn(self, x, t, condition, mask):
        raise NotImplementedError


class Corrector:
    def __init__(self, sde, score_fn, snr, n_steps):
        self.sde, self.score_fn, self.snr, self.n_steps = sde, score_fn, snr, n_steps

    def update_fn(self, x, t, condition, mask):
        raise NotImplementedError


@register_predictor(name="euler_maruyama")
class EulerMaruyamaPredictor(Predictor):
    """x_mean = x + drift * (-1/N); x = x_mean + diffusion sqrt(1/N) z   (reference :180-191)"""

    def update_fn(self, x, t, condition, mask):
        dt = -1.0 / self.rsde.N
        drift, diffusion = self.rsde.sde(x, t, condition, mask)
        x_mean = x + drift * dt
        x = x_mean + diffusion[:, None, None] * np.sqrt(-dt) * torch.randn_like(x)
        return x, x_mean


@register_predictor(name="reverse_diffusion")
class ReverseDiffusionPredictor(Predictor):
    def update_fn(self, x, t, condition, mask):
        f, G = self.rsde.discretize(x, t, condition, mask)
        x_mean = x - f
        return x_mean + G[:, None, None] * torch.randn_like(x), x_mean


@register_predictor(name="ancestral_sampling")
class AncestralSamplingPredictor(Predictor):
    """Ancestral sampling for the discrete VE / VP chains (reference :208-248); no probability-flow form."""

    def __init__(self, sde, score_fn, probability_flow=False):
        super().__init__(sde, score_fn, probability_flow)
        if not isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE)):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")
        assert not probability_flow, "Probability flow not supported by ancestral sampling"

    def update_fn(self, x, t, condition, mask):
        sde = self.sde
        step = (t * (sde.N - 1) / sde.T).long()
        if isinstance(sde, sde_lib.VESDE):
            sig = sde.discrete_sigmas.to(t.device)
            s2 = sig[step] ** 2
            p2 = torch.where(step == 0, torch.zeros_like(t), sig[step - 1]) ** 2
            x_mean = x + self.score_fn(x, t, condition, mask) * (s2 - p2)[:, None, None]
            std = torch.sqrt(p2 * (s2 - p2) / s2)
        else:
            beta = sde.discrete_betas.to(t.device)[step]
            x_mean = (x + beta[:, None, None] * self.score_fn(x, t, condition, mask)) / torch.sqrt(1.0 - beta)[:, None, None]
            std = torch.sqrt(beta)
        return x_mean + std[:, None, None] * torch.randn_like(x), x_mean


@register_predictor(name="none")
class NonePredictor(Predictor):
    def __init__(self, sde, score_fn, probability_flow=False):
        pass

    def update_fn(self, x, t, condition, mask):
        return x, x


@register_corrector(name="none")
class NoneCorrector(Corrector):
    def __init__(self, sde, score_fn, snr, n_steps):
        pass

    def update_fn(self, x, t, condition, mask):
        return x, x


def _corrector_alpha(sde, t):
    """alpha_i of the discrete VP chain, 1 for VE (reference :275-279).  The reference takes the VP branch for
    subVPSDE too, which has no `alphas` table: that combination raises AttributeError there and here."""
    if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
        return sde.alphas.to(t.device)[(t * (sde.N - 1) / sde.T).long()]
    return torch.ones_like(t)


class _CheckedCorrector(Corrector):
    def __init__(self, sde, score_fn, snr, n_steps):
        super().__init__(sde, score_fn, snr, n_steps)
        if not isinstance(sde, (sde_lib.VPSDE, sde_lib.VESDE, sde_lib.subVPSDE)):
            raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")


@register_corrector(name="langevin")
class LangevinCorrector(_CheckedCorrector):
    def update_fn(self, x, t, condition, mask):
        alpha = _corrector_alpha(self.sde, t)
        x_mean = x
        for _ in range(self.n_steps):
            grad = self.score_fn(x, t, condition, mask)
            noise = torch.randn_like(x)
            gn = torch.norm(grad.reshape(grad.shape[0], -1), dim=-1).mean()
            nn_ = torch.norm(noise.reshape(noise.shape[0], -1), dim=-1).mean()
            step = (self.snr * nn_ / gn) ** 2 * 2 * alpha
            x_mean = x + step[:, None, None] * grad
            x = x_mean + torch.sqrt(step * 2)[:, None, None] * noise
        return x, x_mean


@register_corrector(name="ald")
class AnnealedLangevinDynamics(_CheckedCorrector):
    """Annealed Langevin dynamics of NCSN (reference :300-331): step size from the marginal std, not the norms."""

    def update_fn(self, x, t, condition, mask):
        alpha = _corrector_alpha(self.sde, t)
        std = self.sde.marginal_prob(x, t)[1]
        x_mean = x
        for _ in range(self.n_steps):
            grad = self.score_fn(x, t, condition, mask)
            noise = torch.randn_like(x)
            step = (self.snr * std) ** 2 * 2 * alpha
            x_mean = x + step[:, None, None] * grad
            x = x_mean + noise * torch.sqrt(step * 2)[:, None, None]
        return x, x_mean


def shared_predictor_update_fn(x, t, condition, mask, sde, model, predictor, probability_flow, continuous):
    score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
    obj = NonePredictor(sde, score_fn, probability_flow) if predictor is None else predictor(sde, score_fn, probability_flow)
    return obj.update_fn(x, t, condition, mask)


def shared_corrector_update_fn(x, t, condition, mask, sde, model, corrector, continuous, snr, n_steps):
    score_fn = mutils.get_score_fn(sde, model, train=False, continuous=continuous)
    obj = NoneCorrector(sde, score_fn, snr, n_steps) if corrector is None else corrector(sde, score_fn, snr, n_steps)
    return obj.update_fn(x, t, condition, mask)


def get_sampling_fn(config, sde, shape, inverse_scaler, eps, device=None):
    """reference :80-127"""
    device = config.device if device is None else device
    name = config.sampling.method.lower()
    if name != "pc":
        raise NotImplementedError(f"sampler '{name}': the reference's ODE sampler is broken as shipped "
                                  "(SURVEY.md 2, row 4); only 'pc' is provided")
    return get_pc_sampler(sde=sde, shape=shape,
                          predictor=get_predictor(config.sampling.predictor.lower()),
                          corrector=get_corrector(config.sampling.corrector.lower()),
                          inverse_scaler=inverse_scaler, snr=config.sampling.snr,
                          n_steps=config.sampling.n_steps_each, probability_flow=config.sampling.probability_flow,
                          continuous=config.training.continuous, denoise=config.sampling.noise_removal,
                          eps=eps, device=device,
                          oil_steps_hint=getattr(getattr(config, "ZeDO", None), "OIL_iterations", None))


def _state_equal(a, b):
    """(weights handle, plain values...): the handle by identity, the rest by value."""
    return a[0] is b[0] and a[1:] == b[1:]


class _WholeLoop:
    """One table object for the WHOLE loop the sampler is being stepped through, found from the calls themselves.

    The reference calls pc_sampler once per OIL iteration with t = linspace(sde.T, eps, S)[i], t_step = i
    (run/opt_main.py:198-218).  Building a table costs a device allocation, six small dense launches and a
    stream sync; done per call it would dominate the step.  So the first call that reveals S (the configured
    OIL_iterations as a hint, else S solved from (t, t_step) for t_step >= 1) builds ONE table for all S
    timestamps, and every later call whose t is bit-identical to that table's entry t_step reuses it.
    Anything else (a caller stepping its own times) falls back to a one-entry table: same results, slower.
    Subclasses say what the table is: `_table(model, ts)` for a vector of times, `_state(model)` for what it depends on."""

    def __init__(self, sde, eps, hint):
        self.sde, self.eps, self.hint = sde, float(eps), hint
        self.table = self.ts = self.state = None
        self.hits = self.misses = 0

    def _table(self, model, ts):
        raise NotImplementedError

    def _state(self, model):
        return (model.hip_weights(),)

    def _same_state(self, model):
        return self.state is not None and _state_equal(self._state(model), self.state)

    def _try(self, model, S, tval, t_step):
        if S is None or not (2 <= int(S) <= 1 << 20) or t_step >= int(S):
            return False
        ts = torch.linspace(float(self.sde.T), self.eps, int(S), dtype=torch.float32).numpy()
        if ts[t_step] != np.float32(tval):
            return False
        table = self._table(model, ts)
        if table is None:
            return False
        self.state, self.table, self.ts = self._state(model), table, ts
        return True

    def lookup(self, model, tval, t_step):
        """-> (table, index) for SDE time tval at loop position t_step."""
        if t_step is not None and t_step >= 0:
            ok = (self.table is not None and self._same_state(model) and t_step < len(self.ts)
                  and self.ts[t_step] == np.float32(tval))
            if not ok:
                guess = None
                if t_step >= 1 and tval != float(self.sde.T):
                    guess = int(round(t_step * (self.eps - float(self.sde.T)) / (tval - float(self.sde.T)))) + 1
                ok = self._try(model, self.hint, tval, t_step) or self._try(model, guess, tval, t_step)
            if ok:
                self.hits += 1
                return self.table, t_step
        self.misses += 1
        return self._table(model, np.array([tval], np.float32)), 0


class _LoopSchedule(_WholeLoop):
    """The per-step tables (time-bias rows, a_i, c_i) of the shipped configuration: a zedo_hip.Schedule."""

    def _table(self, model, ts):
        return model.hip_schedule(ts, 999.0, self.sde.beta_0, self.sde.beta_1, self.sde.N)

    @property
    def sched(self):
        return self.table


class _NativePlan(_WholeLoop):
    """The per-step scalars and time-bias rows of any other registered combination: a zedo_hip.PcPlan built from
    _pc_coeffs.coefficients.  `plan` is the whole-loop plan once a call has revealed it; one-entry plans of foreign times
    are kept for re-use (a caller may step one time repeatedly)."""

    def __init__(self, sde, eps, hint, coeffs_of):
        super().__init__(sde, eps, hint)
        self.coeffs_of, self.singles = coeffs_of, {}

    @property
    def plan(self):
        return self.table

    def _state(self, model):
        mc = getattr(getattr(model, "config", None), "model", None)
        return (model.hip_weights(), bool(getattr(mc, "scale_by_sigma", False)))

    def _table(self, model, ts):
        import zedo_hip
        single = len(ts) == 1
        if single:
            key = np.float32(ts[0]).tobytes()
            hit = self.singles.get(key)
            if hit is not None and _state_equal(hit[0], self._state(model)):
                return hit[1]
        c = self.coeffs_of(model, ts)
        plan = None if c is None else zedo_hip.PcPlan(model.hip_weights(), c)
        if single and plan is not None:
            if len(self.singles) > 64:
                self.singles.clear()
            self.singles[key] = (self._state(model), plan)
        return plan


def get_pc_sampler(sde, shape, predictor, corrector, inverse_scaler, snr, n_steps=1, probability_flow=False,
                   continuous=False, denoise=True, eps=1e-3, device="cuda", oil_steps_hint=None):
    """One predictor-corrector step per call (reference :400-529).

    Three routes, chosen per call: the shipped configuration is one `zedo_sde_step`; every other combination of the
    registered predictors / correctors with VPSDE / VESDE / subVPSDE is one `zedo_pc_step` (all element-wise work on the
    device, scalars from _pc_coeffs once per plan); anything else - user-registered classes, subclasses, combinations that
    raise in the reference, ZEDO_GENERIC_PC=torch - runs the update rules above as torch operators around model.forward."""
    # the closed form x' = a_i x + c_i eps(x, 999 t_i) is ONE configuration (run/_driver.py::not_fused_because lists the
    # same fields); the two that belong to the model (continuous labels: utils.py:751-777 - for subVPSDE the reference
    # takes the continuous branch either way; eps / sigmas[t] with scale_by_sigma: model.py:294) are checked per call
    fused = (predictor is EulerMaruyamaPredictor and corrector is NoneCorrector and probability_flow
             and isinstance(sde, sde_lib.subVPSDE))
    loop = _LoopSchedule(sde, eps, oil_steps_hint) if fused else None

    def model_is_fusable(model):
        mc = getattr(getattr(model, "config", None), "model", None)
        return not bool(getattr(mc, "scale_by_sigma", False))

    def coeffs_of(model, ts):
        return _pc_coeffs.coefficients(sde, predictor, corrector, probability_flow, continuous, snr, n_steps,
                                       not model_is_fusable(model), getattr(model, "sigmas", None), ts)

    # ZEDO_GENERIC_PC=torch (diagnostics / A-B): pin the torch route.  Read per get_pc_sampler call.
    pinned = os.environ.get("ZEDO_GENERIC_PC", "").strip().lower() == "torch"
    native = None
    if not pinned and _pc_coeffs.is_native(sde, predictor, corrector, probability_flow):
        native = _NativePlan(sde, eps, oil_steps_hint, coeffs_of)

    pred_fn = functools.partial(shared_predictor_update_fn, sde=sde, predictor=predictor,
                                probability_flow=probability_flow, continuous=continuous)
    corr_fn = functools.partial(shared_corrector_update_fn, sde=sde, corrector=corrector, continuous=continuous,
                                snr=snr, n_steps=n_steps)

    def native_step(model, x, tval, t_step, want_mean):
        """-> None (this call is not native) or (x_new, x_mean) on the device; with noise removal both are x_mean, and
        x_mean is None when the caller does not want it.  torch.randn_like is called exactly as often and in the same order
        as the reference calls it (corrector steps, then the predictor - also when its draw is discarded or multiplied by
        zero), so the caller's RNG stream moves as it does there."""
        if native is None or not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
            return None
        import zedo_hip  # noqa: F811
        if model.training:
            model.eval()
        plan, si = native.lookup(model, tval, t_step)
        if plan is None:
            return None
        noise = [torch.randn_like(x) for _ in range(plan.n_draws)]
        if plan.has_predictor and (denoise or plan.pC[si] == 0.0):
            noise[-1] = None                    # drawn for the RNG stream, not handed over: x returns x_mean
            want_mean = False
        noise = [None if z is None else z.contiguous() for z in noise]
        x_new = x.detach().contiguous().clone()
        x_mean = torch.empty_like(x_new) if (want_mean and plan.has_predictor) else None
        zedo_hip.pc_step(plan.weights, plan, si, x_new, noise, x_mean)
        return x_new, (x_new if x_mean is None else x_mean)

    def to_host(x_mean):
        # ONE device-to-host copy into a pinned staging buffer (torch's pageable .cpu() path fans the 180 KB copy out over
        # the host's whole intra-op pool: 1.5 ms per call on a 128-thread host), then plain numpy copies.
        key = (tuple(x_mean.shape), x_mean.device)
        if stage.get("key") != key:
            stage["key"], stage["buf"] = key, torch.empty(x_mean.shape, dtype=torch.float32, pin_memory=True)
        stage["buf"].copy_(x_mean, non_blocking=True)
        torch.cuda.current_stream(x_mean.device).synchronize()
        return stage["buf"].numpy().copy()

    def step_device(model, condition, gradient=None, denoise_x=None, t=None, t_step=None, args=None):
        """The same predictor-corrector step with the result LEFT ON THE DEVICE: -> the tensor the public callable hands back as
        numpy (x_mean with noise removal, else x_new).  For callers that own the loop (run/_driver.py::stepwise_loop): the
        reference's per-step D2H + H2D round trip (:515,525 and run/opt_main.py:220) moves the values and changes no bit, so a
        loop stepped through this entry produces the rows of the numpy surface exactly, without 2 x S synchronising copies.
        `t` may be a Python float (no device read at all) or a tensor."""
        with torch.no_grad():
            x = denoise_x
            tval = float(t)
            if t_step is not None and t_step < 0:      # reference :499 (disabled override, kept for parity)
                tval = 1.0
            if fused and model_is_fusable(model):
                import zedo_hip  # noqa: F811
                if model.training:
                    model.eval()
                sched, si = loop.lookup(model, tval, t_step)
                x_mean = x.detach().float().contiguous().clone()
                zedo_hip.sde_step(model.hip_weights(), sched, si, x_mean)
                return x_mean
            done = native_step(model, x, tval, t_step, want_mean=False)
            if done is not None:
                return done[0]                          # with noise removal x_new IS x_mean
            vec_t = torch.ones(x.shape[0], device=x.device) * tval
            mask = torch.zeros_like(x)
            x1, _ = corr_fn(x, vec_t, condition, mask, model=model)
            x_new, x_mean = pred_fn(x1, vec_t, condition, mask, model=model)
            return x_mean if denoise else x_new

    def pc_sampler(model, condition, gradient=None, denoise_x=None, t=None, t_step=None, args=None):
        with torch.no_grad():
            x = denoise_x
            tval = float(t)
            if t_step is not None and t_step < 0:      # reference :499 (disabled override, kept for parity)
                tval = 1.0
            if fused and model_is_fusable(model):
                import zedo_hip  # noqa: F811
                if model.training:
                    model.eval()
                sched, si = loop.lookup(model, tval, t_step)
                x_mean = x.detach().float().contiguous().clone()
                zedo_hip.sde_step(model.hip_weights(), sched, si, x_mean)
                # diffusion is zero for the probability-flow ODE: x_new == x_mean
                x_mean_np = to_host(x_mean)
                trajs = x_mean_np[None].copy()
                return trajs, (x_mean_np if denoise else x_mean)    # the reference hands back the tensor here (:527)
            done = native_step(model, x, tval, t_step, want_mean=True)
            if done is not None:
                x_new, x_mean = done
                x_mean_np = to_host(x_mean)
                trajs = x_mean_np[None].copy()
                return trajs, (x_mean_np if denoise else x_new)     # the reference hands back the tensor here (:527)
            vec_t = torch.ones(x.shape[0], device=x.device) * tval
            mask = torch.zeros_like(x)
            x1, _ = corr_fn(x, vec_t, condition, mask, model=model)
            x_new, x_mean = pred_fn(x1, vec_t, condition, mask, model=model)
            trajs = np.stack([x_new.cpu().numpy()], axis=0)
            x_mean_np = x_mean.cpu().numpy()
            trajs[-1] = x_mean_np
            return trajs, (x_mean_np if denoise else x_new)     # the reference hands back the tensor here (:527)

    stage = {}
    pc_sampler.loop_schedule = loop          # introspection for tests: hits / misses of the whole-loop schedule
    pc_sampler.native_plan = native          # the same for the native generic route (None: torch route); .plan, .hits, .misses
    pc_sampler.step_device = step_device     # the device-resident twin for loops owned by the driver (no per-step host copies)
    return pc_sampler
