"""GPU tests of the native predictor-corrector step (zedo_pc_step) and of the route through it behind get_pc_sampler:
the C ABI on hand-set coefficients against the network's own eps, chained sampler calls of every generic combination
against float64 captures of the reference (tools/gen_golden.py::gen_pc_generic_loop), the caller's RNG stream, and the
invariants of the route (device twin, determinism, whole-loop plan, chunking, batch-mean semantics of Langevin, fallback)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from _shared import PC_LOOP_CASES, DetNoise, cfg_path, dev, make_sde, model, report_env, zh  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [c[0] for c in PC_LOOP_CASES]
CASE = {c[0]: c for c in PC_LOOP_CASES}


def make_fn(case, rows, eps=0.01, hint=20, predictor=None):
    """get_sampling_fn for one case -> (fn, sde)"""
    from lib.algorithms.advanced import sampling, sde_lib
    from run._driver import load_config
    tag, sname, cont, pred, corr, pf, denoise, _, n_each = case
    cfg = load_config(cfg_path("h36m"))
    cfg.training.sde, cfg.training.continuous = sname, cont
    cfg.sampling.predictor, cfg.sampling.corrector, cfg.sampling.probability_flow = predictor or pred, corr, pf
    cfg.sampling.noise_removal, cfg.sampling.n_steps_each = denoise, n_each
    cfg.ZeDO.OIL_iterations = hint
    sde = make_sde(sde_lib, sname)
    return sampling.get_sampling_fn(cfg, sde, (rows, 17, 3), lambda v: v, eps, device=torch.device("cuda")), sde


def run_chain(fn, sde, model, x0, steps, eps=0.01, snaps=(), device_twin=False):
    """`steps` consecutive calls on t = linspace(T, eps, steps), t_step = i, `res` fed back (run/opt_main.py:210-220)."""
    ts = torch.linspace(float(sde.T), eps, steps)
    x = dev(x0)
    cond = torch.zeros(x.shape[0], 17, 2, device="cuda")
    out = {}
    for i in range(steps):
        if device_twin:
            x = fn.step_device(model, condition=cond, denoise_x=x, t=float(ts[i]), t_step=i)
        else:
            _, res = fn(model, condition=cond, denoise_x=x, t=ts[i], t_step=i)
            x = torch.as_tensor(res).to("cuda")
        if i + 1 in snaps:
            out[i + 1] = x.cpu().numpy()
    return x.cpu().numpy(), out


# ---- 5. one step at the C ABI ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 63, 64, 70, 886])
def test_one_step_abi_is_the_epilogue_fma_and_the_noise_term(zh, weights0, B):
    """x_mean = fma(A, x, fl32(c eps)) with c = fl32(B net_scale) and eps = zedo_score_eps at the same label, to 1 fp32 ulp
    (EPI_BIAS and EPI_SDE share tile shapes and accumulation order); x_new - x_mean = fl32(C z) to 1 ulp of x_new; and the
    x_mean output and the noise launch are optional without a change of bits."""
    W = zh.Weights(weights0)
    label = np.float32(0.37) * np.float32(999)
    A, Bc, C, ns = np.float32(1.0123), np.float32(0.0371), np.float32(0.0816), np.float32(-2.75)
    g = np.random.Generator(np.random.Philox(key=[91, B]))
    x = (0.3 * g.standard_normal((B, 17, 3))).astype(np.float32)
    z = g.standard_normal((B, 17, 3)).astype(np.float32)
    eps = zh.score_eps(W, zh.Schedule(W, [label], label_scale=1.0), 0, dev(x)).cpu().numpy().astype(np.float64)

    def plan(Cv):
        f = lambda v: np.array([v], np.float32)
        return zh.PcPlan(W, SimpleNamespace(label=f(label), net_scale=f(ns), has_predictor=True, pA=f(A), pB=f(Bc), pC=f(Cv),
                                            corrector=0, n_corr=0, corr=None))
    p = plan(C)
    xn, xm = dev(x), torch.empty(B, 17, 3, device="cuda")
    assert zh.pc_step(W, p, 0, xn, [dev(z)], xm) is xn
    xn, xm = xn.cpu().numpy(), xm.cpu().numpy()
    c = np.float32(Bc * ns)
    ref = np.float64(A) * x.astype(np.float64) + (np.float64(c) * eps).astype(np.float32).astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    d = np.abs(xm.astype(np.float64) - ref) / ulp
    print(f"pc_step[B={B}]: x_mean within {d.max():.2f} ulp of fma(A, x, fl32(c eps))")
    assert d.max() <= 1.0
    noise = xn.astype(np.float64) - xm.astype(np.float64)
    want = (np.float64(C) * z.astype(np.float64)).astype(np.float32).astype(np.float64)
    dn = np.abs(noise - want) / np.spacing(np.abs(xn)).astype(np.float64)
    print(f"pc_step[B={B}]: x_new - x_mean within {dn.max():.2f} ulp(x_new) of fl32(C z)")
    assert dn.max() <= 1.0
    # noise removal: the predictor's draw is not handed over -> x returns x_mean; and without the x_mean output
    for noise_arg in ([None], []):
        k = dev(x)
        zh.pc_step(W, p, 0, k, noise_arg, None)
        assert np.array_equal(k.cpu().numpy(), xm)
    # C = 0 (probability flow): the same bits with and without the x_mean output, with and without a draw handed over
    p0 = plan(0.0)
    a, am, b = dev(x), torch.empty(B, 17, 3, device="cuda"), dev(x)
    zh.pc_step(W, p0, 0, a, [dev(z)], am)
    zh.pc_step(W, p0, 0, b, [], None)
    assert torch.equal(a, am) and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), xm)
    assert zh.workspace_bytes(B) == int(zh._lib.zedo_pc_workspace_bytes(p._h, B))


# ---- 6. chained steps against the reference ----------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["native", "torch"])
@pytest.mark.parametrize("tag", CASE_IDS)
def test_chained_steps_against_the_float64_reference(model, golden, monkeypatch, math_mode, tag, route):
    """20 consecutive pc_sampler calls per combination; arbiter = the reference with model and state in float64, yardstick =
    the reference's own fp32 run (gap): max|ours - res64| <= 2 gap + 1e-6 max(1, max|res64|) after steps 1, 10 and 20.
    The same assertion holds for the torch route (ZEDO_GENERIC_PC=torch): the criterion is one the former route meets."""
    g = golden("pc_generic_loop")
    if route == "torch":
        monkeypatch.setenv("ZEDO_GENERIC_PC", "torch")
    else:
        monkeypatch.delenv("ZEDO_GENERIC_PC", raising=False)
    steps, snaps = int(g["steps"]), [int(s) for s in g["snaps"]]
    fn, sde = make_fn(CASE[tag], g["x"].shape[0], eps=float(g["eps"]), hint=steps)
    assert (fn.native_plan is not None) == (route == "native")
    noise = DetNoise()
    monkeypatch.setattr(torch, "randn_like", noise)
    _, got = run_chain(fn, sde, model, g["x"], steps, eps=float(g["eps"]), snaps=snaps)
    assert noise.calls == int(g[f"{tag}_draws"])
    if route == "native":
        assert fn.native_plan.hits == steps and fn.native_plan.misses == 0
    recs, worst = [], 0.0
    for k, s in enumerate(snaps):
        ref, gap = g[f"{tag}_res64"][k], float(g[f"{tag}_gap"][k])
        mag = max(1.0, float(np.abs(ref).max()))
        d = float(np.abs(got[s].astype(np.float64) - ref).max())
        bound = 2.0 * gap + 1e-6 * mag
        recs.append(dict(test="pc_native_chain", route=route, math=math_mode, case=tag, step=s, max_abs_diff=d, ref_gap=gap,
                         magnitude=mag, ratio=d / bound))
        worst = max(worst, d / bound)
        print(f"pc_chain[{tag}, {route}, {math_mode}] step {s}: max|d| {d:.3e}  ref gap {gap:.3e}  magnitude {mag:.3g}  "
              f"ratio to bound {d / bound:.3f}")
    for r in recs:
        report_env(r)
    assert worst <= 1.0, recs


# ---- 7. the caller's RNG stream ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["vp_rd_langevin", "vp_em_none_pf", "ve_anc_langevin", "subvp_rd_none", "vp_em_langevin"])
def test_rng_stream_moves_as_on_the_torch_route(model, golden, monkeypatch, tag):
    """Ten steps with the real generator: the native route draws what the torch route draws (also the predictor's draw that
    noise removal discards and the one probability flow multiplies by zero), so the generator ends in the same state."""
    g = golden("pc_generic_loop")
    states = {}
    for route in ("native", "torch"):
        if route == "torch":
            monkeypatch.setenv("ZEDO_GENERIC_PC", "torch")
        else:
            monkeypatch.delenv("ZEDO_GENERIC_PC", raising=False)
        fn, sde = make_fn(CASE[tag], 70, hint=10)
        torch.manual_seed(0)
        x, _ = run_chain(fn, sde, model, g["x"], 10)
        assert np.isfinite(x).all()
        states[route] = torch.cuda.get_rng_state().clone()
    assert torch.equal(states["native"], states["torch"])


# ---- 8. invariants -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", CASE_IDS)
def test_device_twin_determinism_and_the_callers_tensor(model, golden, monkeypatch, tag):
    g = golden("pc_generic_loop")
    x0 = g["x"]
    runs = []
    for twin in (False, True, False):
        fn, sde = make_fn(CASE[tag], 70, hint=6)
        monkeypatch.setattr(torch, "randn_like", DetNoise())
        runs.append(run_chain(fn, sde, model, x0, 6, device_twin=twin)[0])
        assert fn.native_plan.hits == 6 and fn.native_plan.misses == 0
    assert np.array_equal(runs[0], runs[1]), "step_device must equal pc_sampler bit for bit"
    assert np.array_equal(runs[0], runs[2]), "two runs must be bit-identical"
    # one call: return types, trajs / res convention, the caller's tensor
    fn, sde = make_fn(CASE[tag], 70, hint=6)
    monkeypatch.setattr(torch, "randn_like", DetNoise())
    x = dev(x0)
    trajs, res = fn(model, condition=torch.zeros(70, 17, 2, device="cuda"), denoise_x=x, t=torch.tensor(float(sde.T)), t_step=0)
    assert torch.equal(x, dev(x0))
    assert isinstance(trajs, np.ndarray) and trajs.shape == (1, 70, 17, 3) and trajs.dtype == np.float32
    denoise = CASE[tag][6]
    if denoise:
        assert isinstance(res, np.ndarray) and np.array_equal(res, trajs[0])
    else:
        assert isinstance(res, torch.Tensor) and res.is_cuda and not np.array_equal(res.cpu().numpy(), trajs[0])


def test_whole_loop_plan_is_found_with_and_without_the_hint(model, golden, monkeypatch):
    from lib.algorithms.advanced import sampling
    g = golden("pc_generic_loop")
    case = CASE["vp_rd_langevin"]
    fn, sde = make_fn(case, 70, hint=20)
    monkeypatch.setattr(torch, "randn_like", DetNoise())
    with_hint, _ = run_chain(fn, sde, model, g["x"], 20)
    assert (fn.native_plan.hits, fn.native_plan.misses) == (20, 0) and fn.native_plan.plan.S == 20
    assert fn.loop_schedule is None
    # without the hint S is solved from (t, t_step) at the first call with t_step >= 1
    fn2 = sampling.get_pc_sampler(sde=sde, shape=(70, 17, 3), predictor=sampling.get_predictor(case[3]),
                                  corrector=sampling.get_corrector(case[4]), inverse_scaler=lambda v: v, snr=0.16, n_steps=1,
                                  probability_flow=False, continuous=True, denoise=True, eps=0.01, device=torch.device("cuda"))
    monkeypatch.setattr(torch, "randn_like", DetNoise())
    no_hint, _ = run_chain(fn2, sde, model, g["x"], 20)
    assert (fn2.native_plan.hits, fn2.native_plan.misses) == (19, 1) and fn2.native_plan.plan.S == 20
    assert np.array_equal(with_hint, no_hint)
    # a foreign time falls back to a one-entry plan: the same bits as the whole-loop entry
    ts = torch.linspace(1.0, 0.01, 20)
    outs = []
    for t_step in (5, None, 11):
        monkeypatch.setattr(torch, "randn_like", DetNoise())
        before = (fn.native_plan.hits, fn.native_plan.misses)
        _, r = fn(model, condition=None, denoise_x=dev(g["x"]), t=ts[5], t_step=t_step)
        after = (fn.native_plan.hits, fn.native_plan.misses)
        assert after == ((before[0] + 1, before[1]) if t_step == 5 else (before[0], before[1] + 1))
        outs.append(r)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_langevin_mean_is_over_the_batch_of_the_call(model, golden, monkeypatch):
    """The step size of the Langevin corrector comes from means over the rows of the call (reference :281-283): the same 70
    rows inside a 128-row batch take another step.  A predictor-only plan is row-wise: the 70 rows do not change."""
    g = golden("pc_generic_loop")
    rng = np.random.Generator(np.random.Philox(key=[7, 14]))
    x128 = np.concatenate([g["x"], (0.6 * rng.standard_normal((58, 17, 3))).astype(np.float32)])

    class RowNoise(DetNoise):        # the first 70 rows of a draw do not depend on the batch size
        def __call__(self, x):
            gg = np.random.Generator(np.random.Philox(key=[555, self.calls]))
            self.calls += 1
            return torch.tensor(gg.standard_normal((128, 17, 3))[:x.shape[0]], dtype=x.dtype, device=x.device)
    res = {}
    for tag in ("vp_rd_langevin", "subvp_rd_none"):
        for rows, x0 in ((70, g["x"]), (128, x128)):
            fn, sde = make_fn(CASE[tag], rows)
            monkeypatch.setattr(torch, "randn_like", RowNoise())
            _, r = fn(model, condition=None, denoise_x=dev(x0), t=torch.tensor(0.5), t_step=None)
            res[tag, rows] = r[:70]
    assert np.array_equal(res["subvp_rd_none", 70], res["subvp_rd_none", 128])
    assert not np.array_equal(res["vp_rd_langevin", 70], res["vp_rd_langevin", 128])
    assert np.abs(res["vp_rd_langevin", 70] - res["vp_rd_langevin", 128]).max() > 1e-4


def test_chunked_calls_give_the_same_bits_and_langevin_refuses_chunks(zh, tmp_path):
    """ALD and predictor-only plans give the bits of the unchunked call with ZEDO_CHUNK_ROWS=64 (read once per process: child
    processes): at 70 rows, and at 300 rows - the chunk size is rounded up to 256 rows, so it takes more than 256 rows to
    walk two chunks.  A Langevin mean spans the call, so B above the chunk size is ZEDO_E_BADARG."""
    code = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from types import SimpleNamespace as NS
import zedo_hip as zh
from lib.dataset import synthetic as syn
W = zh.Weights(syn.make_weights(0))
f = lambda *v: np.array(v, np.float32)
base = dict(label=f(311.0, 95.5), net_scale=f(-1.9, -4.2), pA=f(1.004, 1.001), pB=f(0.011, 0.004), pC=f(0.09, 0.05))
out = {}
for rows in (70, 300):
    g = np.random.Generator(np.random.Philox(key=[3, rows]))
    x = (0.3 * g.standard_normal((rows, 17, 3))).astype(np.float32)
    z = [torch.tensor(g.standard_normal((rows, 17, 3)).astype(np.float32), device="cuda") for _ in range(3)]
    for name, kw in (("pred", dict(has_predictor=True, corrector=0, n_corr=0, corr=None)),
                     ("ald", dict(has_predictor=True, corrector=2, n_corr=2, corr=f(3e-4, 1e-4))),
                     ("ald_only", dict(has_predictor=False, corrector=2, n_corr=1, corr=f(3e-4, 1e-4)))):
        p = zh.PcPlan(W, NS(**base, **kw))
        for step in (0, 1):
            xn, xm = torch.tensor(x, device="cuda"), torch.empty(rows, 17, 3, device="cuda")
            zh.pc_step(W, p, step, xn, z[:p.n_draws], xm)
            out[f"{name}_{rows}_{step}_x"], out[f"{name}_{rows}_{step}_m"] = xn.cpu().numpy(), xm.cpu().numpy()
    p = zh.PcPlan(W, NS(**base, has_predictor=True, corrector=1, n_corr=1, corr=f(0.05, 0.05)))
    try:
        zh.pc_step(W, p, 0, torch.tensor(x, device="cuda"), z[:2], None)
        out[f"langevin_{rows}"] = np.array("ran")
    except zh.ZedoError as e:
        out[f"langevin_{rows}"] = np.array("refused" if "(code -1)" in str(e) else str(e))
out["ws_300"] = np.int64(zh.workspace_bytes(300))
np.savez(sys.argv[1], **out)
''' % (os.path.join(ROOT, "zedo-release_amd"), ROOT)
    outs = []
    for tag, env in (("full", {}), ("chunk", {"ZEDO_CHUNK_ROWS": "64"})):
        out = str(tmp_path / f"{tag}.npz")
        env_all = {k: v for k, v in os.environ.items() if k != "ZEDO_CHUNK_ROWS"}
        subprocess.run([sys.executable, "-c", code, out], check=True, env={**env_all, **env})
        outs.append(np.load(out))
    keys = [k for k in outs[0].files if k[-2:] in ("_x", "_m")]
    assert len(keys) == 24
    for k in keys:
        assert np.isfinite(outs[0][k]).all() and np.array_equal(outs[0][k], outs[1][k]), k
    assert not np.array_equal(outs[0]["pred_70_0_x"], outs[0]["pred_70_0_m"])
    assert int(outs[1]["ws_300"]) == 256 * (64 + 2048) * 4 < int(outs[0]["ws_300"])       # 300 rows did walk two chunks
    assert [str(outs[0][f"langevin_{r}"]) for r in (70, 300)] == ["ran", "ran"]
    assert [str(outs[1][f"langevin_{r}"]) for r in (70, 300)] == ["ran", "refused"]


# ---- 9. fallback -------------------------------------------------------------------------------------------------------

def test_user_registered_predictor_stays_on_the_torch_route(model, golden, monkeypatch):
    from lib.algorithms.advanced import sampling
    g = golden("pc_generic_loop")

    @sampling.register_predictor(name="pc_native_test_predictor")
    class MyPredictor(sampling.ReverseDiffusionPredictor):
        pass
    try:
        res = {}
        for route in ("default", "torch"):
            if route == "torch":
                monkeypatch.setenv("ZEDO_GENERIC_PC", "torch")
            else:
                monkeypatch.delenv("ZEDO_GENERIC_PC", raising=False)
            fn, sde = make_fn(CASE["vp_rd_langevin"], 70, predictor="pc_native_test_predictor")
            assert fn.native_plan is None
            monkeypatch.setattr(torch, "randn_like", DetNoise())
            res[route], _ = run_chain(fn, sde, model, g["x"], 3)
        assert np.isfinite(res["default"]).all() and np.array_equal(res["default"], res["torch"])
        # and the registered class itself is native, with close but not identical rows
        monkeypatch.delenv("ZEDO_GENERIC_PC", raising=False)
        fn, sde = make_fn(CASE["vp_rd_langevin"], 70)
        assert fn.native_plan is not None
        monkeypatch.setattr(torch, "randn_like", DetNoise())
        nat, _ = run_chain(fn, sde, model, g["x"], 3)
        assert np.abs(nat - res["torch"]).max() < 1e-4 * max(1.0, np.abs(nat).max())
    finally:
        del sampling._PREDICTORS["pc_native_test_predictor"]


def test_combinations_that_raise_in_the_reference_keep_raising(model, golden):
    g = golden("pc_generic_loop")
    for case, err in ((("x", "subvpsde", True, "ancestral_sampling", "none", False, True, None, 1), NotImplementedError),
                      (("x", "subvpsde", True, "euler_maruyama", "langevin", False, True, None, 1), AttributeError),
                      (("x", "vpsde", True, "ancestral_sampling", "none", True, True, None, 1), AssertionError)):
        fn, sde = make_fn(case, 70)
        assert fn.native_plan is None
        with pytest.raises(err):
            fn(model, condition=None, denoise_x=dev(g["x"]), t=torch.tensor(0.5), t_step=0)
