"""GPU: Pipeline.run_pruned - the OIL loop with hypotheses pruned between stages (zedo_min_reproj + zedo_prune_rank + zedo_prune_gather
between zedo_oil_run segments).  Every comparison is exact:
  - run_pruned equals the same stages spelled with the existing calls, the numpy reference for the table (tests/_prune_ref.py) and torch
    indexing for the gather;
  - every surviving row is, bit for bit, the row of the same (hypothesis, pose) of the unpruned Pipeline.run: a row's bits do not depend
    on the batch it is in (tests/test_large_shards_gpu.py) nor on the segments the loop is cut into;
  - the plan "0:H" returns run()'s buffers with an identity table;
  - select_reproj on the survivors, mapped through the table, is the unpruned select_reproj wherever the unpruned winner survived.
OIL_iterations = 40 puts the switch to the least-squares T at step 8: the plan "7:4,8:2" prunes just before and exactly at it.
Both arithmetic modes.  Whether pruning by reprojection error costs accuracy is not measured here or anywhere."""
import numpy as np
import pytest

from _prune_ref import keep_ref
from _shared import zh  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S, SWITCH = 40, 8
PROBLEMS = [(6, 9), (5, 130)]
PLANS = ["0:3", "7:4,8:2", "12:1"]
_cache = {}


def setup(weights0, math_mode, H, N):
    """(pipeline, x, T of the unpruned run), built once per problem and arithmetic mode and left unchanged."""
    key = (H, N, math_mode)
    if key not in _cache:
        from lib.dataset import synthetic as syn
        from zedo_hip.pipeline import Pipeline, ZeDOConfig
        d = syn.make_poses(N, seed=31 + N)
        pipe = Pipeline(weights0, ZeDOConfig.pw3d(OIL_iterations=S)).load(syn.make_clusters(H, seed=31 + H), d["db_2d"], d["camera_param"])
        assert pipe.weights.math == math_mode and pipe.cfg.OIL_iterations // 5 == SWITCH and pipe.singular_poses == 0
        x, T = pipe.run()
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(T).all())
        _cache[key] = (pipe, x, T)
    return _cache[key]


def same(a, b):
    v = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(v(a), v(b))


def spelled(zh, pipe, plan):
    """The stages of run_pruned with existing calls, the numpy table and torch indexing."""
    c, H, N = pipe.cfg, pipe.H, pipe.N
    R, T = zh.ipo_fit(pipe.x0, pipe.uv, pipe.K, c.IPO_keylist, c.RotAxes, c.IPO_T, c.IPO_minScaleT, c.IPO_maxScaleT, c.IPO_iterations,
                      N * len(c.IPO_keylist) * 2, H * N)
    x = zh.rotate_init(pipe.x0, R, N)
    hyp = torch.arange(H, dtype=torch.int32, device="cuda")[:, None].expand(H, N).contiguous()
    begin = 0
    for step, keep in plan:
        if step > begin:
            zh.oil_run(pipe.weights, pipe.sched, x, pipe.geom, T, begin, step, SWITCH)
        err, _, _ = zh.min_reproj(x, T, pipe.uv, pipe.K, pipe.conf, N)
        tab = torch.tensor(keep_ref(err.cpu().numpy(), N, keep), device="cuda").long()
        g = (tab * N + torch.arange(N, device="cuda")[None, :]).reshape(-1)
        x, T, hyp = x[g].contiguous(), T[g].contiguous(), hyp.reshape(-1)[g].reshape(keep, N).contiguous()
        begin = step
    zh.oil_run(pipe.weights, pipe.sched, x, pipe.geom, T, begin, S, SWITCH)
    return x, T, hyp


@pytest.mark.parametrize("text", PLANS)
@pytest.mark.parametrize("H,N", PROBLEMS, ids=lambda v: str(v))
def test_run_pruned_is_its_stages_and_its_rows_are_the_unpruned_rows(zh, weights0, math_mode, H, N, text):
    from zedo_hip.pipeline import parse_prune_plan
    pipe, xu, Tu = setup(weights0, math_mode, H, N)
    plan = parse_prune_plan(text, H, S)
    Kf = plan[-1][1]
    x, T, hyp = pipe.run_pruned(text)
    assert x.shape == (Kf * N, 17, 3) and T.shape == (Kf * N, 3) and hyp.shape == (Kf, N) and hyp.dtype == torch.int32
    h = hyp.cpu().numpy()
    assert ((h >= 0) & (h < H)).all() and (np.diff(h, axis=0) > 0).all()                  # the survivors in ascending hypothesis order
    xs, Ts, hs = spelled(zh, pipe, plan)
    assert same(x, xs) and same(T, Ts) and same(hyp, hs)
    x2, T2, hyp2 = pipe.run_pruned(plan)                                                   # the parsed plan is accepted too; same bits again
    assert same(x, x2) and same(T, T2) and same(hyp, hyp2)
    # every surviving row is the unpruned run's row of the same (hypothesis, pose)
    g = (hyp.long() * N + torch.arange(N, device="cuda")[None, :]).reshape(-1)
    dx, dT = int((x.view(torch.int32) != xu[g].view(torch.int32)).sum()), int((T.view(torch.int32) != Tu[g].view(torch.int32)).sum())
    print(f"run_pruned {text} H={H} N={N} [{math_mode}]: {dx} of {x.numel()} words of x and {dT} of {T.numel()} of T differ from the unpruned rows")
    assert same(x, xu[g]) and same(T, Tu[g])
    # the selection on the survivors is the unpruned selection wherever the unpruned winner survived
    bu, iu = pipe.select_reproj(xu, Tu)
    bs, slot = zh.min_reproj(x, T, pipe.uv, pipe.K, pipe.conf, N)[1:]
    picked = hyp[slot.long(), torch.arange(N, device="cuda")]
    survived = (hyp == iu[None, :]).any(0)
    print(f"    the unpruned select_reproj winner survives on {int(survived.sum())} of {N} poses")
    assert same(picked[survived], iu[survived]) and torch.equal(bs[survived].view(torch.int64), bu[survived].view(torch.int64))
    assert bool((bs[~survived] >= bu[~survived]).all())


@pytest.mark.parametrize("H,N", PROBLEMS, ids=lambda v: str(v))
def test_the_identity_plan_returns_the_unpruned_buffers(zh, weights0, math_mode, H, N):
    pipe, xu, Tu = setup(weights0, math_mode, H, N)
    ident = torch.arange(H, dtype=torch.int32, device="cuda")[:, None].expand(H, N)
    for plan in (f"0:{H}", f"{SWITCH}:{H}", []):
        x, T, hyp = pipe.run_pruned(plan)
        assert same(x, xu) and same(T, Tu) and same(hyp, ident.contiguous()), plan


def test_run_pruned_refuses_what_run_refuses_and_bad_plans(zh, weights0, math_mode):
    H, N = PROBLEMS[0]
    pipe = setup(weights0, math_mode, H, N)[0]
    for bad in ("8:4,7:2", "7:4,8:4", "7:0", f"7:{H + 1}", f"{S}:2", "junk", [(7, 4), (8, 4)], [(-1, 2)]):
        with pytest.raises(ValueError):
            pipe.run_pruned(bad)
    with pytest.raises(ValueError):
        pipe.run_pruned("12:1", oil_steps=12)                                             # the step is outside a 12-step run
    x, T, hyp = pipe.run_pruned("7:2", oil_steps=8)                                       # a shorter run: like run(oil_steps=8)
    xr, Tr = pipe.run(oil_steps=8)
    g = (hyp.long() * N + torch.arange(N, device="cuda")[None, :]).reshape(-1)
    assert same(x, xr[g]) and same(T, Tr[g])
    pipe.singular_poses, keep = 3, pipe.singular_poses
    try:
        with pytest.raises(zh.ZedoError):
            pipe.run_pruned("7:2")                                                        # the loop would reach the least-squares T
        pipe.run_pruned("7:2", oil_steps=8)                                               # ... and this one does not
    finally:
        pipe.singular_poses = keep
