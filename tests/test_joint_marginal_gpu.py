"""GPU: zedo_joint_marginal - for every joint of every clip the posterior marginals of the hypotheses under the chain model
zedo_joint_temporal_select optimises, at a temperature tau (forward-backward in the log domain, fp64), the posterior mean position, its
covariance and the most probable hypothesis (forward and backward kernels of csrc/zedo_joint_marginal.hip).  Held to the float64
reference of tests/_joint_marginal_ref.py (pinned on its own in tests/test_joint_marginal_ref.py): the log-marginals and |sum_h w - 1|
within marg_bound = 4 L (H + 8 + 8 G) 2^-53, the mean and the covariance within the bounds that follow from it (mean_bound, cov_bound:
derived in the reference file); asserted, and the difference each case shows is printed beside its bound.  The limits tie it to shipped
code: tau -> 0 is the path of zedo_joint_temporal_select, clips of one frame and lambda = 0 are a softmax, tau -> inf is uniform.  cov is
positive semi-definite; a dead (frame, joint) and excluded entries; bit identity across a dirty workspace, a side stream, stream capture,
the alignment of d_x and d_w NULL or not; the refusals of the raw ABI.
Whether the fused pose is closer to ground truth than a selected one is not measured here or anywhere: these tests hold the arithmetic.
The fusion does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, clamped_offsets, cur_stream, dirty, launch_invariant, ptr as P, refusal_sweep, same, sentinels
from _joint_marginal_ref import (IDS, MARGINAL_CASES, chain_reference, cov_bound, hold_marginals, joint_marginal_ref, marg_bound, reference,
                                 softmax_bound, softmax_ref, spread_of)
from _joint_ref import case as reproj_case
from _joint_temporal_ref import camera_frame, case, dead_joint_case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAM, TAU = 100.0, 1.0
SHAPES = lambda N, J, H: (((N, J, 3), torch.float64), ((N, J, 6), torch.float64), ((N, J), torch.int32), ((N, J), torch.float64),
                          ((N, J), torch.float64), ((N, J, H), torch.float64))


def run(zh, x, T, u, seq, lam=LAM, tau=TAU, weights=True):
    out = zh.joint_marginal(dev(u, torch.float64), dev(x), None if T is None else dev(T), seq, lam=lam, tau=tau, return_weights=weights)
    return [t.cpu().numpy() for t in out]


def hold_to(out, r, x, T, N, L, tag):
    """Every output against the reference r within the derived bounds; prints observed against bound.  -> the largest log-marginal error."""
    s = hold_marginals(out, beta=marg_bound(min(L, N), out[5].shape[2], r["G"]), x=x, T=T, N=N, **chain_reference(r))
    print(f"joint-marginal {tag}: G = {r['G']:.3g}; max |log w - ref| = {s['e_lw']:.3e}, |sum w - 1| = {s['e_sum']:.3e}, |logz - ref| = "
          f"{s['e_lz']:.3e} (bound {s['beta']:.3e}); |mean - ref| = {s['e_mean']:.3e} m (bound {s['mean_bound']:.3e}); |cov - ref| = "
          f"{s['e_cov']:.3e} m^2 (smallest bound {s['cov_bound']:.3e}); hmax differs on {s['hmax_differs']} of {out[2].size}")
    return s["e_lw"]


@pytest.mark.parametrize("J,N,H,L", MARGINAL_CASES, ids=IDS)
def test_marginals_mean_and_covariance_match_the_float64_reference(zh, J, N, H, L):
    x, T, u = case(J, N, H)
    out = zh.joint_marginal(dev(u, torch.float64), dev(x), dev(T), clips(N, L), lam=LAM, tau=TAU, return_weights=True)
    for t, (shape, dt) in zip(out, SHAPES(N, J, H)):
        assert tuple(t.shape) == shape and t.dtype == dt
    hold_to([t.cpu().numpy() for t in out], reference(J, N, H, L, LAM, TAU), x, T, N, L, f"J={J} N={N} H={H} L={L}")


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (2, 30, 130, 13)], ids=lambda v: str(v))
def test_without_T_and_at_other_weights(zh, J, N, H, L):
    """d_T = NULL (the motion term on x alone, the mean in the frame of x) and another lambda and temperature."""
    x, T, u = case(J, N, H)
    hold_to(run(zh, x, None, u, clips(N, L)), reference(J, N, H, L, LAM, TAU, False), x, None, N, L, f"J={J} N={N} H={H} L={L} no T")
    r = joint_marginal_ref(u, x, T, clips(N, L), 30.0, 0.25)
    hold_to(run(zh, x, T, u, clips(N, L), 30.0, 0.25), r, x, T, N, L, f"J={J} N={N} H={H} L={L} lambda 30 tau 0.25")


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (2, 30, 130, 13), (3, 130, 7, 130)], ids=lambda v: str(v))
def test_a_cold_chain_is_the_viterbi_path(zh, J, N, H, L):
    """tau = 1e-9: any other path costs at least the 1e-6 gap of check_inputs more, >= 1000 tau - hmax is the path of
    zedo_joint_temporal_select exactly and the mean is that path's X to 1e-2 relative (G is about 1e11 there: a weight is good to about
    1e-4 only).  No term of any log-sum-exp may have underflowed on the way: the largest marginal stays above 0.99."""
    x, T, u = case(J, N, H)
    seq = clips(N, L)
    mean, cov, hmax, wmax, logz, w = run(zh, x, T, u, seq, LAM, 1e-9)
    path, _ = zh.joint_temporal_select(dev(u, torch.float64), dev(x), dev(T), seq, lam=LAM)
    path = path.cpu().numpy()
    assert np.array_equal(hmax, path)
    Xp = camera_frame(x, T, N)[path, np.arange(N)[:, None], np.arange(J)[None, :]]                 # [N, J, 3]
    rel = np.linalg.norm(mean - Xp, axis=2) / np.linalg.norm(Xp, axis=2)
    print(f"tau = 1e-9, J={J} N={N} H={H} L={L}: smallest largest marginal {wmax.min():.6f}, max |mean - X[path]| / |X[path]| = {rel.max():.3e}")
    assert np.isfinite(mean).all() and np.isfinite(logz).all() and rel.max() <= 1e-2 and wmax.min() > 0.99


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (17, 70, 50, 35), (1, 6, 300, 3)], ids=lambda v: str(v))
def test_one_frame_chains_and_lambda_zero_are_a_softmax_and_a_hot_chain_is_uniform(zh, J, N, H, L):
    """Clips of one frame at any lambda, and any clips at lambda = 0: w is the per-(frame, joint) softmax of -u / tau (closed form in
    numpy), its logarithm within _joint_marginal_ref.softmax_bound: marg_bound of the chain length (G: the reference's at these weights)
    plus the two roundings of the closed form itself.  tau = 1e12: every hypothesis gets
    1 / H to 1e-11."""
    x, T, u = case(J, N, H)
    sm = softmax_ref(u, N, TAU)
    for seq, lam, Lc in ((list(range(N + 1)), LAM, 1), (clips(N, L), 0.0, L)):
        w = run(zh, x, T, u, seq, lam, TAU)[5]
        beta = softmax_bound(Lc, H, joint_marginal_ref(u, x, T, seq, lam, TAU)["G"], np.log(sm))
        e = float(np.abs(np.log(w.astype(np.longdouble)) - np.log(sm)).max())
        print(f"softmax limit J={J} N={N} H={H}, chains of {Lc}, lambda {lam:g}: max |log w - log softmax| = {e:.3e} (bound {beta:.3e})")
        assert e <= beta
    w = run(zh, x, T, u, clips(N, L), LAM, 1e12)[5]
    assert np.abs(w - 1.0 / H).max() <= 1e-11


def test_covariance_is_positive_semi_definite(zh):
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    mean, cov, hmax, wmax, logz, w = run(zh, x, T, u, clips(N, L))
    full = cov[:, :, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(N, J, 3, 3)
    ev = np.linalg.eigvalsh(full)
    spread, xmax = spread_of(x, T, N)
    tol = cov_bound(marg_bound(L, H, reference(J, N, H, L, LAM, TAU)["G"]), spread, xmax)
    print(f"covariance: smallest eigenvalue {ev.min():.3e} m^2 (allowed -{tol.min():.3e}); spread sqrt(trace) in {np.sqrt(ev.sum(-1)).min():.4f} .. "
          f"{np.sqrt(ev.sum(-1)).max():.4f} m")
    assert (ev[:, :, 0] >= -3 * tol).all() and (cov[:, :, [0, 3, 5]] >= 0).all()
    # the trace is bounded by the squared diameter of the hypotheses of that (frame, joint)
    assert (cov[:, :, 0] + cov[:, :, 3] + cov[:, :, 5] <= 3 * spread ** 2).all()


def test_excluded_entries_and_a_dead_frame_joint(zh):
    """The hand-built case of _joint_temporal_ref (NaN, +inf and -inf unaries of ONE joint; (frame 4, joint 2) without a finite one): NaN, 0
    and -inf on that (frame, joint) only, its chain split there (two values of logz), w == 0 exactly on every excluded entry, and the
    other joints return the bits of the untouched unaries."""
    x, T, u, j = dead_joint_case()
    clean = case(5, 9, 3)[2]
    r = joint_marginal_ref(u, x, T, [0, 9], LAM, TAU)
    out = run(zh, x, T, u, [0, 9])
    out0 = run(zh, x, T, clean, [0, 9])
    mean, cov, hmax, wmax, logz, w = out
    hold_to(out, r, x, T, 9, 9, "dead (frame 4, joint 2)")
    others = [i for i in range(5) if i != j]
    for a, b in zip(out, out0):
        assert np.array_equal(a[:, others].view(np.int64 if a.dtype == np.float64 else a.dtype),
                              b[:, others].view(np.int64 if b.dtype == np.float64 else b.dtype))
    dead = np.zeros((9, 5), bool)
    dead[4, j] = True
    assert np.array_equal(np.isnan(mean).any(2), dead) and np.array_equal(np.isnan(cov).any(2), dead) and np.array_equal(np.isneginf(logz), dead)
    assert hmax[4, j] == 0 and wmax[4, j] == 0.0 and (w[4, j] == 0.0).all()
    assert len(set(logz[:4, j].tolist())) == 1 and len(set(logz[5:, j].tolist())) == 1 and logz[3, j] != logz[5, j]
    assert len(set(logz[:, others[0]].tolist())) == 1
    excluded = ~np.isfinite(u.reshape(3, 9, 5).transpose(1, 2, 0))
    assert excluded.sum() == 5 and (w[excluded] == 0.0).all() and (w[~excluded & ~dead[:, :, None]] > 0.0).all()
    # a larger case with dead entries at a clip boundary and a hypothesis excluded for every joint of a frame
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    u = u.reshape(H, N, J).copy()
    u[:, 20, 3] = np.nan
    u[:, 34, 5] = np.inf                                             # the last frame of the first clip
    u[:, 35, 5] = -np.inf                                            # the first frame of the second
    u[:, 0, 16] = np.nan                                             # the first frame of all
    u[:, 69, 0] = np.inf                                             # the last
    u[7, 50, :] = np.nan
    u = u.reshape(H * N, J)
    out = run(zh, x, T, u, clips(N, L))
    hold_to(out, joint_marginal_ref(u, x, T, clips(N, L), LAM, TAU), x, T, N, L, "dead entries at clip boundaries")
    assert (out[5][50, :, 7] == 0.0).all()


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (2, 30, 130, 13), (1, 6, 300, 3), (2, 4, 1000, 4)], ids=lambda v: str(v))
def test_the_bits_do_not_depend_on_the_workspace_the_stream_the_alignment_or_d_w(zh, J, N, H, L):
    """A workspace pre-filled with 0xFF bytes at the raw ABI, with d_w and without; a side stream with seq_start as a device tensor; one
    call captured into a graph (a single branch) and replayed twice; d_x at a 12-byte offset."""
    x, T, u = case(J, N, H)
    xd, Td, ud, seq = dev(x), dev(T), dev(u, torch.float64), clips(N, L)
    ref = zh.joint_marginal(ud, xd, Td, seq, lam=LAM, tau=TAU, return_weights=True)
    assert all_same(zh.joint_marginal(ud, xd, Td, seq, lam=LAM, tau=TAU), ref[:5])                 # d_w NULL (through the binding)
    # raw ABI: a dirty workspace, with and without d_w
    nbytes = zh._lib.zedo_joint_marginal_workspace_bytes(N, H, J)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")

    def raw(ws, o, st, with_w=True):
        return zh._lib.zedo_joint_marginal(P(ud), P(xd), P(Td), P(sd), len(seq) - 1, H, N, J, LAM, TAU, P(ws), nbytes, P(o[0]), P(o[1]), P(o[2]),
                                           P(o[3]), P(o[4]), P(o[5]) if with_w else None, st)

    o = sentinels(SHAPES(N, J, H))
    assert raw(dirty(nbytes, 0xFF), o, cur_stream(), with_w=False) == 0
    torch.cuda.synchronize()
    assert all_same(o[:5], ref[:5]) and bool((o[5] == -7).all())

    def via_binding(x=xd, seq_on_device=False):
        # under capture N is given: reading it off the device tensor would synchronise
        return zh.joint_marginal(ud, x, Td, sd if seq_on_device else seq, N=N if torch.cuda.is_current_stream_capturing() else None, lam=LAM,
                                 tau=TAU, return_weights=True)

    launch_invariant(ref, via_binding, xd, raw, SHAPES(N, J, H), nbytes)


def test_clip_offsets_that_break_the_rules_are_clamped(zh):
    """Offsets outside 0 .. N are clamped and never become addresses: [0, N + 1000] and [-5, N] are the one clip [0, N]."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    clamped_offsets(lambda seq: zh.joint_marginal(ud, xd, Td, seq, N=N, return_weights=True), N)


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer other than d_T and d_w, non-positive size, H > 1024, n_seq > N, N J H above INT_MAX, a negative / NaN / infinite
    lambda, tau of 0, negative, NaN and inf, and a misaligned workspace: ZEDO_E_BADARG; a workspace one byte short: ZEDO_E_WORKSPACE;
    nothing written either way.  The same call with valid arguments is accepted, with and without d_T."""
    lib = zh._lib
    J, N, H, L = 5, 12, 3, 4
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    seq = clips(N, L)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")
    need = lib.zedo_joint_marginal_workspace_bytes(N, H, J)
    assert need == N * J * H * 8 + N * J * 4
    assert lib.zedo_joint_marginal_workspace_bytes(3, 3, 1) == 3 * 3 * 8 + 16                       # padded to 8 bytes
    assert lib.zedo_joint_marginal_workspace_bytes(1, 1024, 1) > 0
    for n, h, j in ((0, H, J), (N, 0, J), (N, H, 0), (-1, H, J), (N, 1025, J), (2 ** 16, 2 ** 10, 2 ** 5), (2 ** 30, 1, 2)):
        assert lib.zedo_joint_marginal_workspace_bytes(n, h, j) == 0, (n, h, j)
    ws = dirty(need + 8, 0x5A)
    outs = sentinels(SHAPES(N, J, H))
    ptrs = [P(ud), P(xd), P(Td), P(sd), P(ws)] + [P(t) for t in outs]

    def call(p=ptrs, n_seq=len(seq) - 1, h=H, n=N, j=J, lam=LAM, tau=TAU, nbytes=need):
        return lib.zedo_joint_marginal(p[0], p[1], p[2], p[3], n_seq, h, n, j, lam, tau, p[4], nbytes, p[5], p[6], p[7], p[8], p[9], p[10], None)

    sizes = [dict(n_seq=0), dict(n_seq=N + 1), dict(h=0), dict(n=0), dict(j=0), dict(h=-1), dict(n=-3), dict(j=-1), dict(h=1025, nbytes=2 ** 40),
             dict(h=2 ** 10, n=2 ** 16, j=2 ** 5, nbytes=2 ** 40), dict(h=1, n=2 ** 30, j=2, nbytes=2 ** 40)]
    refusal_sweep(call, ptrs, (0, 1, 3, 4, 5, 6, 7, 8, 9), sizes=sizes, weights=("lam",), taus=("tau",), workspace_slot=4, need=need,
                  untouched=[(t, -7) for t in outs] + [(ws, 0x5A)])
    r = reference(J, N, H, L, LAM, TAU)
    assert np.array_equal(outs[2].cpu().numpy(), r["hmax"]) and bool((ws[need:] == 0x5A).all())
    assert np.abs(outs[5].cpu().numpy() - r["w"]).max() < 1e-9
    assert call([None if i in (2, 10) else p for i, p in enumerate(ptrs)]) == 0        # d_T and d_w may be NULL
    torch.cuda.synchronize()
    assert np.abs(outs[0].cpu().numpy() - reference(J, N, H, L, LAM, TAU, False)["mean"]).max() < 1e-9
    with pytest.raises(ValueError):
        zh.joint_marginal(ud[:-1], xd, Td, seq)
    with pytest.raises(ValueError):
        zh.joint_marginal(ud, xd, Td[:-1], seq)
    with pytest.raises(zh.ZedoError):
        zh.joint_marginal(ud, xd, Td, seq, tau=0.0)
    with pytest.raises(zh.ZedoError):
        zh.joint_marginal(torch.zeros((1025, 1), dtype=torch.float64, device="cuda"), torch.zeros((1025, 1, 3), device="cuda"), None, [0, 1])


def test_pipeline_fuse_joints_temporal(zh, weights0):
    """Pipeline.fuse_joints_temporal on the problem of load() is joint_reproj's per-(row, joint) distances fed to joint_marginal."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)[2]
    for lam, tau, seq in ((100.0, 1.0, [0, 35, N]), (30.0, 0.5, [0, N])):
        ref = zh.joint_marginal(jerr, xd, Td, seq, lam=lam, tau=tau)
        out = pipe.fuse_joints_temporal(xd, Td, seq, lam=lam, tau=tau)
        assert len(out) == 6 and all_same(out[:5], ref) and same(out[5], jerr)
    with pytest.raises(ValueError):
        pipe.fuse_joints_temporal(xd[:N], Td[:N], [0, N])
