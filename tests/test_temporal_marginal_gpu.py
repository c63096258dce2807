"""GPU: zedo_temporal_marginal - per clip the posterior marginals of the WHOLE hypotheses under the chain model zedo_temporal_select
optimises, at a temperature tau (forward-backward in the log domain, fp64), the posterior mean pose, every joint's covariance and the most
probable hypothesis of every frame (csrc/zedo_temporal_marginal.hip).  Held to the float64 reference of tests/_temporal_marginal_ref.py
(pinned on its own in tests/test_temporal_marginal_ref.py) through _joint_marginal_ref.hold_marginals: the log-marginals, |sum_h w - 1| and
logZ within beta = 4 L (H + 8 + 2 (J + 5) G) 2^-53 (derived beside the reference), the mean and the covariance within the bounds that
follow from it, and the arg-max of EVERY live frame (left_out_cap = 0: the reference's two largest log-marginals are at least 1.25e-3
apart, 2 beta is below 2e-7 - test_temporal_marginal_ref.py asserts the condition).  The bits do not depend on the chunk of transition
costs the workspace holds, on the workspace's content, the stream, capture, the alignment of d_x or d_w.  The limits tie it to shipped code:
tau -> 0 is the path of zedo_temporal_select, clips of one frame and lambda = 0 are a softmax, J = 1 without T is zedo_joint_marginal.
Whether the fused pose is closer to ground truth than a selected one is not measured here or anywhere: these tests hold the arithmetic.
The fusion does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, clamped_offsets, cur_stream, dirty, launch_invariant, ptr as P, refusal_sweep, same, sentinels
from _joint_marginal_ref import joint_marginal_ref, marg_bound as joint_marg_bound, mean_bound, softmax_bound, softmax_ref
from _joint_ref import case as reproj_case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_marginal_ref import (CASES, IDS, LAMBDAS, TAUS, case, chain_ref, clips, dead_frame_case, hold_pose_marginals, marg_bound,
                                    reference, temporal_marginal_ref, translation)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAM, TAU = 100.0, 1.0
SHAPES = lambda N, J, H: (((N, J, 3), torch.float64), ((N, J, 6), torch.float64), ((N,), torch.int32), ((N,), torch.float64),
                          ((N,), torch.float64), ((N, H), torch.float64))


def run(zh, x, T, u, seq, lam=LAM, tau=TAU, chunk=0):
    out = zh.temporal_marginal(dev(u, torch.float64), dev(x), None if T is None else dev(T), seq, lam=lam, tau=tau, chunk_frames=chunk,
                               return_weights=True)
    return [t.cpu().numpy() for t in out]


def hold_to(out, r, x, T, N, L, tag):
    """Every output against the reference r within the derived bounds, no arg-max left out; prints observed against bound."""
    s = hold_pose_marginals(out, r, x, T, N, L)
    print(f"temporal-marginal {tag}: G = {r['G']:.3g}; max |log w - ref| = {s['e_lw']:.3e} ({100 * s['e_lw'] / s['beta']:.2f} % of beta = "
          f"{s['beta']:.3e}), |sum w - 1| = {s['e_sum']:.3e}, |logz - ref| = {s['e_lz']:.3e}; |mean - ref| = {s['e_mean']:.3e} m (bound "
          f"{s['mean_bound']:.3e}); |cov - ref| = {s['e_cov']:.3e} m^2 (smallest bound {s['cov_bound']:.3e}); hmax differs on "
          f"{s['hmax_differs']}, left out {s['not_clear']} of {out[2].size} frames x J")
    assert s["not_clear"] == 0
    return s


@pytest.mark.parametrize("J,N,H,L", CASES, ids=IDS)
def test_marginals_mean_and_covariance_match_the_float64_reference(zh, J, N, H, L):
    """Every case at lambda in {30, 100, 300} and tau in {1, 0.25}, with T and with d_T NULL."""
    x, u = case(J, N, H)
    T = translation(N, H)
    xd, ud, Td, seq = dev(x), dev(u, torch.float64), dev(T), clips(N, L)
    for lam in LAMBDAS:
        for tau in TAUS:
            for Tn, Tdev in ((T, Td), (None, None)):
                out = zh.temporal_marginal(ud, xd, Tdev, seq, lam=lam, tau=tau, return_weights=True)
                for t, (shape, dt) in zip(out, SHAPES(N, J, H)):
                    assert tuple(t.shape) == shape and t.dtype == dt
                hold_to([t.cpu().numpy() for t in out], reference(J, N, H, L, lam, tau, Tn is not None), x, Tn, N, L,
                        f"J={J} N={N} H={H} L={L} lambda {lam:g} tau {tau:g}{'' if Tn is not None else ' no T'}")


CHUNK_CASES = [((17, 70, 50), clips(70, 35)), ((17, 130, 130), clips(130, 50)), ((17, 300, 7), clips(300, 300)), ((17, 40, 300), clips(40, 13)),
               ((17, 70, 50), [0, 10, 45, 70])]


@pytest.mark.parametrize("shape,seq", CHUNK_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_the_bits_do_not_depend_on_the_chunk_the_workspace_the_stream_the_alignment_or_d_w(zh, shape, seq):
    """chunk_frames 1, 2, 7 and N give one set of bits - chains that cross many chunk boundaries in both directions, and with [0, 10, 45,
    70] clips that start and end in mid-chunk; then, at chunk_frames = 7: a workspace pre-filled with 0xFF bytes at the raw ABI, with d_w
    and without; a side stream with seq_start as a device tensor; one call captured into a graph and replayed twice; d_x at a 12-byte
    offset."""
    J, N, H = shape
    x, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(translation(N, H)), dev(u, torch.float64)
    ref = zh.temporal_marginal(ud, xd, Td, seq, lam=LAM, tau=TAU, chunk_frames=N, return_weights=True)
    for chunk in (1, 2, 7, 0):
        assert all_same(zh.temporal_marginal(ud, xd, Td, seq, lam=LAM, tau=TAU, chunk_frames=chunk, return_weights=True), ref), chunk
    assert all_same(zh.temporal_marginal(ud, xd, Td, seq, lam=LAM, tau=TAU, chunk_frames=7), ref[:5])   # d_w NULL (through the binding)
    nbytes = zh.temporal_marginal_workspace_bytes(N, H, 7)
    assert nbytes == zh._lib.zedo_temporal_marginal_workspace_bytes(N, H, 7) < zh.temporal_marginal_workspace_bytes(N, H, N)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")

    def raw(ws, o, st, with_w=True):
        return zh._lib.zedo_temporal_marginal(P(ud), P(xd), P(Td), P(sd), len(seq) - 1, H, N, J, LAM, TAU, P(ws), nbytes, P(o[0]), P(o[1]),
                                              P(o[2]), P(o[3]), P(o[4]), P(o[5]) if with_w else None, st)

    o = sentinels(SHAPES(N, J, H))
    assert raw(dirty(nbytes, 0xFF), o, cur_stream(), with_w=False) == 0
    torch.cuda.synchronize()
    assert all_same(o[:5], ref[:5]) and bool((o[5] == -7).all())

    def via_binding(x=xd, seq_on_device=False):
        # under capture N is given: reading it off the device tensor would synchronise
        return zh.temporal_marginal(ud, x, Td, sd if seq_on_device else seq, N=N if torch.cuda.is_current_stream_capturing() else None,
                                    lam=LAM, tau=TAU, chunk_frames=7, return_weights=True)

    launch_invariant(ref, via_binding, xd, raw, SHAPES(N, J, H), nbytes)


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (17, 300, 7, 300), (17, 40, 300, 13)], ids=lambda v: str(v))
def test_a_cold_chain_is_the_viterbi_path(zh, J, N, H, L):
    """tau = 1e-9: any other path costs at least the 1e-6 gap of _temporal_ref.check_inputs more, >= 1000 tau - hmax is the path of
    zedo_temporal_select exactly, and no term of any log-sum-exp may have underflowed on the way: the largest marginal stays above 0.99
    (the reference's lowest is 0.99902, at (17, 300, 7, 300))."""
    x, u = case(J, N, H)
    seq = clips(N, L)
    mean, cov, hmax, wmax, logz, w = run(zh, x, None, u, seq, LAM, 1e-9)
    path, _ = zh.temporal_select(dev(u, torch.float64), dev(x), seq, lam=LAM)
    print(f"tau = 1e-9, J={J} N={N} H={H} L={L}: smallest largest marginal {wmax.min():.6f}")
    assert np.array_equal(hmax, path.cpu().numpy())
    assert np.isfinite(mean).all() and np.isfinite(logz).all() and wmax.min() > 0.99


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (17, 70, 50, 35), (17, 40, 300, 13)], ids=lambda v: str(v))
def test_one_frame_chains_and_lambda_zero_are_a_softmax(zh, J, N, H, L):
    """Clips of one frame at any lambda, and any clips at lambda = 0: w is the per-frame softmax of -u / tau (closed form in numpy), its
    logarithm within _joint_marginal_ref.softmax_bound with the reference's G at these weights.  That bound counts 8 G 2^-53 for the
    error of a recurrence's terms; here there are no terms (one frame) or c m = 0 exactly (lambda = 0), so it holds a fortiori."""
    x, u = case(J, N, H)
    sm = softmax_ref(u[:, None], N, TAU)[:, 0]
    for seq, lam, Lc in ((list(range(N + 1)), LAM, 1), (clips(N, L), 0.0, L)):
        w = run(zh, x, None, u, seq, lam, TAU)[5]
        beta = softmax_bound(Lc, H, chain_ref(u, x, seq, lam, TAU)["G"], np.log(sm))
        e = float(np.abs(np.log(w.astype(np.longdouble)) - np.log(sm)).max())
        print(f"softmax limit J={J} N={N} H={H}, chains of {Lc}, lambda {lam:g}: max |log w - log softmax| = {e:.3e} (bound {beta:.3e})")
        assert e <= beta


@pytest.mark.parametrize("N,H,L", [(7, 2, 7), (40, 50, 13), (6, 300, 3), (3, 1024, 3)], ids=lambda v: str(v))
def test_one_joint_without_T_is_the_joint_wise_call(zh, N, H, L):
    """J = 1, d_T NULL: the pose-level chain IS the joint's chain.  Against zedo_joint_marginal on the same inputs the log-marginals and
    logZ agree within the sum of the two calls' bounds and the mean within the mean bound of that sum - not bit for bit: that call splits
    its sums over parts of the workgroup."""
    x, u = case(1, N, H)
    xd, ud, seq = dev(x), dev(u, torch.float64), clips(N, L)
    mean, cov, hmax, wmax, logz, w = [t.cpu().numpy() for t in zh.temporal_marginal(ud, xd, None, seq, lam=LAM, tau=TAU, return_weights=True)]
    jm, jc, jh, jw, jz, jww = [t.cpu().numpy() for t in zh.joint_marginal(ud[:, None].contiguous(), xd, None, seq, lam=LAM, tau=TAU,
                                                                          return_weights=True)]
    G = chain_ref(u, x, seq, LAM, TAU)["G"]
    beta = marg_bound(min(L, N), H, 1, G) + joint_marg_bound(min(L, N), H, G)
    e = float(np.abs(np.log(w.astype(np.longdouble)) - np.log(jww[:, 0].astype(np.longdouble))).max())
    ez, em = float(np.abs(logz - jz[:, 0]).max()), float(np.abs(mean - jm).max())
    print(f"J = 1 N={N} H={H} L={L} against zedo_joint_marginal: max |log w - log w'| = {e:.3e}, |logz - logz'| = {ez:.3e} (bound {beta:.3e}); "
          f"|mean - mean'| = {em:.3e}")
    assert e <= beta and ez <= beta and em <= mean_bound(beta, float(np.abs(x).max()))
    assert np.array_equal(hmax, jh[:, 0])


def test_excluded_entries_and_a_dead_frame(zh):
    """_temporal_ref.dead_frame_case (H = 3, one clip of 9 frames; frame 4 has no finite unary, frames 2 and 6 an excluded hypothesis):
    NaN, hypothesis 0, 0, -inf and a row of zeros on the dead frame only, the chain split there (two values of logz), w == 0 exactly on
    every excluded entry."""
    x, u = dead_frame_case()
    T = translation(9, 3)
    r = temporal_marginal_ref(u, x, T, [0, 9], LAM, TAU)
    out = run(zh, x, T, u, [0, 9])
    mean, cov, hmax, wmax, logz, w = out
    hold_to(out, r, x, T, 9, 9, "dead frame 4")
    dead = np.arange(9) == 4
    assert np.array_equal(np.isnan(mean).all((1, 2)), dead) and np.array_equal(np.isnan(cov).all((1, 2)), dead)
    assert np.array_equal(np.isnan(mean).any((1, 2)), dead) and np.array_equal(np.isneginf(logz), dead)
    assert hmax[4] == 0 and wmax[4] == 0.0 and (w[4] == 0.0).all()
    assert len(set(logz[:4].tolist())) == 1 and len(set(logz[5:].tolist())) == 1 and logz[3] != logz[5]
    excluded = ~np.isfinite(u.reshape(3, 9).T)
    assert excluded.sum() == 5 and (w[excluded] == 0.0).all() and (w[~excluded & ~dead[:, None]] > 0.0).all()
    # the chunk boundary on the dead frame, before it and behind it: the same bits
    for chunk in (1, 4, 5):
        for a, b in zip(run(zh, x, T, u, [0, 9], chunk=chunk), out):
            assert same(a, b), chunk
    # a larger case: dead frames at a clip boundary, at both ends, and a hypothesis excluded in one frame
    J, N, H, L = 17, 70, 50, 35
    x, u = case(J, N, H)
    u = u.reshape(H, N).copy()
    u[:, 20] = np.nan
    u[:, 34] = np.inf                                                # the last frame of the first clip
    u[:, 35] = -np.inf                                               # the first frame of the second
    u[:, 0] = np.nan                                                 # the first frame of all
    u[:, 69] = np.inf                                                # the last
    u[7, 50] = np.nan
    u = u.reshape(H * N)
    T = translation(N, H)
    out = run(zh, x, T, u, clips(N, L), chunk=3)
    hold_to(out, temporal_marginal_ref(u, x, T, clips(N, L), LAM, TAU), x, T, N, L, "dead frames at clip boundaries")
    assert out[5][50, 7] == 0.0 and (np.flatnonzero(np.isneginf(out[4])) == [0, 20, 34, 35, 69]).all()


def test_clip_offsets_that_break_the_rules_are_clamped(zh):
    """Offsets outside 0 .. N are clamped and never become addresses: [0, N + 1000] and [-5, N] are the one clip [0, N]."""
    J, N, H = 5, 12, 3
    x, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(translation(N, H)), dev(u, torch.float64)
    clamped_offsets(lambda seq: zh.temporal_marginal(ud, xd, Td, seq, N=N, chunk_frames=5, return_weights=True), N)


def test_refusals_at_the_raw_abi_and_the_binding(zh):
    """Every NULL pointer other than d_T and d_w, non-positive size, H > 1024, n_seq > N, H N or N J above INT_MAX, a negative / NaN / infinite
    lambda, tau of 0, negative, NaN and inf, and a misaligned workspace: ZEDO_E_BADARG; a workspace one byte short of ONE frame of
    transition costs: ZEDO_E_WORKSPACE; nothing written either way.  The same call with valid arguments is accepted, with and without
    d_T and d_w, and is what the binding returns."""
    lib = zh._lib
    J, N, H, L = 5, 12, 3, 4
    x, u = case(J, N, H)
    T = translation(N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    seq = clips(N, L)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")
    need = lib.zedo_temporal_marginal_workspace_bytes(N, H, 1)
    assert need == 16 * N * H + 8 * N + 4 * N + 8 * H * H
    ws = dirty(need + 8, 0x5A)
    outs = sentinels(SHAPES(N, J, H))
    ptrs = [P(ud), P(xd), P(Td), P(sd), P(ws)] + [P(t) for t in outs]

    def call(p=ptrs, n_seq=len(seq) - 1, h=H, n=N, j=J, lam=LAM, tau=TAU, nbytes=need):
        return lib.zedo_temporal_marginal(p[0], p[1], p[2], p[3], n_seq, h, n, j, lam, tau, p[4], nbytes, p[5], p[6], p[7], p[8], p[9], p[10], None)

    sizes = [dict(n_seq=0), dict(n_seq=N + 1), dict(h=0), dict(n=0), dict(j=0), dict(h=-1), dict(n=-3), dict(j=-1), dict(h=1025, nbytes=2 ** 40),
             dict(h=2 ** 10, n=2 ** 21, nbytes=2 ** 44), dict(h=2, n=2 ** 30, nbytes=2 ** 40),
             dict(n=2 ** 21, j=2 ** 11, nbytes=2 ** 44)]                       # N J above INT_MAX: one lane per (frame, joint)
    refusal_sweep(call, ptrs, (0, 1, 3, 4, 5, 6, 7, 8, 9), sizes=sizes, weights=("lam",), taus=("tau",), workspace_slot=4, need=need,
                  untouched=[(t, -7) for t in outs] + [(ws, 0x5A)])
    bound = zh.temporal_marginal(ud, xd, Td, seq, lam=LAM, tau=TAU, return_weights=True)              # the binding against the raw call
    assert all_same(outs, bound) and bool((ws[need:] == 0x5A).all())
    hold_to([t.cpu().numpy() for t in outs], reference(J, N, H, L, LAM, TAU), x, T, N, L, "raw ABI")
    assert call([None if i in (2, 10) else p for i, p in enumerate(ptrs)]) == 0                       # d_T and d_w may be NULL
    torch.cuda.synchronize()
    assert all_same(outs[:5], zh.temporal_marginal(ud, xd, None, seq, lam=LAM, tau=TAU)) and same(outs[5], bound[5])
    with pytest.raises(ValueError):
        zh.temporal_marginal(ud[:-1], xd, Td, seq)
    with pytest.raises(ValueError):
        zh.temporal_marginal(ud, xd, Td[:-1], seq)
    with pytest.raises(zh.ZedoError):
        zh.temporal_marginal(ud, xd, Td, seq, tau=0.0)
    with pytest.raises(zh.ZedoError):
        zh.temporal_marginal(torch.zeros((1025,), dtype=torch.float64, device="cuda"), torch.zeros((1025, 1, 3), device="cuda"), None, [0, 1])


def test_pipeline_fuse_temporal(zh, weights0):
    """Pipeline.fuse_temporal on the problem of load() is min_reproj's per-row errors - select_temporal's unaries - fed to
    temporal_marginal."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    err = pipe.select_temporal(xd, Td, [0, 35, N])[2]
    for lam, tau, seq in ((100.0, 1.0, [0, 35, N]), (30.0, 0.5, [0, N])):
        ref = zh.temporal_marginal(err, xd, Td, seq, lam=lam, tau=tau)
        out = pipe.fuse_temporal(xd, Td, seq, lam=lam, tau=tau)
        assert len(out) == 6 and all_same(out[:5], ref) and same(out[5], err)
    with pytest.raises(ValueError):
        pipe.fuse_temporal(xd[:N], Td[:N], [0, N])
