"""GPU: zedo_joint_accel_marginal - for every joint of every clip the posterior marginals of the hypotheses under the chain over PAIRS of
hypotheses that zedo_joint_accel_select optimises, at a temperature tau (forward-backward over pairs in the log domain, fp64), the
posterior mean position, its covariance and the most probable hypothesis (forward and backward kernels of
csrc/zedo_joint_accel_marginal.hip).  Held to the float64 reference of tests/_joint_accel_marginal_ref.py (pinned on its own in
tests/test_joint_accel_marginal_ref.py): the log-marginals, logZ and |sum_h w - 1| within accel_marg_bound, the mean and the covariance
within the bounds that follow from it (mean_bound, cov_bound of _joint_marginal_ref); asserted, and the share of the bound each case uses
is printed.  The limits tie it to shipped code: lambda_a = 0 is zedo_joint_marginal, tau -> 0 the paths of zedo_joint_accel_select,
clips of one frame a softmax, clips of two the first-order chain.  A dead (frame, joint) and excluded entries; bit identity across a
dirty workspace, a side stream, stream capture, the alignment of d_x and d_w NULL or not; the refusals of the raw ABI; the pipeline's
method.  Whether the fused pose is closer to ground truth than any other is not measured here or anywhere: these tests hold the
arithmetic.  The fusion does not depend on the arithmetic mode of the dense layers: one session runs it."""
import numpy as np
import pytest

from _invariance import all_same, clamped_offsets, cur_stream, dirty, launch_invariant, ptr as P, refusal_sweep, same, sentinels
from _joint_accel_marginal_ref import (COLD_CASES, COLD_TAU, IDS, MARGINAL_CASES, SMALL_CASES, WEIGHTS, accel_marg_bound, check_inputs,
                                       joint_accel_marginal_ref, reference)
from _joint_marginal_ref import cov_bound, hold_marginals, joint_marginal_ref, marg_bound, mean_bound, softmax_ref, spread_of
from _joint_ref import case as reproj_case
from _joint_temporal_ref import case, dead_joint_case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAM_V, LAM_A, TAU = WEIGHTS[1]
SHAPES = lambda N, J, H: (((N, J, 3), torch.float64), ((N, J, 6), torch.float64), ((N, J), torch.int32), ((N, J), torch.float64),
                          ((N, J), torch.float64), ((N, J, H), torch.float64))


def run(zh, x, T, u, seq, lam_v=LAM_V, lam_a=LAM_A, tau=TAU):
    out = zh.joint_accel_marginal(dev(u, torch.float64), dev(x), None if T is None else dev(T), seq, lam=lam_v, accel=lam_a, tau=tau,
                                  return_weights=True)
    return [t.cpu().numpy() for t in out]


def log_diff(w, w_ref):
    big = w_ref > 1e-300
    assert (w[big] > 0).all()
    return float(np.abs(np.log(w[big].astype(np.longdouble)) - np.log(w_ref[big].astype(np.longdouble))).max()) if big.any() else 0.0


def hold_to(out, r, x, T, N, L, tag):
    """Every output against the reference r within the derived bounds; prints observed against bound.  -> (the share of the bound the
    log-marginals, logZ and the sums use, the share of live (frame, joint) whose arg-max is not compared)."""
    H = out[5].shape[2]
    with np.errstate(divide="ignore"):
        log_w = np.log(r["w"].astype(np.longdouble))
    s = hold_marginals(out, log_w_ref=log_w, logz_ref=r["logz"], mean_ref=r["mean"], cov_ref=r["cov"], hmax_ref=r["hmax"], w_ref=r["w"],
                       dead=r["dead"], beta=accel_marg_bound(min(L, N), H, r["G"]), x=x, T=T, N=N, left_out_cap=0.01 if H > 1 else None)
    share = max(s["e_lw"], s["e_sum"], s["e_lz"]) / s["beta"]
    print(f"joint-accel-marginal {tag}: G = {r['G']:.3g}; max |log w - ref| = {s['e_lw']:.3e}, |sum w - 1| = {s['e_sum']:.3e}, |logz - ref| = "
          f"{s['e_lz']:.3e} (bound {s['beta']:.3e}: {100 * share:.3f} % used); |mean - ref| = {s['e_mean']:.3e} m (bound {s['mean_bound']:.3e}); "
          f"|cov - ref| = {s['e_cov']:.3e} m^2 (smallest bound {s['cov_bound']:.3e}); hmax not compared on {100 * s['left_out']:.2f} % of the live "
          f"(frame, joint)")
    return share, s["left_out"]


def test_the_inputs_are_what_the_exact_comparisons_assume():
    """On the reference alone (no GPU call): at most 1 % of the live (frame, joint) of any case are left out of the arg-max comparison,
    and at tau = 1e-9 the largest marginal is at least 0.99 everywhere on the cases of the cold limit."""
    worst, cold = check_inputs(verbose=False)
    assert worst <= 0.01 and cold >= 0.99


@pytest.mark.parametrize("J,N,H,L", MARGINAL_CASES, ids=IDS)
def test_marginals_mean_and_covariance_match_the_float64_reference(zh, J, N, H, L):
    """Every case at (lambda_v, lambda_a, tau) = (30, 100, 1); the small cases at the other weight sets as well."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    for lam_v, lam_a, tau in (WEIGHTS if (J, N, H, L) in SMALL_CASES else WEIGHTS[1:2]):
        out = zh.joint_accel_marginal(ud, xd, Td, clips(N, L), lam=lam_v, accel=lam_a, tau=tau, return_weights=True)
        for t, (shape, dt) in zip(out, SHAPES(N, J, H)):
            assert tuple(t.shape) == shape and t.dtype == dt
        hold_to([t.cpu().numpy() for t in out], reference(J, N, H, L, lam_v, lam_a, tau), x, T, N, L,
                f"J={J} N={N} H={H} L={L} lambda_v={lam_v:g} lambda_a={lam_a:g} tau={tau:g}")


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (2, 9, 63, 9)], ids=lambda v: str(v))
def test_without_T(zh, J, N, H, L):
    """d_T = NULL: the motion terms on x alone, the mean in the frame of x."""
    x, T, u = case(J, N, H)
    hold_to(run(zh, x, None, u, clips(N, L)), reference(J, N, H, L, LAM_V, LAM_A, TAU, False), x, None, N, L, f"J={J} N={N} H={H} L={L} no T")


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (1, 20, 17, 20), (3, 40, 64, 9), (3, 130, 7, 130)], ids=lambda v: str(v))
def test_without_the_second_order_term_it_is_the_first_order_fusion(zh, J, N, H, L):
    """lambda_a = 0: the outputs of zedo_joint_marginal on the GPU - log-marginals and logZ within the sum of the two bounds, the mean and
    the covariance within what follows from that sum - with and without T."""
    x, T, u = case(J, N, H)
    xd, Td, ud, seq = dev(x), dev(T), dev(u, torch.float64), clips(N, L)
    for Tq, Tn, lam, tau in ((Td, T, 100.0, 1.0), (None, None, 30.0, 0.25)):
        first = [t.cpu().numpy() for t in zh.joint_marginal(ud, xd, Tq, seq, lam=lam, tau=tau, return_weights=True)]
        out = [t.cpu().numpy() for t in zh.joint_accel_marginal(ud, xd, Tq, seq, lam=lam, accel=0.0, tau=tau, return_weights=True)]
        beta = (marg_bound(min(L, N), H, joint_marginal_ref(u, x, Tn, seq, lam, tau)["G"])
                + accel_marg_bound(min(L, N), H, joint_accel_marginal_ref(u, x, Tn, seq, lam, 0.0, tau)["G"]))
        e_lw, e_lz = log_diff(out[5], first[5]), float(np.abs(out[4] - first[4]).max())
        spread, xmax = spread_of(x, Tn, N)
        print(f"lambda_a = 0, J={J} N={N} H={H} L={L} lambda={lam:g} tau={tau:g}: max |log w - zedo_joint_marginal| = {e_lw:.3e}, |logz| "
              f"{e_lz:.3e} (sum of the bounds {beta:.3e})")
        assert e_lw <= beta and e_lz <= beta
        assert np.abs(out[0] - first[0]).max() <= mean_bound(beta, xmax)
        assert (np.abs(out[1] - first[1]) <= cov_bound(beta, spread, xmax)[:, :, None]).all()


@pytest.mark.parametrize("J,N,H,L", COLD_CASES, ids=lambda v: str(v))
def test_a_cold_chain_is_the_second_order_viterbi_path(zh, J, N, H, L):
    """tau = 1e-9: hmax is the path of zedo_joint_accel_select exactly, on every (frame, joint) - the input check holds that the
    reference's largest marginal is at least 0.99 everywhere on these cases, and the kernel's is checked here: no term of any
    log-sum-exp may have underflowed on the way."""
    x, T, u = case(J, N, H)
    seq = clips(N, L)
    mean, cov, hmax, wmax, logz, w = run(zh, x, T, u, seq, 30.0, 100.0, COLD_TAU)
    path, _ = zh.joint_accel_select(dev(u, torch.float64), dev(x), dev(T), seq, lam=30.0, accel=100.0)
    print(f"tau = 1e-9, J={J} N={N} H={H} L={L}: smallest largest marginal {wmax.min():.6f}")
    assert np.isfinite(mean).all() and np.isfinite(logz).all() and wmax.min() >= 0.99
    assert np.array_equal(hmax, path.cpu().numpy())


@pytest.mark.parametrize("J,N,H,L", [(5, 12, 3, 4), (17, 70, 50, 35), (3, 40, 64, 9)], ids=lambda v: str(v))
def test_clips_of_one_and_two_frames(zh, J, N, H, L):
    """Clips of one frame at any weights: w is the per-(frame, joint) softmax of -u / tau (closed form in numpy).  Clips of two frames have
    no second difference: the outputs of zedo_joint_marginal on the GPU, whatever lambda_a."""
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    sm = softmax_ref(u, N, TAU)
    for lam_v, lam_a in ((0.0, 0.0), (30.0, 1e6)):
        w = run(zh, x, T, u, clips(N, 1), lam_v, lam_a, TAU)[5]
        G = max(float(np.abs(u).max()) / TAU, 4.0 * np.sqrt(3.0) * float(spread_of(x, T, N)[1]) * (lam_v + lam_a) / TAU)
        beta = accel_marg_bound(1, H, G) + 2.0 ** -52 * max(1.0, float(np.abs(np.log(sm)).max()))
        e = log_diff(w, sm)
        print(f"clips of one frame J={J} N={N} H={H} lambda_v={lam_v:g} lambda_a={lam_a:g}: max |log w - log softmax| = {e:.3e} (bound {beta:.3e})")
        assert e <= beta
    first = [t.cpu().numpy() for t in zh.joint_marginal(ud, xd, Td, clips(N, 2), lam=30.0, tau=TAU, return_weights=True)]
    G1, G2 = joint_marginal_ref(u, x, T, clips(N, 2), 30.0, TAU)["G"], joint_accel_marginal_ref(u, x, T, clips(N, 2), 30.0, 0.0, TAU)["G"]
    spread, xmax = spread_of(x, T, N)
    ref_bits = None
    for lam_a in (0.0, 1e6):
        out = zh.joint_accel_marginal(ud, xd, Td, clips(N, 2), lam=30.0, accel=lam_a, tau=TAU, return_weights=True)
        ref_bits = ref_bits or out
        assert all_same(out, ref_bits)                               # no term of a chain of two carries lambda_a
        out = [t.cpu().numpy() for t in out]
        beta = marg_bound(2, H, G1) + accel_marg_bound(2, H, G2)     # (G at lambda_a = 0: no term of these chains carries lambda_a)
        assert log_diff(out[5], first[5]) <= beta and np.abs(out[4] - first[4]).max() <= beta
        assert np.abs(out[0] - first[0]).max() <= mean_bound(beta, xmax)


def test_excluded_entries_and_a_dead_frame_joint(zh):
    """The hand-built case of tests/test_joint_accel_ref.py (NaN, +inf and -inf unaries of ONE joint; (frame 4, joint 2) without a finite
    one): NaN, 0 and -inf on that (frame, joint) only, its chain split there (two values of logz), w == 0 exactly on every excluded entry,
    and the other joints return the bits of the untouched unaries; with (frame 1, joint 2) dead as well that joint has chains of one and
    of two frames; and a larger case with dead entries at clip boundaries and one-frame chains."""
    x, T, u, j = dead_joint_case()
    clean = case(5, 9, 3)[2]
    r = joint_accel_marginal_ref(u, x, T, [0, 9], LAM_V, LAM_A, TAU)
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
    assert np.isnan(mean[4, j]).all() and np.isnan(cov[4, j]).all()
    assert hmax[4, j] == 0 and wmax[4, j] == 0.0 and (w[4, j] == 0.0).all()
    assert len(set(logz[:4, j].tolist())) == 1 and len(set(logz[5:, j].tolist())) == 1 and logz[3, j] != logz[5, j]
    assert len(set(logz[:, others[0]].tolist())) == 1
    excluded = ~np.isfinite(u.reshape(3, 9, 5).transpose(1, 2, 0))
    assert excluded.sum() == 5 and (w[excluded] == 0.0).all() and (w[~excluded & ~dead[:, :, None]] > 0.0).all()
    v = u.reshape(3, 9, 5).copy()
    v[:, 1, j] = np.nan                                              # joint j: chains [0, 1), [2, 4) and [5, 9)
    v = v.reshape(27, 5)
    out2 = run(zh, x, T, v, [0, 9])
    hold_to(out2, joint_accel_marginal_ref(v, x, T, [0, 9], LAM_V, LAM_A, TAU), x, T, 9, 9, "dead (frames 1 and 4, joint 2)")
    for a, b in zip(out2, out0):
        assert np.array_equal(a[:, others].view(np.int64 if a.dtype == np.float64 else a.dtype),
                              b[:, others].view(np.int64 if b.dtype == np.float64 else b.dtype))
    # a larger case with dead entries at a clip boundary, chains of one frame and a hypothesis excluded for every joint of a frame
    J, N, H, L = 17, 70, 50, 35
    x, T, u = case(J, N, H)
    u = u.reshape(H, N, J).copy()
    u[:, 20, 3] = np.nan
    u[:, 34, 5] = np.inf                                             # the last frame of the first clip
    u[:, 35, 5] = -np.inf                                            # the first frame of the second
    u[:, 0, 16] = np.nan                                             # the first frame of all
    u[:, 69, 0] = np.inf                                             # the last
    u[:, 22, 3] = np.nan                                             # (21, 3) is a chain of one frame
    u[:, 67, 0] = np.inf                                             # (68, 0) as well, at the end of the clip
    u[7, 50, :] = np.nan
    u = u.reshape(H * N, J)
    out = run(zh, x, T, u, clips(N, L))
    hold_to(out, joint_accel_marginal_ref(u, x, T, clips(N, L), LAM_V, LAM_A, TAU), x, T, N, L, "dead entries at clip boundaries")
    assert (out[5][50, :, 7] == 0.0).all()


@pytest.mark.parametrize("J,N,H,L", [(17, 70, 50, 35), (3, 40, 64, 9), (1, 20, 17, 20), (2, 11, 4, 3)], ids=lambda v: str(v))
def test_the_bits_do_not_depend_on_the_workspace_the_stream_the_alignment_or_d_w(zh, J, N, H, L):
    """A workspace pre-filled with 0xFF bytes at the raw ABI, with d_w and without; a side stream with seq_start as a device tensor; one
    call captured into a graph (a single branch) and replayed twice; d_x at a 12-byte offset."""
    x, T, u = case(J, N, H)
    xd, Td, ud, seq = dev(x), dev(T), dev(u, torch.float64), clips(N, L)
    kw = dict(lam=LAM_V, accel=LAM_A, tau=TAU)
    ref = zh.joint_accel_marginal(ud, xd, Td, seq, return_weights=True, **kw)
    assert np.array_equal(ref[2].cpu().numpy(), reference(J, N, H, L, LAM_V, LAM_A, TAU)["hmax"])
    assert all_same(zh.joint_accel_marginal(ud, xd, Td, seq, **kw), ref[:5])                        # d_w NULL (through the binding)
    # raw ABI: a dirty workspace, with and without d_w
    nbytes = zh._lib.zedo_joint_accel_marginal_workspace_bytes(N, H, J)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")

    def raw(ws, o, st, with_w=True):
        return zh._lib.zedo_joint_accel_marginal(P(ud), P(xd), P(Td), P(sd), len(seq) - 1, H, N, J, LAM_V, LAM_A, TAU, P(ws), nbytes, P(o[0]),
                                                 P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]) if with_w else None, st)

    o = sentinels(SHAPES(N, J, H))
    assert raw(dirty(nbytes, 0xFF), o, cur_stream(), with_w=False) == 0
    torch.cuda.synchronize()
    assert all_same(o[:5], ref[:5]) and bool((o[5] == -7).all())

    def via_binding(x=xd, seq_on_device=False):
        # under capture N is given: reading it off the device tensor would synchronise
        return zh.joint_accel_marginal(ud, x, Td, sd if seq_on_device else seq, N=N if torch.cuda.is_current_stream_capturing() else None,
                                       return_weights=True, **kw)

    launch_invariant(ref, via_binding, xd, raw, SHAPES(N, J, H), nbytes)


def test_clip_offsets_that_break_the_rules_are_clamped(zh):
    """Offsets outside 0 .. N are clamped and never become addresses: [0, N + 1000] and [-5, N] are the one clip [0, N]."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    clamped_offsets(lambda seq: zh.joint_accel_marginal(ud, xd, Td, seq, N=N, return_weights=True), N)


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer other than d_T and d_w, non-positive size, H > 64, n_seq > N, N J H above INT_MAX, a negative / NaN / infinite
    lambda_v or lambda_a, tau of 0, negative, NaN and inf, and a misaligned workspace: ZEDO_E_BADARG; a workspace one byte short:
    ZEDO_E_WORKSPACE; nothing written either way.  The same call with valid arguments is accepted, with and without d_T, and H = 64 is."""
    lib = zh._lib
    J, N, H, L = 5, 12, 3, 4
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    seq = clips(N, L)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")
    need = lib.zedo_joint_accel_marginal_workspace_bytes(N, H, J)
    assert need == N * J * H * H * 8 + N * J * 4
    assert lib.zedo_joint_accel_marginal_workspace_bytes(3, 3, 1) == 27 * 8 + 16                    # the flags padded to 8 bytes
    assert lib.zedo_joint_accel_marginal_workspace_bytes(1, 64, 1) > 0
    for n, h, j in ((0, H, J), (N, 0, J), (N, H, 0), (-1, H, J), (N, 65, J), (N, 1024, J), (2 ** 20, 2 ** 6, 2 ** 5), (2 ** 30, 1, 2)):
        assert lib.zedo_joint_accel_marginal_workspace_bytes(n, h, j) == 0, (n, h, j)
    ws = dirty(need + 8, 0x5A)
    outs = sentinels(SHAPES(N, J, H))
    ptrs = [P(ud), P(xd), P(Td), P(sd), P(ws)] + [P(t) for t in outs]

    def call(p=ptrs, n_seq=len(seq) - 1, h=H, n=N, j=J, lam_v=LAM_V, lam_a=LAM_A, tau=TAU, nbytes=need):
        return lib.zedo_joint_accel_marginal(p[0], p[1], p[2], p[3], n_seq, h, n, j, lam_v, lam_a, tau, p[4], nbytes, p[5], p[6], p[7], p[8],
                                             p[9], p[10], None)

    sizes = [dict(n_seq=0), dict(n_seq=N + 1), dict(h=0), dict(n=0), dict(j=0), dict(h=-1), dict(n=-3), dict(j=-1), dict(h=65, nbytes=2 ** 40),
             dict(h=2 ** 6, n=2 ** 20, j=2 ** 5, nbytes=2 ** 40), dict(h=1, n=2 ** 30, j=2, nbytes=2 ** 40)]
    refusal_sweep(call, ptrs, (0, 1, 3, 4, 5, 6, 7, 8, 9), sizes=sizes, weights=("lam_a", "lam_v"), taus=("tau",), workspace_slot=4, need=need,
                  untouched=[(t, -7) for t in outs] + [(ws, 0x5A)])
    r = reference(J, N, H, L, LAM_V, LAM_A, TAU)
    assert np.array_equal(outs[2].cpu().numpy(), r["hmax"]) and bool((ws[need:] == 0x5A).all())
    assert np.abs(outs[5].cpu().numpy() - r["w"]).max() < 1e-9
    assert call([None if i in (2, 10) else p for i, p in enumerate(ptrs)]) == 0        # d_T and d_w may be NULL
    torch.cuda.synchronize()
    assert np.abs(outs[0].cpu().numpy() - reference(J, N, H, L, LAM_V, LAM_A, TAU, False)["mean"]).max() < 1e-9
    with pytest.raises(ValueError):
        zh.joint_accel_marginal(ud[:-1], xd, Td, seq)
    with pytest.raises(ValueError):
        zh.joint_accel_marginal(ud, xd, Td[:-1], seq)
    with pytest.raises(zh.ZedoError):
        zh.joint_accel_marginal(ud, xd, Td, seq, tau=0.0)
    with pytest.raises(zh.ZedoError, match="at most 64 hypotheses"):
        zh.joint_accel_marginal(torch.zeros((65, 1), dtype=torch.float64, device="cuda"), torch.zeros((65, 1, 3), device="cuda"), None, [0, 1])
    x64, T64, u64 = case(1, 2, 64)                                   # H = 64 is accepted
    assert len(zh.joint_accel_marginal(dev(u64, torch.float64), dev(x64), dev(T64), [0, 2])) == 5


def test_pipeline_fuse_joints_accel(zh, weights0):
    """Pipeline.fuse_joints_accel on the problem of load() is joint_reproj's per-(row, joint) distances fed to joint_accel_marginal."""
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    J, N, H = 17, 70, 5
    x, T, uv, K, conf = reproj_case(J, N, H)
    cl = problem(J, N, H, general=True)[0]
    pipe = Pipeline(weights0, ZeDOConfig.h36m(OIL_iterations=10)).load(cl, np.concatenate([uv, conf[:, :, None]], -1), K)
    xd, Td = dev(x), dev(T)
    jerr = zh.joint_reproj(xd, Td, dev(uv), dev(K), return_rows=True)[2]
    for lam, accel, tau, seq in ((100.0, 100.0, 1.0, [0, 35, N]), (0.0, 300.0, 0.5, [0, N])):
        ref = zh.joint_accel_marginal(jerr, xd, Td, seq, lam=lam, accel=accel, tau=tau)
        out = pipe.fuse_joints_accel(xd, Td, seq, lam=lam, accel=accel, tau=tau)
        assert len(out) == 6 and all_same(out[:5], ref) and same(out[5], jerr)
    with pytest.raises(ValueError):
        pipe.fuse_joints_accel(xd[:N], Td[:N], [0, N])
