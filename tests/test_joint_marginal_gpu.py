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
import ctypes

import numpy as np
import pytest

from _joint_marginal_ref import (IDS, MARGINAL_CASES, cov_bound, joint_marginal_ref, marg_bound, mean_bound, reference, softmax_bound,
                                 softmax_ref, spread_of)
from _joint_ref import case as reproj_case
from _joint_temporal_ref import camera_frame, case, dead_joint_case
from _shared import dev, one_arithmetic_mode, problem, zh  # noqa: F401  (fixtures; one_arithmetic_mode is autouse)
from _temporal_ref import clips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAM, TAU = 100.0, 1.0


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def all_same(out, ref):
    return len(out) == len(ref) and all(same(a, b) for a, b in zip(out, ref))


def run(zh, x, T, u, seq, lam=LAM, tau=TAU, weights=True):
    out = zh.joint_marginal(dev(u, torch.float64), dev(x), None if T is None else dev(T), seq, lam=lam, tau=tau, return_weights=weights)
    return [t.cpu().numpy() for t in out]


def hold_to(out, r, x, T, N, L, tag):
    """Every output against the reference r within the derived bounds; prints observed against bound.  -> the largest log-marginal error."""
    mean, cov, hmax, wmax, logz, w = out
    H = w.shape[2]
    beta = marg_bound(min(L, N), H, r["G"])
    live = ~r["dead"]
    assert np.array_equal(np.isnan(mean[:, :, 0]), r["dead"]) and (w[r["dead"]] == 0.0).all()
    big = r["w"] > 1e-300
    with np.errstate(invalid="ignore"):                              # a dead (frame, joint): -inf - -inf, not among `big`
        lw_ref = (r["A"] + r["B"] - r["logz"][:, :, None])[big]
    assert (w[big] > 0).all()
    e_lw = float(np.abs(np.log(w[big].astype(np.longdouble)) - lw_ref).max())
    e_sum = float(np.abs(w.sum(2)[live] - 1.0).max())
    e_lz = float(np.abs(logz[live] - r["logz"][live]).max())
    spread, xmax = spread_of(x, T, N)
    mb, cb = mean_bound(beta, xmax), cov_bound(beta, spread, xmax)[:, :, None]
    e_mean = float(np.abs(mean - r["mean"])[live].max())
    e_cov = np.abs(cov - r["cov"])
    print(f"joint-marginal {tag}: G = {r['G']:.3g}; max |log w - ref| = {e_lw:.3e}, |sum w - 1| = {e_sum:.3e}, |logz - ref| = {e_lz:.3e} "
          f"(bound {beta:.3e}); |mean - ref| = {e_mean:.3e} m (bound {mb:.3e}); |cov - ref| = {e_cov[live].max():.3e} m^2 (smallest bound "
          f"{cb[live].min():.3e}); hmax differs on {int((hmax != r['hmax']).sum())} of {hmax.size}")
    assert e_lw <= beta and e_sum <= beta and e_lz <= beta
    assert e_mean <= mb and (e_cov[live] <= np.broadcast_to(cb, cov.shape)[live]).all()
    # the arg-max: the lowest h with the largest of the marginals as written, and the reference's wherever its runner-up is clear of the bound
    assert np.array_equal(hmax[live], np.argmax(w, axis=2)[live]) and np.array_equal(wmax[live], w.max(axis=2)[live])
    assert (hmax[r["dead"]] == 0).all() and (wmax[r["dead"]] == 0.0).all() and np.isneginf(logz[r["dead"]]).all()
    if H > 1:
        top2 = np.sort(r["w"], axis=2)[:, :, -2:]
        with np.errstate(divide="ignore", invalid="ignore"):
            clear = live & (np.log(top2[:, :, 1]) - np.log(top2[:, :, 0]) > 2 * beta)
        assert np.array_equal(hmax[clear], r["hmax"][clear])
    return e_lw


@pytest.mark.parametrize("J,N,H,L", MARGINAL_CASES, ids=IDS)
def test_marginals_mean_and_covariance_match_the_float64_reference(zh, J, N, H, L):
    x, T, u = case(J, N, H)
    out = zh.joint_marginal(dev(u, torch.float64), dev(x), dev(T), clips(N, L), lam=LAM, tau=TAU, return_weights=True)
    for t, shape, dt in zip(out, ((N, J, 3), (N, J, 6), (N, J), (N, J), (N, J), (N, J, H)),
                            (torch.float64, torch.float64, torch.int32, torch.float64, torch.float64, torch.float64)):
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
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    nbytes = zh._lib.zedo_joint_marginal_workspace_bytes(N, H, J)
    sd = torch.tensor(seq, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_w in (True, False):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        assert bool(torch.isnan(ws[:nbytes // 8 * 8].view(torch.float64)).all())
        o = [torch.full(s, -7, dtype=d, device="cuda") for s, d in (((N, J, 3), torch.float64), ((N, J, 6), torch.float64), ((N, J), torch.int32),
                                                                     ((N, J), torch.float64), ((N, J), torch.float64), ((N, J, H), torch.float64))]
        assert zh._lib.zedo_joint_marginal(P(ud), P(xd), P(Td), P(sd), len(seq) - 1, H, N, J, LAM, TAU, P(ws), nbytes, P(o[0]), P(o[1]), P(o[2]),
                                           P(o[3]), P(o[4]), P(o[5]) if with_w else None, st) == 0
        torch.cuda.synchronize()
        assert all_same(o[:5], ref[:5]) and (same(o[5], ref[5]) if with_w else bool((o[5] == -7).all()))
    # a side stream, seq_start as a device tensor (warms the allocator for the capture)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o = zh.joint_marginal(ud, xd, Td, sd, lam=LAM, tau=TAU, return_weights=True)
    torch.cuda.synchronize()
    assert all_same(o, ref)
    # captured (a single branch) and replayed: the call allocates nothing and synchronises nothing of its own
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = zh.joint_marginal(ud, xd, Td, sd, N=N, lam=LAM, tau=TAU, return_weights=True)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all_same(out, ref)
    # d_x 12 bytes past a 16-byte boundary
    buf = torch.empty(H * N * J * 3 + 3, dtype=torch.float32, device="cuda")
    xb = buf[3:].view(H * N, J, 3)
    xb.copy_(xd)
    assert xd.data_ptr() % 16 == 0 and xb.data_ptr() % 16 == 12 and xb.is_contiguous()
    assert all_same(zh.joint_marginal(ud, xb, Td, seq, lam=LAM, tau=TAU, return_weights=True), ref)


def test_clip_offsets_that_break_the_rules_are_clamped(zh):
    """Offsets outside 0 .. N are clamped and never become addresses: [0, N + 1000] and [-5, N] are the one clip [0, N]."""
    J, N, H = 5, 12, 3
    x, T, u = case(J, N, H)
    xd, Td, ud = dev(x), dev(T), dev(u, torch.float64)
    ref = zh.joint_marginal(ud, xd, Td, [0, N], return_weights=True)
    for seq in ([0, N + 1000], [-5, N]):
        assert all_same(zh.joint_marginal(ud, xd, Td, seq, N=N, return_weights=True), ref), seq


def test_refusals_at_the_raw_abi(zh):
    """Every NULL pointer other than d_T and d_w, non-positive size, H > 1024, n_seq > N, N J H above INT_MAX, a negative / NaN / infinite
    lambda, tau of 0, negative, NaN and inf, and a misaligned workspace: ZEDO_E_BADARG; a workspace one byte short: ZEDO_E_WORKSPACE;
    nothing written either way.  The same call with valid arguments is accepted, with and without d_T."""
    lib = zh._lib
    P = lambda t: ctypes.c_void_p(t.data_ptr())
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
    ws = torch.full((need + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    outs = [torch.full(s, -7, dtype=d, device="cuda") for s, d in (((N, J, 3), torch.float64), ((N, J, 6), torch.float64), ((N, J), torch.int32),
                                                                    ((N, J), torch.float64), ((N, J), torch.float64), ((N, J, H), torch.float64))]
    ptrs = [P(ud), P(xd), P(Td), P(sd), P(ws)] + [P(t) for t in outs]

    def call(p=ptrs, n_seq=len(seq) - 1, h=H, n=N, j=J, lam=LAM, tau=TAU, nbytes=need):
        return lib.zedo_joint_marginal(p[0], p[1], p[2], p[3], n_seq, h, n, j, lam, tau, p[4], nbytes, p[5], p[6], p[7], p[8], p[9], p[10], None)

    for k in (0, 1, 3, 4, 5, 6, 7, 8, 9):
        assert call([None if i == k else p for i, p in enumerate(ptrs)]) == -1, k
    assert call(n_seq=0) == -1 and call(n_seq=N + 1) == -1 and call(h=0) == -1 and call(n=0) == -1 and call(j=0) == -1
    assert call(h=-1) == -1 and call(n=-3) == -1 and call(j=-1) == -1
    assert call(h=1025, nbytes=2 ** 40) == -1
    assert call(h=2 ** 10, n=2 ** 16, j=2 ** 5, nbytes=2 ** 40) == -1 and call(h=1, n=2 ** 30, j=2, nbytes=2 ** 40) == -1
    assert call(lam=-1.0) == -1 and call(lam=float("nan")) == -1 and call(lam=float("inf")) == -1
    for tau in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(tau=tau) == -1, tau
    assert call([ctypes.c_void_p(ws.data_ptr() + 4) if i == 4 else p for i, p in enumerate(ptrs)]) == -1
    assert call(nbytes=need - 1) == -3 and call(nbytes=0) == -3
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs) and bool((ws == 0x5A).all())
    assert call() == 0                                               # the control
    torch.cuda.synchronize()
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
