"""What the two sides of a comparison must share, defined once: the noise stream and the case tables of the captures
(tools/gen_golden.py writes a fixture with them, the tests read it with them), the problem builders that
lib.dataset.synthetic does not pin, a BASELINE-size capture regenerated from its fixture's seeds, and the plumbing of the GPU tests.
Imported by the tests, by the child scripts they embed and by tools/ the way tests/_ipo_summary.py is.

Nothing of lib.*, run.*, zedo_hip or zedo_oracle is imported at module level: tools/gen_golden.py runs with the reference's `lib`
first on sys.path, the tests with the mirror's, and each function binds the one its caller has."""
import ctypes
import functools
import hashlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "zedo-release_amd", "zedo_hip", "libzedo_hip.so")


# ---- 1. noise and scores -------------------------------------------------------------------------------------------------

class DetNoise:
    """Replacement for torch.randn_like during capture and test: numpy Philox keyed by the call count, independent of the
    torch build."""

    def __init__(self):
        self.calls = 0

    def __call__(self, x):
        g = np.random.Generator(np.random.Philox(key=[555, self.calls]))
        self.calls += 1
        return torch.tensor(g.standard_normal(tuple(x.shape)), dtype=x.dtype, device=x.device)


class DetNoise32(DetNoise):
    """The same stream rounded to fp32 first: what a float32 run draws, handed to a float64 run unchanged."""

    def __call__(self, x):
        g = np.random.Generator(np.random.Philox(key=[555, self.calls]))
        self.calls += 1
        return torch.tensor(g.standard_normal(tuple(x.shape)).astype(np.float32)).to(x.dtype)


def analytic_score(x, t, condition, mask):
    return -(x - 0.3 * condition) / (0.5 + t)[:, None, None]


def sampler_inputs():
    g = np.random.Generator(np.random.Philox(key=[2024, 3]))
    x = g.standard_normal((6, 17, 3)).astype(np.float32)
    cond = g.standard_normal((6, 17, 3)).astype(np.float32)
    t = np.array([0.9, 0.5, 0.1, 0.013, 0.0005, 0.7], np.float32)     # 0.0005 -> discrete step 0 (VE adjacent sigma = 0)
    return x, cond, t


# ---- 2. case tables ------------------------------------------------------------------------------------------------------

SDE_KW = dict(vpsde=dict(beta_min=0.1, beta_max=20.0, N=1000, T=1.0),
              subvpsde=dict(beta_min=0.1, beta_max=20.0, N=1000, T=1.0),
              vesde=dict(sigma_min=0.01, sigma_max=50.0, N=1000, T=1.0))


def make_sde(sde_lib, name):
    """sde_lib: the caller's module - the reference's in tools/gen_golden.py, the mirror's in the tests."""
    return getattr(sde_lib, dict(vpsde="VPSDE", subvpsde="subVPSDE", vesde="VESDE")[name])(**SDE_KW[name])


def sampler_cases():
    """(sde name) x (predictor, probability_flow) and x (corrector) combinations of tests/golden/samplers.npz."""
    preds = [("euler_maruyama", False), ("euler_maruyama", True), ("reverse_diffusion", False),
             ("reverse_diffusion", True), ("ancestral_sampling", False)]
    corrs = ["langevin", "ald"]
    return list(SDE_KW), preds, corrs


PC_LOOP_CASES = [
    # tag, sde, continuous, predictor, corrector, probability_flow, noise_removal, t (single call; None: chained only), n_steps_each
    ("vp_rd_langevin", "vpsde", True, "reverse_diffusion", "langevin", False, True, 0.31, 1),
    ("vp_anc_none_disc", "vpsde", False, "ancestral_sampling", "none", False, True, 0.52, 1),
    ("vp_em_none_pf", "vpsde", True, "euler_maruyama", "none", True, True, 0.2, 1),
    ("ve_rd_ald", "vesde", True, "reverse_diffusion", "ald", False, True, 0.4, 1),
    ("ve_anc_langevin", "vesde", True, "ancestral_sampling", "langevin", False, False, 0.15, 1),
    ("subvp_em_none_sde", "subvpsde", True, "euler_maruyama", "none", False, False, 0.07, 1),
    ("subvp_rd_none", "subvpsde", True, "reverse_diffusion", "none", False, True, 0.05, 1),
    ("vp_em_langevin", "vpsde", True, "euler_maruyama", "langevin", False, True, None, 2),
]
PC_GENERIC_CASES = [c for c in PC_LOOP_CASES if c[7] is not None]
PC_LOOP_STEPS, PC_LOOP_SNAPS, PC_LOOP_ROWS, PC_LOOP_EPS = 20, (1, 10, 20), 70, 0.01

IPO_CASES = [(N, axes, kname) for N in (8, 64) for axes in ("z", "xyz") for kname in ("h36m", "pw3d")]


# ---- 3. problem builders that lib.dataset.synthetic does not pin ---------------------------------------------------------

IPO_T, IPO_MIN, IPO_MAX = 5.0, 0.5, 2.0
IPO_KEYS = [(2, [0, 1]), (5, [0, 2, 4]), (5, [0, 1, 2, 3, 4]), (21, [0, 1, 4, 20]), (21, list(range(4, 21))), (33, [0, 16, 32]),
            (17, [0, 1, 4])]
KEYS = [(17, [0, 1, 4]), (17, list(range(17))), (5, list(range(5))), (21, [0, 1, 4, 20])]          # the general-intrinsics problems
TWIN_AXES = ["", "x", "y", "xy", "xz", "yz"]                                   # "z" and "xyz": the existing twin tests
# The key-list lengths that IPO_KEYS, KEYS and the keylist_* entries of tests/golden/ipo_custom.npz leave out (tests/test_ipo_key_lists_gpu.py,
# tests/test_ipo_key_lists_ref.py): 5 is coprime to 21, so the k entries (5 i + k) mod 21 are distinct and unsorted; the lists of 10, 11, 15 and 16 reach index 20,
# and the lists of 6, 11, 13 and 16 hold the root, the others do not (tests/test_ipo_key_lists_ref.py pins all of it).  make_ipo_problem(21, N) supplies the problem.
IPO_NEW_LENGTHS = (6, 7, 9, 10, 11, 13, 14, 15, 16)
IPO_LENGTH_KEYS = [(21, [(5 * i + k) % 21 for i in range(k)]) for k in IPO_NEW_LENGTHS]
_K11 = IPO_LENGTH_KEYS[IPO_NEW_LENGTHS.index(11)][1]
# the forms a key list may take beside "ascending, no repeats": the k = 11 list sorted and reversed (the order is a statement about
# rounding only), and a list with two repeated indices (the reference gathers x[:, keylist]; the normaliser counts all 7 entries)
IPO_FORM_KEYS = [(21, sorted(_K11)), (21, _K11[::-1]), (21, [0, 4, 4, 9, 20, 9, 13])]
IPO_FORM_IDS = ["k11-sorted", "k11-reversed", "k7-repeats"]


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def cameras(g, N):
    K = np.zeros((N, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1] = 1145 + 20 * g.standard_normal(N), 1144 + 20 * g.standard_normal(N)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 512 + 5 * g.standard_normal(N), 515 + 5 * g.standard_normal(N), 1
    return K


def general_cameras(g, N):
    from lib.dataset import synthetic as syn
    return syn.general_intrinsics(cameras(g, N), [44, N])


def make_ipo_problem(J, N, H=1):
    """A J-joint problem for the IPO (lib.dataset.synthetic.make_poses is 17-joint and pinned by checksums): H centred random
    cluster poses (0.25 m spread), N detections of a rotated, slightly deformed copy of cluster 0 with its root about 5 m in front
    of the camera, projected with K.  numpy Philox, key [5, J]."""
    g = np.random.Generator(np.random.Philox(key=[5, J]))
    cl = 0.25 * g.standard_normal((H, J, 3))
    cl = cl - cl[:, 0:1]
    K = cameras(g, N)
    q = g.standard_normal((N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, i, j, k = q.T
    R = np.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r), 2 * (i * j + k * r), 1 - 2 * (i * i + k * k),
                  2 * (j * k - i * r), 2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)], -1).reshape(N, 3, 3)
    root = np.stack([0.4 * g.standard_normal(N), 0.4 * g.standard_normal(N), 5 + 0.5 * g.standard_normal(N)], -1)
    p3 = np.einsum("nij,kj->nki", R, cl[0]) + 0.02 * g.standard_normal((N, J, 3)) + root[:, None]
    w = np.einsum("nij,nkj->nki", K.astype(np.float64), p3)
    uv = w[..., :2] / w[..., 2:]
    return cl.astype(np.float32), uv.astype(np.float32), K


def problem(J, N, H=1, general=True):
    """make_ipo_problem; general: its pinhole K replaced by general intrinsics (Philox key [43, 1000 * J + N]) and the detections
    carried over by the homography K_general K_pinhole^-1, i.e. the same 3-D points projected through the general K.
    Returns (clusters [H,J,3], uv [N,J,2], K [N,3,3]), float32."""
    from lib.dataset import synthetic as syn
    cl, uv, Kp = make_ipo_problem(J, N, H)
    if not general:
        return cl, uv, Kp
    K = syn.general_intrinsics(Kp, [43, 1000 * J + N])
    hom = np.concatenate([uv.astype(np.float64), np.ones((N, J, 1))], -1)
    ray = np.einsum("nij,nkj->nki", np.linalg.inv(Kp.astype(np.float64)), hom)
    return cl, syn.project(K, ray), K


def pack(q, sc, mq, vq, ms, vs):
    """An Adam state of the oracle in the layout of zedo_ipo_fit_resume: param[5], exp_avg[5], exp_avg_sq[5]."""
    return np.concatenate([q, sc[:, None], mq, ms[:, None], vq, vs[:, None]], axis=1)


def unpack(st):
    return st[:, 0:4], st[:, 4], st[:, 5:9], st[:, 10:14], st[:, 9], st[:, 14]


# The oracle as the source of optimiser states for zedo_ipo_fit_resume (tests/test_general_intrinsics_gpu.py, tests/test_ipo_state_gpu.py,
# tests/test_ipo_state_ref.py, the single-iteration tests of tests/test_hip_parity.py and tests/test_joint_counts_gpu.py)

def initial_state(N):
    z4, z1 = np.zeros((N, 4)), np.zeros(N)
    q0 = z4.copy()
    q0[:, 0] = 1
    return pack(q0, np.ones(N), z4, z4, z1, z1)


def state_of(t):
    """A trace entry of O.ipo_fit -> the packed state."""
    return pack(t[0], t[1], t[3], t[4], t[5], t[6])


def oracle_args(J, kl, N, general=True):
    import zedo_oracle as O
    cl, uvn, Kn = problem(J, N, 1, general)
    c64, K64 = uvn.astype(np.float64), Kn.astype(np.float64)
    x64 = np.broadcast_to(cl[0][None], (N, J, 3)).astype(np.float64)
    return x64[:, kl], O.ipo_init_T(c64, K64, IPO_T, dtype=np.float64), K64, c64[:, kl]


def oracle_resume(args, axes, norm, state, it0, iters=1, dtype=np.float64, minT=IPO_MIN, maxT=IPO_MAX):
    """``iters`` oracle iterations in ``dtype`` from the packed ``state`` declared to be the one after it0 iterations (state and
    problem are rounded to dtype first: with float32, what the kernel is handed) -> (the packed state after them in float64,
    R, T [B,3], |residual| [iters,B,k,2] of the forwards that produced the gradients)."""
    import zedo_oracle as O
    tr = []
    a = [np.asarray(x, dtype) for x in args]
    R, T = O.ipo_fit(*a, axes, minT, maxT, iters, normaliser=norm, dtype=dtype, trace=tr, init=unpack(np.asarray(state).astype(dtype)), it0=it0)[:2]
    end = state_of(tr[-1]) if tr else np.asarray(state).astype(dtype)
    return end.astype(np.float64), R, T.reshape(-1, 3), np.stack([t[7] for t in tr]) if tr else np.zeros((0,) + a[3].shape)


class MomentRule:
    """The project's rule for a block of Adam moments after one call from a float64 state handed over in fp32:
        |x - x64| <= 2 max |x32 - x64| + ulp32(max |x64|)
    x32 being the fp32 ORACLE's result from the same fp32 state, all three maxima over the clear pose-iterations added.  The factor 2
    is the margin between two fp32 evaluations of one formula (the kernels sum the key joints in a pairing tree, the oracle in einsum
    order); nothing in it is fitted to a kernel."""

    def __init__(self):
        self.delta, self.delta32, self.largest = 0.0, 0.0, 0.0

    def add(self, got, o32, want):
        if want.size:
            self.delta = max(self.delta, float(np.abs(got - want).max()))
            self.delta32 = max(self.delta32, float(np.abs(o32 - want).max()))
            self.largest = max(self.largest, float(np.abs(want).max()))

    @property
    def bound(self):
        return 2.0 * self.delta32 + float(ulp32(np.float64(self.largest)))

    @property
    def ratio(self):
        return self.delta / self.bound if self.bound > 0 else float(self.delta > 0)

    def holds(self):
        return self.delta <= self.bound


@functools.lru_cache(maxsize=None)
def ipo_oracle_trace(J, kl, N, axes, iters=50):
    """The float64 oracle's first ``iters`` iterations on make_ipo_problem(J, N) (pinhole K) with the key list kl (a tuple):
    (oracle arguments, normaliser N k 2, the trace, states[i] = packed state after i iterations, the key joints that move).
    A key joint at the root contributes no gradient: its residual is not counted when a pose-iteration is called ambiguous."""
    import zedo_oracle as O
    kl = list(kl)
    cl, uvn, Kn = make_ipo_problem(J, N)
    norm = N * len(kl) * 2
    c64, K64 = uvn.astype(np.float64), Kn.astype(np.float64)
    x64 = np.broadcast_to(cl[0][None], (N, J, 3)).astype(np.float64)
    args = (x64[:, kl], O.ipo_init_T(c64, K64, IPO_T, dtype=np.float64), K64, c64[:, kl])
    tr = []
    O.ipo_fit(*args, axes, IPO_MIN, IPO_MAX, iters, normaliser=norm, dtype=np.float64, trace=tr)
    states = [initial_state(N)] + [state_of(t) for t in tr]
    moving = np.abs(cl[0][kl]).max(-1) > 0
    return args, norm, tr, states, moving


def ipo_ambiguous(J, kl, N, axes, iters=50):
    """How many of the first ``iters`` x N pose-iterations of ipo_oracle_trace are ambiguous: some residual of a moving key joint is
    below 1e-3 px, so that its sign - the L1 gradient - is not a statement about the arithmetic.  From the oracle alone."""
    _, _, tr, _, moving = ipo_oracle_trace(J, tuple(kl), N, axes, iters)
    return sum(int((t[7][:, moving, :].reshape(N, -1).min(1) < 1e-3).sum()) for t in tr)


def ipo_single_iterations_from_the_oracle(zh, J, kl, N, axes):
    """The one copy of the single-iteration method (tests/test_joint_counts_gpu.py, tests/test_ipo_key_lists_gpu.py): each of the
    first 50 Adam iterations on its own through zedo_ipo_fit_resume from the oracle's float64 state, handed over in fp32.  Asserted
    here, per iteration: |delta parameter| <= 1e-6 on the poses whose residuals are all sign-unambiguous (|e| >= 1e-3 px; a key joint
    at the root is not counted).  The second moments of the same pose-iterations go into a MomentRule.
    -> (largest parameter delta, ambiguous pose-iterations, the rule): the caller asserts its cap on the ambiguous share, the rule,
    and that neither is vacuous."""
    cl, uvn, Kn = make_ipo_problem(J, N)
    x0, uv, K = dev(cl), dev(uvn), dev(Kn)
    args, norm, tr, states, moving = ipo_oracle_trace(J, tuple(kl), N, axes)
    worst, n_amb, rule_v = 0.0, 0, MomentRule()
    for it in range(50):
        st = dev(states[it].astype(np.float32))
        zh.ipo_fit(x0, uv, K, kl, axes, IPO_T, IPO_MIN, IPO_MAX, 1, norm, N, state=st, it_begin=it)
        out = st.cpu().numpy().astype(np.float64)
        clear = tr[it][7][:, moving, :].reshape(N, -1).min(1) >= 1e-3
        n_amb += int((~clear).sum())
        if clear.any():
            d = float(np.abs(out - states[it + 1])[clear, :5].max())
            worst = max(worst, d)
            assert d <= 1e-6, (it, d)
            o32 = oracle_resume(args, axes, norm, states[it], it, 1, np.float32)[0]
            rule_v.add(out[clear, 10:], o32[clear, 10:], states[it + 1][clear, 10:])
    return worst, n_amb, rule_v


@functools.lru_cache(maxsize=None)
def oracle_run(J, kl, N, axes, general=True, iters=50):
    """The float64 oracle's first ``iters`` iterations: states[i] = packed state after i iterations (float64), clear[i] = the poses
    whose residuals in iteration i + 1 are all >= 1e-3 px (a key joint at the root contributes no gradient and is not counted), and
    m32[i] [N,10] = both moment rows (state[:, 5:15]) after ONE fp32 oracle iteration from states[i] rounded to fp32 - what the
    kernel is handed."""
    import zedo_oracle as O
    kl = list(kl)
    cl = problem(J, N, 1, general)[0]
    args = oracle_args(J, kl, N, general)
    norm = N * len(kl) * 2
    tr = []
    O.ipo_fit(*args, axes, IPO_MIN, IPO_MAX, iters, normaliser=norm, dtype=np.float64, trace=tr)
    states = [initial_state(N)] + [state_of(t) for t in tr]
    moving = np.abs(cl[0][kl]).max(-1) > 0
    clear = [t[7][:, moving, :].reshape(N, -1).min(1) >= 1e-3 for t in tr]
    m32 = [oracle_resume(args, axes, norm, states[it], it, 1, np.float32)[0][:, 5:15] for it in range(iters)]
    return states, clear, m32


# The periodic batch of tests/test_launch_shapes_gpu.py and tests/test_launch_shapes_ref.py

LS_P = 67                                                  # odd and prime: within 128 * 67 rows every base row visits every position of a 128-row tile
LS_TS = np.array([0.1, 0.05, 0.011], np.float32)           # the noise levels of test_both_math_modes_are_fp32_accurate_against_the_fp64_oracle
LS_EDGE_ROWS = {3: "zero", 11: "x 100", 19: "x 1e4", 29: "x 1e-20", 37: "x 1e-40 (fp32 denormal)", 43: "constant 5.0", 53: "a row ...",
                59: "... and its negation"}


def launch_shape_base():
    """The base block [67,17,3]: 0.3 N(0,1) rows (numpy Philox, key [67, 17]), eight of them replaced by LS_EDGE_ROWS."""
    g = np.random.Generator(np.random.Philox(key=[67, 17]))
    base = (0.3 * g.standard_normal((LS_P, 17, 3))).astype(np.float32)
    base[3] = 0.0
    base[11] *= np.float32(100.0)
    base[19] *= np.float32(1e4)
    base[29] *= np.float32(1e-20)
    base[37] = (base[37].astype(np.float64) * 1e-40).astype(np.float32)
    base[43] = 5.0
    base[59] = -base[53]
    assert (np.abs(base[37]) < np.finfo(np.float32).tiny).all() and (base[37] != 0).any()
    return base


def launch_shape_reference64(weights, base):
    """O.score_model_forward in float64 on the base block at every LS_TS -> [3,67,17,3]."""
    import zedo_oracle as O
    w64 = O.cast_weights(weights, np.float64)
    return np.stack([O.score_model_forward(w64, base.astype(np.float64), np.float64(t) * 999.0, dtype=np.float64) for t in LS_TS])


# ---- 4. a BASELINE-size capture ------------------------------------------------------------------------------------------

def sha_of(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class Capture:
    """tests/golden/<name>.npz of tools/gen_golden.py::_driver_full_size: poses and clusters regenerated from the fixture's seeds
    (H36M: float64 ground truth) and checked against its hash, the configuration from its fields, the root-centred ground truth
    the way the capture's dataset class centres it (h36m.py:400-401 in millimetres)."""

    def __init__(self, name):
        from lib.dataset import synthetic as syn
        self.name = name
        self.g = g = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.N, self.H, self.S = int(g["N"]), int(g["H"]), int(g["S"])
        self.h36m = str(g["dataset"]) == "h36m"
        self.d = syn.make_poses(self.N, seed=int(g["seed_pose"]), conf_mode=str(g["conf_mode"]),
                                dtype3d=np.float64 if self.h36m else np.float32)
        self.cl = syn.make_clusters(self.H, seed=int(g["seed_cl"]))
        assert sha_of(self.d["db_2d"], self.d["camera_param"], self.cl) == str(g["inputs_sha"]), "inputs differ from the captured run"
        self.K = self.d["camera_param"]
        if self.h36m:
            self.gt = (self.d["db_3d"] * 1000.0 - (self.d["db_3d"] * 1000.0)[:, 0:1]) / 1000.0
        else:
            self.gt = (self.d["db_3d"] - self.d["db_3d"][:, 0:1]).astype(np.float64)

    @property
    def config(self):
        from zedo_hip.pipeline import ZeDOConfig
        g = self.g
        return ZeDOConfig(IPO_keylist=[int(k) for k in g["keylist"]], IPO_T=float(g["ipo_T"]), IPO_minScaleT=float(g["minT"]),
                          OIL_iterations=self.S)

    def detections(self, seed):
        """db_2d with the pixel coordinates moved by -1/0/+1 ulp (stream `seed`; 0: unchanged)."""
        from lib.dataset import synthetic as syn
        db2 = self.d["db_2d"].copy()
        db2[:, :, :2] = syn.perturb_ulp(db2[:, :, :2], seed)
        return db2

    def pipeline(self, weights, seed=None):
        """The fused pipeline loaded with this capture; its configuration is pipe.cfg."""
        from zedo_hip.pipeline import Pipeline
        db2 = self.d["db_2d"] if seed is None else self.detections(seed)
        return Pipeline(weights, self.config, "cuda").load(self.cl, db2, self.K)

    def dataset(self):
        """The object whose eval_multi the reference's run of this capture reported."""
        if self.h36m:
            from lib.dataset.h36m import H36MDataset3D
            return H36MDataset3D.from_arrays(self.d["db_2d"], self.d["db_3d"] * 1000.0, self.K, 2 + (np.arange(self.N) % 15))
        from lib.dataset.pw3d import PW3D
        return PW3D.from_arrays(self.d["db_2d"], self.d["db_3d"], self.K)


# ---- 5. plumbing ---------------------------------------------------------------------------------------------------------

def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host_lib():
    """libzedo_hip.so as a ctypes.CDLL, for the CPU tests of its exports and its host arithmetic; built first if it is missing.  torch
    is imported above: it must precede the dlopen of libzedo_hip.so, since torch bundles its own HIP runtime."""
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def host_fn(name, restype, argtypes):
    fn = getattr(host_lib(), name)
    fn.restype, fn.argtypes = restype, argtypes
    return fn


def cfg_path(name):
    return os.path.join(ROOT, "zedo-release_amd", "configs", "optim", f"concat_pose_optimization_{name}.py")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def report_env(rec):
    """Measured figures go to stdout (-s) and, with ZEDO_PARITY_REPORT=<file>, to that file."""
    print(json.dumps(rec))
    if os.environ.get("ZEDO_PARITY_REPORT"):
        with open(os.environ["ZEDO_PARITY_REPORT"], "a") as f:
            f.write(json.dumps(rec) + "\n")


# The driver tests (tests/test_select_*_driver_gpu.py, tests/test_prune_driver_gpu.py)

def _inference(argv, capsys):
    """run.inference in this process -> (results, errs, what it printed)."""
    import run.inference as inf
    capsys.readouterr()
    res, errs = inf.main(inf.parse_args(["prog"] + argv))
    return res, errs, capsys.readouterr().out


def _problem(n, cfg=None):
    """The detections of the driver's synthetic run of n poses (seeded by the configuration file cfg, default pw3d's): uv, K, conf."""
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    d = syn.make_poses(n, seed=load_config(cfg or cfg_path("pw3d")).seed)
    return d["db_2d"][:, :, :2], d["camera_param"], d["db_2d"][:, :, 2]


def _rows_and_T(n, h, s):
    """The fused loop of the driver's synthetic pw3d run again: x [h n,17,3], T [h n,3] on the device (same kernels, same bits)."""
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    from zedo_hip.pipeline import Pipeline, ZeDOConfig
    cfg = load_config(cfg_path("pw3d"))
    z = cfg.ZeDO
    uv, K, conf = _problem(n)
    pipe = Pipeline(syn.make_weights(seed=cfg.seed), ZeDOConfig(z.IPO_iterations, z.IPO_keylist, z.RotAxes, z.IPO_T, z.IPO_minScaleT, z.IPO_maxScaleT,
                                                                s, z.sampling_eps, 0.1, 1000, 0.1, 20.0), "cuda")
    pipe.load(syn.make_clusters(h, seed=cfg.seed), np.concatenate([uv, conf[:, :, None]], -1), K)
    return pipe.run()


def _sel(runs, name):
    """<out>_selected.npz of a `runs` fixture's entry name -> (results, path of the out file, stdout)."""
    return np.load(str(runs[name][1])[:-4] + "_selected.npz")


def run_two_ranks(argv, cwd):
    """python -m run.inference argv as two fresh processes in cwd: two members of one gloo process group on device 0, each on its own
    row shard, each under its own time limit -> [(stdout, stderr, returncode)] by rank, every exit status asserted 0 first."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ZEDO_FORCE_DIST", "ZEDO_BENCH_FORCE_DIST"):
        env.pop(k, None)
    env.update(ZEDO_SHARE_DEVICE="1", ZEDO_DIST_BACKEND="gloo", ZEDO_NO_BUILD="1", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONPATH=os.path.join(ROOT, "zedo-release_amd") + os.pathsep + env.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "run.inference"] + argv
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), cwd=str(cwd), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    done = [p.communicate() + (p.returncode,) for p in procs]
    for r, (out, err, rc) in enumerate(done):                       # every exit status, before anything else is looked at
        assert rc == 0, (r, rc, out[-2000:], err[-4000:])
    return done


# Fixtures: a test module imports the ones it uses by name (W needs zh beside it).  A module-scope fixture is built once per
# importing module.

@pytest.fixture(scope="module")
def zh():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zedo_hip
    return zedo_hip


@pytest.fixture(scope="module")
def W(zh, weights0, math_mode):
    w = zh.Weights(weights0)              # in the arithmetic mode of this part of the run (conftest.py::math_mode)
    assert w.math == math_mode
    return w


@pytest.fixture(scope="module")
def model(weights0):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lib.algorithms.advanced.model import ScoreModelFC_Adv
    from lib.dataset import synthetic as syn
    from run._driver import load_config
    m = ScoreModelFC_Adv(load_config(cfg_path("h36m")), 17, 3, 1024, 512, 3)
    sd = {k: torch.tensor(v) for k, v in weights0.items()}
    sd["sigmas"] = torch.tensor(syn.sigmas_buffer())
    m.load_state_dict(sd)
    return m.eval()


@pytest.fixture(autouse=True)
def one_arithmetic_mode(request, math_mode):
    """For modules whose subject does not depend on the arithmetic mode of the dense layers: they run in the f32 session only."""
    if math_mode != "f32":
        pytest.skip(f"{request.module.__name__} does not depend on the arithmetic mode of the dense layers: covered by the f32 session")
