"""ctypes binding of libzedo_hip.so (C ABI: include/zedo_hip.h) for torch tensors on an MI355X.

PyTorch is plumbing here: it owns device memory and the HIP stream; every arithmetic step of the
ZeDO hot path runs in the hand-written gfx950 kernels behind the C ABI.  There is NO fallback:
importing this module without the built library, or calling it without a GPU, raises.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load_zedo_build():
    """zedo_build.py sits beside this package; it is loaded BY LOCATION so that importing zedo_hip never edits sys.path
    (the package root also holds the generic top-level names `lib` and `run`, which must not shadow a host application's)."""
    import importlib.util
    import sys
    if "zedo_build" in sys.modules:
        return sys.modules["zedo_build"]
    spec = importlib.util.spec_from_file_location("zedo_build", os.path.join(os.path.dirname(_HERE), "zedo_build.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["zedo_build"] = mod
    spec.loader.exec_module(mod)
    return mod


_zb = _load_zedo_build()

# Not a fallback: the only way to get the hot path is to compile the HIP sources (hipcc cross-compiles gfx950 without a
# GPU).  A missing library is built once, under a lock (N ranks importing at the same time build it once); with
# ZEDO_NO_BUILD=1 (ranks of a launcher that has built already) or when the build fails this raises ImportError.
LIB_PATH = _zb.ensure_library()

_lib = ctypes.CDLL(LIB_PATH)

_vp, _i, _f, _d, _ll, _sz = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double,
                             ctypes.c_longlong, ctypes.c_size_t)

# name -> (restype, argtypes): every symbol declared in include/zedo_hip.h
SIGNATURES = {
    "zedo_abi_version": (_i, []),
    "zedo_error_string": (ctypes.c_char_p, [_i]),
    "zedo_weights_create": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, ctypes.POINTER(_vp)]),
    "zedo_weights_destroy": (None, [_vp]),
    "zedo_weights_set_math": (_i, [_vp, _i, _vp]),
    "zedo_weights_get_math": (_i, [_vp]),
    "zedo_schedule_create": (_i, [_vp, _vp, _i, _f, _f, _f, _i, _vp, ctypes.POINTER(_vp)]),
    "zedo_schedule_destroy": (None, [_vp]),
    "zedo_schedule_read": (_i, [_vp, _vp, _vp, _vp]),
    "zedo_workspace_bytes": (_sz, [_i]),
    "zedo_reproj_prepare": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "zedo_reproj_degenerate": (_i, [_vp, _i, _i, _vp, _vp]),
    "zedo_reproj_grad": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _ll, _vp]),
    "zedo_score_eps": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    "zedo_sde_step": (_i, [_vp, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "zedo_pc_plan_create": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, ctypes.POINTER(_vp)]),
    "zedo_pc_plan_destroy": (None, [_vp]),
    "zedo_pc_workspace_bytes": (_sz, [_vp, _i]),
    "zedo_pc_step": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "zedo_oil_run": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _ll, _vp, _sz, _vp]),
    "zedo_ipo_fit": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _i, _d, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _ll, _vp]),
    "zedo_ipo_fit_resume": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _i, _d, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i,
                                 _i, _ll, _vp]),
    "zedo_rotate_init": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _ll, _vp]),
    "zedo_min_mpjpe": (_i, [_vp, _vp, _i, _i, _i, _ll, _i, _vp, _vp, _vp, _vp]),
    "zedo_min_mpjpe_both": (_i, [_vp, _vp, _i, _i, _i, _ll, _vp, _vp, _vp, _vp]),
    "zedo_min_reproj": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _ll, _vp, _vp, _vp, _vp]),
    "zedo_joint_reproj": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _ll, _vp, _vp, _vp, _vp]),
    "zedo_joint_compose": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "zedo_temporal_workspace_bytes": (_sz, [_i, _i, _i]),
    "zedo_temporal_select": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp]),
    "zedo_joint_temporal_workspace_bytes": (_sz, [_i, _i, _i]),
    "zedo_joint_temporal_select": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _vp, _sz, _vp, _vp, _vp]),
    "zedo_joint_stream_state_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "zedo_joint_stream_reset": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _vp]),
    "zedo_joint_stream_push": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "zedo_temporal_stream_state_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "zedo_temporal_stream_reset": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _vp]),
    "zedo_temporal_stream_push": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _d, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "zedo_joint_accel_workspace_bytes": (_sz, [_i, _i, _i]),
    "zedo_joint_accel_select": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _vp, _sz, _vp, _vp, _vp]),
    "zedo_joint_accel_stream_state_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "zedo_joint_accel_stream_reset": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _vp]),
    "zedo_joint_accel_stream_push": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _d, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "zedo_joint_accel_marginal_workspace_bytes": (_sz, [_i, _i, _i]),
    "zedo_joint_accel_marginal": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zedo_joint_accel_stream_marginal_state_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "zedo_joint_accel_stream_marginal_reset": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _vp]),
    "zedo_joint_accel_stream_marginal_push": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _d, _d, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                                   _vp, _vp, _vp]),
    "zedo_joint_stream_marginal_state_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "zedo_joint_stream_marginal_reset": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _vp]),
    "zedo_joint_stream_marginal_push": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d, _d, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _vp]),
    "zedo_joint_marginal_workspace_bytes": (_sz, [_i, _i, _i]),
    "zedo_joint_marginal": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zedo_temporal_marginal_workspace_bytes": (_sz, [_i, _i, _i]),
    "zedo_temporal_marginal": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _d, _d, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zedo_joint_tree_select": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _d, _vp, _vp, _vp, _vp]),
    "zedo_joint_tree_marginal_max_h": (_i, [_i]),
    "zedo_joint_tree_marginal": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zedo_prune_rank": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "zedo_prune_gather": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zedo_pose_min": (_i, [_vp, _i, _i, _ll, _vp, _vp, _vp]),
    "zedo_probe_mfma_peak": (_i, [_i, _vp, _vp, _vp]),
    "zedo_probe_mfma_peak_f16": (_i, [_i, _vp, _vp, _vp]),
    "zedo_profile_start": (_i, [_i, _i]),
    "zedo_profile_stop": (_i, [_vp, _vp, _vp]),
    "zedo_profile_shader_ghz": (_d, []),
    "zedo_profile_bracket_ms": (_d, []),
}
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(_lib, _name)  # AttributeError here = library/header mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args

N_JOINTS, JOINT_DIM, HIDDEN_DIM, EMBED_DIM = 17, 3, 1024, 512
GEOM_F = 8


class ZedoError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise ZedoError(f"libzedo_hip: {_lib.zedo_error_string(rc).decode()} (code {rc})")


_gpu_seen = False


def _need_gpu():
    global _gpu_seen
    if not _gpu_seen:           # torch.cuda.is_available() costs ~20 us per call; a GPU does not go away
        if not torch.cuda.is_available():
            raise ZedoError("libzedo_hip needs an MI355X (gfx950): no GPU is visible and there is no CPU path")
        _gpu_seen = True


def _p(t, dtype=torch.float32):
    """device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dtype):
        raise ZedoError(f"expected a contiguous {dtype} CUDA tensor, got {type(t)} "
                        f"{getattr(t, 'dtype', None)} {getattr(t, 'device', None)}")
    return ctypes.c_void_p(t.data_ptr())


# ---- streams, devices, threads ------------------------------------------------------------------------------------------
# The C ABI is re-entrant across distinct streams (include/zedo_hip.h); this mirror honours that: every call is
# enqueued on the CURRENT stream of the device its tensors live on (not of whatever device happens to be current), runs
# with that device current (the library's per-device launch state follows hipGetDevice), takes its workspace from torch's
# stream-aware caching allocator per call - so two streams or two host threads never share scratch memory, and a block is
# only handed out again in stream order - and refuses arguments that live on different devices.
def _device_of(*objs):
    """The one CUDA device of the given tensors / handles (None entries skipped); mixed devices are an error."""
    dev = None
    for o in objs:
        if o is None:
            continue
        d = o.device if isinstance(o, (torch.Tensor, Weights, Schedule, PcPlan)) else None
        if d is None:
            continue
        d = torch.device(d)
        if d.type != "cuda":
            raise ZedoError(f"expected CUDA tensors, got one on {d}")
        if d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        if dev is None:
            dev = d
        elif d != dev:
            raise ZedoError(f"arguments live on different devices ({dev} and {d}): one call runs on one GPU")
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _norm_device(device=None):
    """torch.device("cuda", index) for `device` (None / "cuda" = the current device)."""
    d = torch.device("cuda") if device is None else torch.device(device)
    if d.type != "cuda":
        raise ZedoError(f"libzedo_hip runs on CUDA (HIP) devices only, not on {d}")
    return torch.device("cuda", torch.cuda.current_device()) if d.index is None else d


def _stream(device=None):
    """hipStream_t of torch's current stream ON `device` (default: the current device)."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def abi_version():
    return _lib.zedo_abi_version()


# state-dict order of ScoreModelFC_Adv (reference lib/algorithms/advanced/model.py:113-152)
def param_names(n_blocks=2):
    names = ["pre_dense.weight", "pre_dense.bias", "pre_dense_t.weight", "pre_dense_t.bias",
             "pre_gnorm.weight", "pre_gnorm.bias", "shared_time_embed.0.weight", "shared_time_embed.0.bias"]
    for b in range(1, n_blocks + 1):
        for k in (1, 2):
            names += [f"b{b}_dense{k}.weight", f"b{b}_dense{k}.bias", f"b{b}_dense{k}_t.weight",
                      f"b{b}_dense{k}_t.bias", f"b{b}_gnorm{k}.weight", f"b{b}_gnorm{k}.bias"]
    return names + ["post_dense.weight", "post_dense.bias"]


MATH_MODES = {"f32": 0, "f16x3": 1}      # ZEDO_MATH_F32 / ZEDO_MATH_F16X3 of include/zedo_hip.h


def default_math():
    """The arithmetic of the hidden layers for handles created from now on: environment ZEDO_MATH = f32 (default: exact
    fp32 MFMA) | f16x3 (split-fp16 operands on the fp16 matrix pipe, fp32-level accuracy; opt-in)."""
    m = os.environ.get("ZEDO_MATH", "f32").strip().lower() or "f32"
    if m not in MATH_MODES:
        raise ZedoError(f"ZEDO_MATH={m!r}: expected one of {sorted(MATH_MODES)}")
    return m


class Weights:
    """Device copy of a ScoreModelFC_Adv state dict, repacked for the kernels (zedo_weights_create).
    math: "f32" | "f16x3" | None (= default_math(), i.e. the ZEDO_MATH environment variable)."""

    def __init__(self, state_dict, n_joints=N_JOINTS, joint_dim=JOINT_DIM, hidden=HIDDEN_DIM, embed=EMBED_DIM,
                 n_blocks=2, math=None, device=None):
        _need_gpu()
        self.device = _norm_device(device)
        flat = []
        for name in param_names(n_blocks):
            v = state_dict[name]
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            flat.append(np.ascontiguousarray(v, dtype=np.float32).reshape(-1))
        flat = np.concatenate(flat)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(_lib.zedo_weights_create(flat.ctypes.data_as(_vp), flat.size, n_joints, joint_dim, hidden, embed,
                                            n_blocks, _stream(self.device), ctypes.byref(self._h)))
        self.n_joints, self.joint_dim, self.hidden, self.embed, self.n_blocks = n_joints, joint_dim, hidden, embed, n_blocks
        self.set_math(default_math() if math is None else math)

    def set_math(self, math):
        """Not re-entrant with calls that use this handle: switch modes between runs, not during them."""
        if math not in MATH_MODES:
            raise ZedoError(f"math mode {math!r}: expected one of {sorted(MATH_MODES)}")
        with torch.cuda.device(self.device):
            _check(_lib.zedo_weights_set_math(self._h, MATH_MODES[math], _stream(self.device)))
        self.math = math
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:   # _lib is None during interpreter shutdown
            _lib.zedo_weights_destroy(h)
            self._h = None


class Schedule:
    """Per-step tables (time-bias rows, a_i, c_i) for one timestamp vector (zedo_schedule_create)."""

    def __init__(self, weights, ts, beta_min=0.1, beta_max=20.0, n_sde=1000, label_scale=999.0):
        _need_gpu()
        ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float32).reshape(-1))
        self.S = int(ts.size)
        self.ts = ts
        self.weights = weights  # keep alive
        self.device = weights.device
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(_lib.zedo_schedule_create(weights._h, ts.ctypes.data_as(_vp), self.S, label_scale, beta_min, beta_max,
                                             n_sde, _stream(self.device), ctypes.byref(self._h)))

    def read(self):
        nl = 1 + 2 * self.weights.n_blocks
        tb = np.empty((self.S, nl, self.weights.hidden), np.float32)
        a = np.empty(self.S, np.float32)
        c = np.empty(self.S, np.float32)
        _check(_lib.zedo_schedule_read(self._h, tb.ctypes.data_as(_vp), a.ctypes.data_as(_vp), c.ctypes.data_as(_vp)))
        return tb, a, c

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.zedo_schedule_destroy(h)
            self._h = None


PC_CORR = {"none": 0, "langevin": 1, "ald": 2}      # ZEDO_PC_CORR_* of include/zedo_hip.h


class PcPlan:
    """Per-step scalars and time-bias rows of a generic predictor-corrector sampler for S steps (zedo_pc_plan_create).
    `coeffs`: what lib.algorithms.advanced._pc_coeffs.coefficients returns (fp32 arrays of length S)."""

    def __init__(self, weights, coeffs):
        _need_gpu()
        f = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
        ptr = lambda a: None if a is None else a.ctypes.data_as(_vp)
        label, ns, pA, pB, pC, corr = (f(getattr(coeffs, k)) for k in ("label", "net_scale", "pA", "pB", "pC", "corr"))
        self.S = int(label.size)
        for a in (ns, pA, pB, pC, corr):
            if a is not None and a.size != self.S:
                raise ZedoError(f"PcPlan: every coefficient array must have {self.S} entries")
        self.has_predictor, self.corrector, self.n_corr = bool(coeffs.has_predictor), int(coeffs.corrector), int(coeffs.n_corr)
        if self.corrector == PC_CORR["none"]:
            self.n_corr = 0
        self.n_draws = self.n_corr + int(self.has_predictor)
        self.label, self.pC = label, pC
        self.weights = weights  # keep alive
        self.device = weights.device
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(_lib.zedo_pc_plan_create(weights._h, self.S, ptr(label), ptr(ns), int(self.has_predictor), ptr(pA), ptr(pB),
                                            ptr(pC), self.corrector, self.n_corr, ptr(corr), _stream(self.device),
                                            ctypes.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.zedo_pc_plan_destroy(h)
            self._h = None


def workspace_bytes(B):
    return int(_lib.zedo_workspace_bytes(int(B)))


def workspace(B, device=None):
    """A uint8 CUDA tensor large enough for B rows, owned by the CALL that asked for it: a fresh block of torch's caching
    allocator, tagged with the current stream of `device` (so the allocator re-issues it only in stream order once the call's
    reference is gone - the kernels of the call may still be running then) and shared with no other stream or thread.  After
    the first call of a size the block comes out of the allocator's cache: microseconds, no hipMalloc."""
    _need_gpu()
    device = _norm_device(device)
    with torch.cuda.device(device):
        return torch.empty(workspace_bytes(B), dtype=torch.uint8, device=device)


def reproj_prepare(uv, K, conf=None, conf_clamped_out=None):
    """uv [N,J,2], K [N,3,3], conf [N,J] or None -> geom [N,J,8]."""
    _need_gpu()
    dev = _device_of(uv, K, conf, conf_clamped_out)
    N, J = uv.shape[0], uv.shape[1]
    with torch.cuda.device(dev):
        geom = torch.empty((N, J, GEOM_F), dtype=torch.float32, device=dev)
        _check(_lib.zedo_reproj_prepare(_p(uv), _p(K), _p(conf), N, J, _p(geom), _p(conf_clamped_out), _stream(dev)))
    return geom


def reproj_degenerate(geom):
    """Number of poses whose least-squares system for T is singular (zedo_reproj_degenerate; synchronises)."""
    _need_gpu()
    dev = _device_of(geom)
    n = ctypes.c_int(0)
    with torch.cuda.device(dev):
        _check(_lib.zedo_reproj_degenerate(_p(geom), geom.shape[0], geom.shape[1], ctypes.cast(ctypes.byref(n), _vp), _stream(dev)))
    return int(n.value)


SINGULAR_MSG = ("gradient_field_gen: the least-squares system for T is singular for {n} pose(s) - every camera ray of the "
                "pose coincides; the reference's torch.inverse(AtA) raises here (simple_zeroshot_opt.py:89-92)")


def reproj_grad(x, geom, T, solve_T, row_offset=0):
    """gradient_field_gen body: returns g [B,J,3]; T [B,3] is overwritten when solve_T."""
    _need_gpu()
    dev = _device_of(x, geom, T)
    B, J = x.shape[0], x.shape[1]
    with torch.cuda.device(dev):
        g = torch.empty_like(x)
        _check(_lib.zedo_reproj_grad(_p(x), _p(geom), _p(T), int(bool(solve_T)), _p(g), B, geom.shape[0], J,
                                     int(row_offset), _stream(dev)))
    return g


def score_eps(weights, sched, step, x):
    _need_gpu()
    dev = _device_of(weights, sched, x)
    B = x.shape[0]
    with torch.cuda.device(dev):
        ws = workspace(B, dev)
        eps = torch.empty_like(x)
        _check(_lib.zedo_score_eps(weights._h, sched._h, int(step), _p(x), _p(eps), B, _p(ws, torch.uint8), ws.numel(),
                                   _stream(dev)))
    return eps


def sde_step(weights, sched, step, x):
    """x <- a x + c eps(x), in place."""
    _need_gpu()
    dev = _device_of(weights, sched, x)
    B = x.shape[0]
    with torch.cuda.device(dev):
        ws = workspace(B, dev)
        _check(_lib.zedo_sde_step(weights._h, sched._h, int(step), _p(x), B, _p(ws, torch.uint8), ws.numel(), _stream(dev)))
    return x


def pc_step(weights, plan, step, x, noise=(), x_mean=None):
    """One generic predictor-corrector call (zedo_pc_step): x <- x_new in place; x_mean (optional tensor like x) receives the
    noise-free update.  noise: the caller's draws in the reference's order (corrector steps, then the predictor); the predictor's
    entry may be None or missing = keep x_mean only (x then returns x_mean)."""
    _need_gpu()
    noise = list(noise)
    dev = _device_of(weights, plan, x, x_mean, *noise)
    B = x.shape[0]
    if len(noise) < plan.n_corr or len(noise) > plan.n_draws:
        raise ZedoError(f"pc_step: this plan takes {plan.n_corr} to {plan.n_draws} noise draws, got {len(noise)}")
    for z in noise:
        if z is not None and z.shape != x.shape:
            raise ZedoError(f"pc_step: a noise draw has shape {tuple(z.shape)}, the state {tuple(x.shape)}")
    if x_mean is not None and x_mean.shape != x.shape:
        raise ZedoError("pc_step: x_mean must have the shape of x")
    zs = (ctypes.c_void_p * max(plan.n_draws, 1))()
    for i, z in enumerate(noise):
        zs[i] = None if z is None else _p(z).value
    with torch.cuda.device(dev):
        ws = workspace(B, dev)
        _check(_lib.zedo_pc_step(weights._h, plan._h, int(step), _p(x), _p(x_mean), ctypes.cast(zs, _vp), B, _p(ws, torch.uint8),
                                 ws.numel(), _stream(dev)))
    return x


def oil_run(weights, sched, x, geom, T, step_begin, step_end, switch_step, row_offset=0):
    """Fused OIL loop over steps [step_begin, step_end); x [B,J,3] and T [B,3] updated in place."""
    _need_gpu()
    dev = _device_of(weights, sched, x, geom, T)
    B = x.shape[0]
    with torch.cuda.device(dev):
        ws = workspace(B, dev)
        _check(_lib.zedo_oil_run(weights._h, sched._h, _p(x), _p(geom), _p(T), int(step_begin), int(step_end),
                                 int(switch_step), B, geom.shape[0], int(row_offset), _p(ws, torch.uint8), ws.numel(),
                                 _stream(dev)))
    return x, T


def axes_mask(axes):
    """RotOpt's axis string ("", "z", "xy", ... any order) -> the C ABI's axes_mask (bit 0 = x, bit 1 = y, bit 2 = z)."""
    bits = {"x": 1, "y": 2, "z": 4}
    bad = sorted(set(axes) - set(bits))
    if bad:
        raise ZedoError(f"ipo_fit: rotation axes must be letters of 'xyz', got {axes!r} (unknown: {''.join(bad)!r})")
    return sum(bits[a] for a in set(axes))


def ipo_fit(x0, uv, K, keylist, axes, ipo_T, min_scale, max_scale, iters, normaliser, B, row_offset=0,
            return_params=False, state=None, it_begin=0):
    """x0 [H,J,3] centred cluster poses, uv [N,J,2], K [N,3,3] -> R [B,3,3], T [B,3] (, q [B,4], scale [B]).
    state [B,15] (optional, in/out) + it_begin: resume from a captured Adam state (zedo_ipo_fit_resume)."""
    _need_gpu()
    dev = _device_of(x0, uv, K, state)
    N, J, H = uv.shape[0], uv.shape[1], x0.shape[0]
    kl = (ctypes.c_int * len(keylist))(*[int(k) for k in keylist])
    with torch.cuda.device(dev):
        R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
        T = torch.empty((B, 3), dtype=torch.float32, device=dev)
        q = torch.empty((B, 4), dtype=torch.float32, device=dev) if return_params else None
        sc = torch.empty((B,), dtype=torch.float32, device=dev) if return_params else None
        if state is not None:
            _check(_lib.zedo_ipo_fit_resume(_p(x0), _p(uv), _p(K), ctypes.cast(kl, _vp), len(keylist), axes_mask(axes),
                                            float(ipo_T), float(min_scale), float(max_scale), int(iters), float(normaliser),
                                            _p(R), _p(T), _p(q), _p(sc), _p(state), int(it_begin), B, H, N, J,
                                            int(row_offset), _stream(dev)))
        else:
            _check(_lib.zedo_ipo_fit(_p(x0), _p(uv), _p(K), ctypes.cast(kl, _vp), len(keylist), axes_mask(axes),
                                     float(ipo_T), float(min_scale), float(max_scale), int(iters), float(normaliser),
                                     _p(R), _p(T), _p(q), _p(sc), B, H, N, J, int(row_offset), _stream(dev)))
    return (R, T, q, sc) if return_params else (R, T)


def rotate_init(x0, R, N, row_offset=0):
    _need_gpu()
    dev = _device_of(x0, R)
    B, J = R.shape[0], x0.shape[1]
    with torch.cuda.device(dev):
        x = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
        _check(_lib.zedo_rotate_init(_p(x0), _p(R), _p(x), B, x0.shape[0], N, J, int(row_offset), _stream(dev)))
    return x


def min_mpjpe(pred, gt_centred, N, procrustes=False, row_offset=0):
    """pred [B,J,3] fp32 rows (h,n); gt_centred [N,J,3] float64 -> (err [B], best [N], best_h [N])."""
    _need_gpu()
    dev = _device_of(pred, gt_centred)
    B, J = pred.shape[0], pred.shape[1]
    with torch.cuda.device(dev):
        err = torch.empty((B,), dtype=torch.float64, device=dev)
        best = torch.empty((N,), dtype=torch.float64, device=dev)
        best_h = torch.empty((N,), dtype=torch.int32, device=dev)
        _check(_lib.zedo_min_mpjpe(_p(pred), _p(gt_centred, torch.float64), B, N, J, int(row_offset), int(bool(procrustes)),
                                   _p(err, torch.float64), _p(best, torch.float64), _p(best_h, torch.int32), _stream(dev)))
    return err, best, best_h


def min_mpjpe_both(pred, gt_centred, N, row_offset=0):
    """Both protocols from one pass over the rows (zedo_min_mpjpe_both): -> (err [2,B], best [2,N], best_h [2,N]), slot 0 the
    bits of min_mpjpe(procrustes=False), slot 1 those of min_mpjpe(procrustes=True)."""
    _need_gpu()
    dev = _device_of(pred, gt_centred)
    B, J = pred.shape[0], pred.shape[1]
    with torch.cuda.device(dev):
        err = torch.empty((2, B), dtype=torch.float64, device=dev)
        best = torch.empty((2, N), dtype=torch.float64, device=dev)
        best_h = torch.empty((2, N), dtype=torch.int32, device=dev)
        _check(_lib.zedo_min_mpjpe_both(_p(pred), _p(gt_centred, torch.float64), B, N, J, int(row_offset),
                                        _p(err, torch.float64), _p(best, torch.float64), _p(best_h, torch.int32), _stream(dev)))
    return err, best, best_h


def min_reproj(x, T, uv, K, conf=None, N=None, row_offset=0):
    """Selection without ground truth (zedo_min_reproj): x [B,J,3] rows (h,n), T [B,3], uv [N,J,2], K [N,3,3], conf [N,J] or None
    (weight 1) -> (err [B] f64: the confidence-weighted mean reprojection distance of x + T in pixels, best [N] f64, idx [N] i32)."""
    _need_gpu()
    dev = _device_of(x, T, uv, K, conf)
    B, J = x.shape[0], x.shape[1]
    N = uv.shape[0] if N is None else int(N)
    if (tuple(x.shape) != (B, J, 3) or tuple(T.shape) != (B, 3) or tuple(uv.shape) != (N, J, 2) or tuple(K.shape) != (N, 3, 3)
            or (conf is not None and tuple(conf.shape) != (N, J))):
        raise ZedoError(f"min_reproj: x [B,J,3], T [B,3], uv [N,J,2], K [N,3,3], conf [N,J] expected, got {tuple(x.shape)}, "
                        f"{tuple(T.shape)}, {tuple(uv.shape)}, {tuple(K.shape)}, {None if conf is None else tuple(conf.shape)} with N = {N}")
    with torch.cuda.device(dev):
        err = torch.empty((B,), dtype=torch.float64, device=dev)
        best = torch.empty((N,), dtype=torch.float64, device=dev)
        best_h = torch.empty((N,), dtype=torch.int32, device=dev)
        _check(_lib.zedo_min_reproj(_p(x), _p(T), _p(uv), _p(K), _p(conf), B, N, J, int(row_offset), _p(err, torch.float64),
                                    _p(best, torch.float64), _p(best_h, torch.int32), _stream(dev)))
    return err, best, best_h


def joint_reproj(x, T, uv, K, N=None, row_offset=0, return_rows=False):
    """Joint-wise aggregation without ground truth (zedo_joint_reproj): x [B,J,3] rows (h,n), T [B,3], uv [N,J,2], K [N,3,3] ->
    (best [N,J] f64: per (pose, joint) the smallest reprojection distance of x + T in pixels over the local hypotheses, idx [N,J] i32:
    the hypothesis that attains it).  return_rows: also jerr [B,J] f64, every row's per-joint distances (the route through
    zedo_pose_min's kernels; the same bits in best / idx).  Whether the assembled pose is closer to ground truth than the pose-level
    selection of min_reproj is not measured."""
    _need_gpu()
    dev = _device_of(x, T, uv, K)
    B, J = x.shape[0], x.shape[1]
    N = uv.shape[0] if N is None else int(N)
    if tuple(x.shape) != (B, J, 3) or tuple(T.shape) != (B, 3) or tuple(uv.shape) != (N, J, 2) or tuple(K.shape) != (N, 3, 3):
        raise ZedoError(f"joint_reproj: x [B,J,3], T [B,3], uv [N,J,2], K [N,3,3] expected, got {tuple(x.shape)}, {tuple(T.shape)}, "
                        f"{tuple(uv.shape)}, {tuple(K.shape)} with N = {N}")
    with torch.cuda.device(dev):
        jerr = torch.empty((B, J), dtype=torch.float64, device=dev) if return_rows else None
        best = torch.empty((N, J), dtype=torch.float64, device=dev)
        best_h = torch.empty((N, J), dtype=torch.int32, device=dev)
        _check(_lib.zedo_joint_reproj(_p(x), _p(T), _p(uv), _p(K), B, N, J, int(row_offset), _p(jerr, torch.float64),
                                      _p(best, torch.float64), _p(best_h, torch.int32), _stream(dev)))
    return (best, best_h, jerr) if return_rows else (best, best_h)


def joint_compose(x_full, T_full, joint_idx, ref_idx=None, N=None, check=True):
    """The pose assembled joint by joint (zedo_joint_compose): x_full [H*N,J,3] and T_full [H*N,3] (ALL rows, h-major), joint_idx [N,J]
    i32 -> pose [N,J,3] f32, joint (n, j) = x + T of hypothesis joint_idx[n,j]: in the camera frame (ref_idx None) or minus the
    translation of hypothesis ref_idx[n] ([N] i32: root-relative to that hypothesis's frame).  Like take_rows, an index of -1 or one
    outside the hypotheses is a ValueError (synchronises to look; check=False does not look: the call makes such joints NaN)."""
    _need_gpu()
    dev = _device_of(x_full, T_full, joint_idx, ref_idx)
    J = x_full.shape[1]
    N = joint_idx.shape[0] if N is None else int(N)
    rows = x_full.shape[0]
    if (N < 1 or rows % N or tuple(x_full.shape) != (rows, J, 3) or tuple(T_full.shape) != (rows, 3) or tuple(joint_idx.shape) != (N, J)
            or (ref_idx is not None and tuple(ref_idx.shape) != (N,))):
        raise ValueError(f"joint_compose: x [H*N,J,3], T [H*N,3], joint_idx [N,J], ref_idx [N] expected, got {tuple(x_full.shape)}, "
                         f"{tuple(T_full.shape)}, {tuple(joint_idx.shape)}, {None if ref_idx is None else tuple(ref_idx.shape)} with N = {N}")
    H = rows // N
    for name, i in (("joint_idx", joint_idx), ("ref_idx", ref_idx)):
        if check and i is not None and bool(((i < 0) | (i >= H)).any()):
            raise ValueError(f"joint_compose: {name} holds -1 (nothing was selected) or an index outside the {H} hypotheses")
    with torch.cuda.device(dev):
        pose = torch.empty((N, J, 3), dtype=torch.float32, device=dev)
        _check(_lib.zedo_joint_compose(_p(x_full), _p(T_full), _p(joint_idx, torch.int32), _p(ref_idx, torch.int32), H, N, J, _p(pose),
                                       _stream(dev)))
    return pose


def _chain_inputs(name, unary, x_full, T_full, seq_start, N, joint_wise):
    """What the selection and fusion calls along a video share: the device, seq_start as an int32 tensor on it, N (read off seq_start's
    last entry - one synchronisation - when the caller did not give it), H and J, with the shapes checked: unary [H*N,J] (joint_wise) or
    [H*N], x [H*N,J,3], T [H*N,3] or None.  `name`: the public function the ValueError speaks for."""
    _need_gpu()
    dev = _device_of(unary, x_full, T_full, seq_start if isinstance(seq_start, torch.Tensor) and seq_start.is_cuda else None)
    rows, J = x_full.shape[0], x_full.shape[1]
    if isinstance(seq_start, torch.Tensor):
        if seq_start.dtype not in (torch.int32, torch.int64) or seq_start.dim() != 1:
            raise ValueError(f"{name}: seq_start must be a 1-D int tensor, got {seq_start.dtype} {tuple(seq_start.shape)}")
        seq = seq_start.to(device=dev, dtype=torch.int32).contiguous()
    else:
        seq = torch.tensor([int(v) for v in seq_start], dtype=torch.int32, device=dev)
    if N is None:
        N = int(seq[-1].item()) if seq.numel() else 0
    N = int(N)
    if (N < 1 or rows % N or tuple(x_full.shape) != (rows, J, 3) or tuple(unary.shape) != ((rows, J) if joint_wise else (rows,))
            or seq.numel() < 2 or (T_full is not None and tuple(T_full.shape) != (rows, 3))):
        if joint_wise:
            raise ValueError(f"{name}: junary [H*N,J], x [H*N,J,3], T [H*N,3], seq_start [n_seq+1] expected, got "
                             f"{tuple(unary.shape)}, {tuple(x_full.shape)}, {None if T_full is None else tuple(T_full.shape)}, {tuple(seq.shape)} "
                             f"with N = {N}")
        raise ValueError(f"{name}: unary [H*N], x [H*N,J,3], seq_start [n_seq+1] expected, got {tuple(unary.shape)}, "
                         f"{tuple(x_full.shape)}, {tuple(seq.shape)} with N = {N}")
    return dev, seq, N, rows // N, J


def _tree_inputs(name, junary, x_full, T_full, parent, N, weight):
    """What the skeleton-coupled calls share: the device, the parent array as contiguous int32 on the host, N (the weights say how many
    poses there are when the caller did not), H and J, with the shapes checked."""
    _need_gpu()
    dev = _device_of(junary, x_full, T_full, weight)
    rows, J = x_full.shape[0], x_full.shape[1]
    par = np.ascontiguousarray(np.asarray(parent.cpu() if isinstance(parent, torch.Tensor) else parent).astype(np.int32))
    N = (0 if weight is None else weight.shape[0]) if N is None else int(N)
    if (N < 1 or rows % N or tuple(x_full.shape) != (rows, J, 3) or tuple(junary.shape) != (rows, J) or par.shape != (J,)
            or (T_full is not None and tuple(T_full.shape) != (rows, 3)) or (weight is not None and tuple(weight.shape) != (N, J))):
        raise ValueError(f"{name}: junary [H*N,J], x [H*N,J,3], T [H*N,3], parent [J], weight [N,J] expected, got "
                         f"{tuple(junary.shape)}, {tuple(x_full.shape)}, {None if T_full is None else tuple(T_full.shape)}, {par.shape}, "
                         f"{None if weight is None else tuple(weight.shape)} with N = {N}")
    return dev, par, N, rows // N, J


def _marginal_outputs(N, J, H, dev, return_weights):
    """mean [N,J,3], cov [N,J,6], hmax [N,J] i32, wmax [N,J], logz [N,J] and, on request, w [N,J,H] (else None); f64 unless noted."""
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    return (f64(N, J, 3), f64(N, J, 6), torch.empty((N, J), dtype=torch.int32, device=dev), f64(N, J), f64(N, J),
            f64(N, J, H) if return_weights else None)


def _workspace(bytes_fn, dev, *shape):
    """(the bytes the entry point asks for at this shape, a uint8 tensor of at least that and at least 8)"""
    nbytes = int(bytes_fn(*shape))
    return nbytes, torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev)


def temporal_select(unary, x_full, seq_start, N=None, lam=100.0, chunk_frames=0):
    """Selection along a video without ground truth (zedo_temporal_select): unary [H*N] f64 (ALL rows, h-major: e.g. err of min_reproj,
    pixels), x_full [H*N,J,3] f32, seq_start [n_seq+1] (a sequence or an int tensor: strictly ascending from 0 to N, the first frame of
    every clip) -> (path [N] i32, cost [N] f64): per clip the hypothesis sequence that minimises the sum of its unaries plus lam times
    the mean joint displacement between consecutive choices (Viterbi, fp64).  lam is in cost units per metre; the default of 100 (1 cm of
    mean joint jump costs as much as 1 px) is untuned.  chunk_frames: frames of transition costs held at once (0: at most 256 MB); the
    result does not depend on it.  Whether the temporal path is closer to ground truth than the per-frame arg-min is not measured."""
    dev, seq, N, H, J = _chain_inputs("temporal_select", unary, x_full, None, seq_start, N, joint_wise=False)
    with torch.cuda.device(dev):
        nbytes, ws = _workspace(_lib.zedo_temporal_workspace_bytes, dev, N, H, int(chunk_frames))
        path = torch.empty((N,), dtype=torch.int32, device=dev)
        cost = torch.empty((N,), dtype=torch.float64, device=dev)
        _check(_lib.zedo_temporal_select(_p(unary, torch.float64), _p(x_full), _p(seq, torch.int32), seq.numel() - 1, H, N, J, float(lam),
                                         _p(ws, torch.uint8), nbytes, _p(path, torch.int32), _p(cost, torch.float64), _stream(dev)))
    return path, cost


def joint_temporal_select(junary, x_full, T_full, seq_start, N=None, lam=100.0):
    """Joint-wise selection along a video without ground truth (zedo_joint_temporal_select): junary [H*N,J] f64 (ALL rows, h-major: e.g.
    jerr of joint_reproj(return_rows=True), pixels), x_full [H*N,J,3] f32, T_full [H*N,3] f32 or None (the motion term on x alone),
    seq_start [n_seq+1] (a sequence or an int tensor: strictly ascending from 0 to N) -> (path [N,J] i32, cost [N,J] f64): per (clip,
    joint) the hypothesis sequence that minimises the sum of that joint's unaries plus lam times that joint's displacement in the camera
    frame (x + T) between consecutive choices (Viterbi, fp64, one chain per joint).  lam is in cost units per metre; the default of 100 is
    untuned.  At most 1024 hypotheses.  Whether the joint-wise temporal paths are closer to ground truth than the per-frame joint-wise
    arg-min is not measured."""
    dev, seq, N, H, J = _chain_inputs("joint_temporal_select", junary, x_full, T_full, seq_start, N, joint_wise=True)
    with torch.cuda.device(dev):
        nbytes, ws = _workspace(_lib.zedo_joint_temporal_workspace_bytes, dev, N, H, J)
        path = torch.empty((N, J), dtype=torch.int32, device=dev)
        cost = torch.empty((N, J), dtype=torch.float64, device=dev)
        _check(_lib.zedo_joint_temporal_select(_p(junary, torch.float64), _p(x_full), _p(T_full), _p(seq, torch.int32), seq.numel() - 1, H, N,
                                               J, float(lam), _p(ws, torch.uint8), nbytes, _p(path, torch.int32), _p(cost, torch.float64),
                                               _stream(dev)))
    return path, cost


def joint_stream_state_bytes(S, H, J, lag, max_frames):
    """The bytes of state zedo_joint_stream_push needs for S streams of H hypotheses and J joints at this lag and at most max_frames
    frames per push (host arithmetic: no GPU needed); 0 for a shape the calls refuse."""
    return int(_lib.zedo_joint_stream_state_bytes(int(S), int(H), int(J), int(lag), int(max_frames)))


class JointStream:
    """Joint-wise selection on a live video (zedo_joint_stream_push): the chain of joint_temporal_select for S independent streams, fed
    in chunks of at most max_frames frames, every frame decided `lag` frames after it went in - the decision of joint_temporal_select on
    the stream's clip (the frames since its last reset or flush) cut after frame n + lag.  With lag >= the clip's length - 1 and a flush
    at the end the outputs are joint_temporal_select's bits.  Owns the state on `device` and resets it on creation.  lam as in
    joint_temporal_select (untuned); the choice of lag is untuned as well, and whether a fixed-lag path is closer to ground truth than
    the per-frame choice is not measured."""

    _WHAT, _CALL = "JointStream", "zedo_joint_stream"              # the entry points: _CALL + "_state_bytes", "_reset", "_push"
    _RANGE = "1 <= H <= 1024, lag >= 0, sizes >= 1, (lag + max_frames) S J H <= INT_MAX"

    def __init__(self, S, H, J, lag, max_frames, lam=100.0, device=None):
        _need_gpu()
        self.S, self.H, self.J, self.lag, self.max_frames, self.lam = int(S), int(H), int(J), int(lag), int(max_frames), float(lam)
        self.device = _norm_device(device)
        self.state_bytes = int(getattr(_lib, self._CALL + "_state_bytes")(int(S), int(H), int(J), int(lag), int(max_frames)))
        if self.state_bytes == 0:
            raise ZedoError(f"{self._WHAT}: S = {S}, H = {H}, J = {J}, lag = {lag}, max_frames = {max_frames} is outside the range of "
                            f"{self._CALL}_push ({self._RANGE})")
        with torch.cuda.device(self.device):
            self.state = torch.empty((self.state_bytes,), dtype=torch.uint8, device=self.device)
        self.reset()

    def _flags(self, which):
        """None, or `which` as an int32 [S] tensor on the device (a tensor, or a sequence of S truth values)."""
        if which is None:
            return None
        if isinstance(which, torch.Tensor):
            w = which.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            w = torch.tensor([1 if v else 0 for v in which], dtype=torch.int32, device=self.device)
        if tuple(w.shape) != (self.S,):
            raise ValueError(f"{self._WHAT}: one flag per stream ([{self.S}]) expected, got {tuple(w.shape)}")
        return w

    def reset(self, which=None):
        """Empties the streams with which[s] != 0 (None: all); their pending frames are dropped."""
        w = self._flags(which)
        with torch.cuda.device(self.device):
            _check(getattr(_lib, self._CALL + "_reset")(_p(self.state, torch.uint8), self.state_bytes, self.S, self.H, self.J, self.lag,
                                                        self.max_frames, _p(w, torch.int32), _stream(self.device)))

    def _chunk(self, junary, x, T, flush):
        """-> (the flush flags on the device or None, F, the device) of a push; ValueError for shapes that are not a chunk."""
        fl = self._flags(flush)
        S, H, J = self.S, self.H, self.J
        if junary is None:
            if x is not None or T is not None or fl is None:
                raise ValueError(f"{self._WHAT}.push: a push of no frames takes flush and nothing else")
            return fl, 0, self.device
        rows = x.shape[0]
        F = rows // (H * S)
        if (rows != H * S * F or F < 1 or tuple(x.shape) != (rows, J, 3) or tuple(junary.shape) != (rows, J)
                or (T is not None and tuple(T.shape) != (rows, 3))):
            raise ValueError(f"{self._WHAT}.push: junary [H*S*F,J], x [H*S*F,J,3], T [H*S*F,3] with H = {H}, S = {S}, J = {J} expected, "
                             f"got {tuple(junary.shape)}, {tuple(x.shape)}, {None if T is None else tuple(T.shape)}")
        return fl, F, _device_of(junary, x, T, self.state)

    def push(self, junary, x, T=None, flush=None):
        """junary [H*S*F,J] f64, x [H*S*F,J,3] f32, T [H*S*F,3] f32 or None: F <= max_frames new frames of every stream, rows (h, n)
        h-major with n = s F + f - stream s's chunk is a clip of F frames of joint_temporal_select on the same tensors; flush: None, or
        [S] flags - the streams whose clip ends with this chunk.  -> (first [S] i64, count [S] i64, path [S,F+lag,J] i32, cost
        [S,F+lag,J] f64): stream s emits the frames first[s] .. first[s] + count[s] - 1 of its clip in the rows 0 .. count[s] - 1 of
        path[s] and cost[s]; the rows after them are not written.  count[s] = held if flushed, else max(0, held - lag), with held =
        min(lag, frames the clip held before) + F.  junary = None: a push of no frames (flush required)."""
        fl, F, dev = self._chunk(junary, x, T, flush)
        S, H, J = self.S, self.H, self.J
        with torch.cuda.device(dev):
            rows = F + self.lag                                      # lag = 0 and no frames: a row nobody writes keeps the pointers non-NULL
            path = torch.empty((S, max(rows, 1), J), dtype=torch.int32, device=dev)
            cost = torch.empty((S, max(rows, 1), J), dtype=torch.float64, device=dev)
            emit = torch.empty((S, 2), dtype=torch.int64, device=dev)
            _check(_lib.zedo_joint_stream_push(_p(junary, torch.float64), _p(x), _p(T), S, F, H, J, self.lag, self.max_frames, self.lam,
                                               _p(fl, torch.int32), _p(self.state, torch.uint8), self.state_bytes, _p(path, torch.int32),
                                               _p(cost, torch.float64), _p(emit, torch.int64), _stream(dev)))
        return emit[:, 0], emit[:, 1], path[:, :rows], cost[:, :rows]

    def flush(self, which=None):
        """Ends the clips of the streams with which[s] != 0 (None: all) and emits their pending frames: a push of no frames."""
        return self.push(None, None, None, [1] * self.S if which is None else which)


def temporal_stream_state_bytes(S, H, J, lag, max_frames):
    """The bytes of state zedo_temporal_stream_push needs for S streams of H hypotheses and J joints at this lag and at most max_frames
    frames per push (host arithmetic: no GPU needed); 0 for a shape the calls refuse."""
    return int(_lib.zedo_temporal_stream_state_bytes(int(S), int(H), int(J), int(lag), int(max_frames)))


class TemporalStream(JointStream):
    """Pose-level selection on a live video (zedo_temporal_stream_push): the chain of temporal_select for S independent streams, fed in
    chunks of at most max_frames frames, every frame decided `lag` frames after it went in - the decision of temporal_select on the
    stream's clip (the frames since its last reset or flush) cut after frame n + lag.  With lag >= the clip's length - 1 and a flush at
    the end the outputs are temporal_select's bits.  Owns the state on `device` and resets it on creation.  lam as in temporal_select
    (untuned); the choice of lag is untuned as well, and whether a fixed-lag path is closer to ground truth than the per-frame arg-min
    is not measured.  The state holds max_frames H^2 transition costs per stream."""

    _WHAT, _CALL = "TemporalStream", "zedo_temporal_stream"
    _RANGE = "1 <= H <= 1024, lag >= 0, sizes >= 1, (lag + max_frames) S H, S max_frames H^2 and 3 S H J <= INT_MAX"

    def push(self, unary, x, flush=None):
        """unary [H*S*F] f64, x [H*S*F,J,3] f32: F <= max_frames new frames of every stream, rows (h, n) h-major with n = s F + f -
        stream s's chunk is a clip of F frames of temporal_select on the same tensors; flush: None, or [S] flags - the streams whose
        clip ends with this chunk.  -> (first [S] i64, count [S] i64, path [S,F+lag] i32, cost [S,F+lag] f64): stream s emits the frames
        first[s] .. first[s] + count[s] - 1 of its clip in the rows 0 .. count[s] - 1 of path[s] and cost[s]; the rows after them are
        not written.  count[s] = held if flushed, else max(0, held - lag), with held = min(lag, frames the clip held before) + F.
        unary = None: a push of no frames (flush required)."""
        fl = self._flags(flush)
        S, H, J = self.S, self.H, self.J
        if unary is None:
            if x is not None or fl is None:
                raise ValueError(f"{self._WHAT}.push: a push of no frames takes flush and nothing else")
            F, dev = 0, self.device
        else:
            rows = x.shape[0]
            F = rows // (H * S)
            if rows != H * S * F or F < 1 or tuple(x.shape) != (rows, J, 3) or tuple(unary.shape) != (rows,):
                raise ValueError(f"{self._WHAT}.push: unary [H*S*F], x [H*S*F,J,3] with H = {H}, S = {S}, J = {J} expected, got "
                                 f"{tuple(unary.shape)}, {tuple(x.shape)}")
            dev = _device_of(unary, x, self.state)
        with torch.cuda.device(dev):
            rows = F + self.lag                                      # lag = 0 and no frames: a row nobody writes keeps the pointers non-NULL
            path = torch.empty((S, max(rows, 1)), dtype=torch.int32, device=dev)
            cost = torch.empty((S, max(rows, 1)), dtype=torch.float64, device=dev)
            emit = torch.empty((S, 2), dtype=torch.int64, device=dev)
            _check(_lib.zedo_temporal_stream_push(_p(unary, torch.float64), _p(x), S, F, H, J, self.lag, self.max_frames, self.lam,
                                                  _p(fl, torch.int32), _p(self.state, torch.uint8), self.state_bytes, _p(path, torch.int32),
                                                  _p(cost, torch.float64), _p(emit, torch.int64), _stream(dev)))
        return emit[:, 0], emit[:, 1], path[:, :rows], cost[:, :rows]

    def flush(self, which=None):
        """Ends the clips of the streams with which[s] != 0 (None: all) and emits their pending frames: a push of no frames."""
        return self.push(None, None, [1] * self.S if which is None else which)


def joint_stream_marginal_state_bytes(S, H, J, lag, max_frames):
    """The bytes of state zedo_joint_stream_marginal_push needs for S streams of H hypotheses and J joints at this lag and at most
    max_frames frames per push (host arithmetic: no GPU needed); 0 for a shape the calls refuse."""
    return int(_lib.zedo_joint_stream_marginal_state_bytes(int(S), int(H), int(J), int(lag), int(max_frames)))


class JointMarginalStream(JointStream):
    """Joint-wise fusion on a live video (zedo_joint_stream_marginal_push): the chain model of joint_marginal for S independent streams,
    fed in chunks of at most max_frames frames, every frame's marginals formed `lag` frames after it went in - the outputs of
    joint_marginal on the stream's clip (the frames since its last reset or flush) cut after frame n + lag: fixed-lag smoothing.  lag = 0
    gives the filtering marginals; with lag >= the clip's length - 1 and a flush at the end the outputs are joint_marginal's bits.  Owns
    the state on `device` and resets it on creation.  lam and tau as in joint_marginal, the same in every push; lam = 100 and tau = 1
    are untuned, the choice of lag is untuned as well, and whether the fused pose is closer to ground truth than a selected one is not
    measured.  A steady-state push costs F backward walks of lag frames per (stream, joint)."""
    _WHAT, _CALL = "JointMarginalStream", "zedo_joint_stream_marginal"

    def __init__(self, S, H, J, lag, max_frames, lam=100.0, tau=1.0, device=None):
        self.tau = float(tau)
        super().__init__(S, H, J, lag, max_frames, lam, device)

    def push(self, junary, x, T=None, flush=None, return_weights=False):
        """The chunk and flush of JointStream.push -> (first [S] i64, count [S] i64, mean [S,F+lag,J,3] f64, cov [S,F+lag,J,6] f64, hmax
        [S,F+lag,J] i32, wmax [S,F+lag,J] f64, logz [S,F+lag,J] f64[, w [S,F+lag,J,H] f64]): stream s emits the frames first[s] ..
        first[s] + count[s] - 1 of its clip in the rows 0 .. count[s] - 1; the rows after them are not written.  The outputs of a row
        are joint_marginal's: posterior mean position in the camera frame, covariance (xx, xy, xz, yy, yz, zz; m^2), the most probable
        hypothesis, its probability, log Z of the chain cut at the frame's horizon; a dead (frame, joint) reports NaN, 0, 0 and -inf.
        junary = None: a push of no frames (flush required)."""
        fl, F, dev = self._chunk(junary, x, T, flush)
        S, H, J = self.S, self.H, self.J
        with torch.cuda.device(dev):
            rows = F + self.lag                                      # lag = 0 and no frames: a row nobody writes keeps the pointers non-NULL
            mean, cov, hmax, wmax, logz, w = (None if t is None else t.view(S, max(rows, 1), *t.shape[1:])
                                              for t in _marginal_outputs(S * max(rows, 1), J, H, dev, return_weights))
            emit = torch.empty((S, 2), dtype=torch.int64, device=dev)
            _check(_lib.zedo_joint_stream_marginal_push(_p(junary, torch.float64), _p(x), _p(T), S, F, H, J, self.lag, self.max_frames,
                                                        self.lam, self.tau, _p(fl, torch.int32), _p(self.state, torch.uint8),
                                                        self.state_bytes, _p(mean, torch.float64), _p(cov, torch.float64),
                                                        _p(hmax, torch.int32), _p(wmax, torch.float64), _p(logz, torch.float64),
                                                        _p(w, torch.float64), _p(emit, torch.int64), _stream(dev)))
        out = (emit[:, 0], emit[:, 1]) + tuple(t[:, :rows] for t in (mean, cov, hmax, wmax, logz))
        return out + (w[:, :rows],) if return_weights else out

    def flush(self, which=None, return_weights=False):
        """Ends the clips of the streams with which[s] != 0 (None: all) and emits their pending frames: a push of no frames."""
        return self.push(None, None, None, [1] * self.S if which is None else which, return_weights)


def joint_accel_select(junary, x_full, T_full, seq_start, N=None, lam=100.0, accel=100.0):
    """Joint-wise selection along a video with a second-order motion model (zedo_joint_accel_select): the inputs of joint_temporal_select
    and a second weight -> (path [N,J] i32, cost [N,J] f64): per (clip, joint) the hypothesis sequence that minimises the sum of that
    joint's unaries plus lam times its displacement plus accel times its second difference X[n] - 2 X[n-1] + X[n-2] in the camera frame
    (x + T) - a term that is blind to a constant velocity (Viterbi over pairs of hypotheses, fp64, one chain per joint).  cost is the
    cost of the kept path re-accumulated along it.  lam and accel are in cost units per metre; the defaults of 100 are untuned; lam = 0
    is the pure second-order chain.  At most 64 hypotheses; the workspace is one byte per (frame, joint, pair).  Whether these paths are
    closer to ground truth than joint_temporal_select's is not measured."""
    dev, seq, N, H, J = _chain_inputs("joint_accel_select", junary, x_full, T_full, seq_start, N, joint_wise=True)
    with torch.cuda.device(dev):
        nbytes, ws = _workspace(_lib.zedo_joint_accel_workspace_bytes, dev, N, H, J)
        path = torch.empty((N, J), dtype=torch.int32, device=dev)
        cost = torch.empty((N, J), dtype=torch.float64, device=dev)
        _check(_lib.zedo_joint_accel_select(_p(junary, torch.float64), _p(x_full), _p(T_full), _p(seq, torch.int32), seq.numel() - 1, H, N,
                                            J, float(lam), float(accel), _p(ws, torch.uint8), nbytes, _p(path, torch.int32),
                                            _p(cost, torch.float64), _stream(dev)))
    return path, cost


def joint_accel_stream_state_bytes(S, H, J, lag, max_frames):
    """The bytes of state zedo_joint_accel_stream_push needs for S streams of H hypotheses and J joints at this lag and at most
    max_frames frames per push (host arithmetic: no GPU needed); 0 for a shape the calls refuse."""
    return int(_lib.zedo_joint_accel_stream_state_bytes(int(S), int(H), int(J), int(lag), int(max_frames)))


class JointAccelStream(JointStream):
    """Joint-wise selection on a live video under the second-order motion model (zedo_joint_accel_stream_push): the chain over pairs of
    joint_accel_select for S independent streams, fed in chunks of at most max_frames frames, every frame decided `lag` frames after it
    went in - the path of joint_accel_select on the stream's clip (the frames since its last reset or flush) cut after frame n + lag.
    lag = 0 gives the h of the arg-min pair of E[n]; with lag >= the clip's length - 1 and a flush at the end the paths are
    joint_accel_select's bits.  cost is the cost of the best path on the clip cut at the frame's horizon - not joint_accel_select's
    re-accumulated cost: fixed-lag decisions of consecutive frames need not lie on one path.  At most 64 hypotheses.  Owns the state on
    `device` and resets it on creation.  lam, accel and lag are untuned; accuracy on real video is unmeasured."""
    _WHAT, _CALL = "JointAccelStream", "zedo_joint_accel_stream"
    _RANGE = "1 <= H <= 64, lag >= 0, sizes >= 1, (lag + max_frames) S J H^2 <= INT_MAX"

    def __init__(self, S, H, J, lag, max_frames, lam=100.0, accel=100.0, device=None):
        self.accel = float(accel)
        super().__init__(S, H, J, lag, max_frames, lam, device)

    def push(self, junary, x, T=None, flush=None):
        """The chunk and flush of JointStream.push -> (first [S] i64, count [S] i64, path [S,F+lag,J] i32, cost [S,F+lag,J] f64), rows
        as there.  junary = None: a push of no frames (flush required)."""
        fl, F, dev = self._chunk(junary, x, T, flush)
        S, H, J = self.S, self.H, self.J
        with torch.cuda.device(dev):
            rows = F + self.lag                                      # lag = 0 and no frames: a row nobody writes keeps the pointers non-NULL
            path = torch.empty((S, max(rows, 1), J), dtype=torch.int32, device=dev)
            cost = torch.empty((S, max(rows, 1), J), dtype=torch.float64, device=dev)
            emit = torch.empty((S, 2), dtype=torch.int64, device=dev)
            _check(_lib.zedo_joint_accel_stream_push(_p(junary, torch.float64), _p(x), _p(T), S, F, H, J, self.lag, self.max_frames,
                                                     self.lam, self.accel, _p(fl, torch.int32), _p(self.state, torch.uint8),
                                                     self.state_bytes, _p(path, torch.int32), _p(cost, torch.float64),
                                                     _p(emit, torch.int64), _stream(dev)))
        return emit[:, 0], emit[:, 1], path[:, :rows], cost[:, :rows]


def joint_accel_stream_marginal_state_bytes(S, H, J, lag, max_frames):
    """The bytes of state zedo_joint_accel_stream_marginal_push needs for S streams of H hypotheses and J joints at this lag and at most
    max_frames frames per push (host arithmetic: no GPU needed); 0 for a shape the calls refuse."""
    return int(_lib.zedo_joint_accel_stream_marginal_state_bytes(int(S), int(H), int(J), int(lag), int(max_frames)))


class JointAccelMarginalStream(JointStream):
    """Joint-wise fusion on a live video under the second-order motion model (zedo_joint_accel_stream_marginal_push): the chain over pairs
    of joint_accel_marginal for S independent streams, fed in chunks of at most max_frames frames, every frame's marginals formed `lag`
    frames after it went in - the outputs of joint_accel_marginal on the stream's clip (the frames since its last reset or flush) cut
    after frame n + lag: fixed-lag smoothing.  lag = 0 gives the filtering marginals; with lag >= the clip's length - 1 and a flush at
    the end the outputs are joint_accel_marginal's bits.  At most 64 hypotheses; the state holds the pair table of every frame of the
    window, 8 H^2 bytes per (stream, joint, frame).  Owns the state on `device` and resets it on creation.  lam, accel and tau as in
    joint_accel_marginal, the same in every push; lam, accel, tau and the lag are untuned, and accuracy on real video is unmeasured.  A
    steady-state push costs F backward walks of lag frames per (stream, joint)."""
    _WHAT, _CALL = "JointAccelMarginalStream", "zedo_joint_accel_stream_marginal"
    _RANGE = "1 <= H <= 64, lag >= 0, sizes >= 1, (lag + max_frames + 2) S J H^2 <= INT_MAX"

    def __init__(self, S, H, J, lag, max_frames, lam=100.0, accel=100.0, tau=1.0, device=None):
        self.accel, self.tau = float(accel), float(tau)
        super().__init__(S, H, J, lag, max_frames, lam, device)

    def push(self, junary, x, T=None, flush=None, return_weights=False):
        """The chunk and flush of JointStream.push -> the tuple of JointMarginalStream.push: (first [S] i64, count [S] i64, mean
        [S,F+lag,J,3] f64, cov [S,F+lag,J,6] f64, hmax [S,F+lag,J] i32, wmax [S,F+lag,J] f64, logz [S,F+lag,J] f64[, w [S,F+lag,J,H]
        f64]), rows as there; the outputs of a row are joint_accel_marginal's.  junary = None: a push of no frames (flush required)."""
        fl, F, dev = self._chunk(junary, x, T, flush)
        S, H, J = self.S, self.H, self.J
        with torch.cuda.device(dev):
            rows = F + self.lag                                      # lag = 0 and no frames: a row nobody writes keeps the pointers non-NULL
            mean, cov, hmax, wmax, logz, w = (None if t is None else t.view(S, max(rows, 1), *t.shape[1:])
                                              for t in _marginal_outputs(S * max(rows, 1), J, H, dev, return_weights))
            emit = torch.empty((S, 2), dtype=torch.int64, device=dev)
            _check(_lib.zedo_joint_accel_stream_marginal_push(_p(junary, torch.float64), _p(x), _p(T), S, F, H, J, self.lag, self.max_frames,
                                                              self.lam, self.accel, self.tau, _p(fl, torch.int32),
                                                              _p(self.state, torch.uint8), self.state_bytes, _p(mean, torch.float64),
                                                              _p(cov, torch.float64), _p(hmax, torch.int32), _p(wmax, torch.float64),
                                                              _p(logz, torch.float64), _p(w, torch.float64), _p(emit, torch.int64),
                                                              _stream(dev)))
        out = (emit[:, 0], emit[:, 1]) + tuple(t[:, :rows] for t in (mean, cov, hmax, wmax, logz))
        return out + (w[:, :rows],) if return_weights else out

    flush = JointMarginalStream.flush


# the 16 bones every ported dataset's get_skeleton() returns (H36M's 17 joints)
H36M_EDGES = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15),
              (15, 16))


def skeleton_parents(edges, J, root=0):
    """The parent array of a skeleton: edges = J - 1 undirected bones (a, b) as get_skeleton() lists them -> [J] ints, parent[root] = -1,
    by breadth-first search from `root`.  ValueError for an edge list that is not a spanning tree of the J joints (a wrong number of
    bones, a joint outside 0 .. J-1, a bone from a joint to itself, a cycle, or a joint the root does not reach)."""
    J, root = int(J), int(root)
    edges = [(int(a), int(b)) for a, b in edges]
    if J < 1 or not 0 <= root < J:
        raise ValueError(f"skeleton_parents: root {root} is not one of {J} joints")
    if len(edges) != J - 1 or any(a == b or not (0 <= a < J and 0 <= b < J) for a, b in edges):
        raise ValueError(f"skeleton_parents: {J - 1} bones between two different joints in 0 .. {J - 1} expected, got {len(edges)}: not a spanning tree")
    nbr = [[] for _ in range(J)]
    for a, b in edges:
        nbr[a].append(b)
        nbr[b].append(a)
    parent, seen, queue = [-1] * J, [False] * J, [root]
    seen[root] = True
    for v in queue:
        for c in nbr[v]:
            if not seen[c]:
                seen[c], parent[c] = True, v
                queue.append(c)
    if len(queue) != J:                       # J - 1 bones that leave a joint out close a cycle elsewhere
        raise ValueError(f"skeleton_parents: the bones do not connect all {J} joints to joint {root} (a cycle or a disconnected part): not a spanning tree")
    return parent


def joint_tree_select(junary, x_full, T_full, parent, N=None, mu=100.0, weight=None):
    """Skeleton-coupled joint-wise aggregation without ground truth (zedo_joint_tree_select): junary [H*N,J] f64 (ALL rows, h-major: e.g.
    jerr of joint_reproj(return_rows=True), pixels), x_full [H*N,J,3] f32, T_full [H*N,3] f32 or None, parent [J] ints (a forest: -1 for a
    root; skeleton_parents builds it from a get_skeleton() edge list), weight [N,J] f32 or None (confidences, clamped to 1e-4 .. 1 as
    min_reproj clamps them) -> (joint_h [N,J] i32, cost [N] f64, bone [N,J] f64): per pose the assignment of a hypothesis to every joint
    that minimises the sum of the weighted unaries plus mu times, over the bones, the difference between the assembled bone's length and
    the mean of the lengths its two hypotheses give that bone (exact min-sum over the tree, fp64); bone is that difference in metres at
    the kept assignment.  mu is in cost units per metre; the default of 100 is untuned.  mu = 0 is joint_reproj's arg-min, a large mu one
    whole hypothesis per pose.  Whether the coupled pose is closer to ground truth than the per-joint arg-min is not measured."""
    dev, par, N, H, J = _tree_inputs("joint_tree_select", junary, x_full, T_full, parent, N, weight)
    with torch.cuda.device(dev):
        joint_h = torch.empty((N, J), dtype=torch.int32, device=dev)
        cost = torch.empty((N,), dtype=torch.float64, device=dev)
        bone = torch.empty((N, J), dtype=torch.float64, device=dev)
        _check(_lib.zedo_joint_tree_select(_p(junary, torch.float64), _p(x_full), _p(T_full), _p(weight), par.ctypes.data_as(ctypes.c_void_p),
                                           H, N, J, float(mu), _p(joint_h, torch.int32), _p(cost, torch.float64), _p(bone, torch.float64),
                                           _stream(dev)))
    return joint_h, cost, bone


def joint_tree_marginal_max_h(J):
    """The largest number of hypotheses joint_tree_marginal admits at J joints (zedo_joint_tree_marginal_max_h): what fits the LDS of one
    workgroup, 48 J H + 16 H + 8192 <= 163840 bytes, at most 1024; 0 for a J outside 1 .. 64."""
    return int(_lib.zedo_joint_tree_marginal_max_h(int(J)))


def joint_tree_marginal(junary, x_full, T_full, parent, N=None, mu=100.0, tau=1.0, weight=None, return_weights=False):
    """Skeleton-coupled fusion per pose without ground truth (zedo_joint_tree_marginal): the inputs of joint_tree_select and a temperature
    tau > 0 in cost units -> (mean [N,J,3] f64, cov [N,J,6] f64, hmax [N,J] i32, wmax [N,J] f64, logz [N,J] f64, bone [N,J] f64[, w
    [N,J,H] f64]): per pose the exact posterior marginals w of every joint's hypotheses under p(assignment) ~ exp(-(weighted unaries +
    mu * bone mismatches) / tau), the energy joint_tree_select minimises (sum-product over the bone tree, fp64), and from them the
    posterior mean position in the camera frame, its covariance (xx, xy, xz, yy, yz, zz; m^2), the most probable hypothesis, its
    probability, the log-partition value of the joint's component and the expected mismatch of the bone to the parent (metres).  A dead
    joint reports NaN, 0, 0, -inf and 0.  mu = 100 and tau = 1 are untuned.  At most joint_tree_marginal_max_h(J) hypotheses.  Whether the
    fused pose is closer to ground truth than a selected one is not measured."""
    dev, par, N, H, J = _tree_inputs("joint_tree_marginal", junary, x_full, T_full, parent, N, weight)
    with torch.cuda.device(dev):
        mean, cov, hmax, wmax, logz, w = _marginal_outputs(N, J, H, dev, return_weights)
        bone = torch.empty((N, J), dtype=torch.float64, device=dev)
        _check(_lib.zedo_joint_tree_marginal(_p(junary, torch.float64), _p(x_full), _p(T_full), _p(weight), par.ctypes.data_as(ctypes.c_void_p),
                                             H, N, J, float(mu), float(tau), _p(mean, torch.float64), _p(cov, torch.float64),
                                             _p(hmax, torch.int32), _p(wmax, torch.float64), _p(logz, torch.float64), _p(bone, torch.float64),
                                             _p(w, torch.float64), _stream(dev)))
    return (mean, cov, hmax, wmax, logz, bone, w) if return_weights else (mean, cov, hmax, wmax, logz, bone)


def joint_marginal(junary, x_full, T_full, seq_start, N=None, lam=100.0, tau=1.0, return_weights=False):
    """Fusing hypotheses along a video without ground truth (zedo_joint_marginal): the inputs of joint_temporal_select and a temperature
    tau > 0 in cost units -> (mean [N,J,3] f64, cov [N,J,6] f64, hmax [N,J] i32, wmax [N,J] f64, logz [N,J] f64[, w [N,J,H] f64]): per
    (clip, joint) the posterior marginals w of the hypotheses under p(path) ~ exp(-(unaries + lam * displacements) / tau), the chain
    model joint_temporal_select optimises (forward-backward, fp64), and from them the posterior mean position in the camera frame, its
    covariance (xx, xy, xz, yy, yz, zz; m^2), the most probable hypothesis, its probability and the chain's log-partition value.  A dead
    (frame, joint) reports NaN, 0, 0 and -inf.  lam = 100 and tau = 1 are untuned.  At most 1024 hypotheses.  Whether the fused pose is
    closer to ground truth than a selected one is not measured."""
    dev, seq, N, H, J = _chain_inputs("joint_marginal", junary, x_full, T_full, seq_start, N, joint_wise=True)
    with torch.cuda.device(dev):
        nbytes, ws = _workspace(_lib.zedo_joint_marginal_workspace_bytes, dev, N, H, J)
        mean, cov, hmax, wmax, logz, w = _marginal_outputs(N, J, H, dev, return_weights)
        _check(_lib.zedo_joint_marginal(_p(junary, torch.float64), _p(x_full), _p(T_full), _p(seq, torch.int32), seq.numel() - 1, H, N, J,
                                        float(lam), float(tau), _p(ws, torch.uint8), nbytes, _p(mean, torch.float64),
                                        _p(cov, torch.float64), _p(hmax, torch.int32), _p(wmax, torch.float64), _p(logz, torch.float64),
                                        _p(w, torch.float64), _stream(dev)))
    return (mean, cov, hmax, wmax, logz, w) if return_weights else (mean, cov, hmax, wmax, logz)


def temporal_marginal_workspace_bytes(N, H, chunk_frames=0):
    """The bytes of workspace zedo_temporal_marginal takes for N frames of H hypotheses with chunk_frames frames of transition costs held
    at once (0: at most 256 MB of them) - host arithmetic: no GPU needed; 0 for a shape the call refuses."""
    return int(_lib.zedo_temporal_marginal_workspace_bytes(int(N), int(H), int(chunk_frames)))


def temporal_marginal(unary, x_full, T_full, seq_start, N=None, lam=100.0, tau=1.0, chunk_frames=0, return_weights=False):
    """Fusing whole hypotheses along a video without ground truth (zedo_temporal_marginal): the inputs of temporal_select, T_full [H*N,3]
    f32 or None and a temperature tau > 0 in cost units -> (mean [N,J,3] f64, cov [N,J,6] f64, hmax [N] i32, wmax [N] f64, logz [N]
    f64[, w [N,H] f64]): per clip the posterior marginals w of the hypotheses - whole poses - under p(path) ~ exp(-(unaries + lam * mean
    joint displacements) / tau), the chain model temporal_select optimises (forward-backward, fp64), and from them the posterior mean
    pose, every joint's covariance (xx, xy, xz, yy, yz, zz; m^2), the most probable hypothesis of a frame, its probability and the
    chain's log-partition value.  T_full enters only the positions the moments are taken of (x + T), not the motion term.  A dead
    frame reports NaN, 0, 0 and -inf.  lam = 100 and tau = 1 are untuned.  At most 1024 hypotheses.  chunk_frames: frames of transition
    costs held at once (0: at most 256 MB); the result does not depend on it.  Whether the fused pose is closer to ground truth than a
    selected one is not measured."""
    dev, seq, N, H, J = _chain_inputs("temporal_marginal", unary, x_full, T_full, seq_start, N, joint_wise=False)
    with torch.cuda.device(dev):
        nbytes, ws = _workspace(_lib.zedo_temporal_marginal_workspace_bytes, dev, N, H, int(chunk_frames))
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        mean, cov, hmax, wmax, logz = f64(N, J, 3), f64(N, J, 6), torch.empty((N,), dtype=torch.int32, device=dev), f64(N), f64(N)
        w = f64(N, H) if return_weights else None
        _check(_lib.zedo_temporal_marginal(_p(unary, torch.float64), _p(x_full), _p(T_full), _p(seq, torch.int32), seq.numel() - 1, H, N, J,
                                           float(lam), float(tau), _p(ws, torch.uint8), nbytes, _p(mean, torch.float64),
                                           _p(cov, torch.float64), _p(hmax, torch.int32), _p(wmax, torch.float64), _p(logz, torch.float64),
                                           _p(w, torch.float64), _stream(dev)))
    return (mean, cov, hmax, wmax, logz, w) if return_weights else (mean, cov, hmax, wmax, logz)


def joint_accel_marginal(junary, x_full, T_full, seq_start, N=None, lam=100.0, accel=100.0, tau=1.0, return_weights=False):
    """Fusing hypotheses along a video under the second-order motion model (zedo_joint_accel_marginal): the inputs of joint_accel_select
    and a temperature tau > 0 in cost units -> (mean [N,J,3] f64, cov [N,J,6] f64, hmax [N,J] i32, wmax [N,J] f64, logz [N,J] f64[, w
    [N,J,H] f64]): per (clip, joint) the posterior marginals w of the hypotheses under p(path) ~ exp(-(unaries + lam * displacements +
    accel * second differences) / tau), the chain over pairs of hypotheses joint_accel_select optimises (forward-backward over pairs,
    fp64), and from them what joint_marginal reports: the posterior mean position in the camera frame, its covariance (xx, xy, xz, yy,
    yz, zz; m^2), the most probable hypothesis, its probability and the chain's log-partition value.  A dead (frame, joint) reports NaN,
    0, 0 and -inf.  lam = 100, accel = 100 and tau = 1 are untuned; lam = 0 is blind to a constant velocity.  At most 64 hypotheses; the
    workspace is 8 bytes per (frame, joint, pair) - 345 MB at 1 015 frames x 17 joints x 50 hypotheses: cut a long recording into calls of
    whole clips.  Whether the fused pose is closer to ground truth than joint_marginal's is not measured."""
    dev, seq, N, H, J = _chain_inputs("joint_accel_marginal", junary, x_full, T_full, seq_start, N, joint_wise=True)
    if H > 64:
        raise ZedoError(f"joint_accel_marginal: at most 64 hypotheses (the pair tables of a joint stay in the LDS), got H = {H}")
    with torch.cuda.device(dev):
        nbytes, ws = _workspace(_lib.zedo_joint_accel_marginal_workspace_bytes, dev, N, H, J)
        mean, cov, hmax, wmax, logz, w = _marginal_outputs(N, J, H, dev, return_weights)
        _check(_lib.zedo_joint_accel_marginal(_p(junary, torch.float64), _p(x_full), _p(T_full), _p(seq, torch.int32), seq.numel() - 1, H, N,
                                              J, float(lam), float(accel), float(tau), _p(ws, torch.uint8), nbytes,
                                              _p(mean, torch.float64), _p(cov, torch.float64), _p(hmax, torch.int32),
                                              _p(wmax, torch.float64), _p(logz, torch.float64), _p(w, torch.float64), _stream(dev)))
    return (mean, cov, hmax, wmax, logz, w) if return_weights else (mean, cov, hmax, wmax, logz)


def prune_rank(err, N, K):
    """The table of kept slots between two stages of the loop (zedo_prune_rank): err [H*N] f64 (ALL rows of the current slots, h-major:
    e.g. err of min_reproj) -> keep [K,N] i32, per pose the K slots with the smallest error in ascending slot order.  Finite errors
    ascending, then +inf, then NaN, ties to the lower slot: a diverged row is the first to go.  1 <= K <= H <= 1024."""
    _need_gpu()
    dev = _device_of(err)
    N, K = int(N), int(K)
    if N < 1 or err.dim() != 1 or err.shape[0] % N or err.shape[0] == 0:
        raise ValueError(f"prune_rank: err [H*N] expected, got {tuple(err.shape)} with N = {N}")
    H = err.shape[0] // N
    if not 1 <= K <= H:
        raise ValueError(f"prune_rank: 1 <= K <= H = {H} expected, got K = {K}")
    with torch.cuda.device(dev):
        keep = torch.empty((K, N), dtype=torch.int32, device=dev)
        _check(_lib.zedo_prune_rank(_p(err, torch.float64), H, N, K, _p(keep, torch.int32), _stream(dev)))
    return keep


def prune_gather(keep, x, T, hyp=None):
    """The rows of the kept slots, compacted (zedo_prune_gather): keep [K,N] i32 (of prune_rank), x [H*N,J,3] and T [H*N,3] f32 (ALL rows,
    h-major), hyp [H,N] i32 or None: the original hypothesis id of every current slot (None: the slots are the hypotheses) ->
    (x_out [K*N,J,3], T_out [K*N,3], hyp_out [K,N] i32); row (r, n) is the input row (keep[r,n], n).  An entry of keep outside the slots
    gives a NaN row with id -1."""
    _need_gpu()
    dev = _device_of(keep, x, T, hyp)
    if keep.dim() != 2 or x.dim() != 3:
        raise ValueError(f"prune_gather: keep [K,N] and x [H*N,J,3] expected, got {tuple(keep.shape)} and {tuple(x.shape)}")
    K, N = keep.shape
    rows, J = x.shape[0], x.shape[1]
    H = rows // N if N else 0
    if (N < 1 or K < 1 or rows % N or K > H or tuple(x.shape) != (rows, J, 3) or tuple(T.shape) != (rows, 3)
            or (hyp is not None and tuple(hyp.shape) != (H, N))):
        raise ValueError(f"prune_gather: keep [K,N], x [H*N,J,3], T [H*N,3], hyp [H,N] with K <= H expected, got {tuple(keep.shape)}, "
                         f"{tuple(x.shape)}, {tuple(T.shape)}, {None if hyp is None else tuple(hyp.shape)}")
    with torch.cuda.device(dev):
        x_out = torch.empty((K * N, J, 3), dtype=torch.float32, device=dev)
        T_out = torch.empty((K * N, 3), dtype=torch.float32, device=dev)
        hyp_out = torch.empty((K, N), dtype=torch.int32, device=dev)
        _check(_lib.zedo_prune_gather(_p(keep, torch.int32), H, K, N, J, _p(x), _p(T), _p(hyp, torch.int32), _p(x_out), _p(T_out),
                                      _p(hyp_out, torch.int32), _stream(dev)))
    return x_out, T_out, hyp_out


def pose_min(err, N, row_offset=0):
    """Per-pose minimum / first arg-min over the hypotheses of the (possibly edited) per-row errors (zedo_pose_min)."""
    _need_gpu()
    dev = _device_of(err)
    with torch.cuda.device(dev):
        best = torch.empty((N,), dtype=torch.float64, device=dev)
        best_h = torch.empty((N,), dtype=torch.int32, device=dev)
        _check(_lib.zedo_pose_min(_p(err, torch.float64), err.shape[0], N, int(row_offset), _p(best, torch.float64),
                                  _p(best_h, torch.int32), _stream(dev)))
    return best, best_h


def probe_mfma_peak(iters=100000):
    """-> (sustained fp32-MFMA TFLOP/s, shader clock GHz) of this box right now (zedo_probe_mfma_peak)."""
    _need_gpu()
    tf, ghz = ctypes.c_double(), ctypes.c_double()
    _check(_lib.zedo_probe_mfma_peak(int(iters), ctypes.cast(ctypes.byref(tf), _vp), ctypes.cast(ctypes.byref(ghz), _vp), _stream()))
    return tf.value, ghz.value


def probe_mfma_peak_f16(iters=400000):
    """-> (sustained fp16-MFMA TFLOP/s, shader clock GHz): a bare v_mfma_f32_32x32x16_f16 stream on this box right now
    (zedo_probe_mfma_peak_f16) - the attainable ceiling of the split-fp16 mode's matrix pipe under power management."""
    _need_gpu()
    tf, ghz = ctypes.c_double(), ctypes.c_double()
    _check(_lib.zedo_probe_mfma_peak_f16(int(iters), ctypes.cast(ctypes.byref(tf), _vp), ctypes.cast(ctypes.byref(ghz), _vp), _stream()))
    return tf.value, ghz.value


PROF_CLASSES = ("hidden_dense", "pre_dense", "post_dense_sde", "reproj")


def profile_start(sample_every=16, max_samples=8192):
    _check(_lib.zedo_profile_start(int(sample_every), int(max_samples)))


def profile_stop():
    """-> {class: dict(total_ms, samples, launches, avg_ms, avg_ms_raw)} for the sampled kernel launches.  avg_ms is the
    bracketed duration minus what an empty bracket measures on the same stream (zedo_profile_bracket_ms, also returned
    under the key "bracket_ms" of the hidden_dense entry); avg_ms_raw is the bracketed duration itself."""
    n = len(PROF_CLASSES)
    tot = (ctypes.c_double * n)()
    cnt = (ctypes.c_longlong * n)()
    seen = (ctypes.c_longlong * n)()
    _check(_lib.zedo_profile_stop(ctypes.cast(tot, _vp), ctypes.cast(cnt, _vp), ctypes.cast(seen, _vp)))
    br = float(_lib.zedo_profile_bracket_ms())
    out = {k: dict(total_ms=tot[i], samples=int(cnt[i]), launches=int(seen[i]),
                   avg_ms_raw=(tot[i] / cnt[i] if cnt[i] else None),
                   avg_ms=(max(tot[i] / cnt[i] - br, 0.0) if cnt[i] else None)) for i, k in enumerate(PROF_CLASSES)}
    out["hidden_dense"]["shader_clock_ghz"] = float(_lib.zedo_profile_shader_ghz()) or None
    out["hidden_dense"]["bracket_ms"] = br
    return out
