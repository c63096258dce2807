"""The --select modes of run.inference: one table (MODES) that everything naming a mode is derived from - the parser's choices and help,
check_select_args, the --prune refusal, the --eval label - one function per mode that returns what <out>_selected.npz holds, and the
quantities the modes share (SelectInputs), each computed once, on first use.  A new mode is a table entry and a function."""
from functools import cached_property
from typing import NamedTuple

import numpy as np
import torch


def _hip():
    import zedo_hip.pipeline          # on first use, not at import: the parser and its checks work without the built library
    return zedo_hip


def _arrays(**kw):
    """What a mode writes, in the order given: device tensors as numpy arrays, the hypothesis indices among them (the integer ones) as int32."""
    host = lambda t: t.cpu().numpy() if t.is_floating_point() else t.cpu().numpy().astype(np.int32)
    return {k: host(v) if torch.is_tensor(v) else v for k, v in kw.items()}


class SelectInputs:
    """What run() hands a mode - its own rows x [rows,J,3] and T [rows,3] (global rows lo ..), all rows `full`, with --prune the
    survivor table hyp, `why` (None: the fused route, `pipe` loaded; else the step-wise one, `detections` = the dataset's (gt_2d, K))
    - and what the modes derive from it, cached.  The attributes marked COLLECTIVE exchange with the other ranks on first use: every
    rank touches them, in the same order, and a mode touches them in the order its file was always assembled in."""

    def __init__(self, args, N, H, lo, rows, x, T, full, hyp, why, pipe, detections, dataset, device):
        self.args, self.N, self.H, self.J, self.lo, self.rows, self.x, self.T, self.hyp = args, N, H, x.shape[1], lo, rows, x, T, hyp
        self.full, self.why, self.pipe, self.host_detections, self.dataset, self.device = full.contiguous(), why, pipe, detections, dataset, device
        self.zh, self.pl = _hip(), _hip().pipeline

    @cached_property
    def detections(self):                # (uv [N,J,2], K [N,3,3], conf [N,J]) on the device
        if self.why is None:
            return self.pipe.uv, self.pipe.K, self.pipe.conf
        gt_2d, K = self.host_detections
        d2 = torch.tensor(np.ascontiguousarray(gt_2d), dtype=torch.float32, device=self.device)
        return d2[:, :, :2].contiguous(), torch.tensor(np.ascontiguousarray(K), dtype=torch.float32, device=self.device), d2[:, :, 2].contiguous()

    @cached_property
    def seq(self):                       # the clips of a video: --seq_len, else the dataset's seq_start, else one clip
        if self.args.seq_len is not None:
            return np.array(list(range(0, self.N, self.args.seq_len)) + [self.N], np.int32)
        return np.asarray(getattr(self.dataset, "seq_start", [0, self.N]), np.int32)

    @cached_property
    def parent(self):                    # the bone tree: the dataset's skeleton, else H36M's
        skeleton = self.dataset.get_skeleton() if hasattr(self.dataset, "get_skeleton") else self.zh.H36M_EDGES
        return self.zh.skeleton_parents(skeleton, self.J)

    @cached_property
    def row_err(self):
        """zedo_min_reproj on this rank's rows: (err [rows] f64, best [N] f64, idx [N] i32); a rank without rows: (empty, +inf, -1)."""
        if self.rows == 0:
            return (torch.empty((0,), dtype=torch.float64, device=self.device),) + self.pl.empty_selection(self.N, self.device)
        return self.zh.min_reproj(self.x, self.T.contiguous(), *self.detections, self.N, self.lo)

    def pose_level(self, through_pipeline=False):
        """COLLECTIVE.  (best [N] f64, idx [N] i32): per pose the smallest error over all rows and the hypothesis that attains it - this
        rank's from row_err (through_pipeline: from Pipeline.select_reproj on the fused route), MIN over the ranks."""
        if through_pipeline and self.why is None and self.rows:
            best, idx = self.pipe.select_reproj(self.x, self.T, row_offset=self.lo)
        else:
            _, best, idx = self.row_err
        return self.pl.reduce_min_over_ranks(best, idx)

    def no_joint_rows(self):             # what zedo_joint_reproj reports for a rank without rows: (+inf, -1) per (pose, joint)
        return tuple(t.reshape(self.N, self.J) for t in self.pl.empty_selection(self.N * self.J, self.device))

    @cached_property
    def joint_rows(self):
        """COLLECTIVE.  zedo_joint_reproj by the route that writes every row's per-joint distances: (jbest [N,J] f64, jidx [N,J] i32: what
        --select joints keeps, MIN over the ranks; jerr [rows,J] f64: this rank's rows)."""
        if self.rows == 0:
            jbest, jidx, jerr = self.no_joint_rows() + (torch.empty((0, self.J), dtype=torch.float64, device=self.device),)
        else:
            uv, K, _ = self.detections
            jbest, jidx, jerr = self.zh.joint_reproj(self.x, self.T.contiguous(), uv, K, self.N, self.lo, return_rows=True)
        return self.pl.reduce_min_over_ranks(jbest, jidx) + (jerr,)

    def gather(self, t):
        """COLLECTIVE.  This rank's rows of t -> all H*N rows on every rank, split the way x is; with --prune (one rank) t holds them all."""
        if self.hyp is not None:
            return t
        return self.pl.gather_row_shards(t, self.H * self.N, lo=None if self.why is None else self.lo).contiguous()

    # COLLECTIVE, each: all rows' T [H*N,3], row_err's err [H*N] and joint_rows' jerr [H*N,J]
    full_T = cached_property(lambda self: self.gather(self.T.contiguous()))
    full_err = cached_property(lambda self: self.gather(self.row_err[0]))
    full_jerr = cached_property(lambda self: self.gather(self.joint_rows[2]))

    def take(self, rows_full, idx):
        return self.pl.take_rows(rows_full, idx, self.H, self.N)

    def T_sel(self, idx):                # the translation of hypothesis idx[n] of every pose: the frame its pose is written in
        return self.take(self.full_T, idx).contiguous()

    def joint_px(self, jidx):            # per (pose, joint) the distance of the hypothesis jidx names
        return self.full_jerr.reshape(self.H, self.N, self.J).gather(0, jidx.to(torch.int64)[None])[0]

    def score_assembled(self, jidx, idx):
        """(pose, T_sel, px): joint (n, j) of hypothesis jidx[n,j] in the frame of hypothesis idx[n] (zedo_joint_compose), that frame, and
        the pose's confidence-weighted reprojection error: zedo_min_reproj on the assembled poses as a one-hypothesis problem."""
        pose = self.zh.joint_compose(self.full, self.full_T, jidx.contiguous(), idx.contiguous(), self.N)
        T_sel = self.T_sel(idx)
        return pose, T_sel, self.zh.min_reproj(pose, T_sel, *self.detections, self.N, 0)[1]

    def fused(self, mean, cov, idx):
        """(pose, T_sel, spread): a posterior mean in the frame of hypothesis idx[n], that frame, sqrt(trace cov)."""
        T_sel = self.T_sel(idx)
        return (mean - T_sel.to(torch.float64)[:, None, :]).to(torch.float32), T_sel, (cov[:, :, 0] + cov[:, :, 3] + cov[:, :, 5]).sqrt()


def _reproj(s):
    best, idx = s.pose_level(through_pipeline=True)
    full_T = s.full_T
    kept = idx if s.hyp is None else s.take(s.hyp.reshape(-1), idx)        # with --prune idx is a survivor slot: the file names the original hypothesis
    return _arrays(pose=s.take(s.full, idx), hypothesis=kept, reproj_px=best, T=s.take(full_T, idx))


def _joints(s):
    # zedo_joint_reproj by its walking kernel (on the fused route through the pipeline), not the route of joint_rows
    best, idx = s.pose_level(through_pipeline=True)
    if s.rows == 0:
        jbest, jidx = s.no_joint_rows()
    elif s.why is None:
        jbest, jidx = s.pipe.aggregate_reproj(s.x, s.T, row_offset=s.lo)
    else:
        jbest, jidx = s.zh.joint_reproj(s.x, s.T.contiguous(), *s.detections[:2], s.N, s.lo)
    jbest, jidx = s.pl.reduce_min_over_ranks(jbest, jidx)
    pose, T_sel, px = s.score_assembled(jidx, idx)
    return _arrays(pose=pose, joint_hypothesis=jidx, joint_reproj_px=jbest, hypothesis=idx, T=T_sel, reproj_px=px, reproj_px_pose_level=best)


def _joints_tree(s):
    # --select joints with the skeleton as a coupling: min-sum over the bone tree (zedo_joint_tree_select, the confidences as weights)
    (best, idx), jidx0, full_jerr, full_T, bone = s.pose_level(), s.joint_rows[1], s.full_jerr, s.full_T, s.args.bone
    jidx, tcost, jbone = s.zh.joint_tree_select(full_jerr, s.full, full_T, s.parent, s.N, bone, s.detections[2])
    pose, T_sel, px = s.score_assembled(jidx, idx)
    return _arrays(pose=pose, joint_hypothesis=jidx, joint_hypothesis_per_joint=jidx0, joint_reproj_px=s.joint_px(jidx), joint_bone_m=jbone,
                   tree_cost=tcost, hypothesis=idx, T=T_sel, reproj_px=px, reproj_px_pose_level=best, bone=np.float64(bone))


def _joints_tree_fused(s):
    # the soft answer of the same skeleton model: sum-product over the bone tree (zedo_joint_tree_marginal) and, for comparison, its min-sum
    (best, idx), _, full_jerr, full_T, bone, tau = s.pose_level(), s.joint_rows, s.full_jerr, s.full_T, s.args.bone, s.args.temperature
    mean, cov, hmax, wmax, logz, ebone = s.zh.joint_tree_marginal(full_jerr, s.full, full_T, s.parent, s.N, bone, tau, s.detections[2])
    jtree, _, _ = s.zh.joint_tree_select(full_jerr, s.full, full_T, s.parent, s.N, bone, s.detections[2])
    pose, T_sel, spread = s.fused(mean, cov, idx)                             # in the frame --select joints-tree writes in
    return _arrays(pose=pose, joint_cov=cov, joint_spread_m=spread, joint_hypothesis=hmax, joint_weight=wmax, joint_logz=logz, joint_bone_m=ebone,
                   joint_hypothesis_tree=jtree, hypothesis=idx, T=T_sel, reproj_px_pose_level=best, bone=np.float64(bone), temperature=np.float64(tau))


def _temporal(s):
    # the frames are a video: Viterbi over every row's error and the motion between frames (zedo_temporal_select)
    seq, full_err, full_T, smooth = s.seq, s.full_err, s.full_T, s.args.smooth
    per_frame, idx0 = s.zh.pose_min(full_err, s.N)             # what --select reproj keeps
    path, cost = s.zh.temporal_select(full_err, s.full, seq, s.N, smooth)
    return _arrays(pose=s.take(s.full, path), hypothesis=path, hypothesis_per_frame=idx0, reproj_px=s.take(full_err, path),
                   reproj_px_all=full_err.reshape(s.H, s.N).t().contiguous(), path_cost=cost, T=s.take(full_T, path),
                   seq_start=seq.astype(np.int32), smooth=np.float64(smooth))


def _joints_temporal(s):
    # a video, assembled joint by joint: the pose-level Viterbi gives the frame the pose is written in, one chain per joint
    # (zedo_joint_temporal_select; with --accel the second-order zedo_joint_accel_select) the joints
    seq, jidx0, full_err, full_jerr, full_T, smooth = s.seq, s.joint_rows[1], s.full_err, s.full_jerr, s.full_T, s.args.smooth
    idx, _ = s.zh.temporal_select(full_err, s.full, seq, s.N, smooth)
    accel = getattr(s.args, "accel", None)
    if accel is None:
        jpath, jcost = s.zh.joint_temporal_select(full_jerr, s.full, full_T, seq, s.N, smooth)
    else:
        jpath, jcost = s.zh.joint_accel_select(full_jerr, s.full, full_T, seq, s.N, smooth, accel)
    pose, T_sel, px = s.score_assembled(jpath, idx)
    return _arrays(pose=pose, joint_hypothesis=jpath, joint_hypothesis_per_frame=jidx0, joint_reproj_px=s.joint_px(jpath), joint_path_cost=jcost,
                   hypothesis=idx, T=T_sel, reproj_px=px, reproj_px_pose_level=s.take(full_err, idx), seq_start=seq.astype(np.int32),
                   smooth=np.float64(smooth), **({} if accel is None else dict(accel=np.float64(accel))))


def _joints_fused(s):
    # the soft answer of the same chain model: J forward-backward passes (zedo_joint_marginal) and, for comparison, the J Viterbi chains
    seq, _, full_err, full_jerr, full_T, smooth, tau = s.seq, s.joint_rows, s.full_err, s.full_jerr, s.full_T, s.args.smooth, s.args.temperature
    idx, _ = s.zh.temporal_select(full_err, s.full, seq, s.N, smooth)
    mean, cov, hmax, wmax, logz = s.zh.joint_marginal(full_jerr, s.full, full_T, seq, s.N, smooth, tau)
    jpath, _ = s.zh.joint_temporal_select(full_jerr, s.full, full_T, seq, s.N, smooth)
    pose, T_sel, spread = s.fused(mean, cov, idx)                             # in the frame --select joints-temporal writes in
    return _arrays(pose=pose, joint_cov=cov, joint_spread_m=spread, joint_hypothesis=hmax, joint_weight=wmax, joint_logz=logz,
                   joint_hypothesis_viterbi=jpath, hypothesis=idx, T=T_sel, reproj_px_pose_level=s.take(full_err, idx),
                   seq_start=seq.astype(np.int32), smooth=np.float64(smooth), temperature=np.float64(tau))


def _lds_cap(name, H, J):
    cap = _hip().joint_tree_marginal_max_h(J)
    if H > cap:
        raise SystemExit(f"--select {name} admits at most {cap} hypotheses per pose at {J} joints (the model of a pose lives "
                         f"in the LDS of one workgroup), --hypo {H} given: use fewer hypotheses, or --select joints-tree")


class Mode(NamedTuple):
    name: str
    fn: object              # SelectInputs -> what <out>_selected.npz holds; None: nothing is selected
    help: str               # its sentence of the --select help
    switches: dict          # those of SWITCHES it takes -> default (None: none)
    label: str              # what --eval calls the selected pose
    prune: bool             # may --prune accompany it
    admits: object = None   # (name, H, J): SystemExit for a hypothesis count the mode cannot hold


VIDEO = dict(smooth=100.0, seq_len=None)
NONE = Mode("none", None, None, {}, None, True)
MODES = {m.name: m for m in (
    NONE,
    Mode("reproj", _reproj, "reproj = also keep, per pose, the hypothesis whose x + T reprojects closest to the 2D detections (confidence-weighted, "
         "no ground truth needed) -> <out>_selected.npz", {}, "reproj-selected", True),
    Mode("joints", _joints, "joints = keep, per JOINT, the hypothesis whose joint reprojects closest to its detection and assemble the pose from "
         "those joints", {}, "joints-aggregated", False),
    Mode("temporal", _temporal, "temporal = the frames are a video: per clip the hypothesis sequence that minimises reprojection error plus --smooth "
         "times the mean joint displacement between consecutive frames (Viterbi)", VIDEO, "temporal-selected", False),
    Mode("joints-temporal", _joints_temporal, "joints-temporal = both: per clip and per JOINT the hypothesis sequence that minimises that joint's "
         "reprojection distance plus --smooth times that joint's displacement in the camera frame (one Viterbi chain per joint), the pose assembled "
         "from those joints", dict(VIDEO, accel=None), "joints-temporal", False),
    Mode("joints-fused", _joints_fused, "joints-fused = the soft answer of the same chain model at --temperature: per joint the posterior mean "
         "position over the hypotheses, its covariance (the depth ambiguity in metres) and the most probable hypothesis with its probability",
         dict(VIDEO, temperature=1.0), "joints-fused", False),
    Mode("joints-tree", _joints_tree, "joints-tree = joints with the skeleton as a coupling: per pose the assignment of a hypothesis to every joint "
         "that minimises the joints' confidence-weighted reprojection distances plus --bone times, for every bone, the difference between the "
         "assembled bone's length and the length its two hypotheses give that bone (exact min-sum over the bone tree)", dict(bone=100.0),
         "joints-tree", False),
    Mode("joints-tree-fused", _joints_tree_fused, "joints-tree-fused = the soft answer of the same skeleton model at --temperature, from one image: "
         "per joint the posterior mean position over the hypotheses, its covariance, the most probable hypothesis with its probability and every "
         "bone's expected mismatch (exact sum-product over the bone tree)", dict(bone=100.0, temperature=1.0), "joints-tree-fused", False, _lds_cap))}
SELECT_HELP = "run.inference only: " + "; ".join(m.help for m in MODES.values() if m.help)

_weight = (lambda v: np.isfinite(v) and v >= 0, "a finite weight >= 0 expected")
# in the order they are checked: switch, the words it is refused with beside a mode that does not take it, (is the value valid, if not)
SWITCHES = (("bone", "--bone is a switch of --select joints-tree", _weight),
            ("accel", "--accel is a switch of --select joints-temporal", _weight),
            ("temperature", "--temperature is a switch of --select joints-fused", (lambda v: np.isfinite(v) and v > 0, "a finite temperature > 0 expected")),
            ("smooth", "--smooth and --seq_len are switches of --select temporal and --select joints-temporal", _weight),
            ("seq_len", "--smooth and --seq_len are switches of --select temporal and --select joints-temporal", (lambda v: v >= 1, "at least one frame per clip")))


def mode_of(args):
    return MODES[getattr(args, "select", None) or NONE.name]


def check_select_args(args):
    """Every switch of SWITCHES belongs to the modes whose table entry names it: beside another mode it is refused, without a value it
    takes the entry's default (if any), with one the value is checked."""
    takes = mode_of(args).switches
    for name, refusal, (valid, complaint) in SWITCHES:
        v = getattr(args, name, None)
        if name not in takes:
            if v is not None:
                raise SystemExit(refusal)
        elif v is None:
            if takes[name] is not None:
                setattr(args, name, takes[name])
        elif not valid(v):
            raise SystemExit(f"--{name} {v}: {complaint}")


def prune_refusal(select):
    """The words --prune is refused with beside --select `select`; None where the table admits the pair."""
    return None if MODES[select].prune else (f"--prune with --select {select} is not supported yet (a follow-up): the pruned run keeps "
                                             "different hypotheses per pose; use --select reproj or none")
