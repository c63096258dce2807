"""Device-resident ZeDO pipeline: the loop of reference run/opt_main.py:166-224 with all H hypotheses
batched as rows (h, n) and every stage running in libzedo_hip.so.

    ISO  x0[h]   = cluster_h - cluster_h[0]                      (opt_main.py:167-168,173)
    IPO  (R, T)  = zedo_ipo_fit                                   (opt_main.py:177-195)
         x       = R x0                                           (opt_main.py:201)
    OIL  S steps of {reprojection correction, score-network probability-flow step}   (opt_main.py:202-220)
    selection    = per-pose min over hypotheses of (PA-)MPJPE     (eval_multi)
                   or, without ground truth, of the confidence-weighted reprojection error of x + T (select_reproj),
                   or per JOINT of the joint's reprojection distance, the pose assembled from the winners (aggregate_reproj, compose),
                   or along the clips of a video: reprojection error plus a motion cost, by Viterbi (select_temporal),
                   or both: per joint along the clips, one Viterbi chain per joint (select_joints_temporal, compose),
                   or on a live video, fixed-lag: the joints' chains in the frame of the pose-level chain (open_live_joints)
    pruning      = opt-in, DURING the loop: at the steps of a plan keep, per pose, the K hypotheses with the smallest reprojection
                   error and carry on with K x N rows (parse_prune_plan, run_pruned)

Rows may be a contiguous shard of the H*N global rows (one shard per GPU); the only exchange is the final
MIN over ranks, done by the caller (run/opt_main.py, bench.py) with torch.distributed.
"""
import os

import numpy as np
import torch

from . import (H36M_EDGES, SINGULAR_MSG, JointAccelMarginalStream, JointAccelStream, JointMarginalStream, JointStream, Schedule, TemporalStream, Weights, ZedoError, ipo_fit, joint_accel_marginal, joint_accel_select, joint_compose, joint_marginal, joint_reproj,
               joint_temporal_select, joint_tree_marginal, joint_tree_select, skeleton_parents, min_mpjpe_both, min_reproj, oil_run, prune_gather, prune_rank, reproj_degenerate, reproj_prepare, rotate_init, temporal_marginal, temporal_select)


def linspace_f32(start, end, steps):
    """torch.linspace(start, end, steps) in fp32 without touching a device (opt_main.py:198)."""
    return torch.linspace(float(start), float(end), int(steps), dtype=torch.float32).numpy()


def parse_prune_plan(text, H, S):
    """"100:10" or "0:25,200:5" -> [(step, keep), ...]: before OIL step `step` the loop keeps, per pose, the `keep` hypotheses with the
    smallest reprojection error.  Steps strictly ascending in [0, S) (0: after IPO and the initial rotate), keeps strictly descending
    with 1 <= keep <= H; anything else is a ValueError that names the offending item."""
    H, S = int(H), int(S)
    items = [t.strip() for t in str(text).split(",")]
    plan = []
    for item in items:
        parts = item.split(":")
        if len(parts) != 2 or not all(q.strip().isdigit() for q in parts):
            raise ValueError(f"prune plan {text!r}: item {item!r} is not STEP:KEEP (two non-negative integers)")
        step, keep = int(parts[0]), int(parts[1])
        if step >= S:
            raise ValueError(f"prune plan {text!r}: item {item!r}: step {step} is outside the loop's steps 0 .. {S - 1}")
        if not 1 <= keep <= H:
            raise ValueError(f"prune plan {text!r}: item {item!r}: keep {keep} is outside 1 .. {H} hypotheses")
        if plan and step <= plan[-1][0]:
            raise ValueError(f"prune plan {text!r}: item {item!r}: step {step} does not come after step {plan[-1][0]}")
        if plan and keep >= plan[-1][1]:
            raise ValueError(f"prune plan {text!r}: item {item!r}: keep {keep} is not below the {plan[-1][1]} already kept")
        plan.append((step, keep))
    return plan


def prune_row_steps(plan, H, S):
    """(hypothesis-steps per pose that the loop runs under `plan`, the H * S of the unpruned loop)."""
    done, begin, cur = 0, 0, int(H)
    for step, keep in plan:
        done += cur * (step - begin)
        begin, cur = step, keep
    return done + cur * (int(S) - begin), int(H) * int(S)


class ZeDOConfig:
    """The values of configs/optim/concat_pose_optimization_*.py that the path reads."""

    def __init__(self, IPO_iterations=500, IPO_keylist=(0, 1, 4), RotAxes="z", IPO_T=3.0, IPO_minScaleT=0.5,
                 IPO_maxScaleT=2.0, OIL_iterations=1000, sampling_eps=0.01, sde_T=0.1, num_scales=1000,
                 beta_min=0.1, beta_max=20.0):
        self.IPO_iterations, self.IPO_keylist, self.RotAxes = int(IPO_iterations), list(IPO_keylist), RotAxes
        self.IPO_T, self.IPO_minScaleT, self.IPO_maxScaleT = float(IPO_T), float(IPO_minScaleT), float(IPO_maxScaleT)
        self.OIL_iterations, self.sampling_eps, self.sde_T = int(OIL_iterations), float(sampling_eps), float(sde_T)
        self.num_scales, self.beta_min, self.beta_max = int(num_scales), float(beta_min), float(beta_max)

    @classmethod
    def h36m(cls, **kw):
        return cls(**kw)

    @classmethod
    def pw3d(cls, **kw):
        d = dict(IPO_keylist=tuple(range(17)), IPO_T=8.0, IPO_minScaleT=0.2)
        d.update(kw)
        return cls(**d)


class Pipeline:
    def __init__(self, state_dict, cfg, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.weights = state_dict if isinstance(state_dict, Weights) else Weights(state_dict)
            ts = linspace_f32(cfg.sde_T, cfg.sampling_eps, cfg.OIL_iterations)
            self.sched = Schedule(self.weights, ts, cfg.beta_min, cfg.beta_max, cfg.num_scales)

    def _dev(self, a, dtype=torch.float32):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=self.device)

    def load(self, sample_poses, db_2d, camera_param):
        """Upload one problem: clusters [H,17,3], detections [N,17,3]=(u,v,conf), intrinsics [N,3,3]."""
        sp = self._dev(sample_poses)
        self.x0 = (sp - sp[:, 0:1, :]).contiguous()             # ISO initial poses, centred on joint 0
        d2 = self._dev(db_2d)
        self.uv = d2[:, :, :2].contiguous()
        self.conf = d2[:, :, 2].contiguous()
        self.K = self._dev(camera_param)
        self.H, self.N = self.x0.shape[0], self.uv.shape[0]
        with torch.cuda.device(self.device):
            # the reference clamps conf in place inside gradient_field_gen; keep that observable
            self.geom = reproj_prepare(self.uv, self.K, self.conf, self.conf)
            self.singular_poses = reproj_degenerate(self.geom)     # once per problem (the rays do not change)
        return self

    def run(self, row_offset=0, rows=None, oil_steps=None):
        """IPO + OIL for global rows [row_offset, row_offset+rows) -> (x [rows,17,3], T [rows,3]) on device."""
        c = self.cfg
        row_offset = int(row_offset)
        B = self.H * self.N - row_offset if rows is None else int(rows)
        S = c.OIL_iterations if oil_steps is None else int(oil_steps)
        if row_offset < 0 or B < 0 or row_offset + B > self.H * self.N:
            raise ValueError(f"rows [{row_offset}, {row_offset + B}) are outside the {self.H} x {self.N} problem")
        if B == 0:          # more ranks than rows: this rank holds an empty shard
            return (torch.empty((0, self.x0.shape[1], 3), dtype=torch.float32, device=self.device),
                    torch.empty((0, 3), dtype=torch.float32, device=self.device))
        with torch.cuda.device(self.device):
            if S > c.OIL_iterations // 5 and self.singular_poses:     # the loop reaches the least-squares T
                raise ZedoError(SINGULAR_MSG.format(n=self.singular_poses))
            R, T = ipo_fit(self.x0, self.uv, self.K, c.IPO_keylist, c.RotAxes, c.IPO_T, c.IPO_minScaleT,
                           c.IPO_maxScaleT, c.IPO_iterations, self.N * len(c.IPO_keylist) * 2, B, row_offset)
            x = rotate_init(self.x0, R, self.N, row_offset)
            oil_run(self.weights, self.sched, x, self.geom, T, 0, S, c.OIL_iterations // 5, row_offset)
        return x, T

    def run_pruned(self, plan, oil_steps=None):
        """IPO + OIL with hypotheses pruned during the loop -> (x [K*N,17,3], T [K*N,3], hyp [K,N] i32), K the last stage's keep.
        plan: the text of parse_prune_plan or its [(step, keep), ...].  IPO and the rotate run on all H*N rows; for every stage the loop
        runs up to the stage's step, zedo_min_reproj scores the current rows against the problem's detections (the current slot count in
        the role of H), zedo_prune_rank keeps the best `keep` slots per pose and zedo_prune_gather compacts x, T and the ids; the last
        segment runs to the end.  Row (r, n) of the result is hypothesis hyp[r, n] of pose n, ascending in r.  The switch to the
        least-squares T stays at OIL_iterations // 5.  No row_offset: a pose's every hypothesis must be on this device.  A row's bits do
        not depend on the batch it is in, so every surviving row is run()'s row.  Whether pruning by reprojection error costs accuracy
        is not measured."""
        c = self.cfg
        S = c.OIL_iterations if oil_steps is None else int(oil_steps)
        if not isinstance(plan, str):              # a list goes through the same checks as the text
            plan = ",".join(f"{int(s)}:{int(k)}" for s, k in plan)
        plan = parse_prune_plan(plan, self.H, S) if plan else []
        switch = c.OIL_iterations // 5
        with torch.cuda.device(self.device):
            if S > switch and self.singular_poses:     # the loop reaches the least-squares T
                raise ZedoError(SINGULAR_MSG.format(n=self.singular_poses))
            B = self.H * self.N
            R, T = ipo_fit(self.x0, self.uv, self.K, c.IPO_keylist, c.RotAxes, c.IPO_T, c.IPO_minScaleT,
                           c.IPO_maxScaleT, c.IPO_iterations, self.N * len(c.IPO_keylist) * 2, B, 0)
            x = rotate_init(self.x0, R, self.N, 0)
            hyp, begin = None, 0
            for step, keep in plan:
                if step > begin:
                    oil_run(self.weights, self.sched, x, self.geom, T, begin, step, switch, 0)
                err, _, _ = min_reproj(x, T, self.uv, self.K, self.conf, self.N, 0)
                x, T, hyp = prune_gather(prune_rank(err, self.N, keep), x, T, hyp)
                begin = step
            if S > begin:
                oil_run(self.weights, self.sched, x, self.geom, T, begin, S, switch, 0)
            if hyp is None:
                hyp = torch.arange(self.H, dtype=torch.int32, device=self.device)[:, None].expand(self.H, self.N).contiguous()
        return x, T, hyp

    def select(self, x, gt_centred, row_offset=0):
        """-> dict(p1=(best[N], idx[N]), p2=(best[N], idx[N])) for the local rows (fp64 / int32 tensors)."""
        gt = self._dev(gt_centred, torch.float64)
        if x.shape[0] == 0:
            return {k: empty_selection(self.N, self.device) for k in ("p1", "p2")}
        with torch.cuda.device(self.device):
            _, best, idx = min_mpjpe_both(x, gt, self.N, row_offset)     # one pass over the rows: the bits of the two min_mpjpe calls
        return dict(p1=(best[0], idx[0]), p2=(best[1], idx[1]))

    def select_reproj(self, x, T, row_offset=0):
        """Selection without ground truth on the problem of load(): -> (best [N] f64, idx [N] i32) for the local rows x [B,17,3] with
        their final translations T [B,3] - per pose the smallest confidence-weighted reprojection error (pixels) of x + T against the
        detections and the hypothesis that attains it (zedo_min_reproj).  Ranks are combined with reduce_min_over_ranks."""
        if x.shape[0] == 0:
            return empty_selection(self.N, self.device)
        with torch.cuda.device(self.device):
            _, best, idx = min_reproj(x, T, self.uv, self.K, self.conf, self.N, row_offset)
        return best, idx

    def aggregate_reproj(self, x, T, row_offset=0):
        """Joint-wise aggregation without ground truth on the problem of load(): -> (best [N,J] f64, idx [N,J] i32) for the local rows -
        per (pose, joint) the smallest reprojection distance (pixels) of that joint of x + T and the hypothesis that attains it
        (zedo_joint_reproj, the walking kernel).  Ranks are combined with reduce_min_over_ranks (element-wise)."""
        J = self.uv.shape[1]
        if x.shape[0] == 0:
            best, idx = empty_selection(self.N * J, self.device)
            return best.reshape(self.N, J), idx.reshape(self.N, J)
        with torch.cuda.device(self.device):
            return joint_reproj(x, T, self.uv, self.K, self.N, row_offset)

    def _joint_unaries(self, name, x, T, streams=None):
        """What the joint-wise methods below start with: x holds all H*N rows (streams: of a whole number of frames of that many live
        streams) - the ValueError speaks for the method `name` - and jerr [H*N,17] f64, zedo_joint_reproj's per-(row, joint) distances
        on the problem of load(), formed on the pipeline's device."""
        if x.shape[0] != self.H * self.N or (streams is not None and self.N % streams):
            if streams is None:
                raise ValueError(f"{name}: all {self.H * self.N} rows expected, got {x.shape[0]}")
            raise ValueError(f"{name}: all {self.H * self.N} rows of a whole number of frames of {streams} streams expected, "
                             f"got {x.shape[0]} rows for {self.N} poses")
        with torch.cuda.device(self.device):
            return joint_reproj(x, T, self.uv, self.K, self.N, 0, return_rows=True)[2]

    def _open_stream(self, name, cls, S, lag, max_frames, *weights):
        """What the open_*_stream methods below share: a `cls` with H and the joint count of load() - the ZedoError speaks for `name`."""
        if getattr(self, "uv", None) is None:
            raise ZedoError(f"{name}: call load() first (the joint count is the problem's)")
        return cls(S, self.H, self.uv.shape[1], lag, max_frames, *weights, self.device)

    def _push_stream(self, name, js, x, T, flush):
        """What the push_* methods below share: the unaries of _joint_unaries for the streams of js, pushed -> js.push(...) + (jerr,)."""
        jerr = self._joint_unaries(name, x, T, js.S)
        with torch.cuda.device(self.device):
            return js.push(jerr, x, T, flush) + (jerr,)

    def aggregate_tree(self, x, T, mu=100.0, parent=None):
        """aggregate_reproj with the skeleton as a coupling, on the problem of load(): x [H*N,17,3] and T [H*N,3], ALL rows (a pose's every
        hypothesis takes part) -> (joint_h [N,17] i32, cost [N] f64, bone [N,17] f64, jerr [H*N,17] f64): the unaries are
        zedo_joint_reproj's per-(row, joint) distances (pixels) weighted by the pipeline's confidences; the assignment minimises them plus
        mu (pixels per metre, default untuned) times every bone's mismatch between its assembled length and the length its two hypotheses
        give it (zedo_joint_tree_select, exact min-sum over the tree).  parent [17]: the bone tree, default H36M's.
        compose(x, T, joint_h, ref) assembles the pose."""
        jerr = self._joint_unaries("aggregate_tree", x, T)
        if parent is None:
            parent = skeleton_parents(H36M_EDGES, self.uv.shape[1])
        with torch.cuda.device(self.device):
            return joint_tree_select(jerr, x, T, parent, self.N, mu, self.conf) + (jerr,)

    def fuse_tree(self, x, T, mu=100.0, tau=1.0, parent=None):
        """The soft answer of aggregate_tree, on the problem of load(): x [H*N,17,3] and T [H*N,3], ALL rows -> (mean [N,17,3] f64, cov
        [N,17,6] f64, hmax [N,17] i32, wmax [N,17] f64, logz [N,17] f64, bone [N,17] f64, jerr [H*N,17] f64): the unaries and the weights
        are aggregate_tree's - zedo_joint_reproj's per-(row, joint) distances (pixels) and the pipeline's confidences - and the outputs
        the exact posterior marginals of the same energy at the temperature tau (pixels), read as a fused position, its covariance, the
        most probable hypothesis, its probability, the component's log-partition value and every bone's expected mismatch
        (zedo_joint_tree_marginal, sum-product over the tree).  mu and tau: defaults untuned.  parent [17]: the bone tree, default H36M's."""
        jerr = self._joint_unaries("fuse_tree", x, T)
        if parent is None:
            parent = skeleton_parents(H36M_EDGES, self.uv.shape[1])
        with torch.cuda.device(self.device):
            return joint_tree_marginal(jerr, x, T, parent, self.N, mu, tau, self.conf) + (jerr,)

    def compose(self, x_full, T_full, joint_idx, ref_idx=None):
        """The pose assembled from the joints aggregate_reproj selected: x_full [H*N,17,3], T_full [H*N,3] (all global rows), joint_idx
        [N,17] -> [N,17,3], root-relative to hypothesis ref_idx[n] (None: camera frame) (zedo_joint_compose)."""
        if x_full.shape[0] != self.H * self.N:
            raise ValueError(f"compose: all {self.H * self.N} rows expected, got {x_full.shape[0]}")
        with torch.cuda.device(self.device):
            return joint_compose(x_full, T_full, joint_idx, ref_idx, self.N)

    def select_temporal(self, x, T, seq_start, lam=100.0):
        """Selection along a video without ground truth on the problem of load(): x [H*N,17,3] and T [H*N,3], ALL rows (the recurrence
        needs every hypothesis of consecutive frames), seq_start = the first frame of every clip and N -> (path [N] i32, cost [N] f64,
        err_rows [H*N] f64): the unaries are zedo_min_reproj's per-row errors (pixels), the path minimises them plus lam (pixels per
        metre, default untuned) times the mean joint displacement between consecutive choices (zedo_temporal_select).  take(x, path)
        gathers the rows."""
        if x.shape[0] != self.H * self.N:
            raise ValueError(f"select_temporal: all {self.H * self.N} rows expected, got {x.shape[0]}")
        with torch.cuda.device(self.device):
            err, _, _ = min_reproj(x, T, self.uv, self.K, self.conf, self.N, 0)
            path, cost = temporal_select(err, x, seq_start, self.N, lam)
        return path, cost, err

    def select_joints_temporal(self, x, T, seq_start, lam=100.0):
        """Joint-wise selection along a video without ground truth on the problem of load(): x [H*N,17,3] and T [H*N,3], ALL rows,
        seq_start = the first frame of every clip and N -> (joint_path [N,17] i32, joint_cost [N,17] f64, jerr [H*N,17] f64): the unaries
        are zedo_joint_reproj's per-(row, joint) distances (pixels), each joint's path minimises them plus lam (pixels per metre, default
        untuned) times that joint's displacement in the camera frame between consecutive choices (zedo_joint_temporal_select).
        compose(x, T, joint_path, ref) assembles the pose."""
        jerr = self._joint_unaries("select_joints_temporal", x, T)
        with torch.cuda.device(self.device):
            return joint_temporal_select(jerr, x, T, seq_start, self.N, lam) + (jerr,)

    def open_joint_stream(self, S, lag, max_frames, lam=100.0):
        """The state of select_joints_temporal's chain for S live streams (JointStream): H and the joint count are those of the
        pipeline, every frame is decided `lag` frames after it went in, a push holds at most max_frames frames per stream.  lam and the
        choice of lag are untuned."""
        return self._open_stream("open_joint_stream", JointStream, S, lag, max_frames, lam)

    def push_joints_temporal(self, js, x, T, flush=None):
        """select_joints_temporal on live input, on the problem of load() with N = S F poses - F new frames of each of the S streams of
        js = open_joint_stream(...), pose n = s F + f: x [H*N,17,3] and T [H*N,3], ALL rows; flush: None, or [S] flags - the streams
        whose clip ends here.  -> (first [S] i64, count [S] i64, joint_path [S,F+lag,17] i32, joint_cost [S,F+lag,17] f64, jerr
        [H*N,17] f64): the unaries are zedo_joint_reproj's per-(row, joint) distances exactly as select_joints_temporal forms them; stream
        s emits the frames first[s] .. first[s] + count[s] - 1 of its clip (zedo_joint_stream_push).  The caller keeps x and T of the
        frames that are still to come out and assembles their poses with compose."""
        return self._push_stream("push_joints_temporal", js, x, T, flush)

    def open_pose_stream(self, S, lag, max_frames, lam=100.0):
        """The state of select_temporal's chain for S live streams (TemporalStream): H and the joint count are those of the pipeline,
        every frame is decided `lag` frames after it went in, a push holds at most max_frames frames per stream.  lam and the choice of
        lag are untuned."""
        return self._open_stream("open_pose_stream", TemporalStream, S, lag, max_frames, lam)

    def push_temporal(self, ps, x, T, flush=None):
        """select_temporal on live input, on the problem of load() with N = S F poses - F new frames of each of the S streams of
        ps = open_pose_stream(...), pose n = s F + f: x [H*N,17,3] and T [H*N,3], ALL rows; flush: None, or [S] flags - the streams
        whose clip ends here.  -> (first [S] i64, count [S] i64, path [S,F+lag] i32, cost [S,F+lag] f64, err [H*N] f64): the unaries
        are zedo_min_reproj's per-row errors exactly as select_temporal forms them; stream s emits the frames first[s] .. first[s] +
        count[s] - 1 of its clip (zedo_temporal_stream_push)."""
        if x.shape[0] != self.H * self.N or self.N % ps.S:
            raise ValueError(f"push_temporal: all {self.H * self.N} rows of a whole number of frames of {ps.S} streams expected, "
                             f"got {x.shape[0]} rows for {self.N} poses")
        with torch.cuda.device(self.device):
            err, _, _ = min_reproj(x, T, self.uv, self.K, self.conf, self.N, 0)
            return ps.push(err, x, flush) + (err,)

    def open_live_joints(self, S, lag, max_frames, lam=100.0):
        """What a camera needs of --select joints-temporal, for S live streams (LiveJoints): the joints' chains (open_joint_stream) and
        the pose-level chain whose frame their poses are written in (open_pose_stream), at the same S, lag, max_frames and lam, and x
        and T of the up to `lag` frames per stream that have not come out yet.  lam and the choice of lag are untuned."""
        return LiveJoints(self.open_joint_stream(S, lag, max_frames, lam), self.open_pose_stream(S, lag, max_frames, lam))

    def push_live_joints(self, lj, x, T, flush=None):
        """select_joints_temporal and select_temporal on live input, assembled: the problem of load() holds N = S F poses - F new
        frames of each of the S streams of lj = open_live_joints(...), pose n = s F + f; x [H*N,17,3] and T [H*N,3], ALL rows; flush:
        None, or [S] flags (a sequence; a tensor is read back) - the streams whose clip ends here.  -> (first [S] i64, count [S] i64,
        pose [S,F+lag,17,3] f32, joint_path [S,F+lag,17] i32, path [S,F+lag] i32, T_sel [S,F+lag,3] f32): stream s emits the frames
        first[s] .. first[s] + count[s] - 1 of its clip in the rows 0 .. count[s] - 1; pose is zedo_joint_compose of the frame with
        the joint stream's decisions in the frame of the pose stream's decision `path`, T_sel that hypothesis's translation.  Rows at
        and after count[s] are NaN in pose and T_sel and -1 in joint_path and path.  With lag >= the clip's length - 1 and a flush, pose
        is bit for bit the pose --select joints-temporal writes for the clip.  The frame counts are kept on the host from the header's
        formula: d_emit is not read back."""
        js, ps = lj.joints, lj.pose
        S, H, lag = js.S, js.H, js.lag
        J = x.shape[1]
        jerr = self._joint_unaries("push_live_joints", x, T, S)
        F = self.N // S
        if flush is None:
            fl = [0] * S
        else:
            fl = [1 if v else 0 for v in (flush.tolist() if isinstance(flush, torch.Tensor) else flush)]
            if len(fl) != S:
                raise ValueError(f"push_live_joints: one flag per stream ([{S}]) expected, got {len(fl)}")
        with torch.cuda.device(self.device):
            err, _, _ = min_reproj(x, T, self.uv, self.K, self.conf, self.N, 0)
            first, count, jp, _ = js.push(jerr, x, T, flush)
            _, _, pp, _ = ps.push(err, x, flush)
            rows = F + lag
            # the window of a stream: the lag frames before the chunk (those the clip does not hold yet: never read), then the chunk
            win_x = torch.cat([lj.pend_x, x.reshape(H, S, F, J, 3)], 2)
            win_T = torch.cat([lj.pend_T, T.reshape(H, S, F, 3)], 2)
            held = [min(lag, t) + F for t in lj.t]
            cnt = [h if f else max(0, h - lag) for h, f in zip(held, fl)]
            # output row r of stream s is the clip's frame max(0, t - lag) + r: slot lag - min(lag, t) + r of the window
            slot = np.minimum(np.array([lag - min(lag, t) for t in lj.t])[:, None] + np.arange(rows)[None, :], rows - 1)
            valid = torch.as_tensor(np.arange(rows)[None, :] < np.array(cnt)[:, None], device=self.device)
            slot = torch.as_tensor(slot, device=self.device)
            s_ix = torch.arange(S, device=self.device)[:, None]
            gx, gT = win_x[:, s_ix, slot].contiguous(), win_T[:, s_ix, slot].contiguous()      # [H,S,rows,J,3], [H,S,rows,3]
            jidx = torch.where(valid[:, :, None], jp, torch.zeros_like(jp)).reshape(S * rows, J)
            ref = torch.where(valid, pp, torch.zeros_like(pp)).reshape(S * rows)
            pose = joint_compose(gx.view(H * S * rows, J, 3), gT.view(H * S * rows, 3), jidx, ref, S * rows, check=False)
            nan, minus = pose.new_tensor(float("nan")), pp.new_tensor(-1)
            pose = torch.where(valid[:, :, None, None], pose.view(S, rows, J, 3), nan)
            T_sel = torch.gather(gT, 0, ref.view(1, S, rows, 1).expand(1, S, rows, 3).to(torch.int64))[0]
            out = (first, count, pose, torch.where(valid[:, :, None], jp, minus), torch.where(valid, pp, minus),
                   torch.where(valid[:, :, None], T_sel, nan))
            lj.pend_x, lj.pend_T = win_x[:, :, F:].contiguous(), win_T[:, :, F:].contiguous()
            lj.t = [0 if f else t + F for t, f in zip(lj.t, fl)]
        return out

    def select_joints_accel(self, x, T, seq_start, lam=100.0, accel=100.0):
        """select_joints_temporal with a second-order motion model: the same inputs and outputs, each joint's path minimises its unaries
        plus lam times its displacement plus accel (pixels per metre, default untuned) times its second difference X[n] - 2 X[n-1] +
        X[n-2] in the camera frame, which is blind to a constant velocity (zedo_joint_accel_select; at most 64 hypotheses).  joint_cost
        is the cost of the kept path re-accumulated along it."""
        jerr = self._joint_unaries("select_joints_accel", x, T)
        with torch.cuda.device(self.device):
            return joint_accel_select(jerr, x, T, seq_start, self.N, lam, accel) + (jerr,)

    def open_joint_accel_stream(self, S, lag, max_frames, lam=100.0, accel=100.0):
        """The state of select_joints_accel's chain over pairs for S live streams (JointAccelStream): H (at most 64) and the joint count
        are those of the pipeline, every frame is decided `lag` frames after it went in, a push holds at most max_frames frames per
        stream.  lam, accel and the choice of lag are untuned."""
        return self._open_stream("open_joint_accel_stream", JointAccelStream, S, lag, max_frames, lam, accel)

    def push_joints_accel(self, js, x, T, flush=None):
        """select_joints_accel on live input, on the problem of load() with N = S F poses - F new frames of each of the S streams of
        js = open_joint_accel_stream(...), pose n = s F + f: x [H*N,17,3] and T [H*N,3], ALL rows; flush: None, or [S] flags - the
        streams whose clip ends here.  -> (first [S] i64, count [S] i64, joint_path [S,F+lag,17] i32, joint_cost [S,F+lag,17] f64, jerr
        [H*N,17] f64): the unaries are zedo_joint_reproj's per-(row, joint) distances exactly as push_joints_temporal forms them; stream
        s emits the frames first[s] .. first[s] + count[s] - 1 of its clip, each as select_joints_accel decides it on the clip cut `lag`
        frames later (zedo_joint_accel_stream_push); joint_cost is the cost of the best path on that cut clip."""
        return self._push_stream("push_joints_accel", js, x, T, flush)

    def fuse_joints_temporal(self, x, T, seq_start, lam=100.0, tau=1.0):
        """Joint-wise fusion along a video without ground truth on the problem of load(): x [H*N,17,3] and T [H*N,3], ALL rows, seq_start =
        the first frame of every clip and N -> (mean [N,17,3] f64, cov [N,17,6] f64, hmax [N,17] i32, wmax [N,17] f64, logz [N,17] f64,
        jerr [H*N,17] f64): the unaries are zedo_joint_reproj's per-(row, joint) distances (pixels); the posterior mean position of every
        joint in the camera frame, its covariance, the most probable hypothesis and its probability under the chain model
        select_joints_temporal optimises, at the temperature tau in pixels (zedo_joint_marginal; lam and tau untuned)."""
        jerr = self._joint_unaries("fuse_joints_temporal", x, T)
        with torch.cuda.device(self.device):
            return joint_marginal(jerr, x, T, seq_start, self.N, lam, tau) + (jerr,)

    def fuse_temporal(self, x, T, seq_start, lam=100.0, tau=1.0):
        """Pose-level fusion along a video without ground truth on the problem of load(): x [H*N,17,3] and T [H*N,3], ALL rows, seq_start
        = the first frame of every clip and N -> (mean [N,17,3] f64, cov [N,17,6] f64, hmax [N] i32, wmax [N] f64, logz [N] f64, err_rows
        [H*N] f64): the unaries are zedo_min_reproj's per-row errors (pixels), exactly as select_temporal forms them; the posterior mean
        pose in the camera frame (x + T), every joint's covariance, the most probable hypothesis of every frame and its probability
        under the chain model select_temporal optimises, at the temperature tau in pixels (zedo_temporal_marginal; lam and tau untuned;
        whether the fused pose is closer to ground truth than the selected one is not measured)."""
        if x.shape[0] != self.H * self.N:
            raise ValueError(f"fuse_temporal: all {self.H * self.N} rows expected, got {x.shape[0]}")
        with torch.cuda.device(self.device):
            err, _, _ = min_reproj(x, T, self.uv, self.K, self.conf, self.N, 0)
            return temporal_marginal(err, x, T, seq_start, self.N, lam, tau) + (err,)

    def open_joint_fuse_stream(self, S, lag, max_frames, lam=100.0, tau=1.0):
        """The state of fuse_joints_temporal's chain model for S live streams (JointMarginalStream): H and the joint count are those of
        the pipeline, every frame's marginals are formed `lag` frames after it went in, a push holds at most max_frames frames per
        stream.  lam, tau and the choice of lag are untuned."""
        return self._open_stream("open_joint_fuse_stream", JointMarginalStream, S, lag, max_frames, lam, tau)

    def push_fuse_joints_temporal(self, js, x, T, flush=None):
        """fuse_joints_temporal on live input, on the problem of load() with N = S F poses - F new frames of each of the S streams of
        js = open_joint_fuse_stream(...), pose n = s F + f: x [H*N,17,3] and T [H*N,3], ALL rows; flush: None, or [S] flags - the streams
        whose clip ends here.  -> (first [S] i64, count [S] i64, mean [S,F+lag,17,3] f64, cov [S,F+lag,17,6] f64, hmax [S,F+lag,17] i32,
        wmax [S,F+lag,17] f64, logz [S,F+lag,17] f64, jerr [H*N,17] f64): the unaries are zedo_joint_reproj's per-(row, joint) distances
        exactly as push_joints_temporal forms them; stream s emits the frames first[s] .. first[s] + count[s] - 1 of its clip, each as
        fuse_joints_temporal reports it on the clip cut `lag` frames later (zedo_joint_stream_marginal_push)."""
        return self._push_stream("push_fuse_joints_temporal", js, x, T, flush)

    def fuse_joints_accel(self, x, T, seq_start, lam=100.0, accel=100.0, tau=1.0):
        """fuse_joints_temporal under the second-order motion model: the same inputs and outputs - (mean [N,17,3] f64, cov [N,17,6] f64,
        hmax [N,17] i32, wmax [N,17] f64, logz [N,17] f64, jerr [H*N,17] f64) - the posterior mean position of every joint in the camera
        frame, its covariance, the most probable hypothesis and its probability under the chain over pairs of hypotheses
        select_joints_accel optimises: lam times the displacement plus accel times the second difference X[n] - 2 X[n-1] + X[n-2], which is
        blind to a constant velocity, at the temperature tau in pixels (zedo_joint_accel_marginal; at most 64 hypotheses; lam, accel and
        tau untuned)."""
        jerr = self._joint_unaries("fuse_joints_accel", x, T)
        with torch.cuda.device(self.device):
            return joint_accel_marginal(jerr, x, T, seq_start, self.N, lam, accel, tau) + (jerr,)

    def open_joint_accel_fuse_stream(self, S, lag, max_frames, lam=100.0, accel=100.0, tau=1.0):
        """The state of fuse_joints_accel's chain over pairs for S live streams (JointAccelMarginalStream): H (at most 64) and the joint
        count are those of the pipeline, every frame's marginals are formed `lag` frames after it went in, a push holds at most
        max_frames frames per stream.  lam, accel, tau and the lag are untuned; accuracy on real video is unmeasured."""
        return self._open_stream("open_joint_accel_fuse_stream", JointAccelMarginalStream, S, lag, max_frames, lam, accel, tau)

    def push_fuse_joints_accel(self, js, x, T, flush=None):
        """fuse_joints_accel on live input, on the problem of load() with N = S F poses - F new frames of each of the S streams of
        js = open_joint_accel_fuse_stream(...), pose n = s F + f: x [H*N,17,3] and T [H*N,3], ALL rows; flush: None, or [S] flags - the
        streams whose clip ends here.  -> (first [S] i64, count [S] i64, mean [S,F+lag,17,3] f64, cov [S,F+lag,17,6] f64, hmax
        [S,F+lag,17] i32, wmax [S,F+lag,17] f64, logz [S,F+lag,17] f64, jerr [H*N,17] f64): the unaries are zedo_joint_reproj's
        per-(row, joint) distances exactly as push_joints_temporal forms them; stream s emits the frames first[s] .. first[s] + count[s]
        - 1 of its clip, each as fuse_joints_accel reports it on the clip cut `lag` frames later
        (zedo_joint_accel_stream_marginal_push).  lam, accel, tau and the lag are untuned; accuracy on real video is unmeasured."""
        return self._push_stream("push_fuse_joints_accel", js, x, T, flush)

    def take(self, rows_full, idx):
        """The winning row of every pose: rows_full [H*N, ...] (all global rows, h-major), idx [N] -> rows_full.view(H, N, ...)[idx, arange(N)].
        An index of -1 (a pose no row was selected for) is an error."""
        return take_rows(rows_full, idx, self.H, self.N)


class LiveJoints:
    """What Pipeline.push_live_joints keeps between pushes (Pipeline.open_live_joints): .joints, a JointStream, and .pose, a
    TemporalStream of the same S, lag and max_frames; .pend_x [H,S,lag,J,3] and .pend_T [H,S,lag,3], x and T of the last `lag` frames
    pushed per stream - among them the frames that have not come out yet -, on the device; .t [S], the frames every stream's clip
    holds, on the host."""

    def __init__(self, joints, pose):
        assert (joints.S, joints.H, joints.J, joints.lag, joints.max_frames) == (pose.S, pose.H, pose.J, pose.lag, pose.max_frames)
        self.joints, self.pose = joints, pose
        self.pend_x = torch.zeros((joints.H, joints.S, joints.lag, joints.J, 3), dtype=torch.float32, device=joints.device)
        self.pend_T = torch.zeros((joints.H, joints.S, joints.lag, 3), dtype=torch.float32, device=joints.device)
        self.t = [0] * joints.S

    def reset(self):
        """Empties every stream; pending frames are dropped."""
        self.joints.reset()
        self.pose.reset()
        self.t = [0] * self.joints.S


def take_rows(rows_full, idx, H, N):
    """rows_full.view(H, N, ...)[idx, arange(N)] (plain torch indexing); idx [N] with every entry in 0 .. H-1."""
    if rows_full.shape[0] != H * N or tuple(idx.shape) != (N,):
        raise ValueError(f"take: rows [{H * N}, ...] and idx [{N}] expected, got {tuple(rows_full.shape)} and {tuple(idx.shape)}")
    i = idx.to(device=rows_full.device, dtype=torch.int64)
    if bool(((i < 0) | (i >= H)).any()):
        raise ValueError("take: a pose has no selected hypothesis (index -1) or an index outside the hypotheses")
    return rows_full.reshape((H, N) + tuple(rows_full.shape[1:]))[i, torch.arange(N, device=rows_full.device)]


def empty_selection(N, device):
    """What zedo_min_mpjpe reports for poses without a local row: (+inf, -1)."""
    return (torch.full((N,), float("inf"), dtype=torch.float64, device=device),
            torch.full((N,), -1, dtype=torch.int32, device=device))


def force_dist():
    """ZEDO_FORCE_DIST=1 (alias ZEDO_BENCH_FORCE_DIST): take the multi-rank code path (process group, RCCL
    collectives) with WORLD_SIZE = 1 too - how the exchange step is exercised on a one-GPU box."""
    return os.environ.get("ZEDO_FORCE_DIST") == "1" or os.environ.get("ZEDO_BENCH_FORCE_DIST") == "1"


def dist_backend():
    """Transport of the exchange step.  Default `nccl` (= RCCL on ROCm, one rank per GPU, over xGMI).
    ZEDO_DIST_BACKEND=gloo is a REHEARSAL transport: the same collectives on host copies of the (<= 8 KB per pose vector,
    or the gathered rows) tensors, so that N real ranks - N processes, N process-group members, every rank on its own
    row shard - can run where RCCL cannot: RCCL refuses two ranks on one device, and a one-GPU box is all a test has."""
    b = os.environ.get("ZEDO_DIST_BACKEND", "nccl").strip().lower() or "nccl"
    if b not in ("nccl", "gloo"):
        raise ValueError(f"ZEDO_DIST_BACKEND={b!r}: expected nccl or gloo")
    return b


def local_device_index():
    """The GPU of this rank: LOCAL_RANK - or device 0 for every rank with ZEDO_SHARE_DEVICE=1 (N ranks rehearsed on one
    MI355X; only with ZEDO_DIST_BACKEND=gloo)."""
    if os.environ.get("ZEDO_SHARE_DEVICE") == "1":
        if dist_backend() != "gloo":
            raise ValueError("ZEDO_SHARE_DEVICE=1 needs ZEDO_DIST_BACKEND=gloo: RCCL does not accept two ranks on one device")
        return 0
    return int(os.environ.get("LOCAL_RANK", "0"))


def init_dist(rank, world, device, default_port):
    """One process group per run: backend nccl (RCCL) bound to this rank's device, or the gloo rehearsal transport."""
    import datetime
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(default_port))
    if dist_backend() == "gloo":
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=600))
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)   # nccl == RCCL on ROCm
    return dist


def _host_transport(t):
    import torch.distributed as dist
    return t.is_cuda and dist.get_backend() == "gloo"


def all_reduce(t, op):
    """dist.all_reduce in place; over the gloo rehearsal transport a device tensor travels as a host copy."""
    import torch.distributed as dist
    if _host_transport(t):
        h = t.cpu()
        dist.all_reduce(h, op=op)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=op)
    return t


def all_gather_into_tensor(out, t):
    import torch.distributed as dist
    if _host_transport(t):
        ho = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(ho, t.cpu())
        out.copy_(ho)
    else:
        dist.all_gather_into_tensor(out, t)
    return out


def barrier():
    import torch.distributed as dist
    dist.barrier()


def dist_active():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or force_dist())


def reduce_min_over_ranks(best, idx):
    """The one exchange step of the sharded path: MIN over ranks of the per-pose error (RCCL all-reduce),
    then the lowest hypothesis index among the ranks that hold that minimum.  NaN follows np.amin / np.argmin
    (lib/dataset/h36m.py:411-412): a NaN on any rank wins and the lowest NaN hypothesis is reported; it travels
    as -inf (errors are >= 0) because a collective MIN does not define its NaN behaviour."""
    import torch.distributed as dist
    if not dist_active():
        return best, idx
    big = 2 ** 31 - 1
    key = torch.where(torch.isnan(best), torch.full_like(best, float("-inf")), best)
    g = key.clone()
    all_reduce(g, dist.ReduceOp.MIN)
    cand = torch.where((key == g) & (idx >= 0), idx.to(torch.int64), torch.full_like(idx, big, dtype=torch.int64))
    all_reduce(cand, dist.ReduceOp.MIN)
    cand = torch.where(cand == big, torch.full_like(cand, -1), cand)        # a pose no rank holds
    g = torch.where(g == float("-inf"), torch.full_like(g, float("nan")), g)
    return g, cand.to(torch.int32)


def gather_row_shards(x_local, total_rows, lo=None):
    """All ranks' contiguous row shards -> the full [total_rows, ...] tensor on every rank: one all-gather of equally
    sized (padded) shards.  run.inference writes every hypothesis of every pose (run/inference.py:233-236), so its
    result cannot stay sharded.  lo = None: the shards are the split of shard_rows(total_rows, rank, world); lo = this
    rank's first global row: any contiguous, ordered, gap-free split (e.g. whole hypotheses per rank,
    shard_hypotheses) - the shard sizes then travel in one small all-gather first."""
    import torch.distributed as dist
    if not dist_active():
        assert x_local.shape[0] == total_rows
        return x_local
    world = dist.get_world_size()
    tail = tuple(x_local.shape[1:])
    if lo is None:
        per = -(-total_rows // world)
        counts = None
    else:
        mine = torch.tensor([int(lo), x_local.shape[0]], dtype=torch.int64, device=x_local.device)
        allc = torch.empty((world * 2,), dtype=torch.int64, device=x_local.device)
        all_gather_into_tensor(allc, mine)
        counts = allc.reshape(world, 2).cpu().tolist()
        per = max(1, max(c for _, c in counts))
    pad = torch.zeros((per,) + tail, dtype=x_local.dtype, device=x_local.device)
    pad[:x_local.shape[0]] = x_local
    out = torch.empty((world * per,) + tail, dtype=x_local.dtype, device=x_local.device)
    all_gather_into_tensor(out, pad)
    if counts is None:
        return out[:total_rows]
    full = torch.empty((total_rows,) + tail, dtype=x_local.dtype, device=x_local.device)
    covered = 0
    for r, (rlo, cnt) in enumerate(counts):
        if cnt:
            assert rlo == covered, "row shards must be contiguous, ordered and gap-free"
            full[rlo:rlo + cnt] = out[r * per:r * per + cnt]
            covered += cnt
    assert covered == total_rows
    return full


def shard_hypotheses(H, rank, world):
    """Contiguous, unpadded split of the H hypotheses (EvaSampler.py:78-107 applied to hypotheses): for loops that
    cannot split inside a hypothesis (the step-wise sampler surface runs one hypothesis of all N poses at a time)."""
    per = -(-H // world)
    lo = min(rank * per, H)
    return lo, min(lo + per, H) - lo


def shard_rows(total_rows, rank, world):
    """Contiguous, unpadded split of the flattened (h, n) rows (the rule of reference
    lib/dataset/EvaSampler.py:78-107 applied to rows instead of samples)."""
    per = -(-total_rows // world)
    lo = min(rank * per, total_rows)
    hi = min(lo + per, total_rows)
    return lo, hi - lo
