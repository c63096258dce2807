/*
 * zedo_hip.h - C ABI of libzedo_hip.so: the MI355X (gfx950) implementation of ZeDO's
 * optimisation-in-the-loop diffusion sampling path.
 *
 * The reference (ipl-uw/ZeDO-Release) is pure Python/PyTorch and has no FFI; its boundary for
 * this path is a set of Python callables.  Each entry point below is the
 * native body of one of those callables and is bound with ctypes by
 * zedo-release_amd/zedo_hip/__init__.py; INTEGRATION.md shows the binding a reference maintainer
 * would add.  Citations are file:line in the reference tree.
 *
 * Conventions
 *  - every pointer named d_* is a DEVICE pointer to fp32 (unless stated), h_* is a HOST pointer;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued on
 *    it and nothing synchronises unless stated;
 *  - functions write only caller-allocated outputs and the caller-provided workspace; the only
 *    library-owned device memory lives inside zedo_weights_t / zedo_schedule_t handles;
 *  - calls on distinct streams may run concurrently, from one host thread or several, provided each call has its own
 *    workspace and outputs (one process per GPU is the intended use; a second device in the same process works: launch
 *    attributes are cached per device; a call runs on the device that is current when it is made, which must be the
 *    device of its pointers and of `stream`).  Handles are read-only to the row-batched entry points and may be shared
 *    by concurrent calls; zedo_weights_set_math is the exception (switch modes between runs, not during them).
 *    Process-wide state exists only outside the data path: the zedo_profile_* diagnostic (one session at a time; thread
 *    safe; samples launches of every stream) and the ZEDO_CHUNK_ROWS environment value, read once.
 *    tests/test_reentrancy_gpu.py runs two host threads x two streams through this contract;
 *  - rows are hypothesis-major: global row g = h*N + n (h = hypothesis, n = pose) - the order in
 *    which the reference's hypothesis loop produces them (run/opt_main.py:166-222).  A call may
 *    hold any contiguous shard of the global rows: local row b is global row row_offset + b, so
 *    pose = (row_offset+b) % N and hypothesis = (row_offset+b) / N (row_offset = 0 on one GPU);
 *  - return value: 0 on success, a negative ZEDO_E_* code or a positive hipError_t otherwise.
 */
#ifndef ZEDO_HIP_H
#define ZEDO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZEDO_ABI_VERSION 5   /* 3: + zedo_reproj_degenerate, zedo_pose_min, zedo_weights_set_math / zedo_weights_get_math;
                              * 4: + zedo_profile_bracket_ms;  5: + zedo_probe_mfma_peak_f16, workspace rows rounded to 64 again;
                              * still 5 (additive): + zedo_pc_plan_create / _destroy, zedo_pc_workspace_bytes, zedo_pc_step;
                              * still 5 (additive): + zedo_min_mpjpe_both;
                              * still 5 (additive): + zedo_min_reproj;
                              * still 5 (additive): + zedo_joint_reproj, zedo_joint_compose;
                              * still 5 (additive): + zedo_temporal_workspace_bytes, zedo_temporal_select;
                              * still 5 (additive): + zedo_prune_rank, zedo_prune_gather;
                              * still 5 (additive): + zedo_joint_temporal_workspace_bytes, zedo_joint_temporal_select;
                              * still 5 (additive): + zedo_joint_marginal_workspace_bytes, zedo_joint_marginal;
                              * still 5 (additive): + zedo_joint_accel_workspace_bytes, zedo_joint_accel_select;
                              * still 5 (additive): + zedo_joint_accel_marginal_workspace_bytes, zedo_joint_accel_marginal;
                              * still 5 (additive): + zedo_joint_stream_state_bytes, zedo_joint_stream_reset, zedo_joint_stream_push;
                              * still 5 (additive): + zedo_joint_stream_marginal_state_bytes, zedo_joint_stream_marginal_reset,
                              *                       zedo_joint_stream_marginal_push;
                              * still 5 (additive): + zedo_joint_accel_stream_state_bytes, zedo_joint_accel_stream_reset,
                              *                       zedo_joint_accel_stream_push;
                              * still 5 (additive): + zedo_joint_accel_stream_marginal_state_bytes,
                              *                       zedo_joint_accel_stream_marginal_reset, zedo_joint_accel_stream_marginal_push;
                              * still 5 (additive): + zedo_temporal_stream_state_bytes, zedo_temporal_stream_reset,
                              *                       zedo_temporal_stream_push;
                              * still 5 (additive): + zedo_temporal_marginal_workspace_bytes, zedo_temporal_marginal */

#define ZEDO_OK 0
#define ZEDO_E_BADARG (-1)      /* NULL pointer, non-positive size, unsupported dimension */
#define ZEDO_E_NOGPU (-2)       /* no gfx950 device visible */
#define ZEDO_E_WORKSPACE (-3)   /* workspace smaller than zedo_workspace_bytes() */

typedef struct zedo_weights zedo_weights_t;     /* packed ScoreModelFC_Adv parameters on device */
typedef struct zedo_schedule zedo_schedule_t;   /* per-step tables for one timestamp vector */

int zedo_abi_version(void);
const char *zedo_error_string(int code);

/* ---- score network parameters -------------------------------------------------------------
 * Replaces ScoreModelFC_Adv.__init__/load_state_dict (lib/algorithms/advanced/model.py:101-152,
 * run/opt_main.py:120-137).  h_params: the 34 parameter tensors of the state dict, fp32,
 * concatenated in state-dict order WITHOUT the float64 `sigmas` buffer:
 *   pre_dense.{weight[H,J3],bias[H]}, pre_dense_t.{weight[H,E],bias[H]}, pre_gnorm.{weight,bias}[H],
 *   shared_time_embed.0.{weight[E,E],bias[E]},
 *   for b in 1..n_blocks, k in 1..2: b{b}_dense{k}.{weight[H,H],bias[H]},
 *       b{b}_dense{k}_t.{weight[H,E],bias[H]}, b{b}_gnorm{k}.{weight,bias}[H],
 *   post_dense.{weight[J3,H],bias[J3]}
 * Supported: hidden H = 1024 (GroupNorm(32): groups of 32 channels), embed E = 512,
 * 1 <= J3 = n_joints*joint_dim <= 64, n_blocks = 2.  n_floats must equal the exact total.
 * Which entry point takes which size: zedo_score_eps, zedo_sde_step, zedo_pc_step - every J3 of the handle, pose rows
 * [B][J3]; zedo_reproj_prepare, zedo_reproj_degenerate, zedo_rotate_init, zedo_min_mpjpe(_both), zedo_min_reproj, zedo_joint_reproj, zedo_joint_compose - any J >= 1; zedo_ipo_fit(_resume) -
 * any J >= 1 with 1..17 key indices < J; zedo_oil_run (J3 == 51) and zedo_reproj_grad (J == 17) are the 17-joint, 3-coordinate
 * path only and return ZEDO_E_BADARG otherwise (tests/test_joint_counts_gpu.py holds each of these to the float64 oracle).
 * Synchronises `stream` before returning (h_params may be freed by the caller).
 */
int zedo_weights_create(const float *h_params, size_t n_floats, int n_joints, int joint_dim, int hidden,
                        int embed, int n_blocks, void *stream, zedo_weights_t **out);
void zedo_weights_destroy(zedo_weights_t *w);

/* ---- arithmetic of the dense layers (opt-in) ----------------------------------------------------------------------
 * ZEDO_MATH_F32 (default): exact fp32 MFMA (v_mfma_f32_32x32x2_f32), bitwise an fma chain per output.
 * ZEDO_MATH_F16X3: all six dense layers on the fp16 matrix pipe at fp32-level accuracy: every operand travels as two fp16
 *   pieces (a = ah + al + O(2^-24 |a|)), a 16-deep k block costs three fp16 MFMAs (al.bh + ah.bl + ah.bh, fp32
 *   accumulation); W carries a per-layer power-of-two scale undone exactly in the epilogue; activations between the
 *   hidden layers live in the same 4 bytes per element as two fp16 planes.  Per-product error = one fp32 rounding;
 *   measured max |y - y_fp64| of a layer 1.4e-6 (exact-fp32 kernel: 2.3e-6).  Results differ from ZEDO_MATH_F32 in the
 *   last bits, like any two fp32 implementations of the network do; the geometry kernels (reprojection, IPO, metric) and the
 *   fp32 pose state are unchanged.  Activations are stored as unscaled fp16 pieces: the call returns ZEDO_E_BADARG for a
 *   network whose GroupNorm parameters could produce |activation| >= 32768 (bound: sum over the residual path of
 *   max|gamma| sqrt(31) + max|beta|; trained checkpoints: O(10)), for non-finite weights, and for a weight matrix with a non-zero
 *   row whose largest entry is below 2^-8 of the matrix maximum (each matrix carries ONE scale: such a row would lose bits; DESIGN.md
 *   section 3 has the bound).
 *   zedo_weights_set_math builds the split copy of the six weight matrices on first use and
 *   synchronises `stream`; the mode is a property of the handle and applies to every later call that takes it.
 */
#define ZEDO_MATH_F32 0
#define ZEDO_MATH_F16X3 1
int zedo_weights_set_math(zedo_weights_t *w, int mode, void *stream);
int zedo_weights_get_math(const zedo_weights_t *w);

/* ---- per-step tables ----------------------------------------------------------------------
 * For the timestamp vector h_t[S] (torch.linspace(sde.T, eps, S), run/opt_main.py:198) builds on
 * the device, once:
 *   tbias[s][l][:] = W_l_t . SiLU(W_s . posemb(999 t_s) + b_s) + b_l_t + b_l     (model.py:251-281;
 *                    the time branch is identical for every row because vec_t = ones(B)*t,
 *                    advanced/sampling.py:497)
 *   a[s], c[s]     with  x' = a x + c eps_theta(x, 999 t)  == EulerMaruyamaPredictor.update_fn on
 *                    the probability-flow reverse sub-VP SDE with dt = -1/n_sde
 *                    (advanced/sampling.py:185-191, sde_lib.py:93-100,187-198, utils.py:751-777).
 * label_scale: the network is evaluated at labels = h_t * label_scale (fp32 product).  Pass 999 with
 * h_t = SDE times t (utils.py:762), or 1 with h_t = labels when calling the model surface directly
 * (then a, c are computed at t = label/999).
 * Synchronises `stream` before returning.
 */
int zedo_schedule_create(const zedo_weights_t *w, const float *h_t, int S, float label_scale, float beta_min,
                         float beta_max, int n_sde, void *stream, zedo_schedule_t **out);
void zedo_schedule_destroy(zedo_schedule_t *s);
/* debug/parity accessors: copy tables to host (synchronise). tbias: [S][1+2*n_blocks][H]. */
int zedo_schedule_read(const zedo_schedule_t *s, float *h_tbias, float *h_a, float *h_c);

/* Bytes of device workspace needed by the row-batched entry points below for B rows: 8448 bytes per row
 * (rows rounded up to 64) up to 2^20 rows; larger batches are walked in chunks of that many rows, so the
 * workspace never exceeds 8.9 GB (BASELINE configs 3/4: 3.5 M rows per GPU).  Environment (read once):
 * ZEDO_CHUNK_ROWS=<rows> overrides the chunk size (tests). */
size_t zedo_workspace_bytes(int B);

/* ---- reprojection geometry ------------------------------------------------------------------
 * Step-invariant part of gradient_field_gen (simple_zeroshot_opt.py:61-71,99 and the conf clamp
 * :64-66): geom[n][j] = (r_x, r_y, clamp(conf,1e-4,1)^4, 0, rhat_x, rhat_y, rhat_z, 0) with
 * r = Kinv [u v 1]^T / z and rhat = r/|r|.  d_conf may be NULL (weight 1).  d_uv [N,J,2], d_K [N,3,3],
 * d_conf [N,J] -> d_geom [N,J,8].  If d_conf_clamped != NULL the clamped confidences are also
 * written there (the reference clamps the caller's tensor in place).
 */
int zedo_reproj_prepare(const float *d_uv, const float *d_K, const float *d_conf, int N, int J,
                        float *d_geom, float *d_conf_clamped, void *stream);

/* How many of the N poses have a SINGULAR least-squares system for T (simple_zeroshot_opt.py:73-92): with the centred
 * closed form the 3x3 normal matrix is singular exactly when sum_j W_j |r_j - rbar|^2 == 0 - every ray of the pose
 * coincides.  The reference's torch.inverse(AtA) raises there (:89-92); the solve kernels would divide by zero
 * and produce a NaN T.  The quantity depends only on d_geom (not on x or the step), so it is checked ONCE per
 * problem: the host mirror raises like the reference does when a solve is requested and *h_count > 0.
 * Same fp32 arithmetic as the kernels' denominator.  Synchronises `stream`. */
int zedo_reproj_degenerate(const float *d_geom, int N, int J, int *h_count, void *stream);

/* gradient_field_gen (simple_zeroshot_opt.py:46-125, noise_type None):
 *   solve_T != 0 : T = weighted least-squares translation (:73-93, sign fix :93), written to d_T
 *   solve_T == 0 : T = d_T as given (:95-96)
 *   g = ((x+T).r^) r^ - (x+T)  (:99,109) written to d_g.  d_x [B,J,3], d_T [B,3], d_g [B,J,3].
 */
int zedo_reproj_grad(const float *d_x, const float *d_geom, float *d_T, int solve_T, float *d_g, int B,
                     int N, int J, long long row_offset, void *stream);

/* ---- score network / predictor ---------------------------------------------------------------
 * eps = ScoreModelFC_Adv.forward(x, labels = 999 t_step) (model.py:215-298), d_eps [B,J,3]. */
int zedo_score_eps(const zedo_weights_t *w, const zedo_schedule_t *s, int step, const float *d_x,
                   float *d_eps, int B, void *d_workspace, size_t workspace_bytes, void *stream);
/* one pc_sampler call (advanced/sampling.py:450-527): x <- a[step] x + c[step] eps(x). In place. */
int zedo_sde_step(const zedo_weights_t *w, const zedo_schedule_t *s, int step, float *d_x, int B,
                  void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- generic predictor-corrector step -------------------------------------------------------------
 * The native body of pc_sampler for EVERY registered predictor / corrector / SDE combination
 * (advanced/sampling.py:180-331, 400-529; reverse SDE / ODE: sde_lib.py:71-109).  With vec_t = ones(B)*t (:497)
 *   predictor:       x_mean = A x + B score(x),  x_new = x_mean + C z          (:180-248)
 *   corrector step:  x_mean = x + s score(x),    x     = x_mean + sqrt(2 s) z  (:259-331)
 *   score(x) = net_scale * eps(x, label)                                       (utils.py:751-800, model.py:294)
 * and every scalar depends on the step only.  A plan holds them for S steps (host arrays, fp32, length S):
 *   h_label, h_net_scale;  has_predictor != 0: h_pA, h_pB, h_pC (C = 0: no noise term, e.g. probability flow);
 *   corrector ZEDO_PC_CORR_ALD: h_corr = s[S];  ZEDO_PC_CORR_LANGEVIN: h_corr = factor[S] = 2 alpha snr^2 and
 *   s = factor (mean_b ||z_b|| / mean_b ||score_b||)^2 is formed on the device per corrector step (:281-284);
 *   n_corr corrector steps per call (ignored with ZEDO_PC_CORR_NONE).
 * The plan owns the time-bias table of its labels (zedo_schedule_create's machinery, label_scale 1; plans of up to 256
 * steps borrow the weights handle's scratch).  zedo_pc_plan_create is the only call here that allocates or synchronises
 * `stream`; the host arrays may be freed when it returns.
 */
typedef struct zedo_pc_plan zedo_pc_plan_t;
#define ZEDO_PC_CORR_NONE 0
#define ZEDO_PC_CORR_LANGEVIN 1
#define ZEDO_PC_CORR_ALD 2
int zedo_pc_plan_create(const zedo_weights_t *w, int S, const float *h_label, const float *h_net_scale, int has_predictor,
                        const float *h_pA, const float *h_pB, const float *h_pC, int corrector, int n_corr,
                        const float *h_corr, void *stream, zedo_pc_plan_t **out);
void zedo_pc_plan_destroy(zedo_pc_plan_t *p);
/* equals zedo_workspace_bytes(B): eps, the row norms and the step size of a Langevin step live in the network's buffers */
size_t zedo_pc_workspace_bytes(const zedo_pc_plan_t *p, int B);
/* One pc_sampler call (advanced/sampling.py:450-527): n_corr corrector steps, then the predictor, at plan entry `step`.
 * d_x [B,J,3] in: x, out: x_new.  d_x_mean [B,J,3] out, may be NULL (with no predictor it receives x_new, as NonePredictor
 * hands back, :248-256).
 * h_z: HOST array of n_corr + (has_predictor ? 1 : 0) device pointers, each one noise draw [B,J,3] of the caller, in the order
 * the reference draws them (corrector steps first); consumed before the call returns.  The corrector entries are required.
 * The predictor entry may be NULL - and h_z itself when n_corr == 0 - which means "keep x_mean only" (noise_removal: the
 * caller still makes the draw for its RNG stream but does not hand it over): d_x then returns x_mean and the noise launch is
 * skipped, as it is when C[step] == 0.
 * Batches above the chunk size of zedo_workspace_bytes are walked in chunks, except Langevin plans: the mean spans the
 * whole call, so B above the chunk size returns ZEDO_E_BADARG.  The mean is over the B rows of the call - a batch split
 * over several calls (or ranks) gets a different step size than the whole, as it does in the reference.
 * Allocates nothing, copies nothing to the host, synchronises nothing; the Langevin step size never leaves the device:
 * legal under stream capture.  Bit-identical from run to run (fixed-order sums, no atomics).
 */
int zedo_pc_step(const zedo_weights_t *w, const zedo_pc_plan_t *p, int step, float *d_x, float *d_x_mean,
                 const float *const *h_z, int B, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- the fused OIL loop: run/opt_main.py:202-220 -------------------------------------------------
 * for i in [step_begin, step_end): g,T = gradient_field_gen(x, T if i < switch_step else None);
 *                                   x += g;  x = a_i x + c_i eps(x, t_i)
 * State stays on the device; no host round trip.  d_x [B,J,3] in/out, d_T [B,3] in/out,
 * d_geom [N,J,8].  switch_step = S//5 in the reference.
 */
int zedo_oil_run(const zedo_weights_t *w, const zedo_schedule_t *s, float *d_x, const float *d_geom,
                 float *d_T, int step_begin, int step_end, int switch_step, int B, int N, long long row_offset,
                 void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- IPO: run/opt_main.py:177-195 + RotOpt (simple_zeroshot_opt.py:8-31) -----------------------------
 * Per row b=(h,n): T0 = ipo_T * normalise(Kinv [u0 v0 1]); `iters` Adam(lr 0.1) iterations on
 * (rot_vect, rot_vect_<axes>, scale) minimising mean |proj(R x0_h[kl] + T0 clamp(scale)) - uv[kl]|
 * where the mean's divisor is `normaliser` (= N*k*2 of the reference batch; pass the GLOBAL value
 * when rows are sharded).  d_x0 [H,J,3] (centred cluster poses), d_uv [N,J,2], d_K [N,3,3],
 * h_keylist[k] joint indices, axes_mask bit0=x bit1=y bit2=z (RotOpt's `axis`: 0 = rot_vect and scale only ... 7 = "xyz";
 * a value outside 0..7 is rejected with ZEDO_E_BADARG, by zedo_ipo_fit_resume as well).  The parameters and Adam moments of an
 * axis that is not in the mask are never written: d_q holds an exact 0 there (a resumed state: whatever the caller put in).
 * Outputs: d_R [B,3,3], d_T [B,3] = T0*clamp(scale), optional d_q [B,4], d_scale [B] (may be NULL).
 * h_keylist is consumed before the call returns (it travels as a kernel argument); nothing synchronises and nothing is
 * copied (Adam's bias-correction terms are constants of the code object): every call, the first one included, is a plain
 * kernel launch on `stream` - legal under stream capture and safe beside fits on other streams or host threads.
 * The ten gradient sums over the key joints are formed in ONE fixed pairing order by both kernels behind this entry
 * point (one row per half-wave for small batches, one lane per row for large ones): a row's result does not depend on B,
 * row_offset, the shard it is in or the kernel that ran it.
 * H = number of hypotheses in d_x0: row_offset + B > H*N is rejected (ZEDO_E_BADARG).
 */
int zedo_ipo_fit(const float *d_x0, const float *d_uv, const float *d_K, const int *h_keylist, int k,
                 int axes_mask, float ipo_T, float min_scale, float max_scale, int iters, double normaliser,
                 float *d_R, float *d_T, float *d_q, float *d_scale, int B, int H, int N, int J, long long row_offset,
                 void *stream);

/* The same fit, resumable (parity instrument: one Adam iteration from a captured optimiser state).
 * d_state [B,15] fp32 = (param[5], exp_avg[5], exp_avg_sq[5]) in the order (rot_vect, rot_vect_x, _y, _z, scale),
 * i.e. torch.optim.Adam's per-parameter state (opt_main.py:183).  it_begin = iterations already applied to
 * d_state; with it_begin == 0 the input content is ignored and the fit starts from RotOpt's initial values
 * (simple_zeroshot_opt.py:11-16).  Runs iterations [it_begin, it_begin + iters) and writes the state back.
 * A fit split into resumed calls returns the bits of the unsplit fit, in R, T, q, scale and all 15 state columns, in either
 * kernel and across iteration 2048, where Adam's bias corrections leave their constant table (tests/test_ipo_state_gpu.py).
 * Rows of d_state behind row B - 1 are not touched; iters == 0 with it_begin > 0 returns R, T of the state as it is.
 */
int zedo_ipo_fit_resume(const float *d_x0, const float *d_uv, const float *d_K, const int *h_keylist, int k,
                        int axes_mask, float ipo_T, float min_scale, float max_scale, int iters, double normaliser,
                        float *d_R, float *d_T, float *d_q, float *d_scale, float *d_state, int it_begin, int B, int H,
                        int N, int J, long long row_offset, void *stream);

/* x[b] = R[b] . x0[h(b)]   (run/opt_main.py:201).  d_x [B,J,3]; d_x0 [H,J,3]. */
int zedo_rotate_init(const float *d_x0, const float *d_R, float *d_x, int B, int H, int N, int J, long long row_offset,
                     void *stream);

/* ---- hypothesis selection: eval_multi inner loops (lib/dataset/h36m.py:394-417, pw3d.py:302-331) ----
 * err[b] = mean_j || pred[b,j] - gt[n(b),j] ||, after similarity (Procrustes, scaling, reflection
 * 'best': lib/utils/transforms.py:42-127) alignment when procrustes != 0; then per pose n the
 * minimum over the hypotheses present in [0,B) and its hypothesis index.
 * d_pred [B,J,3] fp32 rows (h,n); d_gt [N,J,3] float64, root-centred, metres.
 * d_err [B] float64 (output, required); d_best [N] float64; d_best_h [N] int32 (first minimum, the
 * np.argmin rule).  Poses with no local row get +inf / -1.
 * Any J >= 1.  Alignments of rank 2 (planar joints, three joints) and rank 1 (collinear joints, two joints) return the
 * reference's value: the error does not depend on how the null directions of the SVD are completed.  With procrustes != 0
 * and NO direction at all - J == 1, or every joint of the prediction or of the ground truth in one point - the call is
 * undefined, as the reference is (its SVD is handed 0 / 0 and raises): the kernel writes NaN for such a row, which then
 * poisons its pose's minimum like any NaN.
 */
int zedo_min_mpjpe(const float *d_pred, const double *d_gt, int B, int N, int J, long long row_offset,
                   int procrustes, double *d_err, double *d_best, int *d_best_h, void *stream);

/* Both protocols from ONE pass over the rows: the reference scores every batch of hypotheses twice from the same preds,
 * eval_multi(protocol2=False) then eval_multi(protocol2=True) (run/opt_main.py:227-228); this reads d_pred and d_gt once,
 * evaluates both errors of a row from the same staged operands and takes both arg-mins in one launch.
 * Outputs are protocol-major: d_err [2][B], d_best [2][N], d_best_h [2][N].  Slot 0 holds what
 * zedo_min_mpjpe(..., procrustes = 0, ...) writes, slot 1 what procrustes = 1 writes - bit for bit (the same statements
 * on the same operands): row errors, minima, first arg-min indices, +inf / -1 of poses with no local row, NaN winning
 * the minimum.  With J == 1 slot 1 is NaN (see above) and slot 0 stays finite.  Each half of d_err is a valid input of
 * zedo_pose_min.  Inputs, argument checks (ZEDO_E_BADARG, nothing written) and the contract are those of zedo_min_mpjpe:
 * any J >= 1, any contiguous shard (row_offset); allocates nothing, synchronises nothing, enqueues on `stream` only. */
int zedo_min_mpjpe_both(const float *d_pred, const double *d_gt, int B, int N, int J, long long row_offset,
                        double *d_err, double *d_best, int *d_best_h, void *stream);

/* ---- hypothesis selection WITHOUT ground truth: the minimum reprojection error --------------------------------------
 * The criterion the whole loop optimises, evaluated on its result: how far x + T reprojects from the 2D detections,
 * weighted by detector confidence (the reference's follow-up driver tracks proj2d - condition per step,
 * run/opt_main_infant.py:307-309).  For local row b, pose n = (row_offset + b) % N, in fp64 on the fp32 inputs:
 *   X_j = x[b,j] + T[b];   q_j = K[n] . X_j  (the full 3x3 product of RotOpt.forward, simple_zeroshot_opt.py:20-25: skew,
 *                                             K22 != 1 and a homogeneous row other than (0,0,1) are honoured)
 *   d_j = || q_j.xy / q_j.z - uv[n,j] ||                                     pixels
 *   w_j = d_conf ? clamp(conf[n,j], 1e-4, 1) : 1   (the clamp of gradient_field_gen, :64-66, first power, taken in fp32)
 *   err[b] = sum_j w_j d_j / sum_j w_j             (sums in ascending j)
 * A row with any joint at or behind the camera plane (q_j.z <= 0) gets err = +inf; NaN inputs fall through that test and
 * give NaN.  Then, per pose, the minimum over the hypotheses present in [0,B) and its index exactly as zedo_pose_min
 * takes them: NaN wins (a diverged row does not hide behind a finite one), ties go to the lower hypothesis, a pose with
 * no local row gets +inf / -1, a pose whose every local row is +inf reports +inf and its first local hypothesis.
 * d_x [B,J,3] rows (h,n); d_T [B,3] the loop's final translation of each row; d_uv [N,J,2]; d_K [N,3,3];
 * d_conf [N,J] or NULL (weight 1).  d_err [B] float64 (output, required; a valid input of zedo_pose_min),
 * d_best [N] float64, d_best_h [N] int32.
 * Contract as zedo_min_mpjpe: any J >= 1, any contiguous shard (row_offset); ZEDO_E_BADARG with nothing written for a
 * NULL required pointer, a non-positive size or row_offset < 0; allocates nothing, synchronises nothing, enqueues on
 * `stream` only: legal under stream capture.  Every row's error is the same bits whichever kernel evaluates it (J == 17
 * with a 16-byte aligned d_x: rows staged through the LDS; otherwise one lane per row from global memory). */
int zedo_min_reproj(const float *d_x, const float *d_T, const float *d_uv, const float *d_K, const float *d_conf,
                    int B, int N, int J, long long row_offset, double *d_err, double *d_best, int *d_best_h, void *stream);

/* ---- joint-wise aggregation WITHOUT ground truth: the minimum reprojection error per joint ------------------------------
 * Where zedo_min_reproj keeps one whole hypothesis per pose, this keeps, for every joint of every pose, the hypothesis whose
 * joint reprojects closest to its detection, and zedo_joint_compose assembles the pose from those joints (the joint-wise
 * reprojection-based aggregation of D3DP, Shan et al., ICCV 2023).  A joint assembled in the camera frame is exactly one
 * hypothesis's joint, so the confidence-weighted mean of the per-joint minima never exceeds the smallest per-row weighted mean.
 * Whether this lowers the error against ground truth on real data is not measured.
 * For local row b, pose n = (row_offset + b) % N, in fp64 on the fp32 inputs, with the statements of zedo_min_reproj:
 *   X = x[b,j] + T[b];   q = K[n] . X  (full 3x3 product);   d[b,j] = || q.xy / q.z - uv[n,j] ||          pixels
 * q.z <= 0 gives d[b,j] = +inf for THAT JOINT only (the row-level call makes the whole row +inf); NaN inputs fall through that
 * test and give NaN.  No confidences: a joint's weight is the same for every hypothesis of its pose and cannot change a
 * per-joint arg-min.  d_best [N,J] float64 and d_best_h [N,J] int32 (both required): the minimum over the hypotheses present
 * in [0,B) and the hypothesis that attains it, bit for bit what zedo_pose_min(d_jerr, B*J, N*J, row_offset*J, ...) returns
 * on the flattened [B,J] distances - NaN wins, ties go to the lower hypothesis, no local row gives +inf / -1, a (pose, joint)
 * whose every local entry is +inf reports +inf and its first local hypothesis.
 * d_jerr [B,J] float64 is OPTIONAL.  NULL: one kernel, one lane per (pose, joint), walks the local hypotheses of its pose with
 * uv[n,j] and K[n] in registers and a running minimum - nothing of size [B,J] is written.  Not NULL: d is written (the same
 * bits for any alignment of d_x) and zedo_pose_min's kernels run on it.  Both routes return the same bits in d_best / d_best_h.
 * Contract: any J >= 1, any contiguous shard (row_offset); ZEDO_E_BADARG with nothing written for a NULL required pointer, a
 * non-positive size, row_offset < 0, or B*J or N*J above INT_MAX; allocates nothing, synchronises nothing, enqueues on
 * `stream` only: legal under stream capture; no atomics: bit-identical from run to run. */
int zedo_joint_reproj(const float *d_x, const float *d_T, const float *d_uv, const float *d_K, int B, int N, int J,
                      long long row_offset, double *d_jerr, double *d_best, int *d_best_h, void *stream);

/* The assembled pose, a gather over ALL rows d_x [H*N,J,3], d_T [H*N,3] (rows (h,n)):
 *   pose[n,j,c] = fl32( ((double)x[g,j,c] + (double)T[g,c]) - (d_ref_h ? (double)T[ref_h[n]*N + n, c] : 0) ),  g = joint_h[n,j]*N + n
 * d_joint_h [N,J] int32 (e.g. d_best_h of zedo_joint_reproj after the MIN over ranks); d_ref_h [N] int32 or NULL.  NULL: the
 * camera frame.  Otherwise the root-relative frame of hypothesis ref_h[n] (e.g. zedo_min_reproj's winner): a joint taken from
 * the reference hypothesis itself comes back as x exactly (the fp64 sum of two fp32 numbers is exact unless |x| < 2^-29 |T|).  An index outside 0 .. H-1, in d_joint_h or d_ref_h, makes the
 * affected joints NaN and is never used as an address.  d_pose [N,J,3] fp32.  Contract as zedo_joint_reproj. */
int zedo_joint_compose(const float *d_x, const float *d_T, const int *d_joint_h, const int *d_ref_h, int H, int N, int J,
                       float *d_pose, void *stream);

/* ---- selection along a video WITHOUT ground truth: Viterbi over a unary cost and a motion cost -------------------------
 * zedo_min_reproj and zedo_joint_reproj decide every frame on its own; on the frames of a video the kept hypothesis then
 * jumps between depth-ambiguous solutions.  This keeps, per frame, the hypothesis that minimises its own cost plus lambda
 * times the mean joint displacement to the previous frame's choice - exactly, by dynamic programming over each clip.
 * Whether this lowers the error against ground truth on real video is not measured.
 * d_unary [H*N] float64, rows (h,n) h-major, ALL rows (the recurrence needs every hypothesis of consecutive frames: no
 * row_offset): any per-row cost, e.g. d_err of zedo_min_reproj (pixels), or of zedo_min_mpjpe as an oracle.
 * d_x [H*N,J,3] fp32, the same rows (metres).  lambda: cost units per metre (pixels per metre on zedo_min_reproj's errors).
 * d_seq_start [n_seq+1] int32 ON THE DEVICE: strictly ascending, first 0, last N; clip s is frames seq_start[s] ..
 * seq_start[s+1]-1.  The call cannot look at it without synchronising: every entry is clamped to 0 .. N before use and is
 * never an address; with an array that breaks the rules the result is unspecified.
 * All arithmetic in float64 on the inputs as given:
 *   u[n,h]    = unary[h*N+n] if finite, else +inf (NaN and +-inf: the hypothesis is excluded - NOT zedo_pose_min's "NaN wins":
 *               one diverged row must not own a whole clip);  a frame is DEAD if no u[n,h] is finite
 *   m[n,h',h] = (1/J) sum_j sqrt(sum_c ((double)x[h,n,j,c] - (double)x[h',n-1,j,c])^2)      (sums ascending in c, then in j)
 *   chain start (n first of its clip, or frame n-1 dead):  D[n,h] = u[n,h], back[n,h] = -1
 *   otherwise:  D[n,h] = u[n,h] + min_h' (D[n-1,h'] + lambda m[n,h',h]),  back[n,h] = the lowest h' that attains the minimum
 *   dead frame: D[n,.] = +inf
 * Backwards per clip: at the last frame of a chain (the clip's last frame, or the next frame is dead) path[n] = the lowest h
 * that minimises D[n,.]; inside a chain path[n] = back[n+1, path[n+1]].
 * d_path_h [N] int32; d_cost [N] float64 = D[n, path[n]]; a dead frame reports hypothesis 0 and cost +inf.
 * (x is taken to be finite: a non-finite coordinate makes the affected minima unspecified, never an address.)
 * Workspace (8-byte aligned): D [N,H] float64, back [N,H] int32, two int32 flags per frame, then C*H*H float64 transition
 * costs of a chunk of C frames.  zedo_temporal_workspace_bytes(N, H, chunk_frames) returns the bytes for
 * C = min(chunk_frames, N); chunk_frames <= 0: the largest C whose transition costs stay at or under 256 MB (at least one
 * frame); 0 for sizes the call refuses.  The call uses the largest C that workspace_bytes admits, capped at N, and returns
 * the same bits for every C; ZEDO_E_WORKSPACE with nothing written if not even one frame of transitions fits.  The
 * workspace need not be initialised.
 * Contract: any J >= 1, H >= 1, N >= 1, 1 <= n_seq <= N, finite lambda >= 0; ZEDO_E_BADARG with nothing written for a NULL
 * pointer, a non-positive size, n_seq > N, a negative or non-finite lambda, a workspace that is not 8-byte aligned, or H*N
 * or H*H above INT_MAX; allocates nothing, synchronises nothing, enqueues on `stream` only: legal under stream capture; no
 * atomics: bit-identical from run to run.  One workgroup per clip: a single long clip is serial in time on one CU. */
size_t zedo_temporal_workspace_bytes(int N, int H, int chunk_frames);
int zedo_temporal_select(const double *d_unary, const float *d_x, const int *d_seq_start, int n_seq, int H, int N, int J,
                         double lambda, void *d_workspace, size_t workspace_bytes, int *d_path_h, double *d_cost, void *stream);

/* ---- joint-wise selection along a video WITHOUT ground truth: one Viterbi chain per joint ------------------------------
 * zedo_joint_reproj decides every joint of every frame on its own, zedo_temporal_select keeps whole hypotheses and its motion
 * term is a mean over all joints.  This is their product: for every joint of every clip the hypothesis path that minimises
 * that joint's own cost plus lambda times that joint's displacement to the previous frame's choice, in the camera frame
 * (x + T) - the frame zedo_joint_compose assembles in - exactly, by dynamic programming over each clip, independently for
 * every joint.  Whether this lowers the error against ground truth on real video is not measured.
 * d_junary [H*N,J] float64, rows (h,n) h-major, ALL rows (no row_offset): any per-(row, joint) cost, e.g. d_jerr of
 * zedo_joint_reproj (pixels).  d_x [H*N,J,3] fp32 and d_T [H*N,3] fp32, the same rows (metres); d_T may be NULL: the motion
 * term is then taken on x alone.  lambda: cost units per metre.  d_seq_start [n_seq+1] int32 ON THE DEVICE, the rules of
 * zedo_temporal_select: every entry is clamped to 0 .. N before use and is never an address.
 * All arithmetic in float64 on the inputs as given, independent for every joint j:
 *   X[n,h,j,c]   = (double)x[h*N+n,j,c] + (d_T ? (double)T[h*N+n,c] : 0.0)
 *   u[n,j,h]     = junary[(h*N+n)*J + j] if finite, else +inf (NaN and +-inf: the hypothesis is excluded for that joint);
 *                  (n,j) is DEAD if no u[n,j,h] is finite
 *   m[n,j,h',h]  = sqrt(d0^2 + d1^2 + d2^2),  d_c = X[n,h,j,c] - X[n-1,h',j,c]          (products, then the sum ascending in c)
 *   chain start (n first of its clip, or (n-1,j) dead):  D[n,j,h] = u[n,j,h], back[n,j,h] = -1
 *   otherwise:  D[n,j,h] = u[n,j,h] + min_h' (D[n-1,j,h'] + lambda m[n,j,h',h]),  back[n,j,h] = the lowest h' that attains the minimum
 *   dead (n,j): D[n,j,.] = +inf
 * Backwards per (clip, joint): at the last frame of a chain (the clip's last frame, or (n+1,j) is dead) path[n,j] = the lowest h
 * that minimises D[n,j,.]; inside a chain path[n,j] = back[n+1,j, path[n+1,j]].
 * d_path_h [N,J] int32; d_cost [N,J] float64 = D[n,j, path[n,j]]; a dead (frame, joint) reports hypothesis 0 and cost +inf and
 * splits only that joint's chain.  With d_T == NULL and J == 1 the outputs are the bits of zedo_temporal_select on the same
 * unaries and x (the same statements on the same operands).
 * (x and T are taken to be finite: a non-finite coordinate makes the affected minima unspecified, never an address.)
 * Workspace (8-byte aligned, need not be initialised): D [N,J,H] float64, back [N,J,H] int32, two int32 flags per (frame,
 * joint) - zedo_joint_temporal_workspace_bytes(N, H, J); 0 for sizes the call refuses.  There is no H x H table: a transition
 * cost is one square root of three terms and is computed where the recurrence consumes it.
 * Contract: J >= 1, N >= 1, 1 <= n_seq <= N, 1 <= H <= 1024 (one joint's X[n-1,.] and D[n-1,.] stay in the LDS), N*J*H <=
 * INT_MAX, finite lambda >= 0; ZEDO_E_BADARG with nothing written for a NULL pointer other than d_T, a non-positive size,
 * H > 1024, n_seq > N, N*J*H above INT_MAX, a negative or non-finite lambda, or a workspace that is not 8-byte aligned;
 * ZEDO_E_WORKSPACE with nothing written if workspace_bytes is too small; allocates nothing, synchronises nothing, enqueues on
 * `stream` only: legal under stream capture; no atomics: bit-identical from run to run.  One workgroup per (clip, joint): a
 * single long clip is serial in time on J CUs. */
size_t zedo_joint_temporal_workspace_bytes(int N, int H, int J);
int zedo_joint_temporal_select(const double *d_junary, const float *d_x, const float *d_T, const int *d_seq_start, int n_seq,
                               int H, int N, int J, double lambda, void *d_workspace, size_t workspace_bytes,
                               int *d_path_h, double *d_cost, void *stream);

/* ---- joint-wise selection on a LIVE video: the same chain, fixed-lag, with the state in caller-owned memory ----------------------
 * zedo_joint_temporal_select needs the whole clip before it answers.  This is its first-order chain as an online call for S
 * independent streams at once: frames are pushed in chunks of any size, the tables live in d_state between the calls, and the
 * decision for a frame comes out `lag` frames after the frame went in.  It is the decision of zedo_joint_temporal_select on the
 * clip cut after frame n + lag; with a lag of at least the clip's length - 1 and a flush at the end the outputs are that call's
 * bits.  The choice of lag is untuned; whether a fixed-lag path is closer to ground truth than the per-frame choice on real video
 * is not measured.
 * A stream's CLIP is the frames pushed since its last reset or flush, t = 0, 1, ..  X, u, m, DEAD, "chain start", D and back are
 * those of zedo_joint_temporal_select, word for word, on that clip: prefix quantities, which do not depend on how the frames were
 * cut into calls.  With lag >= 0:
 *   frame n of a clip is EMITTED by the first push after which the clip holds frame n + lag, or by the push that flushes the
 *   stream, whichever comes first; all joints of a frame together, in frame order.
 *   For a live (n,j) let c_j(n) be the last frame of n's chain on the frames the clip holds after that push - the first m >= n
 *   whose successor is dead or absent - and e = min(n + lag, c_j(n)).  Then
 *     h_e = the lowest h that minimises D[e,j,.];  h_{m-1} = back[m,j,h_m] for m = e .. n+1;
 *     path[n,j] = h_n;  cost[n,j] = D[n,j,h_n].
 *   A dead (n,j) reports hypothesis 0 and cost +inf.  After a flush the stream's next frame is t = 0 of a new clip.
 * So lag = 0 gives the lowest arg-min of D[n,j,.], and the outputs do not depend on the chunking.
 * zedo_joint_stream_push: the chunk is N = S*F frames in the layout of zedo_joint_temporal_select - rows (h,n) h-major with
 * n = s*F + f: d_junary [H*N,J] float64, d_x [H*N,J,3] fp32, d_T [H*N,3] fp32 or NULL - stream s's chunk is a "clip" of F frames
 * of an offline call on the same tensors.  d_flush [S] int32 ON THE DEVICE (NULL: none): stream s is flushed after its chunk if
 * d_flush[s] != 0.  F = 0 is legal only with d_flush; d_junary, d_x and d_T are then unused.
 * Outputs: d_path_h [S, F+lag, J] int32 and d_cost [S, F+lag, J] float64, row r of stream s = the r-th frame this push emits for
 * it; d_emit [S,2] int64 = the clip-local index of the first emitted frame (of the next one to be emitted if the count is 0) and
 * the count.  Rows at and after the count are not written.  With t the frames the clip held before the push, the count is
 *   held = min(lag, t) + F;   count = held if the stream is flushed, else max(0, held - lag);   first = max(0, t - lag)
 * - computable on the host without reading d_emit.
 * zedo_joint_stream_reset empties the streams with d_which[s] != 0 (d_which [S] int32 ON THE DEVICE; NULL: all of them); pending
 * frames are dropped.  The state need not be initialised before its first reset, and must have been reset before its first push.
 * State (8-byte aligned), with R = lag + max_frames rows per ring and SJ = S*J chains, in this order:
 *   D float64 [SJ,R,H] | X float64 [SJ,H,3] and D float64 [SJ,H] of the clip's last frame | the clip's frame count int64 [S] |
 *   back int32 [SJ,R,H] | the dead flags of the ring's frames int32 [SJ,R] | the dead flag of the last frame int32 [SJ]
 * - zedo_joint_stream_state_bytes = 8 (SJ R H + 4 SJ H + S) + 4 (SJ R H + SJ R + SJ) rounded up to 8; 0 for shapes the calls
 * refuse.  Frame m of a clip sits in row m % R.  The emitted count is not stored: it is max(0, frame count - lag).  A push writes
 * the rows of its F <= max_frames frames and then reads at most the lag frames before them: never a row it has overwritten.
 * Contract: 1 <= H <= 1024, J >= 1, S >= 1, max_frames >= 1, 0 <= F <= max_frames, lag >= 0, (lag + max_frames)*S*J*H <= INT_MAX,
 * finite lambda >= 0; ZEDO_E_BADARG with nothing written and the state untouched for a NULL pointer other than d_T, d_flush
 * (F > 0) and d_which, a size out of these ranges, F = 0 without d_flush, a negative or non-finite lambda, or a state that is not
 * 8-byte aligned; ZEDO_E_WORKSPACE with nothing written and the state untouched if state_bytes is too small; allocates nothing,
 * synchronises nothing, enqueues on `stream` only: legal under stream capture - a replay advances the state.  No atomics: the
 * bits do not depend on the run, the chunking, the content of the state before its reset or the alignment of d_x.  Every value
 * read from the state is clamped before it is an index.  One workgroup per (stream, joint) for the recurrence, one wave per
 * (emitted frame, stream, joint) for the decision: at most lag dependent reads of back. */
size_t zedo_joint_stream_state_bytes(int S, int H, int J, int lag, int max_frames);
int zedo_joint_stream_reset(void *d_state, size_t state_bytes, int S, int H, int J, int lag, int max_frames, const int *d_which,
                            void *stream);
int zedo_joint_stream_push(const double *d_junary, const float *d_x, const float *d_T, int S, int F, int H, int J, int lag,
                           int max_frames, double lambda, const int *d_flush, void *d_state, size_t state_bytes, int *d_path_h,
                           double *d_cost, long long *d_emit, void *stream);

/* ---- pose-level selection on a LIVE video: the chain of zedo_temporal_select, fixed-lag, with the state in caller-owned memory ----
 * Offline, every joint-wise answer along a video is assembled in the frame of the pose-level path of zedo_temporal_select
 * (zedo_joint_compose with d_ref_h = that path), and that call needs the whole clip.  This is its chain as an online call for S
 * independent streams at once, the sibling of zedo_joint_stream_push: frames are pushed in chunks of any size, the tables live in
 * d_state between the calls, and the decision for a frame comes out `lag` frames after the frame went in.  It is the decision of
 * zedo_temporal_select on the clip cut after frame n + lag; with a lag of at least the clip's length - 1 and a flush at the end
 * the outputs are that call's bits.  The choice of lag is untuned; whether a fixed-lag path is closer to ground truth than the
 * per-frame choice on real video is not measured.
 * A stream's CLIP is the frames pushed since its last reset or flush, t = 0, 1, ..  u, m (the mean over J of the joint distances on
 * x alone - there is no T here -, the sums ascending in c, then in j, divided by J), DEAD, "chain start", D and back are those of
 * zedo_temporal_select, word for word, on that clip: prefix quantities, which do not depend on how the frames were cut into
 * calls.  With lag >= 0:
 *   frame n of a clip is EMITTED by the first push after which the clip holds frame n + lag, or by the push that flushes the
 *   stream, whichever comes first, in frame order.
 *   For a live frame n let c(n) be the last frame of n's chain on the frames the clip holds after that push - the first m >= n
 *   whose successor is dead or absent - and e = min(n + lag, c(n)).  Then
 *     h_e = the lowest h that minimises D[e,.];  h_{m-1} = back[m,h_m] for m = e .. n+1;
 *     path[n] = h_n;  cost[n] = D[n,h_n].
 *   A dead frame reports hypothesis 0 and cost +inf.  After a flush the stream's next frame is t = 0 of a new clip.
 * So lag = 0 gives the lowest arg-min of D[n,.]; the outputs do not depend on the chunking; with lag >= the clip's length - 1 and
 * a flush they are the bits of zedo_temporal_select on the clip, and at any lag those of that call on the clip cut after frame
 * n + lag; with J = 1 they are the bits of zedo_joint_stream_push with d_T = NULL on the same tensors (as the offline pair).
 * zedo_temporal_stream_push: the chunk is N = S*F frames in the layout of zedo_temporal_select - rows (h,n) h-major with
 * n = s*F + f: d_unary [H*N] float64, d_x [H*N,J,3] fp32 - stream s's chunk is a "clip" of F frames of an offline call on the same
 * tensors.  d_flush [S] int32 ON THE DEVICE (NULL: none): stream s is flushed after its chunk if d_flush[s] != 0.  F = 0 is legal
 * only with d_flush; d_unary and d_x are then unused.
 * Outputs: d_path_h [S, F+lag] int32 and d_cost [S, F+lag] float64, row r of stream s = the r-th frame this push emits for it;
 * d_emit [S,2] int64 = the clip-local index of the first emitted frame (of the next one to be emitted if the count is 0) and the
 * count.  Rows at and after the count are not written.  With t the frames the clip held before the push, the count is
 *   held = min(lag, t) + F;   count = held if the stream is flushed, else max(0, held - lag);   first = max(0, t - lag)
 * - the formula of zedo_joint_stream_push, computable on the host without reading d_emit.
 * zedo_temporal_stream_reset empties the streams with d_which[s] != 0 (d_which [S] int32 ON THE DEVICE; NULL: all of them);
 * pending frames are dropped.  The state need not be initialised before its first reset, and must have been reset before its
 * first push.
 * State (8-byte aligned), with R = lag + max_frames rows per ring, in this order:
 *   D float64 [S,R,H] | D float64 [S,H] of the clip's last frame | the clip's frame count int64 [S] |
 *   the transition costs of the current push float64 [S,max_frames,H,H] (scratch: its content between pushes is unspecified) |
 *   back int32 [S,R,H] | the dead flags of the ring's frames int32 [S,R] | the dead flag of the last frame int32 [S] |
 *   x of the clip's last frame AS THE fp32 IT ARRIVED IN [S,H,J,3] (the offline call converts x at each use: the same bits)
 * - zedo_temporal_stream_state_bytes = 8 (S R H + S H + S + S max_frames H^2) + 4 (S R H + S R + S + 3 S H J) rounded up to 8; 0
 * for shapes the calls refuse.  Frame m of a clip sits in row m % R.  A push writes the rows of its F <= max_frames frames and then
 * reads at most the lag frames before them: never a row it has overwritten (R = 1 - lag 0, max_frames 1 - included).
 * Contract: 1 <= H <= 1024 (D[t-1,.] stays in the LDS: the resident recurrence of zedo_temporal_select only), J >= 1, S >= 1,
 * max_frames >= 1, 0 <= F <= max_frames, lag >= 0, (lag + max_frames)*S*H, S*max_frames*H*H and 3*S*H*J each <= INT_MAX, finite
 * lambda >= 0; ZEDO_E_BADARG with nothing written and the state untouched for a NULL pointer other than d_flush (F > 0) and
 * d_which, a size out of these ranges, F = 0 without d_flush, a negative or non-finite lambda, or a state that is not 8-byte
 * aligned; ZEDO_E_WORKSPACE with nothing written and the state untouched if state_bytes is too small; allocates nothing,
 * synchronises nothing, enqueues on `stream` only: legal under stream capture - a replay advances the state.  No atomics: the
 * bits do not depend on the run, the chunking, the content of the state before its reset or the alignment of d_x.  Every value
 * read from the state is clamped before it is an index.  Five launches per push: the dead flags, the transition costs (parallel
 * over frame, h' and h), one workgroup per stream for the recurrence, one wave per (emitted frame, stream) for the decision - at
 * most lag dependent reads of back - and the frame counts. */
size_t zedo_temporal_stream_state_bytes(int S, int H, int J, int lag, int max_frames);
int zedo_temporal_stream_reset(void *d_state, size_t state_bytes, int S, int H, int J, int lag, int max_frames, const int *d_which,
                               void *stream);
int zedo_temporal_stream_push(const double *d_unary, const float *d_x, int S, int F, int H, int J, int lag, int max_frames,
                              double lambda, const int *d_flush, void *d_state, size_t state_bytes, int *d_path_h, double *d_cost,
                              long long *d_emit, void *stream);

/* ---- joint-wise fusion on a LIVE video WITHOUT ground truth: fixed-lag streaming sum-product ----------------------------------
 * zedo_joint_stream_push is a hard decision: one hypothesis per joint, no spread.  zedo_joint_marginal (below) gives the soft
 * answer of the same chain - posterior mean, covariance, most probable hypothesis - but needs the whole clip.  This call gives
 * that soft answer on live streams, every frame `lag` frames after it went in: fixed-lag smoothing.  Whether a few frames of lag
 * buy most of the whole-clip answer on real video is not measured; lag, lambda and tau are untuned.
 * A stream's CLIP, X, u, l, m, DEAD, "chain start", A, B, logZ and w are those of zedo_joint_marginal and
 * zedo_joint_stream_push, word for word.  A is a prefix quantity of the clip: it does not depend on how the frames were cut
 * into pushes.  With lag >= 0:
 *   frame n of a clip is EMITTED by the first push after which the clip holds frame n + lag, or by the push that flushes the
 *   stream, whichever comes first - the rule, the count and the `first` of zedo_joint_stream_push.
 *   For a live (n,j) let c_j(n) be the last frame of n's chain on the frames the clip holds after that push and
 *   e = min(n + lag, c_j(n)).  Then B[e,j,.] = 0 and logZ = LSE_h A[e,j,h]; B[m,j,.] for m = e-1 .. n by the backward recurrence
 *   of zedo_joint_marginal; w[n,j,h] = exp(A[n,j,h] + B[n,j,h] - logZ).
 *   mean, cov (from the centred differences), hmax (the lowest h with the largest w), wmax and logz follow from w exactly as
 *   zedo_joint_marginal forms them; a dead (n,j) reports that call's dead outputs.
 * In words: the outputs for frame n are those of zedo_joint_marginal on the stream's clip cut after frame n + lag.  lag = 0 gives
 * the filtering marginals, the softmax of A[n,j,.]; the outputs do not depend on the chunking; with lag >= the clip's length - 1
 * and a flush they are the offline call's, bit for bit.
 * zedo_joint_stream_marginal_push: the chunk (d_junary, d_x, d_T; rows (h,n) h-major, n = s*F + f), d_flush, F = 0 and d_emit
 * [S,2] are those of zedo_joint_stream_push.  Outputs: d_mean [S,F+lag,J,3], d_cov [S,F+lag,J,6], d_hmax (int32), d_wmax and
 * d_logz [S,F+lag,J], and the optional d_w [S,F+lag,J,H] (NULL: not written); row r of stream s = the r-th frame this push emits
 * for it.  Rows at and after the count are not written.
 * zedo_joint_stream_marginal_reset is zedo_joint_stream_reset on this state.
 * State (8-byte aligned), with R = lag + max_frames rows per ring and SJ = S*J chains, in this order:
 *   A float64 [SJ,R,H] | X float64 [SJ,R,H,3] | l float64 [SJ,R,H] | the clip's frame count int64 [S] |
 *   the dead flags of the ring's frames int32 [SJ,R] | the dead flag of the clip's last frame int32 [SJ]
 * - zedo_joint_stream_marginal_state_bytes = 8 (5 SJ R H + S) + 4 (SJ R + SJ) rounded up to 8; 0 for shapes the calls refuse.
 * Frame m of a clip sits in row m % R.  The forward step's "previous frame" is the ring's own row (t - 1) % R, read before any
 * row of the push is written; only the dead flag of the last frame has a slot of its own (with lag = 0 and F = max_frames the
 * chunk's flags have reused that row by then).  A push writes the rows of its F frames and then reads at most the lag frames
 * before them: never a row it has overwritten.
 * Contract: that of zedo_joint_stream_push - 1 <= H <= 1024, J >= 1, S >= 1, max_frames >= 1, 0 <= F <= max_frames, lag >= 0,
 * (lag + max_frames)*S*J*H <= INT_MAX, finite lambda >= 0 - and finite tau > 0; ZEDO_E_BADARG with nothing written and the
 * state untouched for a NULL pointer other than d_T, d_w, d_flush (F > 0) and d_which, a size out of these ranges, F = 0
 * without d_flush, a negative or non-finite lambda, tau <= 0 or not finite, or a state that is not 8-byte aligned;
 * ZEDO_E_WORKSPACE with nothing written and the state untouched if state_bytes is too small; allocates nothing, synchronises
 * nothing, enqueues on `stream` only: legal under stream capture - a replay advances the state.  No atomics: the bits do not
 * depend on the run, the chunking, the content of the state before its reset, the alignment of d_x or whether d_w is given.
 * Every value read from the state is clamped before it is an index.  lambda and tau are taken to be the same in every push
 * between a frame going in and coming out; otherwise the outputs are unspecified, never an address.
 * One workgroup per (stream, joint) for the forward recurrence; one workgroup per (stream, output row, joint) for the backward
 * walk, where frames of one (stream, joint) that share a horizon - a chain that ends inside the window: a flush or a dead
 * (frame, joint) - are served by ONE walk.  A whole clip pushed with lag = L - 1 and flushed costs one backward pass, as
 * offline; a steady-state push costs F walks of lag frames per (stream, joint), which is inherent in fixed-lag smoothing. */
size_t zedo_joint_stream_marginal_state_bytes(int S, int H, int J, int lag, int max_frames);
int zedo_joint_stream_marginal_reset(void *d_state, size_t state_bytes, int S, int H, int J, int lag, int max_frames,
                                     const int *d_which, void *stream);
int zedo_joint_stream_marginal_push(const double *d_junary, const float *d_x, const float *d_T, int S, int F, int H, int J,
                                    int lag, int max_frames, double lambda, double tau, const int *d_flush, void *d_state,
                                    size_t state_bytes, double *d_mean, double *d_cov, int *d_hmax, double *d_wmax,
                                    double *d_logz, double *d_w, long long *d_emit, void *stream);

/* ---- fusing hypotheses along a video WITHOUT ground truth: per-joint posterior mean and spread ------------------------------
 * zedo_joint_temporal_select answers with one hypothesis per (frame, joint) and says nothing of the others.  This is the
 * sum-product twin of its max-product recurrence: the same energy read as a probability at a temperature tau,
 *   p(path of joint j over a chain) proportional to exp(-(sum_n u[n,j,h_n] + lambda sum_n m[n,j,h_{n-1},h_n]) / tau),
 * and from it, exactly (forward-backward in the log domain), the posterior marginal of every hypothesis of every (frame,
 * joint), the posterior mean position, its covariance - the spread of the hypotheses in metres, weighted by what the model
 * believes - and the most probable hypothesis with its probability.  Whether the fused pose is closer to ground truth than a
 * selected one on real video is not measured.
 * Inputs: exactly those of zedo_joint_temporal_select - d_junary [H*N,J] float64 rows (h,n) ALL rows, d_x [H*N,J,3] and d_T
 * [H*N,3] fp32 (d_T may be NULL), d_seq_start [n_seq+1] int32 ON THE DEVICE, every entry clamped to 0 .. N before use and
 * never an address - and tau > 0, the temperature in cost units (pixels on zedo_joint_reproj's distances).
 * All arithmetic in float64.  X, u, m, DEAD and "chain start" are those of zedo_joint_temporal_select, word for word: a
 * non-finite unary excludes that hypothesis for that joint; a (frame, joint) with no finite unary is dead and splits only that
 * joint's chain.  With l[n,j,h] = -u[n,j,h] / tau (-inf when excluded), c = lambda / tau, LSE the log of a sum of exponentials:
 *   forward   chain start:  A[n,j,h] = l[n,j,h]
 *             otherwise:    A[n,j,h] = l[n,j,h] + LSE_h' (A[n-1,j,h'] - c m[n,j,h',h])
 *   backward  chain end (the clip's last frame, or (n+1,j) dead):  B[n,j,h] = 0  and  logZ = LSE_h A[n,j,h]
 *             otherwise:    B[n,j,h] = LSE_h' (l[n+1,j,h'] + B[n+1,j,h'] - c m[n+1,j,h,h'])
 *   marginal  w[n,j,h] = exp(A[n,j,h] + B[n,j,h] - logZ);  an excluded hypothesis has w = 0 exactly
 * Every LSE is evaluated shifted by the TRUE maximum of its terms (two walks over the terms; where the h' are split over parts
 * of a workgroup, each part shifts by its own maximum and the parts are combined shifted by the largest): safe for any finite
 * c m, and at a small tau the largest term contributes exactly 1.  (lambda / tau and u / tau are taken to be finite.)
 * Outputs (all required but d_w):
 *   d_mean [N,J,3]  sum_h w X, camera frame (metres)
 *   d_cov  [N,J,6]  sum_h w (X - mean)(X - mean)^T in the order xx, xy, xz, yy, yz, zz (m^2), from the centred differences
 *   d_hmax [N,J] int32  the lowest h with the largest marginal;  d_wmax [N,J]  that marginal
 *   d_logz [N,J]    the chain's log-partition value logZ, repeated on every frame of the chain
 *   d_w    [N,J,H]  optional (NULL: not written): the marginals
 * A dead (frame, joint) reports NaN in mean and cov, hypothesis 0, wmax = 0, logz = -inf and a row of zeros in d_w.
 * Workspace (8-byte aligned, need not be initialised): A [N,J,H] float64 and one int32 flag per (frame, joint) -
 * zedo_joint_marginal_workspace_bytes(N, H, J); 0 for sizes the call refuses.  B never leaves the LDS.
 * Contract: that of zedo_joint_temporal_select - J >= 1, N >= 1, 1 <= n_seq <= N, 1 <= H <= 1024, N*J*H <= INT_MAX, finite
 * lambda >= 0 - and finite tau > 0; ZEDO_E_BADARG with nothing written for a NULL pointer other than d_T and d_w, a
 * non-positive size, H > 1024, n_seq > N, N*J*H above INT_MAX, a negative or non-finite lambda, tau <= 0 or not finite, or a
 * workspace that is not 8-byte aligned; ZEDO_E_WORKSPACE with nothing written if workspace_bytes is too small; allocates
 * nothing, synchronises nothing, enqueues on `stream` only: legal under stream capture; no atomics, every sum in a fixed
 * order: bit-identical from run to run, for any alignment of d_x and any workspace content, with and without d_w.  One
 * workgroup per (clip, joint), twice: a single long clip is serial in time on J CUs. */
size_t zedo_joint_marginal_workspace_bytes(int N, int H, int J);
int zedo_joint_marginal(const double *d_junary, const float *d_x, const float *d_T, const int *d_seq_start, int n_seq,
                        int H, int N, int J, double lambda, double tau, void *d_workspace, size_t workspace_bytes,
                        double *d_mean, double *d_cov, int *d_hmax, double *d_wmax, double *d_logz, double *d_w, void *stream);

/* ---- fusing WHOLE hypotheses along a video WITHOUT ground truth: posterior mean pose and spread ----------------------------
 * zedo_temporal_select answers with one hypothesis index per frame: it cannot say how sure it is, and the selected pose jumps
 * where the index changes.  This is the sum-product twin of its max-product recurrence, exactly as zedo_joint_marginal is the
 * twin of zedo_joint_temporal_select: the same energy read as a probability at a temperature tau,
 *   p(path over a chain) proportional to exp(-(sum_n u[n,h_n] + lambda sum_n m[n,h_{n-1},h_n]) / tau),
 * and from it, exactly (forward-backward in the log domain), the posterior marginal of every hypothesis of every frame - a
 * state is a whole pose the network produced, with real bone lengths -, the posterior mean pose, the covariance of every joint
 * under those marginals and the most probable hypothesis with its probability.  Whether the fused pose is closer to ground
 * truth than a selected one on real video is UNMEASURED; lambda = 100 and tau = 1, the binding's defaults, are UNTUNED.
 * Inputs: d_unary [H*N] float64, d_x [H*N,J,3] fp32 and d_seq_start [n_seq+1] int32 ON THE DEVICE are those of
 * zedo_temporal_select, word for word: rows (h,n) h-major, ALL rows; every entry of d_seq_start is clamped to 0 .. N before use
 * and is never an address, and with an array that breaks its rules the result is unspecified.  tau: finite, > 0, the
 * temperature in cost units (pixels on zedo_min_reproj's errors).  d_T [H*N,3] fp32 is optional and enters ONLY the position
 * the moments are taken of, X[h,n,j,c] = (double)x[h,n,j,c] + (double)T[h,n,c] (x alone when it is NULL) - not the motion
 * term, which stays that of zedo_temporal_select.
 * All arithmetic in float64.  u, DEAD, "chain start" and m[n,h',h] = (1/J) sum_j sqrt(sum_c (x[h,n,j,c] - x[h',n-1,j,c])^2)
 * (sums ascending in c, then in j) are those of zedo_temporal_select.  With l[n,h] = -u[n,h] / tau (-inf when the hypothesis is
 * excluded), c = lambda / tau, LSE the log of a sum of exponentials:
 *   forward   chain start:  A[n,h] = l[n,h]
 *             otherwise:    A[n,h] = l[n,h] + LSE_h' (A[n-1,h'] - c m[n,h',h])
 *   backward  chain end (the clip's last frame, or frame n+1 dead):  B[n,h] = 0  and  logZ = LSE_h A[n,h]
 *             otherwise:    B[n,h] = LSE_h' (l[n+1,h'] + B[n+1,h'] - c m[n+1,h,h'])
 *   marginal  w[n,h] = exp((A[n,h] + B[n,h]) - logZ);  an excluded hypothesis has w = 0 exactly
 * Every LSE takes two walks over its terms and is shifted by their TRUE maximum: safe for any finite c m, and at a small tau
 * the largest term contributes exactly 1.  (lambda / tau and u / tau are taken to be finite.)  Every sum runs in a fixed order:
 * the LSE of a recurrence over h' ascending, by the one lane that owns h (no split to combine); logZ over the workgroup of
 * T = min(256, H rounded up to 64) lanes - lane t adds h = t, t + T, .. ascending, then a butterfly inside each wave of 64
 * (offsets 32, 16, .. 1), then the waves ascending; the mean and the covariance over h ascending, by one lane per (frame,
 * joint).
 * Outputs (all required but d_w):
 *   d_mean [N,J,3]  sum_h w X (metres; the frame of x, or of x + T)
 *   d_cov  [N,J,6]  sum_h w (X - mean)(X - mean)^T in the order xx, xy, xz, yy, yz, zz (m^2), from the centred differences
 *   d_hmax [N] int32  the lowest h with the largest marginal;  d_wmax [N]  that marginal
 *   d_logz [N]      the chain's log-partition value logZ, repeated on every frame of the chain
 *   d_w    [N,H]    optional (NULL: not written, and every other output keeps its bits): the marginals
 * A dead frame reports NaN in mean and cov, hypothesis 0, wmax = 0, logz = -inf and a row of zeros in d_w.
 * Workspace (8-byte aligned, need not be initialised): A [N,H] float64, B [N,H] float64 (overwritten by the marginals at the
 * end), logZ [N] float64, one int32 flag per frame (padded to 8 bytes), then C*H*H float64 transition costs of a chunk of C
 * frames.  zedo_temporal_marginal_workspace_bytes(N, H, chunk_frames) returns the bytes for C = min(chunk_frames, N);
 * chunk_frames <= 0: the largest C whose transition costs stay at or under 256 MB (at least one frame); 0 for sizes the call
 * refuses.  The call uses the largest C that workspace_bytes admits, capped at N, and returns the SAME BITS for every C: A, B
 * and logZ of every frame live in the workspace, and what crosses a chunk boundary - A of the frame before, B of the frame
 * after, the chain's logZ - goes through them.  The forward pass walks the chunks ascending, the backward pass DESCENDING, and
 * the backward pass computes the transition costs of its chunk AGAIN, in the transposed layout its lanes read coalesced (the
 * same bits: (a - b)^2 = (b - a)^2 exactly, and the joint order is unchanged): every transition cost is computed twice,
 * whatever C is.  That is the price of a workspace that holds one chunk of them.
 * Contract: 1 <= H <= 1024 (A[n-1,.] stays in the LDS: the resident recurrence only, as zedo_temporal_stream_push), J >= 1,
 * N >= 1, 1 <= n_seq <= N, finite lambda >= 0, finite tau > 0; ZEDO_E_BADARG with nothing written for a NULL pointer other
 * than d_T and d_w, a non-positive size, H > 1024, n_seq > N, H*N (or N*J: one lane per (frame, joint)) above INT_MAX, a
 * negative or non-finite lambda, tau <= 0 or not finite, or a workspace that is not 8-byte aligned; ZEDO_E_WORKSPACE with
 * nothing written if not even one frame of transition costs fits; allocates nothing, synchronises nothing, enqueues on
 * `stream` only: legal under stream capture; no atomics: bit-identical from run to run, for any alignment of d_x and any
 * workspace content, with and without d_w.  One workgroup per clip, twice: a single long clip is serial in time on one CU,
 * as in zedo_temporal_select.  The moments are parallel over (frame, joint) and read d_x twice (the mean, then the centred
 * differences). */
size_t zedo_temporal_marginal_workspace_bytes(int N, int H, int chunk_frames);
int zedo_temporal_marginal(const double *d_unary, const float *d_x, const float *d_T, const int *d_seq_start, int n_seq,
                           int H, int N, int J, double lambda, double tau, void *d_workspace, size_t workspace_bytes,
                           double *d_mean, double *d_cov, int *d_hmax, double *d_wmax, double *d_logz, double *d_w, void *stream);

/* ---- joint-wise selection along a video WITHOUT ground truth: a second-order motion model ----------------------------------
 * zedo_joint_temporal_select charges lambda times the DISPLACEMENT of a joint between consecutive choices: a zero-velocity
 * prior.  Real motion is common to all hypotheses and enters under the square root, so the faster a limb moves the cheaper a
 * switch between hypotheses becomes.  This call adds lambda_a times the SECOND DIFFERENCE X[n] - 2 X[n-1] + X[n-2], which is
 * blind to a constant velocity.  The state of a chain is then a PAIR of hypotheses: H^2 states and H^3 transitions per
 * (frame, joint).  Whether this lowers the error against ground truth on real video is not measured.
 * Inputs: exactly those of zedo_joint_temporal_select - d_junary [H*N,J] float64 rows (h,n) ALL rows, d_x [H*N,J,3] and d_T
 * [H*N,3] fp32 (d_T may be NULL), d_seq_start [n_seq+1] int32 ON THE DEVICE, every entry clamped to 0 .. N before use and
 * never an address - and two weights in cost units per metre: lambda_v on the displacement, lambda_a on the second difference.
 * All arithmetic in float64, independent for every joint j.  X, u, m and DEAD are those of zedo_joint_temporal_select, word
 * for word; a CHAIN is a maximal run c0 .. c1-1 of frames of one clip at which (n,j) is not dead.
 *   a[n,j,h'',h',h] = sqrt(e0^2 + e1^2 + e2^2),  e_c = (X[n,h,j,c] - 2 X[n-1,h',j,c]) + X[n-2,h'',j,c]
 *                     (the product by 2, the difference, the sum; then the squares and their sum ascending in c)
 *   c1 - c0 == 1:  path[c0] = the lowest h that minimises u[c0,j,.]
 *   n == c0+1:     E[n][h',h] = u[n-1,j,h'] + (u[n,j,h] + lambda_v m[n,j,h',h])
 *   n >= c0+2:     E[n][h',h] = u[n,j,h] + (lambda_v m[n,j,h',h] + min_h'' (E[n-1][h'',h'] + lambda_a a[n,j,h'',h',h])),
 *                  back2[n][h',h] = the lowest h'' that attains the minimum (strict comparison, h'' ascending)
 *   end of chain:  (h',h) = the pair with the smallest E[c1-1], ties to the lowest h' H + h;  path[c1-1] = h, path[c1-2] = h',
 *                  and downwards path[n-2] = back2[n][path[n-1], path[n]]
 * d_path_h [N,J] int32.  d_cost [N,J] float64 is the cost of the kept path RE-ACCUMULATED along it, with p_n = path[n,j]:
 *   cost[c0] = u[c0,j,p]
 *   cost[c0+1] = cost[c0] + (u[n,j,p_n] + lambda_v m[n,j,p_{n-1},p_n])
 *   cost[n] = cost[n-1] + (u[n,j,p_n] + (lambda_v m[n,j,p_{n-1},p_n] + lambda_a a[n,j,p_{n-2},p_{n-1},p_n]))   for n >= c0+2
 * - E is not kept for all frames (that would be 8 N J H^2 bytes), so cost[c1-1] equals the minimum of E[c1-1] up to the
 * rounding of a different order of the same additions.  A dead (frame, joint) reports hypothesis 0 and cost +inf and splits
 * only that joint's chain.  With lambda_a == 0 the paths are those of zedo_joint_temporal_select wherever its minima are
 * unique beyond rounding.  (x and T are taken to be finite, as there.)
 * Workspace (8-byte aligned, need not be initialised): back2 as one byte per (frame, joint, h', h), rounded up to 4 bytes, and
 * two int32 flags per (frame, joint) - zedo_joint_accel_workspace_bytes(N, H, J); 0 for sizes the call refuses.  That is 43 MB
 * at 1 015 frames x 17 joints x 50^2 and 3.0 GB at 70 880 frames: cut a long recording into calls of whole clips.
 * Contract: J >= 1, N >= 1, 1 <= n_seq <= N, 1 <= H <= 64 (the pair table of one joint, 8 H^2 bytes, stays in the LDS), N*J*H
 * <= INT_MAX, finite lambda_v >= 0 and lambda_a >= 0; ZEDO_E_BADARG with nothing written for a NULL pointer other than d_T, a
 * non-positive size, H > 64, n_seq > N, N*J*H above INT_MAX, a negative or non-finite lambda_v or lambda_a, or a workspace
 * that is not 8-byte aligned; ZEDO_E_WORKSPACE with nothing written if workspace_bytes is too small; allocates nothing,
 * synchronises nothing, enqueues on `stream` only: legal under stream capture; no atomics: bit-identical from run to run.
 * One workgroup per (clip, joint): a single long clip is serial in time on J CUs. */
size_t zedo_joint_accel_workspace_bytes(int N, int H, int J);
int zedo_joint_accel_select(const double *d_junary, const float *d_x, const float *d_T, const int *d_seq_start, int n_seq,
                            int H, int N, int J, double lambda_v, double lambda_a, void *d_workspace, size_t workspace_bytes,
                            int *d_path_h, double *d_cost, void *stream);

/* ---- the second-order model on a LIVE video: fixed-lag streaming Viterbi over pairs -----------------------------------------
 * zedo_joint_stream_push serves live input with the first-order chain, whose motion term gets cheaper the faster a limb moves;
 * zedo_joint_accel_select fixes that but needs the whole clip.  This is zedo_joint_accel_select's chain over pairs as an online
 * call for S independent streams: frames are pushed in chunks of any size, the tables live in d_state between the calls, and the
 * decision for a frame comes out `lag` frames after the frame went in.  lambda_v, lambda_a and the lag are UNTUNED; accuracy on
 * real video is UNMEASURED.
 * The chunk (d_junary, d_x, d_T; rows (h,n) h-major, n = s*F + f), d_flush, d_which, d_emit [S,2], the emitted count and the
 * `first` emitted frame, F = 0 being legal only with d_flush, rows at and after the count not being written, a dead (n,j)
 * reporting hypothesis 0 and cost +inf, and the frame after a flush being t = 0 of a new clip are those of
 * zedo_joint_stream_push, word for word.  X, u, m, a, DEAD, "chain", E, back2 and the tie rules are those of
 * zedo_joint_accel_select on the stream's clip, word for word: prefix quantities, which do not depend on the chunking.
 *   For a live (n,j) let c_j(n) be the last frame of n's chain on the frames the clip holds after the push that emits n, c0 the
 *   chain's first frame, and e = min(n + lag, c_j(n)).  Then
 *     e == c0 (a chain of one frame so far):  path[n,j] = the lowest h that minimises u[e,j,.];  cost[n,j] = that minimum
 *     otherwise:  (h',h) = the pair with the smallest E[e], ties to the lowest h' H + h;  p_e = h, p_{e-1} = h';
 *                 p_{m-2} = back2[m][p_{m-1}, p_m] for m = e .. n+2;  path[n,j] = p_n;  cost[n,j] = min E[e]
 * d_cost is the cost of the best path on the clip cut after e, a path that passes through path[n,j].  It is deliberately NOT
 * the re-accumulated cost of zedo_joint_accel_select: fixed-lag decisions of consecutive frames need not lie on one path, so
 * there is no path to re-accumulate along.
 * So the decision for frame n is the path of zedo_joint_accel_select on the clip cut after frame n + lag; lag = 0 gives the h of
 * the arg-min pair of E[n]; the outputs do not depend on the chunking; with lag >= the clip's length - 1 and a flush the paths
 * are the offline call's bits.
 * Outputs: d_path_h [S, F+lag, J] int32, d_cost [S, F+lag, J] float64, d_emit [S,2] int64, as zedo_joint_stream_push.
 * zedo_joint_accel_stream_reset is zedo_joint_stream_reset on this state.
 * State (8-byte aligned, need not be initialised before its first reset, must have been reset before its first push), with
 * R = lag + max_frames rows per ring, SJ = S*J chains and HH = H*H, in this order:
 *   one 16-byte record per frame of the ring [SJ,R]: min E (a chain's first frame: min u) float64, the arg-min pair h' H + h (a
 *   chain's first frame: h) int32, the frame's kind (0 dead, 1 first of a chain, 2 inside one) int32 | one block of HH + 7 H + 1
 *   float64 per chain [SJ]: E [HH], X [H,3] of the clip's last frame, X [H,3] of the one before, u [H] of the last frame, and the
 *   dead flags of those two frames as two int32 | the clip's frame count int64 [S] | the dead flags of the ring's frames int32
 *   [SJ,R] | back2, one byte per pair, uint8 [SJ,R,HH]
 * - zedo_joint_accel_stream_state_bytes = 8 (SJ R + SJ HH + 7 SJ H + S) + 4 (3 SJ R + 2 SJ) + SJ R HH rounded up to 8; 0 for
 * shapes the calls refuse.  That is 27 MB at S = 16, J = 17, H = 50, lag = 30, max_frames = 1.  E is not kept for the ring's
 * frames (8 HH bytes per frame).  Frame m of a clip sits in row m % R.  A push writes the rows of its F <= max_frames frames and
 * then reads at most the lag frames before them: never a row it has overwritten.  The flags of the two frames before a chunk
 * have slots of their own (with lag = 0 and F = max_frames the chunk has reused their rows).
 * Contract: 1 <= H <= 64 (the pair table stays in the LDS), J >= 1, S >= 1, max_frames >= 1, 0 <= F <= max_frames, lag >= 0,
 * (lag + max_frames)*S*J*H*H <= INT_MAX, finite lambda_v >= 0 and lambda_a >= 0; ZEDO_E_BADARG with nothing written and the
 * state untouched for a NULL pointer other than d_T, d_flush (F > 0) and d_which, a size out of these ranges, H > 64, F = 0
 * without d_flush, a negative or non-finite lambda_v or lambda_a, or a state that is not 8-byte aligned; ZEDO_E_WORKSPACE with
 * nothing written and the state untouched if state_bytes is too small; allocates nothing, synchronises nothing, enqueues on
 * `stream` only: legal under stream capture - a replay advances the state.  No atomics, no scratch: the bits do not depend on
 * the run, the chunking, the content of the state before its reset or the alignment of d_x.  Every value read from the state is
 * clamped before it is an index.  lambda_v and lambda_a are taken to be the same in every push between a frame going in and
 * coming out.  One workgroup per (stream, joint) for the recurrence - the H^3 walk of zedo_joint_accel_select plus one block
 * reduction per live frame; one wave per (emitted frame, stream, joint) for the decision: at most max(0, lag - 1) dependent
 * reads of back2. */
size_t zedo_joint_accel_stream_state_bytes(int S, int H, int J, int lag, int max_frames);
int zedo_joint_accel_stream_reset(void *d_state, size_t state_bytes, int S, int H, int J, int lag, int max_frames,
                                  const int *d_which, void *stream);
int zedo_joint_accel_stream_push(const double *d_junary, const float *d_x, const float *d_T, int S, int F, int H, int J,
                                 int lag, int max_frames, double lambda_v, double lambda_a, const int *d_flush, void *d_state,
                                 size_t state_bytes, int *d_path_h, double *d_cost, long long *d_emit, void *stream);

/* ---- fusing hypotheses along a video under the second-order motion model: exact sum-product over pairs ----------------------
 * The soft answer of zedo_joint_accel_select, as zedo_joint_marginal is the soft answer of zedo_joint_temporal_select: the same
 * energy read as a probability at a temperature tau,
 *   p(path of joint j over a chain) proportional to exp(-(sum u + lambda_v sum m + lambda_a sum a) / tau),
 * and from it, exactly (forward-backward over PAIRS of hypotheses in the log domain), the posterior marginal of every
 * hypothesis of every (frame, joint), the posterior mean position, its covariance and the most probable hypothesis.  The
 * marginals of zedo_joint_marginal spread over more hypotheses the faster a limb moves (its motion term is a zero-velocity
 * prior); these are blind to a constant velocity at lambda_v = 0.  The defaults of the bindings (lambda_v = lambda_a = 100, tau
 * = 1) are untuned, and whether the fused pose is closer to ground truth than any other on real video is not measured.
 * Inputs, X, u, m, a, DEAD, the chains (a maximal run c0 .. c1-1 of live frames of one joint inside a clip) and the exclusion of
 * a hypothesis with a non-finite unary, for that joint only, are those of zedo_joint_accel_select, word for word; tau > 0 is
 * the temperature in cost units.  All arithmetic in float64, independent for every joint j.  With l[n,h] = -u[n,j,h] / tau (-inf
 * when excluded), c_v = lambda_v / tau, c_a = lambda_a / tau, LSE the log of a sum of exponentials:
 *   c1 - c0 == 1:   w[c0,h] = exp(l[c0,h] - logZ),  logZ = LSE_h l[c0,h]
 *   n == c0+1:      A2[n][h',h] = l[n-1,h'] + (l[n,h] - c_v m[n,h',h])
 *   n >= c0+2:      A2[n][h',h] = l[n,h] + (-c_v m[n,h',h] + LSE_h'' (A2[n-1][h'',h'] - c_a a[n,h'',h',h]))
 *   chain end:      B2[c1-1] = 0  and  logZ = LSE over all pairs (h',h) of A2[c1-1][h',h]
 *   below it:       M[h+][h] = (l[n+1,h+] - c_v m[n+1,h,h+]) + B2[n+1][h,h+],
 *                   B2[n][h',h] = LSE_h+ (M[h+][h] - c_a a'[n+1,h',h,h+])
 *   pair marginal:  pi[n][h',h] = exp((A2[n][h',h] + B2[n][h',h]) - logZ)
 *   marginal:       w[n,h] = sum_h' pi[n][h',h] for n >= c0+1;  w[c0,h'] = sum_h pi[c0+1][h',h]
 * Every sum over a hypothesis index runs ascending; logZ of a chain of two frames or more adds exp(A2 - max) over the pairs a
 * lane owns in ascending q = h' H + h (q = lane, lane + 256, ..), then a butterfly over the 64 lanes of a wave, then the four
 * waves in ascending order.  Every LSE is evaluated shifted by the TRUE maximum of its terms (two walks over the terms): at a
 * small tau the largest term contributes exactly 1 and nothing that matters underflows.  An excluded hypothesis has w = 0
 * exactly.  a is the term of zedo_joint_accel_select, e_c = (X[n,h] - 2 X[n-1,h']) + X[n-2,h''], in the forward pass; the
 * backward pass forms a' with e_c = (X[n-1,h'] - 2 X[n,h]) + X[n+1,h+]: the same second difference in another association,
 * one rounding apart; the error bound of tests/_joint_accel_marginal_ref.py covers either.
 * Outputs and a dead (frame, joint) are those of zedo_joint_marginal, word for word: d_mean [N,J,3]; d_cov [N,J,6] from the
 * centred differences; d_hmax [N,J] int32, the lowest h with the largest marginal; d_wmax [N,J]; d_logz [N,J], repeated on
 * every frame of the chain; d_w [N,J,H] optional (NULL: not written); a dead (frame, joint) reports NaN in mean and cov,
 * hypothesis 0, wmax = 0, logz = -inf and a row of zeros in d_w.
 * Workspace (8-byte aligned, need not be initialised): A2 as [J,N,H,H] float64 - the frames of one chain are contiguous - and
 * one int32 flag per (frame, joint), padded to 8 bytes: zedo_joint_accel_marginal_workspace_bytes(N, H, J) = 8 N J H^2 +
 * pad8(4 N J); 0 for sizes the call refuses.  That is 345 MB at 1 015 frames x 17 joints x 50^2: cut a long recording into
 * calls of whole clips (the chains of different clips are independent).  B2, M and pi never leave the LDS.
 * Contract: that of zedo_joint_accel_select - J >= 1, N >= 1, 1 <= n_seq <= N, 1 <= H <= 64, N*J*H <= INT_MAX, finite
 * lambda_v >= 0 and lambda_a >= 0 - and finite tau > 0; ZEDO_E_BADARG with nothing written for a NULL pointer other than d_T
 * and d_w, a non-positive size, H > 64, n_seq > N, N*J*H above INT_MAX, a negative or non-finite lambda_v or lambda_a, tau <= 0
 * or not finite, or a workspace that is not 8-byte aligned; ZEDO_E_WORKSPACE with nothing written if workspace_bytes is too
 * small; allocates nothing, synchronises nothing, enqueues on `stream` only: legal under stream capture; no atomics, every sum
 * in a fixed order: bit-identical from run to run, for any alignment of d_x and any workspace content, with and without d_w.
 * One workgroup per (clip, joint), twice: a single long clip is serial in time on J CUs. */
size_t zedo_joint_accel_marginal_workspace_bytes(int N, int H, int J);
int zedo_joint_accel_marginal(const double *d_junary, const float *d_x, const float *d_T, const int *d_seq_start, int n_seq,
                              int H, int N, int J, double lambda_v, double lambda_a, double tau,
                              void *d_workspace, size_t workspace_bytes,
                              double *d_mean, double *d_cov, int *d_hmax, double *d_wmax, double *d_logz, double *d_w, void *stream);

/* ---- second-order fusion on a LIVE video: fixed-lag streaming sum-product over pairs ----------------------------------------
 * zedo_joint_stream_marginal_push is the only soft answer on live input, and its motion term is a zero-velocity prior: the
 * faster a limb moves, the more hypotheses share the mass.  zedo_joint_accel_marginal fixes that but needs the whole clip.  This
 * is zedo_joint_accel_marginal's chain over pairs as an online call for S independent streams: frames are pushed in chunks of
 * any size, the tables live in d_state between the calls, and a frame's marginals come out `lag` frames after the frame went in.
 * lambda_v, lambda_a, tau and the lag are UNTUNED; accuracy on real video is UNMEASURED.
 * The chunk (d_junary, d_x, d_T; rows (h,n) h-major, n = s*F + f), d_flush, d_which, d_emit [S,2], the emitted count and the
 * `first` emitted frame, F = 0 being legal only with d_flush, rows at and after the count not being written, the outputs d_mean
 * [S,F+lag,J,3], d_cov [S,F+lag,J,6], d_hmax (int32), d_wmax and d_logz [S,F+lag,J] and the optional d_w [S,F+lag,J,H] (NULL:
 * not written), and the outputs of a dead (n,j) are those of zedo_joint_stream_marginal_push, word for word.  X, u, l, m, a, a',
 * DEAD, the chains, A2, B2, M, pi, the order of every sum and the exclusion of a hypothesis are those of
 * zedo_joint_accel_marginal on the stream's clip, word for word; A2 is a prefix quantity, which does not depend on the chunking.
 *   For a live (n,j) let c0 be the first frame of n's chain, c_j(n) the chain's last frame on the frames the clip holds after
 *   the push that emits n, and e = min(n + lag, c_j(n)).  Then
 *     e == c0 (a chain of one frame so far):  logZ = LSE_h l[e,h]  and  w[n,h] = exp(l[n,h] - logZ)
 *     otherwise:  B2[e] = 0 and logZ = LSE over all pairs of A2[e], in the order zedo_joint_accel_marginal takes;
 *                 B2[m] for m = e-1 .. max(n, c0+1) by the backward recurrence;  pi[m] = exp((A2[m] + B2[m]) - logZ);
 *                 w[n,h] = sum_h' pi[n][h',h] for n >= c0+1;  w[c0,h'] = sum_h pi[c0+1][h',h];  both sums ascending
 *   d_logz is that logZ; mean, cov, hmax and wmax follow from w exactly as zedo_joint_accel_marginal forms them.
 * In words: the outputs for frame n are those of zedo_joint_accel_marginal on the stream's clip cut after frame n + lag.  lag =
 * 0 gives the filtering marginals, the column sums of the softmax of A2[n]; the outputs do not depend on the chunking; with
 * lag >= the clip's length - 1 and a flush they are the offline call's bits; on a clip cut short, at any lag, they are the
 * bits of the offline call on that cut.
 * zedo_joint_accel_stream_marginal_reset is zedo_joint_stream_reset on this state.
 * State (8-byte aligned, need not be initialised before its first reset, must have been reset before its first push), with
 * R = lag + max_frames + 2 rows per ring, SJ = S*J chains and HH = H*H, in this order:
 *   A2 float64 [SJ,R,HH] | X float64 [SJ,R,H,3] | l float64 [SJ,R,H] | the clip's frame count int64 [S] |
 *   the dead flags of the ring's frames int32 [SJ,R]
 * - zedo_joint_accel_stream_marginal_state_bytes = 8 (SJ R (HH + 4 H) + S) + 4 SJ R rounded up to 8; 0 for shapes the calls
 * refuse.  That is 194 MB at S = 16, J = 17, H = 50, lag = 30, max_frames = 1, where zedo_joint_accel_stream_push holds 27 MB:
 * the pair table of every frame in the window stays, 8 HH bytes per frame.  Frame m of a clip sits in row m % R.  The two extra
 * rows stand where the sibling streams carry blocks of their own: with t the clip's frames before a push of F <= max_frames
 * frames, the push writes the rows of frames t .. t+F-1 (their dead flags first); its forward step reads A2, X, l and the flag
 * of frame t-1 and X and the flag of frame t-2; its emission reads frames >= max(0, t - lag) and X of the frame before the
 * lowest of them, t - lag - 1.  The lowest frame read is t - lag - 1 (lag >= 1) or t - 2 (lag = 0); the highest written is
 * t + F - 1; their distance is F + lag <= R - 2 or F + 1 <= R - 1: below R, so no row that is read has been overwritten, with
 * lag = 0 and F = max_frames as well.
 * Contract: that of zedo_joint_accel_stream_push plus tau - 1 <= H <= 64, J >= 1, S >= 1, max_frames >= 1, 0 <= F <=
 * max_frames, lag >= 0, (lag + max_frames + 2)*S*J*H*H <= INT_MAX, finite lambda_v >= 0 and lambda_a >= 0, finite tau > 0;
 * ZEDO_E_BADARG with nothing written and the state untouched for a NULL pointer other than d_T, d_w, d_flush (F > 0) and
 * d_which, a size out of these ranges, H > 64, F = 0 without d_flush, a negative or non-finite lambda_v or lambda_a, tau <= 0
 * or not finite, or a state that is not 8-byte aligned; ZEDO_E_WORKSPACE with nothing written and the state untouched if
 * state_bytes is too small; allocates nothing, synchronises nothing, enqueues on `stream` only: legal under stream capture - a
 * replay advances the state.  No atomics, no scratch: the bits do not depend on the run, the chunking, the content of the state
 * before its reset, the alignment of d_x or whether d_w is given.  Every value read from the state is clamped before it is an
 * index.  lambda_v, lambda_a and tau are taken to be the same in every push between a frame going in and coming out.
 * One workgroup per (stream, joint) for the forward recurrence; one workgroup per (stream, output row, joint) for the backward
 * walk, 104.7 KB of LDS each (one per CU), where frames of one (stream, joint) that share a closed horizon - a flush or a dead
 * (frame, joint) - are served by ONE walk.  A whole clip pushed with lag = L - 1 and flushed costs one backward pass, as
 * offline; a steady-state push costs F walks of lag frames per (stream, joint), which is inherent in fixed-lag smoothing. */
size_t zedo_joint_accel_stream_marginal_state_bytes(int S, int H, int J, int lag, int max_frames);
int zedo_joint_accel_stream_marginal_reset(void *d_state, size_t state_bytes, int S, int H, int J, int lag, int max_frames,
                                           const int *d_which, void *stream);
int zedo_joint_accel_stream_marginal_push(const double *d_junary, const float *d_x, const float *d_T, int S, int F, int H, int J,
                                          int lag, int max_frames, double lambda_v, double lambda_a, double tau,
                                          const int *d_flush, void *d_state, size_t state_bytes,
                                          double *d_mean, double *d_cov, int *d_hmax, double *d_wmax, double *d_logz, double *d_w,
                                          long long *d_emit, void *stream);

/* ---- skeleton-coupled joint-wise aggregation WITHOUT ground truth: exact min-sum over the bone tree ------------------------
 * zedo_joint_reproj picks every joint of a pose on its own, and the chain models above couple a joint to itself along time.
 * A pose assembled by zedo_joint_compose can therefore take the two ends of a bone from different depth solutions; the bone
 * then has a length no hypothesis has.  This call couples a joint to its neighbours in the skeleton, per pose: the assembled
 * bone should be as long as the two hypotheses that supply its ends say this bone is.  A pose taken whole from one hypothesis
 * pays nothing.  The skeleton is a tree, so the minimum is exact: min-sum dynamic programming from the leaves to the roots.
 * Whether this lowers the error against ground truth is not measured.
 * Inputs: d_junary [H*N,J] float64, rows (h,n) h-major, ALL rows: any per-(row, joint) cost, e.g. d_jerr of zedo_joint_reproj
 * (pixels).  d_x [H*N,J,3] fp32 and d_T [H*N,3] fp32 or NULL, the same rows (metres).  d_weight [N,J] fp32 or NULL: a
 * confidence per (pose, joint).  h_parent [J] int32 ON THE HOST, read during the call (as h_keylist of zedo_ipo_fit is): any
 * forest - parent[j] in -1 .. J-1, never j itself, no cycle, at least one -1.  The host derives the processing order
 * (post-order, children in ascending index) and hands it to the kernel by value: no device allocation, no copy.  mu: cost
 * units per metre of bone mismatch.
 * Per pose n, independent of every other pose, all arithmetic in float64 on the inputs as given:
 *   X[n,h,j,c]  = (double)x[h*N+n,j,c] + (d_T ? (double)T[h*N+n,c] : 0.0)
 *   w[n,j]      = d_weight ? (double)clamp(weight[n,j], 1e-4f, 1.0f) : 1.0   (the clamp in fp32, as zedo_min_reproj takes it)
 *   u[n,j,h]    = w[n,j] * junary[(h*N+n)*J+j] if that product is finite, else +inf (the hypothesis is excluded for that joint);
 *                 (n,j) is DEAD if no u[n,j,h] is finite
 * For a joint g with parent p = parent[g] >= 0:
 *   own[n,g,h]      = sqrt(e0^2+e1^2+e2^2),  e_c = X[n,h,g,c]  - X[n,h,p,c]        (products, then the sum ascending in c)
 *   mix[n,g,hp,hc]  = sqrt(d0^2+d1^2+d2^2),  d_c = X[n,hc,g,c] - X[n,hp,p,c]
 *   b[n,g,hp,hc]    = | mix[n,g,hp,hc] - 0.5 * (own[n,g,hc] + own[n,g,hp]) |        metres; exactly 0 when hc == hp
 *   energy(assignment h_.) = sum_j u[n,j,h_j] + mu * sum_{g: parent live} b[n,g,h_p,h_g]
 * The recurrence, children before parents and siblings in ascending index:
 *   S[j,h] starts as u[n,j,h]
 *   for a live g with a live parent p:  M_g[hp] = min_hc (S[g,hc] + mu * b[n,g,hp,hc]),  back[g,hp] = the lowest hc that
 *       attains it,  S[p,hp] += M_g[hp]
 *   a ROOT is a live joint with parent -1 or with a dead parent:  h_root = the lowest arg-min of S[root,.]
 *   downwards:  h_g = back[g, h_parent]
 * A dead joint reports hypothesis 0 and bone 0, sends nothing to its parent and turns its children into roots: it cuts the
 * tree there and nowhere else.
 * Outputs, all required: d_joint_h [N,J] int32, the kept assignment;  d_cost [N] float64 = the sum over the roots, in
 * ascending index, of min S[root,.], +inf if the pose has no live joint;  d_bone [N,J] float64 = b[n,g,h_p,h_g] at the kept
 * assignment, 0 for roots and dead joints.
 * Two limits hold by construction: at mu = 0 with d_weight == NULL d_joint_h is bit for bit d_best_h of zedo_joint_reproj on
 * the same rows; as mu grows the assignment becomes one whole hypothesis per pose, the arg-min over h of sum_j u[n,j,h].
 * (x and T are taken to be finite: a non-finite coordinate makes the affected minima unspecified and is never an address.)
 * There is no workspace: S, back and the positions live in the LDS of the pose's workgroup, which bounds the sizes:
 *   34 J H + 16 H + 4096 <= 163840 bytes, the 160 KiB of a gfx950 CU
 *   (24 J H of positions, 8 J H of S, 2 J H of back as 16-bit entries, 16 H of bone lengths, 4096 of minima and flags),
 * and 1 <= J <= 64 (the cap of the network entry points), 1 <= H <= 1024.  That admits H <= 268 at J = 17, H <= 72 at J = 64,
 * H <= 1024 for J <= 4.
 * Contract: N >= 1, the caps above, H*N*J <= INT_MAX, finite mu >= 0; ZEDO_E_BADARG with nothing written for a NULL pointer
 * other than d_T / d_weight, a non-positive size, a size above the caps, H*N*J above INT_MAX, a parent array that breaks the
 * rules, or a negative or non-finite mu; allocates nothing, synchronises nothing, enqueues on `stream` only: legal under
 * stream capture; no atomics, every sum in a fixed order (S[p,.] takes its children in ascending index whatever the launch
 * shape): bit-identical from run to run.  One workgroup of 256 lanes per pose, one launch. */
int zedo_joint_tree_select(const double *d_junary, const float *d_x, const float *d_T, const float *d_weight,
                           const int *h_parent, int H, int N, int J, double mu,
                           int *d_joint_h, double *d_cost, double *d_bone, void *stream);

/* ---- skeleton-coupled FUSION per pose WITHOUT ground truth: exact sum-product over the bone tree --------------------------
 * The soft answer of zedo_joint_tree_select, as zedo_joint_marginal is the soft answer of zedo_joint_temporal_select: the same
 * energy read as a probability at a temperature tau.  From one image (no clip is needed) every joint gets a fused position, an
 * error bar and the probability of its likeliest hypothesis.  The skeleton is a tree, so the marginals are exact: one pass from
 * the leaves to the roots, one back.  Whether the fused pose is closer to ground truth is not measured.
 * Inputs: those of zedo_joint_tree_select, word for word - rows (h,n) h-major, ALL rows; d_T and d_weight may be NULL;
 * h_parent [J] int32 ON THE HOST, any forest, validated by the same rules, the host derives the same post-order and passes
 * it by value - and tau: finite, > 0, in cost units (an assignment that costs tau more is e times less probable).
 * X, the clamp of the weights, u, DEAD, own, mix and b are those of zedo_joint_tree_select, statement for statement.
 * Per pose n, all arithmetic in float64:
 *   p(assignment h_.) ~ exp(-(sum_j u[n,j,h_j] + mu * sum_{g: live, parent live} b[n,g,h_p,h_g]) / tau)
 * With l[j,h] = -u[n,j,h] / tau (-inf where the hypothesis is excluded) and c = mu / tau:
 *   upwards, children before parents and siblings in ascending index:  S[j,.] starts as l[j,.];  for a live g with a live parent p
 *       M_g[hp] = LSE_hc (S[g,hc] - c * b[n,g,hp,hc]),  S[p,hp] += M_g[hp]
 *   a ROOT is a live joint with parent -1 or with a dead parent:  logZ_root = LSE_h S[root,h],  Dn[root,.] = 0
 *   downwards, parents before children:  E_g[hp] = l[p,hp] + sum_{children k != g of p} M_k[hp] + Dn[p,hp], formed as
 *       S[p,hp] - M_g[hp] + Dn[p,hp];  Dn[g,hc] = LSE_hp (E_g[hp] - c * b[n,g,hp,hc])
 *   w[j,h] = exp(S[j,h] + Dn[j,h] - logZ of j's component): exactly 0 for an excluded hypothesis
 *   pi[g,hp,hc] = exp(E_g[hp] - c * b[n,g,hp,hc] + S[g,hc] - logZ): the pair marginal of a bone, never stored
 * Every LSE is shifted by the TRUE maximum of its terms (two walks over them; the bone term is recomputed, not kept), so a
 * small tau underflows nothing that matters.  Where the inner index is split over parts of the workgroup each part shifts
 * by its own maximum and the parts combine in ascending order, shifted by the largest.
 * Outputs, all required but d_w:
 *   d_mean [N,J,3] float64 = sum_h w X (camera frame, metres);
 *   d_cov  [N,J,6] float64 = sum_h w (X - mean)(X - mean)^T in the order xx, xy, xz, yy, yz, zz, from centred differences;
 *   d_hmax [N,J] int32 = the lowest h with the largest marginal;  d_wmax [N,J] float64 = that marginal;
 *   d_logz [N,J] float64 = the log-partition value of the joint's component (the tree after dead joints cut it), repeated on
 *       every joint of that component;
 *   d_bone [N,J] float64 = sum_{hp,hc} pi[g,hp,hc] * b[n,g,hp,hc], the EXPECTED bone mismatch in metres, 0 for roots and dead
 *       joints;
 *   d_w [N,J,H] float64 or NULL: the marginals.
 * A dead joint reports NaN in mean and cov, hypothesis 0, wmax 0, logz -inf, bone 0 and a row of zeros in d_w; it sends
 * nothing up and turns its children into roots, as in zedo_joint_tree_select.
 * Limits that hold by construction: as tau -> 0 d_hmax becomes d_joint_h of zedo_joint_tree_select and d_bone its d_bone; at
 * mu = 0 the marginals are the per-joint softmax of -u / tau.
 * (x and T are taken to be finite, as in zedo_joint_tree_select.)
 * There is no workspace: X, S, the messages M and Dn and the bone lengths live in the LDS of the pose's workgroup:
 *   48 J H + 16 H + 8192 <= 163840 bytes, the 160 KiB of a gfx950 CU
 *   (24 J H of positions, 8 J H each of S, M and Dn, 16 H of bone lengths and E_g, 8192 of the parts' sums, logZ and flags),
 * and 1 <= J <= 64, 1 <= H <= 1024.  zedo_joint_tree_marginal_max_h(J) returns the largest H this admits at J - 187 at
 * J = 17, 50 at J = 64, 1024 for J <= 2 - and 0 for a J outside 1 .. 64.
 * Contract: N >= 1, H <= zedo_joint_tree_marginal_max_h(J), H*N*J <= INT_MAX, finite mu >= 0, finite tau > 0, finite mu / tau;
 * ZEDO_E_BADARG with nothing written for a NULL pointer other than d_T / d_weight / d_w, a non-positive size, a size above
 * the caps, H*N*J above INT_MAX, a parent array that breaks the rules, a negative or non-finite mu, tau <= 0 or not finite,
 * or mu / tau not finite; allocates nothing, synchronises nothing, enqueues on `stream` only: legal under stream capture; no
 * atomics, every sum in a fixed order: bit-identical from run to run and with or without d_w.  One workgroup of 256 lanes
 * per pose, one launch. */
int zedo_joint_tree_marginal_max_h(int J);
int zedo_joint_tree_marginal(const double *d_junary, const float *d_x, const float *d_T, const float *d_weight,
                             const int *h_parent, int H, int N, int J, double mu, double tau,
                             double *d_mean, double *d_cov, int *d_hmax, double *d_wmax, double *d_logz,
                             double *d_bone, double *d_w, void *stream);

/* ---- pruning hypotheses DURING the loop, without ground truth: keep the K best of a pose, compact the rows ----------------
 * zedo_oil_run takes step_begin / step_end and a row's bits do not depend on the batch it is in, so a run can be cut into
 * stages that carry fewer and fewer rows.  These two calls are the piece between two stages.  Whether pruning by
 * reprojection error costs accuracy against ground truth is not measured.
 * zedo_prune_rank: d_err [H*N] float64, ALL rows (h,n) h-major of the CURRENT slots (no row_offset: a pose's every
 * hypothesis takes part), e.g. d_err of zedo_min_reproj.  For pose n, slot a comes before slot b iff
 *   err_a is not NaN and err_b is NaN,  or  neither is NaN and err_a < err_b,
 *   or neither of these separates them and a < b   (equal values, -0.0 and 0.0, two NaNs: the lower slot first)
 * - finite ascending, then +inf, then NaN.  NOT zedo_pose_min's "NaN wins": a diverged row is the first to go, as in
 * zedo_temporal_select.  The kept set is the K first slots of that order; d_keep [K,N] int32, d_keep[r*N + n] = the r-th
 * kept slot of pose n in ASCENDING SLOT order (K == H: the identity table).
 * Contract: 1 <= K <= H <= 1024, N >= 1, H*N <= INT_MAX; anything else, or a NULL pointer: ZEDO_E_BADARG, nothing written.
 * zedo_prune_gather: out of place; with g = keep[r,n]*N + n:  x_out[(r,n)] = x[g] ([.,J,3] fp32),  T_out[(r,n)] = T[g]
 * ([.,3] fp32),  hyp_out[r,n] = d_hyp ? d_hyp[g] : keep[r,n].  d_hyp [H,N] int32: the ORIGINAL hypothesis id of every
 * current slot - it chains from stage to stage; NULL: the slots are the hypotheses.  A keep entry outside 0 .. H-1 is never
 * an address: that output row is NaN in x_out and T_out and its id is -1.  With the identity table the outputs are the
 * inputs bit for bit.
 * Contract: any J >= 1, 1 <= K <= H, N >= 1, H*N <= INT_MAX; ZEDO_E_BADARG with nothing written otherwise, for a NULL pointer
 * other than d_hyp, and for an output pointer equal to an input (x_out == x, T_out == T, hyp_out == d_hyp or d_keep).
 * Both: allocate nothing, synchronise nothing, enqueue on `stream` only: legal under stream capture; no atomics:
 * bit-identical from run to run. */
int zedo_prune_rank(const double *d_err, int H, int N, int K, int *d_keep, void *stream);
int zedo_prune_gather(const int *d_keep, int H, int K, int N, int J, const float *d_x, const float *d_T, const int *d_hyp,
                      float *d_x_out, float *d_T_out, int *d_hyp_out, void *stream);

/* The second half of zedo_min_mpjpe on its own: per pose n the minimum of d_err over the hypotheses present in
 * [0,B) and the first hypothesis index that attains it (np.amin / np.argmin, NaN wins: h36m.py:411-412).  For
 * callers that edit the per-row errors first - eval_multi's `valid_ind` (h36m.py:396-397: hypotheses not listed for
 * a pose are skipped) sets them to +inf - including on a row shard (row_offset). */
int zedo_pose_min(const double *d_err, int B, int N, long long row_offset, double *d_best, int *d_best_h, void *stream);

/* ---- diagnostics: sampled per-kernel timing ---------------------------------------------------------
 * Between zedo_profile_start and zedo_profile_stop every `sample_every`-th launch of each kernel class
 * issued by zedo_oil_run / zedo_sde_step / zedo_score_eps is bracketed by two hipEvents recorded on the
 * launch stream (at most max_samples pairs).  zedo_profile_stop synchronises those events and fills,
 * per class, the summed elapsed milliseconds, the number of sampled launches and the number of launches
 * seen.  Process-wide diagnostic state; not part of the data path.  Arrays have ZEDO_PROF_CLASSES entries.
 */
#define ZEDO_PROF_HIDDEN 0  /* the four 1024x1024 dense layers (+GroupNorm+SiLU[+residual]) */
#define ZEDO_PROF_PRE 1     /* pre_dense (+GroupNorm+SiLU) */
#define ZEDO_PROF_POST 2    /* post_dense + SDE update */
#define ZEDO_PROF_REPROJ 3  /* reprojection correction (stand-alone launch: first iteration of a zedo_oil_run call) */
#define ZEDO_PROF_CLASSES 4
int zedo_profile_start(int sample_every, int max_samples);
/* What this box's matrix pipe sustains right now: `iters` x 16 back-to-back v_mfma_f32_32x32x2_f32 per wave on every
 * SIMD (two waves each) -> TFLOP/s, and the shader clock seen over that run.  Boxes of one pool differ by a few per
 * cent in clock / power state; bench.py reports the dominant kernel against this number next to the datasheet peak.
 * Synchronises `stream`.  Diagnostic, not part of the data path. */
int zedo_probe_mfma_peak(int iters, double *h_tflops, double *h_shader_ghz, void *stream);
/* The same for the fp16 matrix pipe the opt-in split-fp16 mode runs on: `iters` x 16 back-to-back v_mfma_f32_32x32x16_f16 per wave,
 * two waves per SIMD, operands that differ per lane and per instruction, no LDS / memory traffic.  Under a dense fp16 MFMA stream power
 * management grants well below the 2.4 GHz the 2.5 PFLOP/s datasheet peak is quoted at: this is the ceiling attainable on this box. */
int zedo_probe_mfma_peak_f16(int iters, double *h_tflops, double *h_shader_ghz, void *stream);
int zedo_profile_stop(double *h_total_ms, long long *h_samples, long long *h_launches);
/* Shader clock (GHz) the sampled hidden-layer launches of the last profiling session really ran at: shader cycles over
 * 100 MHz wall ticks, taken by workgroup 0 of each sampled launch around its tile.  0 if nothing was sampled. */
double zedo_profile_shader_ghz(void);
/* What the sampling bracket itself measures (milliseconds): the median of 15 EMPTY event pairs recorded by the last
 * zedo_profile_stop on the stream its samples came from.  Every sampled duration contains it once; the sums returned by
 * zedo_profile_stop are raw - subtract samples x this value for the kernels' own time (bench.py does, and checks that
 * the per-class times of one OIL iteration then add up to no more than the wall time of an iteration).  0 if nothing
 * was sampled. */
double zedo_profile_bracket_ms(void);

#ifdef __cplusplus
}
#endif
#endif /* ZEDO_HIP_H */
