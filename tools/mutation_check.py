#!/usr/bin/env python3
"""Sensitivity of the GPU parity suite: fifty-four one-line mutations of the HIP path, each of which must turn
at least one `-m gpu` test red (run on the GPU box from the repo root: `python tools/mutation_check.py [out.txt]`).

Each mutant is the product library built with ONE extra -D flag (the hooks are `#ifdef ZEDO_MUT_*` lines in csrc/,
compiled out of the product); the whole `-m gpu` suite runs against it and the failing tests are listed.  The clean
library is rebuilt and re-tested at the end (row "none": must be all green), so no mutant is left in the tree.
"""
import os
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zedo-release_amd", "csrc")

MUTANTS = [
    ("ZEDO_MUT_GN_EPS", "GroupNorm eps 1e-5 -> 2e-5 (zedo_tile.h epilogue, both math modes; reference model.py:116)"),
    ("ZEDO_MUT_SDE_C", "c_i * (1 + 1e-4): score coefficient of x' = a x + c eps (zedo_capi.hip schedule; sde_lib.py:187-198)"),
    ("ZEDO_MUT_CONF2", "least-squares weight conf^4 -> conf^2 (zedo_geom.hip; simple_zeroshot_opt.py:85-88)"),
    ("ZEDO_MUT_SWITCH", "switch to the least-squares T one iteration late (zedo_capi.hip; run/opt_main.py:203-206)"),
    ("ZEDO_MUT_ARGMIN_TIE", "arg-min ties to the HIGHER hypothesis index (zedo_metric.hip; np.argmin, h36m.py:412)"),
    # round 4: the rewritten IPO kernel and the split post_dense of small batches
    ("ZEDO_MUT_IPO_JOINT", "IPO: the 17th key joint (lane 16 of the half-wave) drops out of the gradient sums (zedo_geom.hip; opt_main.py:189-191)"),
    ("ZEDO_MUT_POST_Q3", "post_dense of batches <= 2048 rows: the fourth K quarter is read from the third (zedo_geom.hip post_reduce_kernel)"),
    # round 5: the split-fp16 mode (every GPU test runs in both modes; these two must turn f16x3 cells red and leave f32 cells green)
    ("ZEDO_MUT_F16_DROP_LH", "f16x3: the W_low x X_high MFMA of every k block is dropped - W as plain fp16 (zedo_gemm16.hip mma)"),
    ("ZEDO_MUT_F16_XLOW0", "f16x3: the low pieces of the activations are lost in the first of the 64 k blocks of every dense layer (zedo_gemm16.hip)"),
    # the native predictor-corrector step (zedo_pc_step)
    ("ZEDO_MUT_PC_NOISE", "pc step: the predictor's noise coefficient C * (1 + 1e-4) (zedo_capi.hip plan; advanced/sampling.py:185-191)"),
    ("ZEDO_MUT_PC_MEAN", "pc step, Langevin: mean ||eps|| divided by the padded row count instead of B (zedo_pc.hip; advanced/sampling.py:281-283)"),
    # skeletons other than 17 x 3 (tests/test_joint_counts_gpu.py): both leave every 51-coordinate test green
    ("ZEDO_MUT_KZERO8", "pre_dense: k = 56..63 vouched zero for every handle, also J3 = 57..64 (zedo_capi.hip pre_args)"),
    ("ZEDO_MUT_PACK51", "pack_rows copies at most 51 coordinates of a pose row: J3 = 52..64 lose their last columns (zedo_geom.hip)"),
    # general intrinsics and all axis subsets (tests/test_general_intrinsics_gpu.py): all three leave every pinhole-K, "z" / "xyz" test green
    ("ZEDO_MUT_IPO_GPY_K1", "IPO backward: K[1] g_w0 dropped from g_py = (K^T g_w)_y - zero in a pinhole K (zedo_geom.hip ipo_joint_terms)"),
    ("ZEDO_MUT_IPO_W2_K6", "IPO forward: K[6] p_x dropped from the homogeneous coordinate w2 - zero in a pinhole K (zedo_geom.hip ipo_joint_terms)"),
    ("ZEDO_MUT_IPO_AXIS_XY", "IPO: rot_vect_y is updated under the x bit of axes_mask, in both kernels - the same for \"z\" and \"xyz\" (zedo_geom.hip)"),    # the one-pass selection (tests/test_selection_both_gpu.py): leaves every test of the single-protocol entry points green
    ("ZEDO_MUT_BOTH_SLOT", "zedo_min_mpjpe_both: the aligned (P2) row error is written into slot 0 as well (zedo_metric.hip store_row_error)"),
    # the label-free selection (tests/test_select_reproj_gpu.py): leaves every other test green
    ("ZEDO_MUT_REPROJ_WEIGHT", "zedo_min_reproj: every joint weighs 1 although confidences were given (zedo_metric.hip row_reproj_error)"),
    # the joint-wise aggregation (tests/test_joint_reproj_gpu.py): leaves every other test green
    ("ZEDO_MUT_JOINT_TIE", "zedo_joint_reproj without d_jerr: the running minimum takes ties, the HIGHER hypothesis wins (zedo_metric.hip joint_reproj_walk_kernel)"),
    # the temporal selection (tests/test_temporal_select_gpu.py, tests/test_select_temporal_driver_gpu.py): leaves every other test green
    ("ZEDO_MUT_TEMPORAL_LAMBDA", "zedo_temporal_select: the motion term enters the recurrence unweighted, lambda is dropped (zedo_temporal.hip temporal_scan_kernel)"),
    # the pruning between two stages of the loop (tests/test_prune_gpu.py, tests/test_prune_pipeline_gpu.py, tests/test_prune_driver_gpu.py):
    # leaves every other test green
    ("ZEDO_MUT_PRUNE_TIE", "zedo_prune_rank: the tie rule a < b becomes a <= b, a slot comes before itself (zedo_prune.hip prune_precedes)"),
    # tile tails and dispatch branches of the selection, pruning and video kernels (profiles/mutation_boundaries.txt): each leaves the
    # tests of these entry points green as they stood before their case tables crossed the constants named here
    ("ZEDO_MUT_TT_PIECE", "zedo_temporal_select: joint pieces after the first (J > TT_J = 32) stage joints 0.. of the pose again (zedo_temporal.hip temporal_transition_kernel)"),
    ("ZEDO_MUT_TB_WALK", "zedo_temporal_select: the walk in memory (H > TB_INTS = 8192) reads back row n instead of n + 1 (zedo_temporal.hip temporal_backtrack_kernel)"),
    ("ZEDO_MUT_PR_P32", "zedo_prune_rank: tiles of 32 poses (256 < H <= 512) count the kept slots below a - 1 for the output position (zedo_prune.hip prune_rank_kernel)"),
    ("ZEDO_MUT_PG_TRIP", "zedo_prune_gather: the grid-stride loop over the rows stops after its first trip (zedo_prune.hip prune_gather_kernel)"),
    ("ZEDO_MUT_PMIN_LANE_H", "lane-per-pose arg-min (N >= 8192): reports h - h0, the hypothesis counted from the shard's first (zedo_metric.hip pose_min_kernel)"),
    # the joint-wise temporal selection (tests/test_joint_temporal_gpu.py, tests/test_select_joints_temporal_driver_gpu.py), since the
    # streaming scan takes the statement from the same place the live streams (tests/test_joint_stream_gpu.py), and the tests that hold
    # another call to the first-order one (in tests/test_joint_accel_gpu.py and tests/test_select_joints_accel_driver_gpu.py); leaves
    # tests/test_joint_accel_marginal_gpu.py green (profiles/chain_shared_scan.txt: run against these six files)
    ("ZEDO_MUT_JT_NO_T", "zedo_joint_temporal_select and zedo_joint_stream_push: the motion term is taken on x alone although d_T was given (zedo_chain.h ZEDO_CHAIN_STEP_T: joint_temporal_scan_kernel and joint_stream_scan_kernel)"),
    # the joint-wise selection on live streams (tests/test_joint_stream_gpu.py): leaves every other test green
    ("ZEDO_MUT_JS_HORIZON", "zedo_joint_stream_push: the horizon of frame n is taken as n + lag - 1, one frame short (zedo_joint_stream.hip joint_stream_emit_kernel)"),
    # the pose-level selection on live streams (tests/test_temporal_stream_gpu.py; profiles/mutation_temporal_stream.txt): leaves every
    # other test green, and in that file the tests that push every clip whole or carry one frame per clip
    ("ZEDO_MUT_TSTREAM_LASTX", "zedo_temporal_stream_push: the state's copy of x is not refreshed after a push, the next push's first transition is taken from stale poses (zedo_temporal_stream.hip temporal_stream_scan_kernel)"),
    # the joint-wise fusion on live streams (tests/test_joint_stream_marginal_gpu.py; profiles/mutation_joint_stream_marginal.txt): leaves
    # every other test green, and of that file the lag-0 comparisons, the cells whose clips end before the shortened horizon matters, the
    # clip of one frame and the refusals; the tests that compare the call with itself go red - every one of them also holds it to the
    # offline call or to the reference
    ("ZEDO_MUT_JSM_HORIZON", "zedo_joint_stream_marginal_push: the horizon of frame n is taken as n + lag - 1, one frame short (zedo_joint_stream_marginal.hip joint_stream_marginal_emit_kernel)"),
    # the joint-wise fusion (tests/test_joint_marginal_gpu.py, tests/test_select_joints_fused_driver_gpu.py): leaves every other test green
    ("ZEDO_MUT_JM_NO_BACKWARD", "zedo_joint_marginal: B = 0 on every frame - the filtering marginals, not the smoothed ones (zedo_joint_marginal.hip joint_marginal_backward_kernel)"),
    # the pose-level fusion (tests/test_temporal_marginal_gpu.py; profiles/mutation_temporal_marginal.txt): leaves every other test green,
    # and of that file the case of one frame (1, 1, 1, 1), the five tests of the bits against the chunk, the workspace, the stream, capture,
    # the alignment and d_w and the clamped offsets, which compare the call with itself, and the pipeline test
    ("ZEDO_MUT_TM_NO_BACKWARD", "zedo_temporal_marginal: B = 0 on every frame - the filtering marginals, not the smoothed ones (zedo_temporal_marginal.hip temporal_marginal_backward_kernel)"),
    # the second-order joint-wise selection (tests/test_joint_accel_gpu.py, tests/test_select_joints_accel_driver_gpu.py) and, since its
    # sum-product twin shares the statement, the second-order fusion (tests/test_joint_accel_marginal_gpu.py); leaves the tests of the
    # first-order chain green (tests/test_joint_temporal_gpu.py, tests/test_joint_stream_gpu.py, tests/test_select_joints_temporal_driver_gpu.py;
    # profiles/chain_shared_scan.txt: run against these six files)
    ("ZEDO_MUT_JA_FIRST_DIFF", "zedo_joint_accel_select and zedo_joint_accel_marginal: the second difference is taken as X[n] - X[n-1] + X[n-2], the factor 2 is dropped (zedo_chain.h accel_lead: the scan and cost kernels of the selection, the forward and backward kernels of the fusion)"),
    # the second-order selection on live streams (tests/test_joint_accel_stream_gpu.py; profiles/mutation_joint_accel_stream.txt): leaves
    # every other test green, and of that file the lag-0 comparisons, the clips that end before the shortened horizon matters and the refusals
    ("ZEDO_MUT_JAS_HORIZON", "zedo_joint_accel_stream_push: the horizon of frame n is taken as n + lag - 1, one frame short (zedo_joint_accel_stream.hip joint_accel_stream_emit_kernel)"),
    # the second-order fusion on live streams (tests/test_joint_accel_stream_marginal_gpu.py; profiles/mutation_joint_accel_stream_marginal.txt):
    # leaves every other test green, and of that file the lag-0 comparisons, the clips that end before the shortened horizon matters, the
    # binding's and the pipeline's tests and the refusals
    ("ZEDO_MUT_JASM_HORIZON", "zedo_joint_accel_stream_marginal_push: the horizon of frame n is taken as n + lag - 1, one frame short (zedo_joint_accel_stream_marginal.hip joint_accel_stream_marginal_emit_kernel)"),
    # the skeleton-coupled aggregation (tests/test_joint_tree_gpu.py, tests/test_select_joints_tree_driver_gpu.py) and, since its sum-product
    # twin shares the statement, the skeleton-coupled fusion's tests: leaves every other test green
    ("ZEDO_MUT_TREE_NO_HALF", "zedo_joint_tree_select and zedo_joint_tree_marginal: the bone term compares the assembled length with the SUM of the two hypotheses' lengths, the 0.5 is dropped (zedo_chain.h tr_bone: the recurrences and bone[n,.])"),
    # the skeleton-coupled fusion (tests/test_joint_tree_marginal_gpu.py, tests/test_select_joints_tree_fused_driver_gpu.py): leaves every other
    # test green
    # the second-order joint-wise fusion (tests/test_joint_accel_marginal_gpu.py): leaves every other test green
    ("ZEDO_MUT_JAM_NO_BACK_ACCEL", "zedo_joint_accel_marginal: the c_a a term is dropped from the backward pass only - B2 is the first-order one, A2 keeps the term (zedo_joint_accel_marginal.hip joint_accel_marginal_backward_kernel)"),
    # the accuracy of the Procrustes alignment (tests/test_procrustes_gpu.py and the oracle-at-the-bound assertions beside the 3e-7 ones):
    # both move P2 by 1e-8 and less, below every tolerance the selection tests had (profiles/mutation_procrustes.txt)
    ("ZEDO_MUT_JACOBI_EARLY", "P2: the Jacobi sweeps of polar_from_svd stop at off < 1e-2 instead of 1e-15 (zedo_metric.hip)"),
    ("ZEDO_MUT_ALIGN_F32", "P2: the 3x3 alignment matrix M is rounded through fp32 before polar_from_svd (zedo_metric.hip row_error)"),
    # the accuracy of the reprojection solve (tests/test_reproj_accuracy_gpu.py, tests/test_reproj_fused_gpu.py and the float64-at-the-bound
    # assertions beside the captures) and its row shards: both leave every test green that existed before (profiles/mutation_reproj.txt)
    ("ZEDO_MUT_REPROJ_UNCENTRED", "reproj_row: the numerator of T_z without the centring of b, d_x b_x + d_y b_y - equal in exact arithmetic, in every launch form (zedo_internal.h)"),
    ("ZEDO_MUT_RGRAD_OFFSET", "zedo_reproj_grad: row_offset is ignored, the pose of row b is b mod N (zedo_geom.hip reproj_grad_kernel)"),
    # one tile of one launch shape (tests/test_launch_shapes_gpu.py; profiles/mutation_launch_shapes.txt): each touches exactly one tile that is
    # neither the first nor the last of its launch, and leaves every test green that existed before
    ("ZEDO_MUT_PAIR_SEAM", "exact-fp32 pair kernels: the first remainder tile behind the 128x128 tiles takes its bias from the next column block (zedo_gemm.hip layer_pair_kernel)"),
    ("ZEDO_MUT_F16_PAIR_SEAM", "f16x3 pair kernels: the first 64x64 tile behind the big tiles takes its bias from the next column block (zedo_gemm16.hip layer16_pair_kernel)"),
    ("ZEDO_MUT_POST64_POSE", "post_dense on 64x64 tiles (above 8 192 rows): the fused reprojection tail of the third tile takes the pose of row b + 1 (zedo_gemm.hip layer_tile)"),
    # the time-bias table of a schedule (tests/test_schedule_gpu.py; profiles/mutation_schedule.txt): the first is reached only by schedules
    # of more than 1 024 timestamps and leaves every test green that existed before; the second stays inside that file's float64 criterion
    # (0.68 of it at label 2000) and is caught by tests/test_pc_native_gpu.py::test_chained_steps_against_the_float64_reference
    ("ZEDO_MUT_BIAS_TILE", "schedule tables above 1 024 rows: in the three cost-model shapes of launch_small ONE EPI_BIAS tile, the second row tile of the second column block, takes its bias from the next column block (zedo_gemm.hip layer_tile)"),
    ("ZEDO_MUT_POSEMB_FAST", "posemb_kernel: __sinf / __cosf, the hardware fast forms without range reduction, in place of sinf / cosf (zedo_geom.hip)"),
    # the resumable IPO state (tests/test_ipo_state_gpu.py and the second-moment assertions of the single-iteration tests;
    # profiles/mutation_ipo_state.txt: run against the six files that launch the IPO kernels).  None of them changes an address.
    ("ZEDO_MUT_IPO_CLAMP_LO", "IPO: the clamp backward tests scale <= max only, the lower bound is forgotten, in both kernels - three cells of the earlier single-iteration tests reach it from trajectory states, none at the boundary or in the lane-per-row kernel (zedo_geom.hip)"),
    ("ZEDO_MUT_IPO_STORE_V", "zedo_ipo_fit_resume: the scale's exp_avg is stored into the slot of its exp_avg_sq, state[14] (zedo_geom.hip ipo_store)"),
    ("ZEDO_MUT_IPO_ROW_LOAD_V", "zedo_ipo_fit_resume: the lane-per-row kernel resumes with exp_avg_sq = 0, the half-wave kernel does not (zedo_geom.hip ipo_row_kernel)"),
    # every key-list length the ABI accepts (tests/test_ipo_key_lists_gpu.py; profiles/mutation_ipo_key_lists.txt: run against the seven
    # files that launch the IPO kernels).  It changes no address and leaves every test green that existed before: none launched the
    # lane-per-row kernel with eleven key joints
    ("ZEDO_MUT_IPO_ROW_CASE", "IPO: case 11 of the lane-per-row dispatch launches ipo_row_kernel<10>, the eleventh key joint is lost in that kernel only - the slip a 17-line macro switch invites (zedo_geom.hip launch_ipo_fit)"),
    ("ZEDO_MUT_TREEMARG_NO_DOWN", "zedo_joint_tree_marginal: Dn = 0 on every joint - the downward pass is dropped, a joint hears from its subtree only (zedo_joint_tree_marginal.hip joint_tree_marginal_kernel)"),
]


def build(flag):
    # ZEDO_MUT_LIBS=<dir>: libraries built beforehand (<dir>/<flag>.so, <dir>/none.so for the product) are copied into place instead
    # of compiling here - hipcc cross-compiles gfx950 on a host without a GPU
    if os.environ.get("ZEDO_MUT_LIBS"):
        shutil.copyfile(os.path.join(os.environ["ZEDO_MUT_LIBS"], (flag or "none") + ".so"), os.path.join(ROOT, "zedo-release_amd", "zedo_hip", "libzedo_hip.so"))
        return
    for f in os.listdir(CSRC):
        if f.endswith(".hip"):
            os.utime(os.path.join(CSRC, f))
    subprocess.run(["make", "-C", CSRC, "-j4", f"EXTRA={'-D' + flag if flag else ''}"], check=True,
                   stdout=subprocess.DEVNULL)


def run_suite(modes=None):
    """modes: None = both arithmetic modes of the suite (tests/conftest.py), "f32" / "f16x3" = that one only (ZEDO_TEST_MATH)."""
    t0 = time.time()
    # ZEDO_MUT_TESTS: the test files to run instead of the whole suite, separated by blanks (a mutant of one kernel family against
    # the files that launch it)
    cmd = [sys.executable, "-m", "pytest"] + (os.environ.get("ZEDO_MUT_TESTS", "").split() or ["tests"]) + ["-m", "gpu", "-q", "--no-header", "-rf", "-p", "no:cacheprovider"]
    if os.environ.get("ZEDO_MUT_DESELECT"):          # e.g. the three-minute end-to-end ensembles: "not lie_inside and not pooled"
        cmd += ["-k", os.environ["ZEDO_MUT_DESELECT"]]
    env = dict(os.environ)
    env.pop("ZEDO_TEST_MATH", None)
    if modes:
        env["ZEDO_TEST_MATH"] = modes
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    failed = sorted(set(re.findall(r"^FAILED (\S+)", out, re.M)))
    m = re.search(r"(\d+) passed", out)
    return failed, int(m.group(1)) if m else 0, time.time() - t0, out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gpurun_out", "mutation_check.txt")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    rows, ok = [], True
    try:
        # e.g. ZEDO_MUT_ONLY=ZEDO_MUT_IPO_JOINT: one mutant (+ the clean rebuild); several: separated by commas
        only = [f for f in os.environ.get("ZEDO_MUT_ONLY", "").split(",") if f]
        assert all(f in dict(MUTANTS) for f in only), only
        for flag, what in MUTANTS:
            if only and flag not in only:
                continue
            build(flag)
            # mutations of code both modes share are hunted in the exact-fp32 cells (half the suite time); the two mutations of the
            # split-fp16 kernels run BOTH modes: they must turn f16x3 cells red and leave every f32 cell green
            f16_only = flag.startswith("ZEDO_MUT_F16_")
            failed, passed, dt, out = run_suite(None if f16_only else "f32")
            if f16_only and any("[f32" in t for t in failed):
                ok = False
            rows.append((flag, what + (" [both modes]" if f16_only else " [f32 cells]"), failed, passed, dt))
            with open(dst + ".partial", "a") as f:        # a run cut short by a time limit still leaves every finished row behind
                f.write(f"-D{flag} | {rows[-1][1]} | {len(failed)} | {passed} | {dt:.0f}\n" + "".join(f"    RED {t}\n" for t in failed))
            ok &= len(failed) > 0
            print(f"{flag}: {len(failed)} red / {passed} green in {dt:.0f} s", flush=True)
    finally:
        build(None)
    # the clean library in the cells the mutants ran in
    clean_modes = "f32" if only and not any(f.startswith("ZEDO_MUT_F16_") for f in only) else None
    failed, passed, dt, out = run_suite(clean_modes)
    rows.append(("none", "the product library (rebuilt without any mutation)" + (" [f32 cells]" if clean_modes else " [both modes]"), failed, passed, dt))
    ok &= len(failed) == 0
    with open(dst, "w") as f:
        f.write("mutation | what | red tests | green | suite seconds\n")
        for flag, what, failed, passed, dt in rows:
            f.write(f"-D{flag} | {what} | {len(failed)} | {passed} | {dt:.0f}\n")
            for t in failed:
                f.write(f"    RED {t}\n")
        f.write("VERDICT: " + ("every mutation is caught and the product is green\n" if ok else
                               "NOT every mutation is caught (or the product is red)\n"))
    print(open(dst).read())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
