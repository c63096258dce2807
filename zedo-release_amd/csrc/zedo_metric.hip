// Hypothesis selection for gfx950: per-(hypothesis,pose) MPJPE / Procrustes-aligned MPJPE in fp64 and the
// per-pose minimum over hypotheses (reference lib/dataset/h36m.py:394-417, lib/dataset/pw3d.py:302-331,
// lib/utils/transforms.py:42-127).  One lane per row for the errors, the rows of a wave staged through the LDS
// with coalesced loads; the arg-min with one wavefront per pose (few poses) or one lane per pose (many: coalesced
// reads of one hypothesis' errors at a time).  Both protocols of a batch (run/opt_main.py:227-228) come from one pass: the <true> instantiations
// of the row-error kernels evaluate both errors on the tile they have staged, and one arg-min launch serves both (zedo_min_mpjpe_both).
// Without ground truth (zedo_min_reproj): the confidence-weighted reprojection error of x + T in pixels per row, staged the same way, then the
// same arg-min.  Per joint (zedo_joint_reproj): the same per-joint distance, its minimum over the hypotheses per (pose, joint) - one lane
// per (pose, joint) walking the hypotheses, or every row's distances and the same arg-min on them flattened - and the gather that assembles
// a pose from the winning joints (zedo_joint_compose).
#include "zedo_internal.h"

#include <algorithm>

namespace zedo {

// One-sided Jacobi on the 3x3 matrix M (columns rotated until orthogonal): M V = U diag(s).
// Returns R = V U^T (the rotation/reflection of procrustes(..., reflection='best'), transforms.py:93-96)
// and the sum of singular values.
__device__ void polar_from_svd(double M[3][3], double R[3][3], double &strace) {
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; ++i) { al += M[i][p] * M[i][p]; be += M[i][q] * M[i][q]; ga += M[i][p] * M[i][q]; }
                if (fabs(ga) <= 1e-300 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                off = fmax(off, fabs(ga) / sqrt(al * be));
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double mp = M[i][p], mq = M[i][q];
                    M[i][p] = c * mp - s * mq; M[i][q] = s * mp + c * mq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
                }
            }
#ifdef ZEDO_MUT_JACOBI_EARLY  // tools/mutation_check.py only: the sweeps stop at columns orthogonal to 1e-2
        if (off < 1e-2) break;
#else
        if (off < 1e-15) break;
#endif
    }
    double s[3], U[3][3];
    double smax = 0;
    for (int c = 0; c < 3; ++c) {
        s[c] = sqrt(M[0][c] * M[0][c] + M[1][c] * M[1][c] + M[2][c] * M[2][c]);
        smax = fmax(smax, s[c]);
    }
    int nbad = 0, bad = -1, good = -1;
    for (int c = 0; c < 3; ++c) {
        if (s[c] > 1e-14 * smax && s[c] > 0) {
            for (int i = 0; i < 3; ++i) U[i][c] = M[i][c] / s[c];
            good = c;
        } else { ++nbad; bad = c; }
    }
    if (nbad == 1) {
        // rank-2 input (planar pose): complete U with the cross product of the other two columns and pick
        // the sign that makes R a proper rotation.  numpy's LAPACK picks an arbitrary sign here.
        const int a = (bad + 1) % 3, b = (bad + 2) % 3;
        U[0][bad] = U[1][a] * U[2][b] - U[2][a] * U[1][b];
        U[1][bad] = U[2][a] * U[0][b] - U[0][a] * U[2][b];
        U[2][bad] = U[0][a] * U[1][b] - U[1][a] * U[0][b];
        const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                            V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
        if (detV < 0) for (int i = 0; i < 3; ++i) U[i][bad] = -U[i][bad];
        s[bad] = 0;
    } else if (nbad == 2) {
        // rank-1 input (a two-joint skeleton, collinear joints): one column of U is known, V is orthogonal already.  Any
        // orthonormal completion of U gives the reference's error: the aligned pose has no component along the two null
        // directions of the ground truth, and the length of the prediction's component there does not depend on the basis.
        const int g = good, a = (g + 1) % 3, b = (g + 2) % 3;
        int m = 0;                                                 // the coordinate axis farthest from the known column
        for (int i = 1; i < 3; ++i) if (fabs(U[i][g]) < fabs(U[m][g])) m = i;
        double e[3] = {0, 0, 0};
        e[m] = 1.0;
        double ua[3] = {U[1][g] * e[2] - U[2][g] * e[1], U[2][g] * e[0] - U[0][g] * e[2], U[0][g] * e[1] - U[1][g] * e[0]};
        const double na = sqrt(ua[0] * ua[0] + ua[1] * ua[1] + ua[2] * ua[2]);
        for (int i = 0; i < 3; ++i) U[i][a] = ua[i] / na;
        U[0][b] = U[1][g] * U[2][a] - U[2][g] * U[1][a];
        U[1][b] = U[2][g] * U[0][a] - U[0][g] * U[2][a];
        U[2][b] = U[0][g] * U[1][a] - U[1][g] * U[0][a];
        s[a] = 0; s[b] = 0;
    } else if (nbad > 2) {
        // no direction at all (a zero or non-finite matrix: one joint, or every joint of a set in one point)
        for (int c = 0; c < 3; ++c) for (int i = 0; i < 3; ++i) U[i][c] = (i == c);
        for (int c = 0; c < 3; ++c) for (int i = 0; i < 3; ++i) V[i][c] = (i == c);
    }
    strace = s[0] + s[1] + s[2];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + V[i][2] * U[j][2];
}

// Error of one row from its staged operands: p = the row's J*3 fp32 coordinates, g = its pose's J*3 fp64 ground-truth coordinates
// (both register / LDS resident: every access below is a plain indexed read).  The statements - and therefore every rounding - are the
// ones of rounds 1-5's one-lane-per-row kernel; only where the operands come from has changed.
template <class P, class G>
__device__ __forceinline__ double row_error(const P &p, const G &g, int J, int procrustes) {
    double e = 0.0;
    if (!procrustes) {
        for (int j = 0; j < J; ++j) {
            const double dx = (double)p[3 * j] - g[3 * j], dy = (double)p[3 * j + 1] - g[3 * j + 1],
                         dz = (double)p[3 * j + 2] - g[3 * j + 2];
            e += sqrt(dx * dx + dy * dy + dz * dz);
        }
        return e / J;
    }
    // procrustes(A = gt, B = pred, scaling=True, reflection='best').Z  (transforms.py:42-127)
    double ab[3] = {0, 0, 0}, bb[3] = {0, 0, 0};
    for (int j = 0; j < J; ++j)
        for (int c = 0; c < 3; ++c) { ab[c] += g[3 * j + c]; bb[c] += (double)p[3 * j + c]; }
    for (int c = 0; c < 3; ++c) { ab[c] /= J; bb[c] /= J; }
    double ssA = 0, ssB = 0, M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int j = 0; j < J; ++j) {
        double a0[3], b0[3];
        for (int c = 0; c < 3; ++c) { a0[c] = g[3 * j + c] - ab[c]; b0[c] = (double)p[3 * j + c] - bb[c]; }
        for (int c = 0; c < 3; ++c) { ssA += a0[c] * a0[c]; ssB += b0[c] * b0[c]; }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) M[r][c] += a0[r] * b0[c];   // A0^T B0 (un-normalised)
    }
    const double An = sqrt(ssA), Bn = sqrt(ssB);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] /= (An * Bn);
#ifdef ZEDO_MUT_ALIGN_F32     // tools/mutation_check.py only: the alignment matrix passes through fp32
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = (double)(float)M[r][c];
#endif
    double R[3][3], st;
    polar_from_svd(M, R, st);
    const double scale = An * st / Bn;   // Z = A_norm * S_trace * (B0/B_norm) R + A_bar
    for (int j = 0; j < J; ++j) {
        double b0[3], z[3];
        for (int c = 0; c < 3; ++c) b0[c] = (double)p[3 * j + c] - bb[c];
        for (int c = 0; c < 3; ++c) z[c] = scale * (b0[0] * R[0][c] + b0[1] * R[1][c] + b0[2] * R[2][c]) + ab[c];
        const double dx = z[0] - g[3 * j], dy = z[1] - g[3 * j + 1], dz = z[2] - g[3 * j + 2];
        e += sqrt(dx * dx + dy * dy + dz * dz);
    }
    return e / J;
}

// What a row-error kernel writes for local row `loc` from the operands it has staged.  One protocol: err[loc].  BOTH (zedo_min_mpjpe_both,
// opt_main.py:227-228 scores every batch under both protocols): the same operands are read twice, err [2][B] protocol-major - err[loc] the
// MPJPE, err[B + loc] the Procrustes-aligned one; `procrustes` is not read.  The statements are row_error's either way: the same bits.
template <bool BOTH, class P, class G>
__device__ __forceinline__ void store_row_error(const P &p, const G &g, int J, int procrustes, double *__restrict__ err, long long loc, int B) {
    if constexpr (!BOTH) err[loc] = row_error(p, g, J, procrustes);
    else {
        const double e1 = row_error(p, g, J, 0), e2 = row_error(p, g, J, 1);
#ifdef ZEDO_MUT_BOTH_SLOT   // tools/mutation_check.py only: the aligned error lands in the slot of the plain one as well
        (void)e1;
        err[loc] = e2;
#else
        err[loc] = e1;
#endif
        err[(long long)B + loc] = e2;
    }
}

// Any joint count: one lane per row straight from global memory (rows are J*12 bytes apart: every load instruction touches 64 cache lines).
template <bool BOTH>
__global__ __launch_bounds__(128) void row_error_kernel(const float *__restrict__ pred, const double *__restrict__ gt, int B, int N, int J,
                                                        long long row_offset, int procrustes, double *__restrict__ err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n = (int)((row_offset + b) % N);
    store_row_error<BOTH>(pred + (size_t)b * J * 3, gt + (size_t)n * J * 3, J, procrustes, err, b, B);
}

// J = 17 (every dataset of the path), round 6: the 64 rows of a wave arrive as ONE contiguous 13 KB piece of the pose tensor, fetched with
// coalesced 16-byte loads (a lane's own row would be 204 bytes from its neighbour's: 64 cache lines per load instruction, 427 GB/s
// at 3.5 M rows), and the rows' ground-truth poses - consecutive poses n = (row_offset + b) mod N, 408 bytes each - with coalesced
// 8-byte loads; both land in the LDS ([row][51], odd row stride: a lane reading its own row is bank-conflict free), all loads of the
// tile in flight at once; then one lane per row as before.
constexpr int RE_ROWS = 64, RE_D = 17 * 3;
static_assert(RE_ROWS == 64, "the staged kernels are one wavefront per workgroup: their LDS hand-over relies on it");
template <bool BOTH>
__global__ __launch_bounds__(RE_ROWS) void row_error17_kernel(const float *__restrict__ pred, const double *__restrict__ gt, int B, int N,
                                                               long long row_offset, int procrustes, double *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) float sp[RE_ROWS * RE_D];
    __shared__ double sg[RE_ROWS * RE_D];
    const int tid = threadIdx.x, b0 = blockIdx.x * RE_ROWS;
    const int rows = min(RE_ROWS, B - b0);
    const int nf = rows * RE_D;                                   // floats of this tile (the last tile of a batch is short)
    const float *src = pred + (size_t)b0 * RE_D;                  // 16-byte aligned: b0 * 204 bytes, b0 a multiple of 64
    for (int c = tid; c * 4 + 3 < nf; c += RE_ROWS) *reinterpret_cast<f32x4 *>(sp + c * 4) = *reinterpret_cast<const f32x4 *>(src + c * 4);
    if (tid < (nf & 3)) sp[(nf & ~3) + tid] = src[(nf & ~3) + tid];
    // ground truth of row r: pose n_r = (row_offset + b0 + r) mod N - consecutive poses, wrapping to 0 behind N - 1 (several times in one
    // tile when N < 64): the pose index is wave-uniform and advances by scalar increment / compare, no division per element; lanes 0..50
    // fetch the pose's 51 doubles (408 contiguous bytes) per row
    int n = (int)((row_offset + b0) % N);
    if (tid < RE_D) {
#pragma unroll 16
        for (int r = 0; r < rows; ++r) {       // (unrolled: sixteen independent loads in flight per lane)
            sg[r * RE_D + tid] = gt[(size_t)n * RE_D + tid];
            n = (n + 1 == N) ? 0 : n + 1;
        }
    }
    __syncthreads();
    if (tid < rows) store_row_error<BOTH>(sp + tid * RE_D, sg + tid * RE_D, 17, procrustes, err, b0 + tid, B);
}

// np.amin / np.argmin order: NaN is smaller than everything (a diverged hypothesis poisons the pose, and the first
// NaN index is reported), otherwise the smaller value, ties to the lower hypothesis index.
__device__ __forceinline__ bool min_takes(double ov, int oh, double v, int h) {
    if (oh < 0) return false;
    if (h < 0) return true;
    const bool on = ov != ov, vn = v != v;
    if (on || vn) return on && (!vn || oh < h);
#ifdef ZEDO_MUT_ARGMIN_TIE  // tools/mutation_check.py only: ties to the HIGHER hypothesis index
    return ov < v || (ov == v && oh > h);
#else
    return ov < v || (ov == v && oh < h);
#endif
}

// min / first arg-min (np.argmin tie rule) over the hypotheses held locally.  min_takes is a strict total order on (value, hypothesis):
// the minimum does not depend on the order in which the candidates are visited, so both kernels below return the same bits.
// Few poses (N below POSE_MIN_LANE_N): one WAVEFRONT per pose, lanes stride over the hypotheses (N * 8 bytes apart: one cache line per
// lane), butterfly reduction - the parallelism is across hypotheses, a pass is one load deep.
// blockIdx.y (both kernels): the protocol of a protocol-major err [gridDim.y][B] -> best / best_h [gridDim.y][N]; 0 in a launch of one.
__global__ void pose_min_wave_kernel(const double *__restrict__ err, int B, int N, long long row_offset,
                                     double *__restrict__ best, int *__restrict__ best_h) {
    err += (size_t)blockIdx.y * B; best += (size_t)blockIdx.y * N; best_h += (size_t)blockIdx.y * N;
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    // global rows of pose n: n, n+N, n+2N, ... ; local index = global - row_offset
    long long h0 = (row_offset - n + N - 1) / N;     // first hypothesis with h*N + n >= row_offset
    if (row_offset <= n) h0 = 0;
    double e = __builtin_huge_val();
    int hi = -1;
    for (long long h = h0 + lane;; h += 64) {
        const long long loc = h * N + n - row_offset;
        if (loc >= B) break;
        const double v = err[loc];
        if (min_takes(v, (int)h, e, hi)) { e = v; hi = (int)h; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double oe = __shfl_xor(e, off);
        const int oh = __shfl_xor(hi, off);
        if (min_takes(oe, oh, e, hi)) { e = oe; hi = oh; }
    }
    if (lane == 0) { best[n] = (hi >= 0) ? e : __builtin_huge_val(); best_h[n] = hi; }
}

// Many poses (round 6): one LANE per pose, hypotheses walked in ascending order - the 64 lanes of a wave read 64 consecutive poses of one
// hypothesis, 512 contiguous bytes per load, where the wave-per-pose kernel touches H cache lines per pose.
constexpr int POSE_MIN_LANE_N = 8192;
__global__ void pose_min_kernel(const double *__restrict__ err, int B, int N, long long row_offset,
                                double *__restrict__ best, int *__restrict__ best_h) {
    err += (size_t)blockIdx.y * B; best += (size_t)blockIdx.y * N; best_h += (size_t)blockIdx.y * N;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    long long h0 = (row_offset - n + N - 1) / N;
    if (row_offset <= n) h0 = 0;
    double e = __builtin_huge_val();
    int hi = -1;
    for (long long h = h0;; ++h) {
        const long long loc = h * N + n - row_offset;
        if (loc >= B) break;
        const double v = err[loc];
        if (min_takes(v, (int)h, e, hi)) { e = v; hi = (int)h; }
    }
    best[n] = (hi >= 0) ? e : __builtin_huge_val();
#ifdef ZEDO_MUT_PMIN_LANE_H   // tools/mutation_check.py only: the hypothesis is counted from the shard's first one
    best_h[n] = hi >= 0 ? hi - (int)h0 : hi;
#else
    best_h[n] = hi;
#endif
}

// Many poses (N >= POSE_MIN_LANE_N), J = 17, round 6: the row errors POSE-MAJOR.  One wave per (64 consecutive poses, chunk of the local
// hypotheses): the poses' ground truth is staged once (26 KB, coalesced) and stays in the LDS while the wave walks its hypotheses in
// ascending order; the 64 rows of hypothesis h are 13 KB of contiguous pose tensor, fetched with 16-byte loads into registers one
// hypothesis AHEAD of the arithmetic and dropped into the LDS behind it (a lane then reads its own row at an odd word stride: conflict
// free).  Where the row-major kernel reads a pose's ground truth once per ROW (from the L2), this reads it once per chunk.  The hypotheses
// are cut into chunks only to have enough workgroups to balance over the chip (1 108 pose tiles alone are 1.08 rounds of 1 024 resident
// waves: the second round would run 8 % full); the arg-min over hypotheses follows in pose_min_kernel (28 MB of errors, coalesced).
// Same row_error statements as every other kernel of this file: the same bits
// (tests/test_hip_parity.py::test_selection_pose_major_kernel_is_bitwise_the_row_major_pair).
constexpr int SEL_CHUNKS = (RE_ROWS * RE_D + 3) / 4 + 1;          // 16-byte chunks that cover 64 rows at any 4-byte alignment of their first element
constexpr int SEL_T = (SEL_CHUNKS + RE_ROWS - 1) / RE_ROWS;       // per lane
template <bool BOTH>
__global__ __launch_bounds__(RE_ROWS) void row_error17_pose_major_kernel(const float *__restrict__ pred, const double *__restrict__ gt, int B, int N,
                                                                          long long row_offset, int procrustes, int h_per_chunk,
                                                                          double *__restrict__ err) {
    __shared__ double sg[RE_ROWS * RE_D];
    __shared__ __attribute__((aligned(16))) float sp[SEL_CHUNKS * 4];
    const int lane = threadIdx.x, n0 = blockIdx.x * RE_ROWS, n = n0 + lane;
    const int poses = min(RE_ROWS, N - n0);
    const long long total = (long long)B * RE_D;                   // floats of the local pose tensor
    const long long h_lo = row_offset / N + (long long)blockIdx.y * h_per_chunk;
    const long long h_hi = min((row_offset + B - 1) / N, h_lo + h_per_chunk - 1);
    if (h_lo > h_hi) return;
    for (int q = lane; q < poses * RE_D; q += RE_ROWS) sg[q] = gt[(size_t)n0 * RE_D + q];
    __builtin_amdgcn_wave_barrier();                               // one wave: no instruction, the compiler may not move LDS accesses across it
    // chunk c of hypothesis h: floats [a + 4 c, a + 4 c + 4) of the tensor, a = the first element of the tile rounded down to a multiple of 4
    f32x4 nxt[SEL_T];
    auto fetch = [&](long long h) {
        const long long e0 = (h * N + n0 - row_offset) * RE_D, a = e0 & ~3LL;
#pragma unroll
        for (int t = 0; t < SEL_T; ++t) {
            const int c = lane + t * RE_ROWS;
            const long long lo = a + 4LL * c;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c < SEL_CHUNKS) {
                if (lo >= 0 && lo + 3 < total) v = *reinterpret_cast<const f32x4 *>(pred + lo);
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (lo + e >= 0 && lo + e < total) v[e] = pred[lo + e];
            }
            nxt[t] = v;
        }
    };
    auto drop = [&]() {
#pragma unroll
        for (int t = 0; t < SEL_T; ++t) {
            const int c = lane + t * RE_ROWS;
            if (c < SEL_CHUNKS) *reinterpret_cast<f32x4 *>(sp + 4 * c) = nxt[t];
        }
    };
    fetch(h_lo);
    for (long long h = h_lo; h <= h_hi; ++h) {
        drop();                                                    // tile h: registers -> LDS (one wave: LDS operations execute in order)
        __builtin_amdgcn_wave_barrier();
        if (h < h_hi) fetch(h + 1);                                // tile h + 1 on its way while tile h is worked on
        const long long loc = h * N + n - row_offset;
        if (n < N && loc >= 0 && loc < B) {
            const int shift = (int)(((h * N + n0 - row_offset) * RE_D) & 3LL);
            store_row_error<BOTH>(sp + shift + lane * RE_D, sg + lane * RE_D, 17, procrustes, err, loc, B);   // (BOTH: sp / sg read twice, here)
        }
        __builtin_amdgcn_wave_barrier();                           // the next drop() overwrites what the lanes have just read
    }
}

hipError_t launch_pose_min(const double *err, int B, int N, long long row_offset, double *best, int *best_h, hipStream_t st, int protocols) {
    if (N >= POSE_MIN_LANE_N) hipLaunchKernelGGL(pose_min_kernel, dim3((N + 127) / 128, protocols), dim3(128), 0, st, err, B, N, row_offset, best, best_h);
    else hipLaunchKernelGGL(pose_min_wave_kernel, dim3((N + 3) / 4, protocols), dim3(256), 0, st, err, B, N, row_offset, best, best_h);
    return hipGetLastError();
}

// ---- selection without ground truth (zedo_min_reproj): the confidence-weighted mean reprojection distance of x + T, in pixels -------
// Reprojection error of one row from its operands: p = the row's J*3 fp32 coordinates, T = its 3 translation components, uv = its pose's
// J*2 detections, K = the pose's 3x3 intrinsics (row-major, all nine entries: the full product of RotOpt.forward,
// simple_zeroshot_opt.py:20-25), cf = the pose's J confidences (read only when has_conf).  fp64 on the fp32 inputs; the weight is the
// clamp of gradient_field_gen (:64-66: above 1 -> 1, below 1e-4 -> 1e-4, NaN stays NaN) at the first power, taken in fp32.  A joint at or
// behind the camera plane (q.z <= 0) makes the row +inf; a NaN falls through that test and ends in the quotient.  The operands are plain
// indexed reads (global memory or the LDS): both kernels below run these statements and return the same bits.
// The per-joint part, the one copy every kernel of this section runs (zedo_min_reproj and zedo_joint_reproj): the distance in pixels
// between the projection of (X, Y, Z) = x[b,j] + T[b] through K (k[9], row-major) and the detection (u, v); `behind` is set when the
// joint is at or behind the camera plane (the value returned is then whatever the quotient gives: the caller replaces it).
__device__ __forceinline__ double joint_reproj_dist(const double (&k)[9], double X, double Y, double Z, double u, double v, bool &behind) {
    const double qx = k[0] * X + k[1] * Y + k[2] * Z, qy = k[3] * X + k[4] * Y + k[5] * Z, qz = k[6] * X + k[7] * Y + k[8] * Z;
    behind = qz <= 0.0;
    const double dx = qx / qz - u, dy = qy / qz - v;
    return sqrt(dx * dx + dy * dy);
}

template <class P, class TT, class O>
__device__ __forceinline__ double row_reproj_error(const P &p, const TT &T, const O &uv, const O &K, const O &cf, bool has_conf, int J) {
    const double k[9] = {K[0], K[1], K[2], K[3], K[4], K[5], K[6], K[7], K[8]};
    const double t0 = T[0], t1 = T[1], t2 = T[2];
    double num = 0.0, den = 0.0;
    bool behind = false;
    for (int j = 0; j < J; ++j) {
        bool bj;
        const double d = joint_reproj_dist(k, (double)p[3 * j] + t0, (double)p[3 * j + 1] + t1, (double)p[3 * j + 2] + t2,
                                           (double)uv[2 * j], (double)uv[2 * j + 1], bj);
        behind |= bj;
        double w = 1.0;
        if (has_conf) {
            float c = cf[j];
            if (c > 1.0f) c = 1.0f;
            if (c < 1e-4f) c = 1e-4f;
            w = (double)c;
#ifdef ZEDO_MUT_REPROJ_WEIGHT   // tools/mutation_check.py only: every joint weighs 1 although confidences were given
            w = 1.0;
#endif
        }
        num += w * d;
        den += w;
    }
    if (behind) return __builtin_huge_val();
    return num / den;
}

// Any joint count, any alignment of x: one lane per row straight from global memory; the per-pose operands come through the L2.
__global__ __launch_bounds__(128) void row_reproj_kernel(const float *__restrict__ x, const float *__restrict__ T, const float *__restrict__ uv,
                                                         const float *__restrict__ K, const float *__restrict__ conf, int B, int N, int J,
                                                         long long row_offset, double *__restrict__ err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const size_t n = (size_t)((row_offset + b) % N);
    const float *cf = conf ? conf + n * J : uv;                    // (not read without confidences)
    err[b] = row_reproj_error(x + (size_t)b * J * 3, T + (size_t)b * 3, uv + n * J * 2, K + n * 9, cf, conf != nullptr, J);
}

// J = 17: the 64 rows of a wave staged through the LDS exactly as row_error17_kernel stages them (one contiguous 13 KB piece, 16-byte
// loads, [row][51]); the rows' per-pose operands - 34 detections, 9 intrinsics, 17 confidences = 60 floats of three arrays, consecutive
// poses wrapping behind N - 1 - by lanes 0..59, one float each per row (240 contiguous bytes in three pieces), into [row][61]: an odd
// row stride again, a lane reading its own row is bank-conflict free.  T is 12 bytes per row, read by the row's lane from global memory
// (768 contiguous bytes per wave).
constexpr int RP_UV = 0, RP_K = 34, RP_CF = 43, RP_OPS = 60, RP_LD = 61;
static_assert(RP_OPS <= RE_ROWS && RP_LD > RP_OPS && (RP_LD & 1), "one lane per operand float, odd row stride");
__global__ __launch_bounds__(RE_ROWS) void row_reproj17_kernel(const float *__restrict__ x, const float *__restrict__ T, const float *__restrict__ uv,
                                                               const float *__restrict__ K, const float *__restrict__ conf, int B, int N,
                                                               long long row_offset, double *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) float sp[RE_ROWS * RE_D];
    __shared__ float so[RE_ROWS * RP_LD];
    const int tid = threadIdx.x, b0 = blockIdx.x * RE_ROWS;
    const int rows = min(RE_ROWS, B - b0);
    const int nf = rows * RE_D;                                   // floats of this tile (the last tile of a batch is short)
    const float *src = x + (size_t)b0 * RE_D;                     // 16-byte aligned: b0 * 204 bytes, b0 a multiple of 64
    for (int c = tid; c * 4 + 3 < nf; c += RE_ROWS) *reinterpret_cast<f32x4 *>(sp + c * 4) = *reinterpret_cast<const f32x4 *>(src + c * 4);
    if (tid < (nf & 3)) sp[(nf & ~3) + tid] = src[(nf & ~3) + tid];
    const float *op = nullptr;                                    // this lane's float of a pose's operands, `stride` floats from pose to pose
    int stride = 0;
    if (tid < RP_K) { op = uv + tid; stride = 34; }
    else if (tid < RP_CF) { op = K + (tid - RP_K); stride = 9; }
    else if (tid < RP_OPS && conf) { op = conf + (tid - RP_CF); stride = 17; }
    int n = (int)((row_offset + b0) % N);                         // wave-uniform, advanced by increment / compare as in row_error17_kernel
    if (op) {
#pragma unroll 16
        for (int r = 0; r < rows; ++r) {
            so[r * RP_LD + tid] = op[(size_t)n * stride];
            n = (n + 1 == N) ? 0 : n + 1;
        }
    }
    __syncthreads();                                              // the lanes read what other lanes have staged
    if (tid < rows) {
        const float *o = so + tid * RP_LD;
        err[b0 + tid] = row_reproj_error(sp + tid * RE_D, T + (size_t)(b0 + tid) * 3, o + RP_UV, o + RP_K, o + RP_CF, conf != nullptr, 17);
    }
}

hipError_t launch_min_reproj(const float *x, const float *T, const float *uv, const float *K, const float *conf, int B, int N, int J,
                             long long row_offset, double *err, double *best, int *best_h, hipStream_t st) {
    // (the staged kernel fetches the pose tensor with 16-byte loads: a row pointer that is not 16-byte aligned takes the generic kernel)
    if (J == 17 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
        hipLaunchKernelGGL(row_reproj17_kernel, dim3((B + RE_ROWS - 1) / RE_ROWS), dim3(RE_ROWS), 0, st, x, T, uv, K, conf, B, N, row_offset, err);
    else
        hipLaunchKernelGGL(row_reproj_kernel, dim3((B + 127) / 128), dim3(128), 0, st, x, T, uv, K, conf, B, N, J, row_offset, err);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_pose_min(err, B, N, row_offset, best, best_h, st);
}

// ---- joint-wise aggregation without ground truth (zedo_joint_reproj, zedo_joint_compose) ----------------------------------------------
// Per (pose, joint) the hypothesis whose joint reprojects closest to its detection: d[b,j] = joint_reproj_dist of x[b,j] + T[b], +inf
// for a joint at or behind the camera plane (that joint only), no confidences (a joint's weight is the same for every hypothesis of its
// pose).  [B,J] flattened is an error vector over B*J rows with N*J "poses" and row offset row_offset*J: the selection is zedo_pose_min's.
//
// The walking route (d_jerr == NULL): one lane per (pose, joint) p = n*J + j.  For a fixed hypothesis the elements
// x[h,n,j,:] over p are contiguous, so the 64 lanes of a wave read 768 contiguous bytes of x per hypothesis (12 per lane) and their
// poses' T (12 bytes, shared by the J lanes of a pose) - no staging.  uv[n,j] and K[n] stay in registers, the next hypothesis's loads
// are issued before the current one's fp64 arithmetic, the running minimum and its hypothesis stay in registers: 12 bytes written per
// lane at the end, no [B,J] intermediate, no LDS, no scratch.  Hypotheses are visited in ascending order, so "takes over" below is
// min_takes for a candidate with a higher index than the holder: the bits of launch_pose_min on the row kernel's vector.
__global__ __launch_bounds__(256) void joint_reproj_walk_kernel(const float *__restrict__ x, const float *__restrict__ T, const float *__restrict__ uv,
                                                                const float *__restrict__ K, int B, int N, int J, long long row_offset,
                                                                double *__restrict__ best, int *__restrict__ best_h) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N * J) return;
    const int n = p / J;
    const double u = uv[2 * (size_t)p], v = uv[2 * (size_t)p + 1];
    const float *Kn = K + (size_t)n * 9;
    const double k[9] = {Kn[0], Kn[1], Kn[2], Kn[3], Kn[4], Kn[5], Kn[6], Kn[7], Kn[8]};
    long long h = (row_offset - n + N - 1) / N;                   // first hypothesis with h*N + n >= row_offset
    if (row_offset <= n) h = 0;
    long long loc = h * N + n - row_offset;                        // local row of (h, n): >= 0; the pose's next one is N further
    const float *xe = x + ((size_t)loc * J + (p - n * J)) * 3;     // (loc < B is tested before anything is read through these)
    const float *Te = T + (size_t)loc * 3;
    const size_t xs = (size_t)N * J * 3, Ts = (size_t)N * 3;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (loc < B) { c0 = xe[0]; c1 = xe[1]; c2 = xe[2]; t0 = Te[0]; t1 = Te[1]; t2 = Te[2]; }
    double e = __builtin_huge_val();
    int hi = -1;
    for (; loc < B; loc += N, ++h) {
        // hypothesis h + 1 on its way while h is worked on.  Unconditional loads: behind a branch the compiler waits for them at the join,
        // before the arithmetic; the last hypothesis re-reads its own 24 bytes instead (a valid address, a cache hit, values not used)
        if (loc + N < B) { xe += xs; Te += Ts; }
        const float n0 = xe[0], n1 = xe[1], n2 = xe[2], s0 = Te[0], s1 = Te[1], s2 = Te[2];
        bool behind;
        double d = joint_reproj_dist(k, (double)c0 + (double)t0, (double)c1 + (double)t1, (double)c2 + (double)t2, u, v, behind);
        if (behind) d = __builtin_huge_val();
        bool takes;
        if (hi < 0) takes = true;
        else if (e != e) takes = false;                            // a NaN holds: the lowest NaN hypothesis is reported
        else if (d != d) takes = true;                             // NaN wins
        else
#ifdef ZEDO_MUT_JOINT_TIE   // tools/mutation_check.py only: ties to the HIGHER hypothesis index
            takes = d <= e;
#else
            takes = d < e;
#endif
        if (takes) { e = d; hi = (int)h; }
        c0 = n0; c1 = n1; c2 = n2; t0 = s0; t1 = s1; t2 = s2;
    }
    best[p] = e;                                                   // (+inf when the pose has no local row)
    best_h[p] = hi;
}

// The row route (d_jerr != NULL): one lane per element (b, j) of d [B,J] - x, uv and d are read / written contiguously by a wave at any
// alignment of x and any J, K[n] and T[b] come through the L2 - then launch_pose_min on the flattened vector.
__global__ __launch_bounds__(256) void joint_reproj_rows_kernel(const float *__restrict__ x, const float *__restrict__ T, const float *__restrict__ uv,
                                                                const float *__restrict__ K, int B, int N, int J, long long row_offset,
                                                                double *__restrict__ jerr) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B * J) return;
    const int b = q / J, j = q - b * J;
    const size_t n = (size_t)((row_offset + b) % N);
    const float *Kn = K + n * 9, *xe = x + (size_t)q * 3, *Te = T + (size_t)b * 3, *uve = uv + (n * J + j) * 2;
    const double k[9] = {Kn[0], Kn[1], Kn[2], Kn[3], Kn[4], Kn[5], Kn[6], Kn[7], Kn[8]};
    bool behind;
    const double d = joint_reproj_dist(k, (double)xe[0] + (double)Te[0], (double)xe[1] + (double)Te[1], (double)xe[2] + (double)Te[2],
                                       (double)uve[0], (double)uve[1], behind);
    jerr[q] = behind ? __builtin_huge_val() : d;
}

hipError_t launch_joint_reproj(const float *x, const float *T, const float *uv, const float *K, int B, int N, int J, long long row_offset,
                               double *jerr, double *best, int *best_h, hipStream_t st) {
    if (!jerr) {
        hipLaunchKernelGGL(joint_reproj_walk_kernel, dim3((N * J + 255) / 256), dim3(256), 0, st, x, T, uv, K, B, N, J, row_offset, best, best_h);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(joint_reproj_rows_kernel, dim3((B * J + 255) / 256), dim3(256), 0, st, x, T, uv, K, B, N, J, row_offset, jerr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_pose_min(jerr, B * J, N * J, row_offset * J, best, best_h, st);
}

// The assembled pose: joint (n, j) taken from hypothesis joint_h[n,j] of ALL rows x [H*N,J,3], T [H*N,3], in the camera frame
// (ref_h == nullptr) or brought back into the root-relative frame of hypothesis ref_h[n]; fp64 on the fp32 inputs, rounded once.  An
// index outside 0 .. H-1 makes the joint NaN and is never used as an address.  One lane per output joint.
__global__ __launch_bounds__(256) void joint_compose_kernel(const float *__restrict__ x, const float *__restrict__ T, const int *__restrict__ joint_h,
                                                            const int *__restrict__ ref_h, int H, int N, int J, float *__restrict__ pose) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N * J) return;
    const int n = p / J, j = p - n * J;
    const int jh = joint_h[p], rh = ref_h ? ref_h[n] : 0;
    float *o = pose + (size_t)p * 3;
    if (jh < 0 || jh >= H || rh < 0 || rh >= H) {
        o[0] = o[1] = o[2] = __builtin_nanf("");
        return;
    }
    const size_t g = (size_t)jh * N + n, r = (size_t)rh * N + n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = (double)x[(g * J + j) * 3 + c] + (double)T[g * 3 + c];
        if (ref_h) a = a - (double)T[r * 3 + c];
        o[c] = (float)a;
    }
}

hipError_t launch_joint_compose(const float *x, const float *T, const int *joint_h, const int *ref_h, int H, int N, int J, float *pose,
                                hipStream_t st) {
    hipLaunchKernelGGL(joint_compose_kernel, dim3((N * J + 255) / 256), dim3(256), 0, st, x, T, joint_h, ref_h, H, N, J, pose);
    return hipGetLastError();
}

// The one dispatch of the row-error kernels (zedo_min_mpjpe: BOTH = false; zedo_min_mpjpe_both: BOTH = true, err [2][B]).
template <bool BOTH>
static hipError_t launch_row_errors(const float *pred, const double *gt, int B, int N, int J, long long row_offset, int procrustes,
                                    double *err, hipStream_t st) {
    // (the staged kernels fetch the pose tensor with 16-byte loads: a row pointer that is not 16-byte aligned takes the generic kernel)
    const bool aligned = (reinterpret_cast<uintptr_t>(pred) & 15) == 0;
    if (J == 17 && aligned && N >= POSE_MIN_LANE_N) {              // many poses: the row errors pose-major
        const int tiles = (N + RE_ROWS - 1) / RE_ROWS;
        const long long h_local = (row_offset + B - 1) / N - row_offset / N + 1;              // hypotheses this shard touches
        // enough workgroups for ~8 rounds of the resident waves (4 per CU: 39 KB of LDS each), at least 2 hypotheses per chunk
        long long chunks = (8LL * 4 * num_cus() + tiles - 1) / tiles;
        chunks = std::max(1LL, std::min(chunks, (h_local + 1) / 2));
        const int per = (int)((h_local + chunks - 1) / chunks);
        chunks = (h_local + per - 1) / per;
        hipLaunchKernelGGL(row_error17_pose_major_kernel<BOTH>, dim3(tiles, (unsigned)chunks), dim3(RE_ROWS), 0, st, pred, gt, B, N, row_offset, procrustes, per, err);
    } else
    if (J == 17 && aligned)
        hipLaunchKernelGGL(row_error17_kernel<BOTH>, dim3((B + RE_ROWS - 1) / RE_ROWS), dim3(RE_ROWS), 0, st, pred, gt, B, N, row_offset, procrustes, err);
    else
        hipLaunchKernelGGL(row_error_kernel<BOTH>, dim3((B + 127) / 128), dim3(128), 0, st, pred, gt, B, N, J, row_offset, procrustes, err);
    return hipGetLastError();
}

// both: err [2][B], best / best_h [2][N], protocol-major (`procrustes` is not read); otherwise the one protocol asked for
hipError_t launch_min_mpjpe(const float *pred, const double *gt, int B, int N, int J, long long row_offset,
                            int procrustes, bool both, double *err, double *best, int *best_h, hipStream_t st) {
    const hipError_t e = both ? launch_row_errors<true>(pred, gt, B, N, J, row_offset, 0, err, st)
                              : launch_row_errors<false>(pred, gt, B, N, J, row_offset, procrustes, err, st);
    if (e != hipSuccess) return e;
    return launch_pose_min(err, B, N, row_offset, best, best_h, st, both ? 2 : 1);
}

}  // namespace zedo
