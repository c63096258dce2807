// Fusing hypotheses along a video under the second-order motion model for gfx950 (zedo_joint_accel_marginal): the sum-product twin of
// zedo_joint_accel.hip, as zedo_joint_marginal.hip is the twin of zedo_joint_temporal.hip.  For every joint of every clip the posterior
// marginals of the hypotheses under the chain over PAIRS of hypotheses that zedo_joint_accel_select optimises, at a temperature tau -
// forward-backward over the H^2 pairs in the log domain, fp64 - and from them the posterior mean, its covariance and the most probable
// hypothesis of every (frame, joint).  Three kernels:
//   joint_temporal_dead_kernel             (zedo_joint_temporal.hip) one lane per (frame, joint): does it have a finite unary at all?
//   joint_accel_marginal_forward_kernel    A2[n][h',h], one workgroup per (clip, joint): joint_accel_scan_kernel with (min, +) replaced by
//                                          (log-sum-exp, +); the table of every frame goes to the workspace ([J,N,H,H] float64)
//   joint_accel_marginal_backward_kernel   B2[n][h',h] from the clip's end, one workgroup per (clip, joint); B2 and the pair marginals never
//                                          leave the LDS: a frame's marginals, mean, covariance and arg-max are formed where its B2 is
//                                          (zedo_chain.h's ZEDO_CHAIN_MOMENTS, shared with zedo_joint_marginal.hip); log Z of a chain is
//                                          reduced from A2 of its last frame, which this kernel reads anyway
// The H^2 pairs are dealt to the 256 lanes as in zedo_joint_accel.hip (dispatch_pairs: KA = 1, 2, 4, 7, 10, 13 or 16 pairs per lane).  A
// log-sum-exp over the third hypothesis takes two walks: the largest term, then the sum of exp(term - largest) in ascending order; the
// second difference and its square root are recomputed in the second walk rather than kept.
// LDS: forward 8 H^2 (A2[n-1]) + 3 x 24 H (X) + 2 x 8 H (l) + reductions = 38 400 bytes at the cap H = 64; backward 3 x 8 H^2 (B2, M, the
// pair marginals) + 3 x 24 H + 3 x 8 H + reductions = 104 656 bytes: below the 160 KiB of a CU, one workgroup per CU.
// Resources (hipcc -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage, gfx950), KA = 1, 2, 4, 7, 10, 13, 16: scratch 0 bytes per
// lane in all fourteen instantiations; forward 113, 117, 124, 236, 251, 256 + 41 and 256 + 96 registers (architectural + accumulation
// VGPRs: with one wave per SIMD a lane may hold 512, and the compiler parks the second walk's state in the accumulation half rather than
// in memory), 4, 4, 4, 2, 2, 1, 1 waves per SIMD; backward 184, 189, 207, 256 + 7, 256 + 74, 256 + 140 and 256 + 207, one wave per SIMD
// throughout (its LDS admits one workgroup per CU anyway).
// No atomics.
#include "zedo_chain.h"

namespace zedo {

// The forward recurrence of one (clip, joint): the lane layout, the LDS slots and the two barriers per frame of joint_accel_scan_kernel.
// In the LDS: the table A2[n-1] as sA[h'' H + h'] (h''-major: what frame n-1 wrote at its own q), X of frames n, n-1 and n-2 and
// l = -u / tau (-inf where the unary is not finite) of frames n and n-1.  A lane keeps g_c = X[n,h,c] - 2 X[n-1,h',c] of its pairs.
//   start (n first of its clip, or (n-1, j) dead), or (n, j) dead:  no table
//   second (n-1 is a start):  A2[n][h',h] = l[n-1,h'] + (l[n,h] - c_v m[n,h',h])
//   otherwise:  A2[n][h',h] = l[n,h] + (-c_v m[n,h',h] + LSE_h'' (A2[n-1][h'',h'] - c_a a[n,h'',h',h]))
template <int KA>
__global__ __launch_bounds__(CHAIN_T) void joint_accel_marginal_forward_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                            const float *__restrict__ Tr, const int *__restrict__ seq_start,
                                                                            const int *__restrict__ dead, int H, int N, int J, double c_v,
                                                                            double c_a, double tau, double *__restrict__ A2) {
    __shared__ double sA[JAM_CAP * JAM_CAP];
    __shared__ double sX[3][JAM_CAP * 3], sL[2][JAM_CAP];
    const int tid = threadIdx.x, HH = H * H;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;                                            // (workgroup-uniform)
    const double ninf = -__builtin_huge_val();
    int qh1[KA], qh0[KA];
    lane_pairs<KA>(tid, H, qh1, qh0);
    // X[n,h,j,.] and l[n,j,h] of hypothesis h = tid (a lane past H reads hypothesis H-1 and stores nothing)
    double xn[3], ln;
    auto fetch = [&](int n) {
        const size_t g = (size_t)min(tid, H - 1) * N + n;
        load_cam(x, Tr, g, J, j, xn);
        const double u0 = junary[g * J + j];
        ln = finite64(u0) ? -u0 / tau : ninf;
    };
    int s0 = 0, s1 = 2, s2 = 1;                                    // the slots of X[n], X[n-1], X[n-2]
    fetch(a);
    if (tid < H) {
        sX[s0][tid * 3] = xn[0]; sX[s0][tid * 3 + 1] = xn[1]; sX[s0][tid * 3 + 2] = xn[2];
        sL[a & 1][tid] = ln;
    }
    fetch(min(a + 1, b - 1));
    double *const A2_j = A2 + (size_t)j * N * HH;                  // A2 [J,N,H,H]: the frames of one chain are contiguous
    for (int n = a; n < b; ++n) {
        const double xc[3] = {xn[0], xn[1], xn[2]}, lc = ln;       // frame n+1
        fetch(min(n + 2, b - 1));                                  // unconditional: in flight over the barriers of this frame
        const size_t nj = (size_t)n * J + j;
        const bool is_dead = dead[nj] != 0, start = (n > a ? dead[nj - J] : 1) != 0;      // (dead[] is read inside the clip only)
        const bool second = !start && (n - 1 > a ? dead[nj - 2 * (size_t)J] : 1) != 0;
        const bool scan = !is_dead && !start;                      // (all workgroup-uniform)
        const double *X0 = sX[s0], *X1 = sX[s1], *X2 = sX[s2], *L0 = sL[n & 1], *L1 = sL[(n & 1) ^ 1];
        double an[KA];
        __syncthreads();                                           // A: A2[n-1], X[n], X[n-1], X[n-2], l[n], l[n-1] are in the LDS
        ZEDO_CHAIN_PAIR_FORWARD(KA)                                // the frame's value (zedo_chain.h): A2[n] of the lane's pairs into an
        __syncthreads();                                           // B: the LDS of frame n has been read by every lane
        if (scan) {
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                const int q = tid + k * CHAIN_T;
                if (q < HH) {
                    sA[q] = an[k];                                 // A2[n][h',h] at h' H + h: the next frame reads it h''-major
                    A2_j[(size_t)n * HH + q] = an[k];
                }
            }
        }
        if (tid < H) {
            sX[s2][tid * 3] = xc[0]; sX[s2][tid * 3 + 1] = xc[1]; sX[s2][tid * 3 + 2] = xc[2];
            sL[(n & 1) ^ 1][tid] = lc;
        }
        { const int t = s2; s2 = s1; s1 = s0; s0 = t; }
    }
}

// The backward recurrence of one (clip, joint) from the clip's last frame, with everything that is read off a frame's marginals.  In the
// LDS: sB = B2[n+1][h,h+] at h H + h+ (what frame n+1 wrote at its own q), X and l of frames n+1, n and n-1 (three rotating slots), the
// table M and the pair marginals of frame n.  x, T and junary of frame n-3 and A2[n-1] are fetched BEFORE the barriers of frame n.
//   chain of one frame:  log Z = LSE_h l[n,h],  w[n,h] = exp(l[n,h] - log Z)
//   chain end (n has pairs; the clip's last frame, or (n+1, j) dead):  B2[n] = 0,  log Z = LSE over all pairs of A2[n]
//   otherwise, once per frame:  M[h+][h] = (l[n+1,h+] - c_v m[n+1,h,h+]) + B2[n+1][h,h+], stored h+-major: the walk's lanes of consecutive h
//              read consecutive doubles; then  B2[n][h',h] = LSE_h+ (M[h+][h] - c_a a[n+1,h',h,h+]) - one square root per transition.  A lane
//              keeps X[n-1,h'] - 2 X[n,h] and adds X[n+1,h+]: the second difference in ANOTHER association than the forward pass
//   pi[n][h',h] = exp((A2[n][h',h] + B2[n][h',h]) - log Z) into the LDS;  w[n,h] = sum_h' pi[n][h',h], ascending, by lane h; the first
//              frame c0 of a chain has no table: w[c0,h'] = sum_h pi[c0+1][h',h], ascending, formed at frame c0+1
// exactly 0 for an excluded hypothesis (A2 = -inf).  The mean, the covariance, the arg-max and d_w: ZEDO_CHAIN_MOMENTS, by the first H lanes.
template <int KA>
__global__ __launch_bounds__(CHAIN_T) void joint_accel_marginal_backward_kernel(
    const double *__restrict__ junary, const float *__restrict__ x, const float *__restrict__ Tr, const int *__restrict__ seq_start,
    const int *__restrict__ dead, const double *__restrict__ A2, int H, int N, int J, double c_v, double c_a, double tau,
    double *__restrict__ mean, double *__restrict__ cov, int *__restrict__ hmax, double *__restrict__ wmax, double *__restrict__ logz,
    double *__restrict__ wout) {
    __shared__ double sB[JAM_CAP * JAM_CAP], sM[JAM_CAP * JAM_CAP], sP[JAM_CAP * JAM_CAP];
    __shared__ double sX[3][JAM_CAP * 3], sL[3][JAM_CAP];
    __shared__ double sred[CHAIN_W * 6];
    __shared__ int sredi[CHAIN_W];
    const int tid = threadIdx.x, HH = H * H;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;                                            // (workgroup-uniform)
    const double ninf = -__builtin_huge_val(), qnan = __builtin_nan("");
#ifdef ZEDO_MUT_JAM_NO_BACK_ACCEL   // tools/mutation_check.py only: the c_a a term dropped from the backward pass (the forward pass keeps it)
    const double c_a_back = 0.0 * c_a;
#else
    const double c_a_back = c_a;
#endif
    int qh1[KA], qh0[KA];
    lane_pairs<KA>(tid, H, qh1, qh0);
    const int hx = min(tid, H - 1);                                // a lane past H reads hypothesis H-1 and stores nothing
    double xn[3], ln, an[KA];
    auto fetch = [&](int n) {
        const size_t g = (size_t)hx * N + n;
        load_cam(x, Tr, g, J, j, xn);
        const double u0 = junary[g * J + j];
        ln = finite64(u0) ? -u0 / tau : ninf;
    };
    const double *const A2_j = A2 + (size_t)j * N * HH;
    auto fetch_table = [&](int n) {                                // (a frame without pairs: whatever the workspace holds, never used)
#pragma unroll
        for (int k = 0; k < KA; ++k) an[k] = A2_j[(size_t)n * HH + min(tid + k * CHAIN_T, HH - 1)];
    };
    auto put = [&](int s) {
        if (tid < H) {
            sX[s][tid * 3] = xn[0]; sX[s][tid * 3 + 1] = xn[1]; sX[s][tid * 3 + 2] = xn[2];
            sL[s][tid] = ln;
        }
    };
    int sp = 2, s0 = 0, s1 = 1;                                    // the slots of frames n+1, n, n-1
    fetch(b - 1);
    put(s0);
    fetch(max(b - 2, a));
    put(s1);
    fetch(max(b - 3, a));
    fetch_table(b - 1);
    double lz = ninf;                                              // log Z of the chain the walk is in
    for (int n = b - 1; n >= a; --n) {
        const double xc[3] = {xn[0], xn[1], xn[2]}, lc = ln;       // frame n-2
        double ac[KA];                                             // A2[n] of this lane's pairs
#pragma unroll
        for (int k = 0; k < KA; ++k) ac[k] = an[k];
        fetch(max(n - 3, a));                                      // unconditional: in flight over the barriers of this frame
        fetch_table(max(n - 1, a));
        const size_t nj = (size_t)n * J + j;
        const bool is_dead = dead[nj] != 0, start = (n > a ? dead[nj - J] : 1) != 0;      // (dead[] is read inside the clip only)
        const bool second = !start && (n - 1 > a ? dead[nj - 2 * (size_t)J] : 1) != 0;
        const bool ends = (n + 1 < b ? dead[nj + J] : 1) != 0;
        const bool pairs = !is_dead && !start;                     // (all workgroup-uniform) frame n has a table
        const double *Xp = sX[sp], *X0 = sX[s0], *X1 = sX[s1], *Lp = sL[sp], *L0 = sL[s0];
        ZEDO_CHAIN_PAIR_BACKWARD(KA, nj, true)                     // the frame's body (zedo_chain.h): B2[n], the pair marginals, the outputs
        if (tid < H) {                                             // frame n-2 into the slot of frame n+1: its last reader is above C
            sX[sp][tid * 3] = xc[0]; sX[sp][tid * 3 + 1] = xc[1]; sX[sp][tid * 3 + 2] = xc[2];
            sL[sp][tid] = lc;
        }
        { const int t = sp; sp = s0; s0 = s1; s1 = t; }
    }
}

// Workspace: A2 [J,N,H,H] f64 | dead [N,J] i32 (padded to 8 bytes)
struct JointAccelMarginalWs {
    Carve c;
    double *A2;
    int *dead;
    size_t bytes;
    JointAccelMarginalWs(void *ws, size_t nj, size_t H) : c(ws), A2(c.take<double>(nj * H * H)), dead(c.take<int>(nj)), bytes(c.bytes(8)) {}
};
size_t joint_accel_marginal_bytes(int N, int H, int J) { return JointAccelMarginalWs(nullptr, (size_t)N * J, H).bytes; }

hipError_t launch_joint_accel_marginal(const double *junary, const float *x, const float *T, const int *seq_start, int n_seq, int H, int N,
                                       int J, double c_v, double c_a, double tau, void *ws, double *mean, double *cov, int *hmax,
                                       double *wmax, double *logz, double *w, hipStream_t st) {
    const JointAccelMarginalWs t(ws, (size_t)N * J, H);
    const dim3 grid((unsigned)n_seq * (unsigned)J);                // n_seq <= N and N J H <= INT_MAX
    const hipError_t e = launch_joint_temporal_dead(junary, H, N * J, t.dead, st);
    if (e != hipSuccess) return e;
    dispatch_pairs(H, [&](auto KA) {
        hipLaunchKernelGGL((joint_accel_marginal_forward_kernel<KA()>), grid, dim3(CHAIN_T), 0, st, junary, x, T, seq_start, t.dead, H, N, J,
                           c_v, c_a, tau, t.A2);
        hipLaunchKernelGGL((joint_accel_marginal_backward_kernel<KA()>), grid, dim3(CHAIN_T), 0, st, junary, x, T, seq_start, t.dead, t.A2, H, N,
                           J, c_v, c_a, tau, mean, cov, hmax, wmax, logz, w);
    });
    return hipGetLastError();
}

}  // namespace zedo
