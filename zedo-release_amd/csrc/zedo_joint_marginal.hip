// Fusing hypotheses along a video for gfx950 (zedo_joint_marginal): the sum-product twin of zedo_joint_temporal.hip.  For every joint of
// every clip the posterior marginals of the hypotheses under the chain model the Viterbi recurrence optimises, at a temperature tau -
// forward-backward in the log domain, fp64 - and from them the posterior mean position, its covariance and the most probable hypothesis
// of every (frame, joint).  Three kernels:
//   joint_temporal_dead_kernel      (zedo_joint_temporal.hip) one lane per (frame, joint): does it have a finite unary at all?
//   joint_marginal_forward_kernel   A[n,j,.], one workgroup per (clip, joint), written to the workspace
//   joint_marginal_backward_kernel  B[n,j,.] from the clip's end, one workgroup per (clip, joint); B never leaves the LDS: the marginals,
//                                   the mean, the covariance and the arg-max of a frame are formed where its B is
// Both recurrences are a Viterbi scan with (min, +) replaced by (log-sum-exp, +), on the lane split of zedo_chain.h (whose clip
// prologue and reductions they use as well): two barriers per frame, the next frame fetched before the first of them.  A log-sum-exp
// takes two walks over the h': the first finds the largest term, the second adds exp(term - largest) in ascending h' - shifted by
// the TRUE maximum of the terms, so at a small tau the largest term contributes exactly 1 and nothing that matters underflows.  The
// transition cost of a pair is recomputed in the second walk (one square root of three terms) rather than kept.  With P > 1 every part
// shifts by its own maximum and part 0 combines (max_p, sum_p) in ascending part order.  Sums over the hypotheses of a frame (log Z, the
// mean, the covariance) are block_sum's: a fixed order, no atomics.
#include "zedo_chain.h"

namespace zedo {

// The forward recurrence of one (clip, joint) on ChainLanes<P, K>: the lane (part, slot) owns h = slot + k SLOTS of frame n and walks its
// part of the h' of frame n-1, which sits in the LDS.  (A lane past H reads hypothesis H-1 and stores nothing.)
//   l[n,j,h] = -u[n,j,h] / tau, -inf where the unary is not finite
//   chain start (first frame of the clip, or (n-1, j) dead):  A[n,j,h] = l[n,j,h]
//   otherwise:  A[n,j,h] = l[n,j,h] + LSE_h' (A[n-1,j,h'] - c m[n,j,h',h]),  c = lambda / tau
//   dead (n, j): A[n,j,.] = -inf
template <int P, int K>
__global__ __launch_bounds__(CHAIN_T) void joint_marginal_forward_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                      const float *__restrict__ Tr, const int *__restrict__ seq_start,
                                                                      const int *__restrict__ dead, int H, int N, int J, double c, double tau,
                                                                      double *__restrict__ A) {
    using L = ChainLanes<P, K>;
    constexpr int SLOTS = L::SLOTS;
    __shared__ double sX[L::CAP * 3], sV[L::CAP];
    __shared__ double sPm[CHAIN_T], sPs[CHAIN_T];                        // the parts' maxima and sums (P > 1)
    const int tid = threadIdx.x;
    const L ln(tid, H);
    const int part = ln.part, slot = ln.slot;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;                                            // (workgroup-uniform)
    const double ninf = -__builtin_huge_val();
    double xn[K][3], un[K] = {};
    auto fetch = [&](int n) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const size_t g = (size_t)min(slot + k * SLOTS, H - 1) * N + n;
            load_cam(x, Tr, g, J, j, xn[k]);
            if (P == 1 || part == 0) un[k] = junary[g * J + j];    // only the owners use the unary
        }
    };
    fetch(a);
    for (int n = a; n < b; ++n) {
        double xc[K][3], uc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uc[k] = un[k];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) xc[k][cc] = xn[k][cc];
        }
        fetch(min(n + 1, b - 1));                                  // unconditional (the last frame re-reads its own): in flight over the barriers
        const size_t nj = (size_t)n * J + j;
        const bool is_dead = dead[nj] != 0, start = (n > a ? dead[nj - J] : 1) != 0;      // (dead[] is read inside the clip only)
        const bool chain = !is_dead && !start;                     // (workgroup-uniform)
        double mx[K], sm[K];
        __syncthreads();                                           // A: X[n-1,.] and A[n-1,.] are in the LDS
        if (chain) {
            jm_walk<K>(sX, sV, ln.q0, ln.q1, xc, c, mx, sm);
            if (P > 1) { sPm[tid] = mx[0]; sPs[tid] = sm[0]; }
        }
        __syncthreads();                                           // B: frame n-1 has been read by every lane
        if (part == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int h = slot + k * SLOTS;
                if (h < H) {
                    ZEDO_CHAIN_FORWARD_VALUE(k)
                    A[nj * H + h] = v;
                    sV[h] = v;
                    sX[h * 3] = xc[k][0]; sX[h * 3 + 1] = xc[k][1]; sX[h * 3 + 2] = xc[k][2];
                }
            }
        }
    }
}

// The backward recurrence of one (clip, joint) from the clip's last frame, with everything that is read off a frame's marginals.  The
// LDS holds X[n+1,.] and l[n+1,j,.] + B[n+1,j,.]; the lane that owns h walks the h'.
//   chain end (last frame of the clip, or (n+1, j) dead):  B[n,j,h] = 0,  log Z = LSE_h A[n,j,h]  (kept for the frames of the chain)
//   otherwise:  B[n,j,h] = LSE_h' (l[n+1,j,h'] + B[n+1,j,h'] - c m[n+1,j,h,h'])
//   w[n,j,h] = exp(A[n,j,h] + B[n,j,h] - log Z): exactly 0 for an excluded hypothesis (A = -inf)
//   mean = sum_h w X;  cov = sum_h w (X - mean)(X - mean)^T, from the centred differences;  hmax = the lowest h with the largest w
template <int P, int K>
__global__ __launch_bounds__(CHAIN_T) void joint_marginal_backward_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                       const float *__restrict__ Tr, const int *__restrict__ seq_start,
                                                                       const int *__restrict__ dead, const double *__restrict__ A, int H,
                                                                       int N, int J, double c, double tau, double *__restrict__ mean,
                                                                       double *__restrict__ cov, int *__restrict__ hmax,
                                                                       double *__restrict__ wmax, double *__restrict__ logz,
                                                                       double *__restrict__ wout) {
    using L = ChainLanes<P, K>;
    constexpr int SLOTS = L::SLOTS;
    __shared__ double sX[L::CAP * 3], sV[L::CAP];
    __shared__ double sPm[CHAIN_T], sPs[CHAIN_T];
    __shared__ double sred[CHAIN_W * 6];
    __shared__ int sredi[CHAIN_W];
    const int tid = threadIdx.x;
    const L ln(tid, H);
    const int part = ln.part, slot = ln.slot;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;                                            // (workgroup-uniform)
    const double ninf = -__builtin_huge_val(), qnan = __builtin_nan("");
    double xn[K][3], un[K] = {}, an[K] = {};
    auto fetch = [&](int n) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int h = min(slot + k * SLOTS, H - 1);
            const size_t g = (size_t)h * N + n;
            load_cam(x, Tr, g, J, j, xn[k]);
            if (P == 1 || part == 0) {                             // only the owners use the unary and A: the other parts walk with X alone
                un[k] = junary[g * J + j];
                an[k] = A[((size_t)n * J + j) * H + h];
            }
        }
    };
    fetch(b - 1);
    double lz = ninf;                                              // log Z of the chain the walk is in
    for (int n = b - 1; n >= a; --n) {
        double xc[K][3], uc[K], ac[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uc[k] = un[k];
            ac[k] = an[k];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) xc[k][cc] = xn[k][cc];
        }
        fetch(max(n - 1, a));                                      // unconditional (the first frame re-reads its own): in flight over the barriers
        const size_t nj = (size_t)n * J + j;
        const bool is_dead = dead[nj] != 0, ends = (n + 1 < b ? dead[nj + J] : 1) != 0;   // (dead[] is read inside the clip only)
        const bool chain = !is_dead && !ends;                      // (workgroup-uniform) frame n+1 continues this chain
        double mx[K], sm[K];
        __syncthreads();                                           // A: X[n+1,.] and (l + B)[n+1,.] are in the LDS
        if (chain) {
            jm_walk<K>(sX, sV, ln.q0, ln.q1, xc, c, mx, sm);
            if (P > 1) { sPm[tid] = mx[0]; sPs[tid] = sm[0]; }
        }
        __syncthreads();                                           // B: frame n+1 has been read by every lane
        double ab[K];                                              // A + B of this lane's hypotheses (-inf: excluded, or nobody's)
#pragma unroll
        for (int k = 0; k < K; ++k) ab[k] = ninf;
        if (part == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int h = slot + k * SLOTS;
                if (h < H) {
                    const double l = finite64(uc[k]) ? -uc[k] / tau : ninf;
#ifdef ZEDO_MUT_JM_NO_BACKWARD   // tools/mutation_check.py only: B = 0 on every frame - the filtering marginals, not the smoothed ones
                    const double Bv = 0.0;
#else
                    const double Bv = chain ? jm_combine<P>(mx[k], sm[k], sPm, sPs, SLOTS, slot, ln.np) : 0.0;
#endif
                    sV[h] = is_dead ? ninf : l + Bv;
                    sX[h * 3] = xc[k][0]; sX[h * 3 + 1] = xc[k][1]; sX[h * 3 + 2] = xc[k][2];
                    ab[k] = is_dead ? ninf : ac[k] + Bv;
                }
            }
        }
        if (is_dead) {                                             // (workgroup-uniform) NaN, hypothesis 0, weight 0, log Z = -inf, a row of zeros
            ZEDO_CHAIN_DEAD_OUTPUTS(K, slot, SLOTS, part == 0, nj)
            continue;
        }
        if (ends) {                                                // (workgroup-uniform) B = 0: log Z = LSE_h A[n,j,h], shifted by the largest A
            double v = ninf;
            int vh = INT_MAX;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (ab[k] > v) { v = ab[k]; vh = slot + k * SLOTS; }
            block_arg<true>(v, vh, sred, sredi, tid);
            __syncthreads();                                       // sred is block_sum's next
            double e[1] = {0.0};
#pragma unroll
            for (int k = 0; k < K; ++k) e[0] += exp(ab[k] - v);    // exp(-inf) = 0 for what is excluded or nobody's
            block_sum<1>(e, sred, tid);
            lz = v + log(e[0]);
        }
        ZEDO_CHAIN_MOMENTS(K, slot, SLOTS, part == 0 && h < H, exp(ab[k] - lz), xc, nj)
    }
}

// Workspace: A [N,J,H] f64 | dead [N,J] i32 (padded to 8 bytes)
struct JointMarginalWs {
    Carve c;
    double *A;
    int *dead;
    size_t bytes;
    JointMarginalWs(void *ws, size_t nj, size_t H) : c(ws), A(c.take<double>(nj * H)), dead(c.take<int>(nj)), bytes(c.bytes(8)) {}
};
size_t joint_marginal_bytes(int N, int H, int J) { return JointMarginalWs(nullptr, (size_t)N * J, H).bytes; }

hipError_t launch_joint_marginal(const double *junary, const float *x, const float *T, const int *seq_start, int n_seq, int H, int N, int J,
                                 double c, double tau, void *ws, double *mean, double *cov, int *hmax, double *wmax, double *logz, double *w,
                                 hipStream_t st) {
    const JointMarginalWs t(ws, (size_t)N * J, H);
    const dim3 grid((unsigned)n_seq * (unsigned)J);                // n_seq <= N and N J H <= INT_MAX
    const hipError_t e = launch_joint_temporal_dead(junary, H, N * J, t.dead, st);
    if (e != hipSuccess) return e;
    dispatch_pk(H, [&](auto P, auto K) {
        hipLaunchKernelGGL((joint_marginal_forward_kernel<P(), K()>), grid, dim3(CHAIN_T), 0, st, junary, x, T, seq_start, t.dead, H, N, J, c,
                           tau, t.A);
        hipLaunchKernelGGL((joint_marginal_backward_kernel<P(), K()>), grid, dim3(CHAIN_T), 0, st, junary, x, T, seq_start, t.dead, t.A, H, N, J,
                           c, tau, mean, cov, hmax, wmax, logz, w);
    });
    return hipGetLastError();
}

}  // namespace zedo
