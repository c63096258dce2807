// Joint-wise fusion on a live video for gfx950 (zedo_joint_stream_marginal_push): the sum-product chain of zedo_joint_marginal.hip, fed in
// chunks, with A, X and l of the last lag + max_frames frames in caller-owned state and every frame's marginals formed `lag` frames after
// it went in - fixed-lag smoothing.  Per push, in stream order:
//   joint_stream_dead_kernel              (zedo_joint_stream.hip) one lane per (stream, chunk frame, joint): the dead flag, into the ring
//   joint_stream_marginal_forward_kernel  the forward recurrence of joint_marginal_forward_kernel, one workgroup per (stream, joint): the
//                                         same lanes, the same two barriers per frame, the same prefetch; its first frame continues from
//                                         the ring's row of the frame before; A, X and l of every frame go into the ring
//   joint_stream_marginal_emit_kernel     the backward recurrence of joint_marginal_backward_kernel from a frame's horizon down to it, one
//                                         workgroup per (stream, output row, joint); everything it reads comes from the ring, B never
//                                         leaves the LDS.  Frames of one (stream, joint) that share a horizon are served by ONE walk, that
//                                         of the lowest of them: the other workgroups return at once
//   joint_stream_advance_kernel           (zedo_joint_stream.hip) one lane per stream: d_emit and the clip's frame count
// The statements that decide a bit - jm_walk, jm_combine, the forward value, the moments, the dead outputs - are zedo_chain.h's, the ones
// the offline kernels run, on the same operands: X and l in the ring are the doubles the offline kernels form from x, T and u.  The ring
// holds lag + max_frames frames: frame m of a clip sits in row m % R, a push writes the rows of frames t .. t+F-1 and its emission reads
// frames >= max(0, t - lag) > t + F - 1 - R - rows this push has not overwritten.  No atomics, no scratch.
#include "zedo_chain.h"

namespace zedo {

// The state of S streams, R = lag + max_frames, SJ = S J:
//   A f64 [SJ,R,H] | X f64 [SJ,R,H,3] | l f64 [SJ,R,H] | t i64 [S] | dead i32 [SJ,R] | lastdead i32 [SJ]   (padded to 8)
// t: the frames of the stream's clip so far; max(0, t - lag) of them have been emitted.  t = 0 is all an empty stream needs: nothing
// else is read before it is written.
struct JointStreamMarginalState {
    Carve c;
    double *A, *X, *l;
    long long *t;
    int *dead, *lastdead;
    size_t bytes;
    JointStreamMarginalState(void *st, size_t S, size_t H, size_t J, size_t R)
        : c(st), A(c.take<double>(S * J * R * H)), X(c.take<double>(S * J * R * H * 3)), l(c.take<double>(S * J * R * H)),
          t(c.take<long long>(S)), dead(c.take<int>(S * J * R)), lastdead(c.take<int>(S * J)), bytes(c.bytes(8)) {}
};
size_t joint_stream_marginal_bytes(int S, int H, int J, int lag, int max_frames) {
    return JointStreamMarginalState(nullptr, S, H, J, (size_t)lag + max_frames).bytes;
}

// joint_marginal_forward_kernel on the F frames of stream s's chunk (rows n = s F + f of the call), continued from the ring: frame t + f
// of the clip.  "Chain start" is t + f == 0 or the frame before is dead - for f = 0 that flag is the state's lastdead, not the ring's
// (with lag = 0 and F = max_frames the dead kernel has just reused that row).  The previous frame's A and X are the ring's own row
// (t - 1) % R: the lane that owns h reads them into the LDS before it - or any lane - writes a row of this push (barrier A comes first).
template <int P, int K>
__global__ __launch_bounds__(CHAIN_T) void joint_stream_marginal_forward_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                                const float *__restrict__ Tr, int F, int H, int N, int J, int R,
                                                                                double c, double tau, const long long *__restrict__ tcount,
                                                                                double *__restrict__ A, double *__restrict__ X,
                                                                                double *__restrict__ Lg, const int *__restrict__ dead,
                                                                                int *__restrict__ lastdead) {
    using L = ChainLanes<P, K>;
    constexpr int SLOTS = L::SLOTS;
    __shared__ double sX[L::CAP * 3], sV[L::CAP];
    __shared__ double sPm[CHAIN_T], sPs[CHAIN_T];                        // the parts' maxima and sums (P > 1)
    const int tid = threadIdx.x;
    const L ln(tid, H);
    const int part = ln.part, slot = ln.slot;
    const int s = blockIdx.x / J, j = (int)blockIdx.x - s * J;
    const size_t sj = blockIdx.x;
    const long long t0 = clip_frames(tcount[s]);
    const int a = s * F, b = a + F;
    const double ninf = -__builtin_huge_val();
    double *const Ar = A + sj * R * H, *const Xr = X + sj * R * H * 3, *const lr = Lg + sj * R * H;
    const int *const dr = dead + sj * R;
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
    int prev_dead = t0 > 0 ? lastdead[sj] : 1;                     // (workgroup-uniform)
    int row = (int)(t0 % R);
    if (t0 > 0 && part == 0) {                                     // X[t-1,.] and A[t-1,.] of the clip: visible after barrier A
        const size_t prow = row == 0 ? R - 1 : row - 1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int h = slot + k * SLOTS;
            if (h < H) {
                sV[h] = Ar[prow * H + h];
                sX[h * 3] = Xr[(prow * H + h) * 3]; sX[h * 3 + 1] = Xr[(prow * H + h) * 3 + 1]; sX[h * 3 + 2] = Xr[(prow * H + h) * 3 + 2];
            }
        }
    }
    for (int n = a; n < b; ++n) {
        double xc[K][3], uc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uc[k] = un[k];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) xc[k][cc] = xn[k][cc];
        }
        fetch(min(n + 1, b - 1));                                  // unconditional (the last frame re-reads its own): in flight over the barriers
        const bool is_dead = dr[row] != 0, start = prev_dead != 0;
        const bool chain = !is_dead && !start;                     // (workgroup-uniform)
        const bool last = n + 1 == b;
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
                    const size_t at = (size_t)row * H + h;
                    Ar[at] = v;
                    lr[at] = l;
                    Xr[at * 3] = xc[k][0]; Xr[at * 3 + 1] = xc[k][1]; Xr[at * 3 + 2] = xc[k][2];
                    sV[h] = v;
                    sX[h * 3] = xc[k][0]; sX[h * 3 + 1] = xc[k][1]; sX[h * 3 + 2] = xc[k][2];
                }
            }
        }
        if (last && tid == 0) lastdead[sj] = is_dead ? 1 : 0;      // the next push continues from here
        prev_dead = is_dead ? 1 : 0;
        row = row + 1 == R ? 0 : row + 1;
    }
}

// One workgroup per (stream, output row r, joint): frame n = e0 + r of the clip, if the push emits it.  A dead (n, j) writes its dead
// outputs.  Otherwise the horizon eh = min(n + lag, the last frame of n's chain on the clip's t1 frames) comes from the ring's dead flags
// (64 per step, by ballot; every wave does the same), and `closed`: is eh that chain's last frame.  Frames of one chain whose horizon is
// eh are n itself and, if closed, every m with m + lag >= eh; the workgroup of the LOWEST of them that this push emits - r = 0, or
// (n-1, j) dead, or n - 1 + lag < eh - walks B from eh (B = 0, log Z = LSE_h A[eh,j,h]) down to n with X[m+1] and (l + B)[m+1] in the
// LDS, as joint_marginal_backward_kernel does, and forms the outputs of each of those frames where its B is; the others return.  All
// of [n, eh] is live and in the ring.  Everything the workgroup branches on is workgroup-uniform.
template <int P, int K>
__global__ __launch_bounds__(CHAIN_T) void joint_stream_marginal_emit_kernel(const long long *__restrict__ tcount, const int *__restrict__ flush,
                                                                             int F, int H, int J, int R, int lag, double c,
                                                                             const double *__restrict__ A, const double *__restrict__ X,
                                                                             const double *__restrict__ Lg, const int *__restrict__ dead,
                                                                             double *__restrict__ mean, double *__restrict__ cov,
                                                                             int *__restrict__ hmax, double *__restrict__ wmax,
                                                                             double *__restrict__ logz, double *__restrict__ wout) {
    using L = ChainLanes<P, K>;
    constexpr int SLOTS = L::SLOTS;
    __shared__ double sX[L::CAP * 3], sV[L::CAP];
    __shared__ double sPm[CHAIN_T], sPs[CHAIN_T];
    __shared__ double sred[CHAIN_W * 6];
    __shared__ int sredi[CHAIN_W];
    const int tid = threadIdx.x, lane = tid & 63;
    const L ln(tid, H);
    const int part = ln.part, slot = ln.slot;
    const int rows = F + lag;
    const size_t wg = blockIdx.x;                                  // (s rows + r) J + j: the output row of frame n
    const int j = (int)(wg % J), r = (int)(wg / J % rows), s = (int)(wg / J / rows);
    const StreamEmit em = stream_emit(tcount[s], F, lag, flush && flush[s] != 0);
    if (r >= em.cnt) return;                                       // (workgroup-uniform, as every return below)
    const long long n = em.e0 + r;
    const size_t sj = (size_t)s * J + j;
    const double *const Ar = A + sj * R * H, *const Xr = X + sj * R * H * 3, *const lr = Lg + sj * R * H;
    const int *const dr = dead + sj * R;
    const double ninf = -__builtin_huge_val(), qnan = __builtin_nan("");
    if (dr[(int)(n % R)] != 0) {                                   // NaN, hypothesis 0, weight 0, log Z = -inf, a row of zeros
        ZEDO_CHAIN_DEAD_OUTPUTS(K, slot, SLOTS, part == 0, wg)
        return;
    }
#ifdef ZEDO_MUT_JSM_HORIZON   // tools/mutation_check.py only: the horizon is taken one frame short
    const long long hi = min(max(n + lag - 1, n), em.t1 - 1);
#else
    const long long hi = min(n + lag, em.t1 - 1);
#endif
    long long eh = hi;
    for (long long m0 = n + 1; m0 <= hi; m0 += 64) {
        const long long m = m0 + lane;
        const int d = m <= hi ? dr[(int)(m % R)] : 0;
        const unsigned long long mask = __ballot(d != 0);
        if (mask) { eh = m0 + (__ffsll((long long)mask) - 1) - 1; break; }
    }
    const bool closed = eh + 1 >= em.t1 || dr[(int)((eh + 1) % R)] != 0;
    if (r > 0 && dr[(int)((n - 1) % R)] == 0 && n - 1 + lag >= eh) return;   // frame n - 1 shares the horizon: a lower frame walks
    const long long e1 = em.e0 + em.cnt;
    int row = (int)(eh % R);
    double xn[K][3], un[K] = {}, an[K] = {};
    auto fetch = [&](int rw) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const size_t at = (size_t)rw * H + min(slot + k * SLOTS, H - 1);
            xn[k][0] = Xr[at * 3]; xn[k][1] = Xr[at * 3 + 1]; xn[k][2] = Xr[at * 3 + 2];
            if (P == 1 || part == 0) {                             // only the owners use l and A: the other parts walk with X alone
                un[k] = lr[at];
                an[k] = Ar[at];
            }
        }
    };
    fetch(row);
    double lz = ninf;                                              // log Z of the truncated chain
    for (long long m = eh; m >= n; --m) {
        double xc[K][3], lc[K], ac[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            lc[k] = un[k];
            ac[k] = an[k];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) xc[k][cc] = xn[k][cc];
        }
        row = row == 0 ? R - 1 : row - 1;
        if (m > n) fetch(row);                                     // (workgroup-uniform) in flight over the barriers; never a row below frame n
        const bool chain = m < eh;                                 // frame m+1 continues this chain towards the horizon
        const bool emits = m == n || (closed && m + lag >= eh && m < e1);
        double mx[K], sm[K];
        __syncthreads();                                           // A: X[m+1,.] and (l + B)[m+1,.] are in the LDS
        if (chain) {
            jm_walk<K>(sX, sV, ln.q0, ln.q1, xc, c, mx, sm);
            if (P > 1) { sPm[tid] = mx[0]; sPs[tid] = sm[0]; }
        }
        __syncthreads();                                           // B: frame m+1 has been read by every lane
        double ab[K];                                              // A + B of this lane's hypotheses (-inf: excluded, or nobody's)
#pragma unroll
        for (int k = 0; k < K; ++k) ab[k] = ninf;
        if (part == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int h = slot + k * SLOTS;
                if (h < H) {
                    const double Bv = chain ? jm_combine<P>(mx[k], sm[k], sPm, sPs, SLOTS, slot, ln.np) : 0.0;
                    sV[h] = lc[k] + Bv;
                    sX[h * 3] = xc[k][0]; sX[h * 3 + 1] = xc[k][1]; sX[h * 3 + 2] = xc[k][2];
                    ab[k] = ac[k] + Bv;
                }
            }
        }
        if (!chain) {                                              // the horizon: B = 0, log Z = LSE_h A[eh,j,h], shifted by the largest A
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
        if (emits) {
            const size_t nj = wg + (size_t)(m - n) * J;            // the output row of frame m: r + (m - n)
            ZEDO_CHAIN_MOMENTS(K, slot, SLOTS, part == 0 && h < H, exp(ab[k] - lz), xc, nj)
        }
    }
}

hipError_t launch_joint_stream_marginal_reset(void *state, int S, int H, int J, int lag, int max_frames, const int *which, hipStream_t st) {
    const JointStreamMarginalState w(state, S, H, J, (size_t)lag + max_frames);
    hipLaunchKernelGGL(joint_stream_reset_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, which, S, w.t);
    return hipGetLastError();
}

hipError_t launch_joint_stream_marginal_push(const double *junary, const float *x, const float *T, int S, int F, int H, int J, int lag,
                                             int max_frames, double c, double tau, const int *flush, void *state, double *mean,
                                             double *cov, int *hmax, double *wmax, double *logz, double *wout, long long *emit,
                                             hipStream_t st) {
    const int R = lag + max_frames;                                // R S J H <= INT_MAX
    const JointStreamMarginalState w(state, S, H, J, R);
    const size_t groups = (size_t)S * (F + lag) * J;               // F <= max_frames: at most R S J
    dispatch_pk(H, [&](auto P, auto K) {
        if (F > 0) {
            const int N = S * F;
            hipLaunchKernelGGL(joint_stream_dead_kernel, dim3((unsigned)(((size_t)N * J + 255) / 256)), dim3(256), 0, st, junary, w.t, S, F, H,
                               J, R, w.dead);
            hipLaunchKernelGGL((joint_stream_marginal_forward_kernel<P(), K()>), dim3((unsigned)S * (unsigned)J), dim3(CHAIN_T), 0, st, junary,
                               x, T, F, H, N, J, R, c, tau, w.t, w.A, w.X, w.l, w.dead, w.lastdead);
        }
        if (groups)
            hipLaunchKernelGGL((joint_stream_marginal_emit_kernel<P(), K()>), dim3((unsigned)groups), dim3(CHAIN_T), 0, st, w.t, flush, F, H, J,
                               R, lag, c, w.A, w.X, w.l, w.dead, mean, cov, hmax, wmax, logz, wout);
    });
    hipLaunchKernelGGL(joint_stream_advance_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, flush, S, F, lag, w.t, emit);
    return hipGetLastError();
}

}  // namespace zedo
