// Fusing hypotheses on a live video under the second-order motion model for gfx950 (zedo_joint_accel_stream_marginal_push): the
// sum-product chain over pairs of zedo_joint_accel_marginal.hip, fed in chunks, with A2, X and l of the last lag + max_frames + 2 frames in
// caller-owned state and every frame's marginals formed `lag` frames after it went in - fixed-lag smoothing.  Per push, in stream order:
//   joint_stream_dead_kernel                    (zedo_joint_stream.hip) one lane per (stream, chunk frame, joint): the dead flag, into the ring
//   joint_accel_stream_marginal_forward_kernel  the forward recurrence of joint_accel_marginal_forward_kernel, one workgroup per (stream,
//                                               joint): the same pairs per lane, the same two barriers per frame, the same prefetch of frame
//                                               n+2; its first frame continues from the ring's rows of the two frames before; A2, X and l of
//                                               every frame go into the ring
//   joint_accel_stream_marginal_emit_kernel     the backward recurrence of joint_accel_marginal_backward_kernel from a frame's horizon down to
//                                               it, one workgroup per (stream, output row, joint); everything it reads comes from the ring,
//                                               B2, M and the pair marginals never leave the LDS.  Frames of one (stream, joint) that share a
//                                               closed horizon are served by ONE walk, that of the lowest of them: the others return at once
//   joint_stream_advance_kernel                 (zedo_joint_stream.hip) one lane per stream: d_emit and the clip's frame count
// The statements that decide a bit - jam_walk, jam_block_lse, the pair terms, the forward value, the backward body, the moments, the dead
// outputs - are zedo_chain.h's, the ones the offline kernels run, on the same operands: X and l in the ring are the doubles the offline
// kernels form from x, T and u.
// The ring holds R = lag + max_frames + 2 frames, frame m of a clip in row m % R.  A push of F <= max_frames frames onto a clip of t frames
// writes the rows of frames t .. t+F-1 (the dead kernel their flags, before anything else runs).  The forward step reads A2, X, l and the
// flag of frame t-1 and X and the flag of frame t-2; the emission reads frames >= max(0, t - lag) and X of the frame before the lowest of
// them, t - lag - 1.  The lowest frame read, t - lag - 1 (lag >= 1) or t - 2 (lag = 0), is less than R below the highest written, t + F - 1:
// (t + F - 1) - (t - lag - 1) = F + lag <= R - 2 and (t + F - 1) - (t - 2) = F + 1 <= R - 1.  So no row that is read has been overwritten,
// and the two frames before a chunk need no slots of their own - with lag = 0 and F = max_frames as well.
// LDS: forward 38 400 bytes, emission 104 656 bytes (one workgroup per CU), as the offline kernels.  No atomics, no scratch.
#include "zedo_chain.h"

namespace zedo {

// The state of S streams, R = lag + max_frames + 2, SJ = S J, HH = H^2:
//   A2 f64 [SJ,R,HH] | X f64 [SJ,R,H,3] | l f64 [SJ,R,H] | t i64 [S] | dead i32 [SJ,R]   (padded to 8)
// t: the frames of the stream's clip so far; max(0, t - lag) of them have been emitted.  t = 0 is all an empty stream needs: nothing
// else is read before it is written.
struct JointAccelStreamMarginalState {
    Carve c;
    double *A2, *X, *l;
    long long *t;
    int *dead;
    size_t bytes;
    JointAccelStreamMarginalState(void *st, size_t S, size_t H, size_t J, size_t R)
        : c(st), A2(c.take<double>(S * J * R * H * H)), X(c.take<double>(S * J * R * H * 3)), l(c.take<double>(S * J * R * H)),
          t(c.take<long long>(S)), dead(c.take<int>(S * J * R)), bytes(c.bytes(8)) {}
};
size_t joint_accel_stream_marginal_bytes(int S, int H, int J, int lag, int max_frames) {
    return JointAccelStreamMarginalState(nullptr, S, H, J, (size_t)lag + max_frames + 2).bytes;
}

// joint_accel_marginal_forward_kernel on the F frames of stream s's chunk (rows n = s F + f of the call), continued from the ring: frame
// t + f of the clip.  "start" (the frame before is dead or absent) and "second" (the one before that is) are read from the ring's dead
// flags at every frame, as the offline kernel reads its own (carried along the chunk as two ints instead, the instantiation of 16 pairs
// per lane spills; this form has the offline kernel's registers - profiles/joint_accel_stream_marginal_build.txt).  The LDS is the offline kernel's: sA =
// A2[n-1] h''-major, X of frames n, n-1, n-2 in three rotating slots, l of frames n and n-1 in two (by the parity of f).  A2[t-1], X[t-1],
// X[t-2] and l[t-1] are read from the ring before barrier A of the first frame, i.e. before any lane writes a row of this push.
template <int KA>
__global__ __launch_bounds__(CHAIN_T) void joint_accel_stream_marginal_forward_kernel(
    const double *__restrict__ junary, const float *__restrict__ x, const float *__restrict__ Tr, int F, int H, int N, int J, int R, double c_v,
    double c_a, double tau, const long long *__restrict__ tcount, const int *__restrict__ dead, double *__restrict__ A2,
    double *__restrict__ X, double *__restrict__ Lg) {
    __shared__ double sA[JAM_CAP * JAM_CAP];
    __shared__ double sX[3][JAM_CAP * 3], sL[2][JAM_CAP];
    const int tid = threadIdx.x, HH = H * H;
    const int s = blockIdx.x / J, j = (int)blockIdx.x - s * J;
    const size_t sj = blockIdx.x;
    const long long t0 = clip_frames(tcount[s]);
    const int a = s * F, b = a + F;
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
        sL[0][tid] = ln;
    }
    fetch(min(a + 1, b - 1));
    double *const A2r = A2 + sj * R * HH, *const Xr = X + sj * R * H * 3, *const lr = Lg + sj * R * H;   // this chain's rows of the ring
    const int *const dr = dead + sj * R;
    int row = (int)(t0 % R);
    const int row1 = row == 0 ? R - 1 : row - 1, row2 = row1 == 0 ? R - 1 : row1 - 1;     // the rows of frames t-1 and t-2
    const bool dead1 = (t0 > 0 ? dr[row1] : 1) != 0, dead2 = (t0 > 1 ? dr[row2] : 1) != 0;     // (workgroup-uniform) frames t-1 and t-2
    if (t0 > 0 && tid < H) {                                       // X[t-1], X[t-2], l[t-1]: visible after barrier A
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sX[s1][tid * 3 + c] = Xr[((size_t)row1 * H + tid) * 3 + c];
            sX[s2][tid * 3 + c] = Xr[((size_t)row2 * H + tid) * 3 + c];
        }
        sL[1][tid] = lr[(size_t)row1 * H + tid];
    }
    if (!dead1 && !dead2) {                                        // A2[t-1], at the q its owners wrote it
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int q = tid + k * CHAIN_T;
            if (q < HH) sA[q] = A2r[(size_t)row1 * HH + q];
        }
    }
    double *A2w = A2r + (size_t)row * HH;                          // the row of frame n
    for (int n = a; n < b; ++n) {
        const int par = (n - a) & 1;
        const double xc[3] = {xn[0], xn[1], xn[2]}, lc = ln;       // frame n+1
        fetch(min(n + 2, b - 1));                                  // unconditional: in flight over the barriers of this frame
        const int rm1 = row == 0 ? R - 1 : row - 1, rm2 = rm1 == 0 ? R - 1 : rm1 - 1;     // the rows of frames n-1 and n-2
        const long long tn = t0 + (n - a);                         // frame n of the call is frame tn of the clip
        const bool is_dead = dr[row] != 0, start = (tn > 0 ? dr[rm1] : 1) != 0;
        const bool second = !start && (tn > 1 ? dr[rm2] : 1) != 0;
        const bool scan = !is_dead && !start;                      // (all workgroup-uniform)
        const double *X0 = sX[s0], *X1 = sX[s1], *X2 = sX[s2], *L0 = sL[par], *L1 = sL[par ^ 1];
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
                    A2w[q] = an[k];
                }
            }
        }
        if (tid < H) {                                             // X and l of frame n into the ring (their slots stay as they are below)
            const size_t at = (size_t)row * H + tid;
            Xr[at * 3] = X0[tid * 3]; Xr[at * 3 + 1] = X0[tid * 3 + 1]; Xr[at * 3 + 2] = X0[tid * 3 + 2];
            lr[at] = L0[tid];
            sX[s2][tid * 3] = xc[0]; sX[s2][tid * 3 + 1] = xc[1]; sX[s2][tid * 3 + 2] = xc[2];
            sL[par ^ 1][tid] = lc;
        }
        { const int t = s2; s2 = s1; s1 = s0; s0 = t; }
        A2w = row + 1 == R ? A2r : A2w + HH;
        row = row + 1 == R ? 0 : row + 1;
    }
}

// One workgroup per (stream, output row r, joint): frame n = e0 + r of the clip, if the push emits it.  A dead (n, j) writes its dead
// outputs.  Otherwise the horizon eh = min(n + lag, the last frame of n's chain on the clip's t1 frames) comes from the ring's dead flags
// (stream_horizon; every wave does the same), and `closed`: is eh that chain's last frame.  Frames of one chain whose horizon is eh are n
// itself and, if closed, every m >= n; the workgroup of the LOWEST of them that this push emits - r = 0, or (n-1, j) dead, or n - 1 + lag <
// eh - walks B2 from eh (B2 = 0, log Z = LSE over the pairs of A2[eh]) down with the backward body of the offline kernel and forms the
// outputs of each of those frames where its B2 is; the others return.  The chain's first frame c0 has no table: where n == c0 the walk
// stops at c0+1 and writes c0 from the row sums of the pair marginals there - with an open horizon c0 alone; a chain of one frame so far (eh
// == n == c0) is the softmax of l[n].  All of [n, eh] is live and in the ring, and so is X of frame n-1 where n > c0.  Everything the
// workgroup branches on is workgroup-uniform.
template <int KA>
__global__ __launch_bounds__(CHAIN_T) void joint_accel_stream_marginal_emit_kernel(
    const long long *__restrict__ tcount, const int *__restrict__ flush, int F, int H, int J, int R, int lag, double c_v, double c_a,
    const double *__restrict__ A2, const double *__restrict__ X, const double *__restrict__ Lg, const int *__restrict__ dead,
    double *__restrict__ mean, double *__restrict__ cov, int *__restrict__ hmax, double *__restrict__ wmax, double *__restrict__ logz,
    double *__restrict__ wout) {
    __shared__ double sB[JAM_CAP * JAM_CAP], sM[JAM_CAP * JAM_CAP], sP[JAM_CAP * JAM_CAP];
    __shared__ double sX[3][JAM_CAP * 3], sL[3][JAM_CAP];
    __shared__ double sred[CHAIN_W * 6];
    __shared__ int sredi[CHAIN_W];
    const int tid = threadIdx.x, lane = tid & 63, HH = H * H;
    const int rows = F + lag;
    const size_t wg = blockIdx.x;                                  // (s rows + r) J + j: the output row of frame n
    const int j = (int)(wg % J), r = (int)(wg / J % rows), s = (int)(wg / J / rows);
    const StreamEmit em = stream_emit(tcount[s], F, lag, flush && flush[s] != 0);
    if (r >= em.cnt) return;                                       // (workgroup-uniform, as every return below)
    const long long n = em.e0 + r;
    const size_t sj = (size_t)s * J + j;
    const double *const A2r = A2 + sj * R * HH, *const Xr = X + sj * R * H * 3, *const lr = Lg + sj * R * H;
    const int *const dr = dead + sj * R;
    const double ninf = -__builtin_huge_val(), qnan = __builtin_nan("");
    const int rn = (int)(n % R);
    auto ring = [&](int d) { return (rn + d + R) % R; };           // the row of frame n + d, -1 <= d <= lag
    if (dr[rn] != 0) {                                             // NaN, hypothesis 0, weight 0, log Z = -inf, a row of zeros
        ZEDO_CHAIN_DEAD_OUTPUTS(1, tid, 0, true, wg)
        return;
    }
#ifdef ZEDO_MUT_JASM_HORIZON   // tools/mutation_check.py only: the horizon is taken one frame short
    const long long hi = min(max(n + lag - 1, n), em.t1 - 1);
#else
    const long long hi = min(n + lag, em.t1 - 1);
#endif
    const long long eh = stream_horizon(dr, n, hi, R, lane);
    const int de = (int)(eh - n);                                  // 0 .. lag
    const bool closed = eh + 1 >= em.t1 || dr[ring(de + 1)] != 0;  // (de + 1 <= lag + 1 < R)
    const bool first = n == 0 || dr[ring(-1)] != 0;                // n is the first frame of its chain
    if (r > 0 && !first && n - 1 + lag >= eh) return;              // frame n - 1 shares the horizon: a lower frame walks
    const int served = closed ? (int)min((long long)de, em.e0 + em.cnt - 1 - n) : 0;      // the frames n .. n + served come out of this walk
    const int dlo = first && de > 0 ? 1 : 0, dx = first ? 0 : -1;  // the walk goes down to frame n + dlo and reads X from frame n + dx on
    const double c_a_back = c_a;
    int qh1[KA], qh0[KA];
    lane_pairs<KA>(tid, H, qh1, qh0);
    const int hx = min(tid, H - 1);                                // a lane past H reads hypothesis H-1 and stores nothing
    double xn[3], ln, an[KA];
    auto fetch = [&](int d) {                                      // X and l of frame n + d
        const size_t at = (size_t)ring(d) * H + hx;
        xn[0] = Xr[at * 3]; xn[1] = Xr[at * 3 + 1]; xn[2] = Xr[at * 3 + 2];
        ln = lr[at];
    };
    auto fetch_table = [&](int d) {                                // A2 of frame n + d (a frame without pairs: whatever the ring holds, never used)
        const size_t at = (size_t)ring(d) * HH;
#pragma unroll
        for (int k = 0; k < KA; ++k) an[k] = A2r[at + min(tid + k * CHAIN_T, HH - 1)];
    };
    auto put = [&](int sl) {
        if (tid < H) {
            sX[sl][tid * 3] = xn[0]; sX[sl][tid * 3 + 1] = xn[1]; sX[sl][tid * 3 + 2] = xn[2];
            sL[sl][tid] = ln;
        }
    };
    int sp = 2, s0 = 0, s1 = 1;                                    // the slots of frames m+1, m, m-1
    fetch(de);
    put(s0);
    fetch(max(de - 1, dx));
    put(s1);
    fetch(max(de - 2, dx));
    fetch_table(de);
    double lz = ninf;                                              // log Z of the truncated chain
    for (int d = de; d >= dlo; --d) {                              // frame m = n + d
        const double xc[3] = {xn[0], xn[1], xn[2]}, lc = ln;       // frame m-2
        double ac[KA];                                             // A2[m] of this lane's pairs
#pragma unroll
        for (int k = 0; k < KA; ++k) ac[k] = an[k];
        fetch(max(d - 3, dx));                                     // unconditional: in flight over the barriers of this frame
        fetch_table(max(d - 1, dlo));
        const bool is_dead = false, start = first && d == 0;       // (start: a chain of one frame so far)
        const bool second = first && d == 1, ends = d == de;
        const bool pairs = !start;                                 // (all workgroup-uniform) frame m has a table
        const double *Xp = sX[sp], *X0 = sX[s0], *X1 = sX[s1], *Lp = sL[sp], *L0 = sL[s0];
        const size_t nj = wg + (size_t)d * J;                      // the output row of frame m: r + d
        ZEDO_CHAIN_PAIR_BACKWARD(KA, nj, d <= served)              // the frame's body (zedo_chain.h); d = 0 is always served
        if (tid < H) {                                             // frame m-2 into the slot of frame m+1: its last reader is above C
            sX[sp][tid * 3] = xc[0]; sX[sp][tid * 3 + 1] = xc[1]; sX[sp][tid * 3 + 2] = xc[2];
            sL[sp][tid] = lc;
        }
        { const int t = sp; sp = s0; s0 = s1; s1 = t; }
    }
}

hipError_t launch_joint_accel_stream_marginal_reset(void *state, int S, int H, int J, int lag, int max_frames, const int *which,
                                                    hipStream_t st) {
    const JointAccelStreamMarginalState w(state, S, H, J, (size_t)lag + max_frames + 2);
    hipLaunchKernelGGL(joint_stream_reset_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, which, S, w.t);
    return hipGetLastError();
}

hipError_t launch_joint_accel_stream_marginal_push(const double *junary, const float *x, const float *T, int S, int F, int H, int J, int lag,
                                                   int max_frames, double c_v, double c_a, double tau, const int *flush, void *state,
                                                   double *mean, double *cov, int *hmax, double *wmax, double *logz, double *wout,
                                                   long long *emit, hipStream_t st) {
    const int R = lag + max_frames + 2;                            // R S J H^2 <= INT_MAX
    const JointAccelStreamMarginalState w(state, S, H, J, R);
    const size_t groups = (size_t)S * (F + lag) * J;               // F <= max_frames: fewer than R S J
    dispatch_pairs(H, [&](auto KA) {
        if (F > 0) {
            const int N = S * F;
            hipLaunchKernelGGL(joint_stream_dead_kernel, dim3((unsigned)(((size_t)N * J + 255) / 256)), dim3(256), 0, st, junary, w.t, S, F, H,
                               J, R, w.dead);
            hipLaunchKernelGGL((joint_accel_stream_marginal_forward_kernel<KA()>), dim3((unsigned)S * (unsigned)J), dim3(CHAIN_T), 0, st,
                               junary, x, T, F, H, N, J, R, c_v, c_a, tau, w.t, w.dead, w.A2, w.X, w.l);
        }
        if (groups)
            hipLaunchKernelGGL((joint_accel_stream_marginal_emit_kernel<KA()>), dim3((unsigned)groups), dim3(CHAIN_T), 0, st, w.t, flush, F, H,
                               J, R, lag, c_v, c_a, w.A2, w.X, w.l, w.dead, mean, cov, hmax, wmax, logz, wout);
    });
    hipLaunchKernelGGL(joint_stream_advance_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, flush, S, F, lag, w.t, emit);
    return hipGetLastError();
}

}  // namespace zedo
