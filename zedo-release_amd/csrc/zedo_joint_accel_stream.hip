// Joint-wise selection on a live video under the second-order motion model for gfx950 (zedo_joint_accel_stream_push): the chain over
// pairs of hypotheses of zedo_joint_accel.hip, fed in chunks, with its tables in caller-owned state and every frame decided `lag` frames
// after it went in.  Per push, in stream order:
//   joint_stream_dead_kernel        (zedo_joint_stream.hip) one lane per (stream, chunk frame, joint): the dead flag, into this state's ring
//   joint_accel_stream_scan_kernel  the forward recurrence of joint_accel_scan_kernel, one workgroup per (stream, joint): the same pairs per
//                                   lane, the same two barriers per frame, the same prefetch of frame n+2, the pair table E[n-1] in the LDS;
//                                   its first frame continues from the state's E, X of the two frames before, u of the frame before and
//                                   their dead flags, its last frame puts them back; back2 goes into the ring.  Every live frame can be a
//                                   horizon, so every live frame leaves the lowest arg-min pair of E[n] and its value in the ring (of a
//                                   chain's first frame: the lowest arg-min of u) - one block reduction per frame beside the H^3 walk
//   joint_accel_stream_emit_kernel  one wave per (emitted frame, stream, joint): the horizon from the ring's dead flags, the pair kept
//                                   there, at most lag - 1 bytes of back2, all read from the ring; nothing of it is in the scan's loop
//   joint_stream_advance_kernel     (zedo_joint_stream.hip) one lane per stream: d_emit and the clip's frame count (0 after a flush)
// The statements of a frame's step are the offline kernel's (zedo_chain.h: the second-order chain's frame step), on the same operands: the
// bits of E and back2 are its bits.  The ring holds R = lag + max_frames frames: frame m of a clip sits in row m % R, a push writes the
// rows of frames t .. t+F-1 and its emission reads frames >= max(0, t - lag) > t + F - 1 - R only - rows this push has not overwritten,
// and rows an earlier push of this clip has written: back2[m] is read for m >= n + 2, two frames above a frame of m's own chain, where
// the scan has stored it.  No atomics, no scratch.
#include "zedo_chain.h"

namespace zedo {

constexpr int JAS_CAP = 64;                                        // the H of zedo_joint_accel.hip: the pair table stays in the LDS

// The state of S streams, R = lag + max_frames, SJ = S J, HH = H^2:
//   arg {f64 v, i32 q, i32 kind} [SJ,R] | last f64 [SJ, HH + 7 H + 1] | t i64 [S] | dead i32 [SJ,R] | back2 u8 [SJ,R,HH]   (padded to 8)
// arg: of the ring's frame, q the lowest arg-min pair h' H + h of E and v its value (a chain's first frame: h and u; dead: 0 and +inf),
// kind 0 dead, 1 the first frame of a chain, 2 inside one - one 16-byte record, one pointer in the scan's loop.  last, one block per
// chain - one pointer carried over the loop: E [HH], X [H,3] and - behind the next X - u [H] of the clip's last frame, X [H,3] of the
// frame before it, and in the last 8 bytes the dead flags of those two frames as two int32 - with lag = 0 and F = max_frames the chunk
// has reused both rows of the ring by the time the scan wants their flags.  t: the frames of the stream's clip so far.  t = 0 is all an
// empty stream needs: nothing else is read before it is written.
struct StreamArg { double v; int q, kind; };
static_assert(sizeof(StreamArg) == 16 && alignof(StreamArg) == 8, "the ring's record is what the header documents");
struct JointAccelStreamState {
    Carve c;
    StreamArg *arg;
    double *last;
    long long *t;
    int *dead;
    unsigned char *back2;
    size_t bytes;
    JointAccelStreamState(void *st, size_t S, size_t H, size_t J, size_t R)
        : c(st), arg(c.take<StreamArg>(S * J * R)), last(c.take<double>(S * J * (H * H + 7 * H + 1))), t(c.take<long long>(S)),
          dead(c.take<int>(S * J * R)), back2(c.take<unsigned char>(S * J * R * H * H)), bytes(c.bytes(8)) {}
};
size_t joint_accel_stream_bytes(int S, int H, int J, int lag, int max_frames) {
    return JointAccelStreamState(nullptr, S, H, J, (size_t)lag + max_frames).bytes;
}

// joint_accel_scan_kernel on the F frames of stream s's chunk (rows n = s F + f of the call), continued from the state: frame t + f of the
// clip.  "start" (the frame before is dead or absent) and "second" (the one before that is) come from two flags carried along the chunk;
// for its first two frames they are the state's lastdead, not the ring's.  The LDS is the offline kernel's: sE = E[n-1] h''-major, X of
// frames n, n-1, n-2 in three rotating slots, u of frames n and n-1 in two (by the parity of f).  E of the frame before is loaded only
// where the first frame can read it: it continues a chain of two frames or more.
template <int KA>
__global__ __launch_bounds__(CHAIN_T) void joint_accel_stream_scan_kernel(
    const double *__restrict__ junary, const float *__restrict__ x, const float *__restrict__ Tr, int F, int H, int N, int J, int R,
    double lambda_v, double lambda_a, const long long *__restrict__ tcount, const int *__restrict__ dead, unsigned char *__restrict__ back2,
    StreamArg *__restrict__ arg, double *__restrict__ last) {
    __shared__ double sE[JAS_CAP * JAS_CAP];
    __shared__ double sX[3][JAS_CAP * 3], sU[2][JAS_CAP];
    __shared__ double rv[CHAIN_W];
    __shared__ int rq[CHAIN_W];
    const int tid = threadIdx.x, HH = H * H;
    const int s = blockIdx.x / J, j = (int)blockIdx.x - s * J;
    const size_t sj = blockIdx.x;
    const long long t0 = clip_frames(tcount[s]);
    const int a = s * F, b = a + F;
    const double inf = __builtin_huge_val();
    int qh1[KA], qh0[KA];                                          // h' and h of pair k
    ZEDO_CHAIN_LANE_PAIRS(KA)
    // X[n,h,j,.] and u[n,j,h] of hypothesis h = tid (a lane past H reads hypothesis H-1 and stores nothing)
    double xn[3], un;
    auto fetch = [&](int n) {
        const size_t g = (size_t)min(tid, H - 1) * N + n;
        load_cam(x, Tr, g, J, j, xn);
        const double u0 = junary[g * J + j];
        un = finite64(u0) ? u0 : inf;
    };
    int s0 = 0, s1 = 2, s2 = 1;                                    // the slots of X[n], X[n-1], X[n-2]
    fetch(a);
    if (tid < H) {
        sX[s0][tid * 3] = xn[0]; sX[s0][tid * 3 + 1] = xn[1]; sX[s0][tid * 3 + 2] = xn[2];
        sU[0][tid] = un;
    }
    fetch(min(a + 1, b - 1));
    const int *const dr = dead + sj * R;
    unsigned char *const back_r = back2 + sj * R * HH;
    StreamArg *const ar = arg + sj * R;                            // this chain's rows of the ring
    double *const lE = last + sj * (HH + 7 * H + 1), *const lX = lE + HH, *const lU = lX + H * 6;     // this chain's block of `last`
    int *const lastdead = reinterpret_cast<int *>(lU + H);
    int dead1 = t0 > 0 ? (lastdead[0] != 0 ? 1 : 0) : 1;          // (workgroup-uniform) the flags of frames t-1 and t-2 of the clip
    int dead2 = t0 > 1 ? (lastdead[1] != 0 ? 1 : 0) : 1;
    if (t0 > 0 && tid < H) {                                       // X[t-1], X[t-2], u[t-1]: visible after barrier A
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sX[s1][tid * 3 + c] = lX[tid * 3 + c];
            sX[s2][tid * 3 + c] = lX[H * 3 + tid * 3 + c];
        }
        sU[1][tid] = lU[tid];
    }
    if (!dead1 && !dead2) {                                        // E[t-1], at the q its owners wrote it
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int q = tid + k * CHAIN_T;
            if (q < HH) sE[q] = lE[q];
        }
    }
    int row = (int)(t0 % R);
    for (int n = a; n < b; ++n) {
        const int par = (n - a) & 1;
        const double xc[3] = {xn[0], xn[1], xn[2]}, uc = un;       // frame n+1
        fetch(min(n + 2, b - 1));                                  // unconditional: in flight over the barriers of this frame
        const bool is_dead = dr[row] != 0, start = dead1 != 0;
        const bool second = !start && dead2 != 0;
        const bool scan = !is_dead && !start;                      // (all workgroup-uniform)
        const double *X0 = sX[s0], *X1 = sX[s1], *X2 = sX[s2], *U0 = sU[par], *U1 = sU[par ^ 1];
        double en[KA];
        int bn[KA];
        __syncthreads();                                           // A: E[n-1], X[n], X[n-1], X[n-2], u[n], u[n-1] are in the LDS
        ZEDO_CHAIN_PAIR_STEP(KA)                                   // the frame's step (zedo_chain.h): E[n] into en, the lowest h'' into bn
        double v = inf;                                            // a chain's first frame: the candidates are u[n,.]
        int vq = INT_MAX;
        if (!is_dead && start && tid < H) { v = U0[tid]; vq = tid; }
        __syncthreads();                                           // B: the LDS of frame n has been read by every lane
        if (scan) {
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                const int q = tid + k * CHAIN_T;
                if (q < HH) {
                    sE[q] = en[k];                                 // E[n][h',h] at h' H + h: the next frame reads it h''-major
                    if (!second) back_r[(size_t)row * HH + q] = (unsigned char)bn[k];
                    if (arg_better<false>(en[k], q, v, vq)) { v = en[k]; vq = q; }       // (q ascends with k)
                }
            }
        }
        if (tid < H) {
            sX[s2][tid * 3] = xc[0]; sX[s2][tid * 3 + 1] = xc[1]; sX[s2][tid * 3 + 2] = xc[2];
            sU[par ^ 1][tid] = uc;
        }
        { const int t = s2; s2 = s1; s1 = s0; s0 = t; }
        if (!is_dead) block_arg<false>(v, vq, rv, rq, tid);        // (workgroup-uniform) every live frame can be a horizon
        if (tid == 0) ar[row] = {v, vq == INT_MAX ? 0 : vq, is_dead ? 0 : (start ? 1 : 2)};
        dead2 = dead1;
        dead1 = is_dead ? 1 : 0;
        row = row + 1 == R ? 0 : row + 1;
    }
    // The next push continues from here: after the last rotation X of the chunk's last frame is in slot s1, X of the frame before in s2,
    // u of the last frame in sU[(F - 1) & 1], E of the last frame - where it scanned - in sE.  Every lane reads back what it wrote itself
    // (or loaded from the state above): no barrier.
    if (tid < H) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lX[tid * 3 + c] = sX[s1][tid * 3 + c];
            lX[H * 3 + tid * 3 + c] = sX[s2][tid * 3 + c];
        }
        lU[tid] = sU[(F - 1) & 1][tid];
    }
    if (!dead1 && !dead2) {
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int q = tid + k * CHAIN_T;
            if (q < HH) lE[q] = sE[q];
        }
    }
    if (tid == 0) { lastdead[0] = dead1; lastdead[1] = dead2; }
}

// One wave per (stream, output row r, joint): frame n = e0 + r of the clip, if the push emits it.  The horizon e = min(n + lag, the last
// frame of n's chain on the clip's t1 frames) (stream_horizon).  e == n at a chain's first frame: the h kept there.  Otherwise the pair
// (h', h) kept at e is (p_{e-1}, p_e), and p_{m-2} = back2[m][p_{m-1}, p_m] for m = e .. n+2 - every lane walks the same addresses.
// cost = the value kept at e.  Every value read from the ring is clamped before it is an index.  Everything the wave branches on is
// wave-uniform.
__global__ __launch_bounds__(CHAIN_T) void joint_accel_stream_emit_kernel(const long long *__restrict__ tcount, const int *__restrict__ flush,
                                                                          int S, int F, int H, int J, int R, int lag,
                                                                          const int *__restrict__ dead, const StreamArg *__restrict__ arg,
                                                                          const unsigned char *__restrict__ back2, int *__restrict__ path,
                                                                          double *__restrict__ cost) {
    const int lane = threadIdx.x & 63, rows = F + lag, HH = H * H;
    const size_t w = (size_t)blockIdx.x * CHAIN_W + (threadIdx.x >> 6), total = (size_t)S * rows * J;
    if (w >= total) return;
    const int j = (int)(w % J), r = (int)(w / J % rows), s = (int)(w / J / rows);
    const StreamEmit em = stream_emit(tcount[s], F, lag, flush && flush[s] != 0);
    if (r >= em.cnt) return;
    const long long n = em.e0 + r;
    const size_t sj = (size_t)s * J + j;
    const int *const dr = dead + sj * R;
    const unsigned char *const br = back2 + sj * R * HH;
    const int rn = (int)(n % R);
    if (dr[rn] != 0) {
        if (lane == 0) { path[w] = 0; cost[w] = __builtin_huge_val(); }
        return;
    }
#ifdef ZEDO_MUT_JAS_HORIZON   // tools/mutation_check.py only: the horizon is taken one frame short
    const long long hi = min(max(n + lag - 1, n), em.t1 - 1);
#else
    const long long hi = min(n + lag, em.t1 - 1);
#endif
    const long long e = stream_horizon(dr, n, hi, R, lane);
    int re = (int)(e % R);
    const StreamArg at = arg[sj * R + re];                         // (e == n: frame n's own record)
    const int q0 = at.q;
    int h;
    if (e == n && at.kind == 1) h = clampi(q0, 0, H - 1);
    else {
        const int q = clampi(q0, 0, HH - 1);
        int pa = q / H, pb = q - pa * H;                           // p_{m-1}, p_m at m = e
        for (long long m = e; m >= n + 2; --m) {
            const int p = clampi(br[(size_t)re * HH + pa * H + pb], 0, H - 1);
            pb = pa;
            pa = p;
            re = re == 0 ? R - 1 : re - 1;
        }
        h = e == n ? pb : pa;
    }
    if (lane == 0) { path[w] = h; cost[w] = at.v; }
}

hipError_t launch_joint_accel_stream_reset(void *state, int S, int H, int J, int lag, int max_frames, const int *which, hipStream_t st) {
    const JointAccelStreamState w(state, S, H, J, (size_t)lag + max_frames);
    hipLaunchKernelGGL(joint_stream_reset_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, which, S, w.t);
    return hipGetLastError();
}

hipError_t launch_joint_accel_stream_push(const double *junary, const float *x, const float *T, int S, int F, int H, int J, int lag,
                                          int max_frames, double lambda_v, double lambda_a, const int *flush, void *state, int *path,
                                          double *cost, long long *emit, hipStream_t st) {
    const int R = lag + max_frames;                                // R S J H^2 <= INT_MAX
    const JointAccelStreamState w(state, S, H, J, R);
    if (F > 0) {
        const int N = S * F;
        hipLaunchKernelGGL(joint_stream_dead_kernel, dim3((unsigned)(((size_t)N * J + 255) / 256)), dim3(256), 0, st, junary, w.t, S, F, H, J,
                           R, w.dead);
        dispatch_pairs(H, [&](auto KA) {
            hipLaunchKernelGGL((joint_accel_stream_scan_kernel<KA()>), dim3((unsigned)S * (unsigned)J), dim3(CHAIN_T), 0, st, junary, x, T, F,
                               H, N, J, R, lambda_v, lambda_a, w.t, w.dead, w.back2, w.arg, w.last);
        });
    }
    const size_t waves = (size_t)S * (F + lag) * J;
    if (waves)
        hipLaunchKernelGGL(joint_accel_stream_emit_kernel, dim3((unsigned)((waves + CHAIN_W - 1) / CHAIN_W)), dim3(CHAIN_T), 0, st, w.t, flush,
                           S, F, H, J, R, lag, w.dead, w.arg, w.back2, path, cost);
    hipLaunchKernelGGL(joint_stream_advance_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, flush, S, F, lag, w.t, emit);
    return hipGetLastError();
}

}  // namespace zedo
