// Joint-wise selection on a live video for gfx950 (zedo_joint_stream_push): the first-order chain of zedo_joint_temporal.hip, fed in
// chunks, with the tables in caller-owned state and every frame decided `lag` frames after it went in.  Per push, in stream order:
//   joint_stream_dead_kernel     one lane per (stream, chunk frame, joint): the dead flag, into the ring
//   joint_stream_scan_kernel     the forward recurrence of joint_temporal_scan_kernel, one workgroup per (stream, joint): the same lanes,
//                                the same two barriers per frame, the same prefetch; its first frame continues from the state's X and D of
//                                the frame before, its rows of D and back go into the ring, its last frame's X and D back into the state
//   joint_stream_emit_kernel     one wave per (emitted frame, stream, joint): the horizon from the ring's dead flags, the lowest arg-min
//                                of D there, at most `lag` back pointers, all read from the ring; nothing of it is in the scan's loop
//   joint_stream_advance_kernel  one lane per stream: d_emit and the clip's frame count (0 after a flush)
// The two scans are two kernels - their arguments differ - that take the statements of a frame's step from one place, zedo_chain.h.
// The ring holds lag + max_frames frames: frame m of a clip sits in row m % R, a push writes the rows of frames t .. t+F-1 and its
// emission reads frames >= max(0, t - lag) > t + F - 1 - R - rows this push has not overwritten.  No atomics, no scratch.
#include "zedo_chain.h"

namespace zedo {

// The state of S streams, R = lag + max_frames, SJ = S J:
//   D f64 [SJ,R,H] | lastX f64 [SJ,H,3] | lastD f64 [SJ,H] | t i64 [S] | back i32 [SJ,R,H] | dead i32 [SJ,R] | lastdead i32 [SJ]   (padded to 8)
// t: the frames of the stream's clip so far; max(0, t - lag) of them have been emitted.  t = 0 is all an empty stream needs: nothing
// else is read before it is written.
struct JointStreamState {
    Carve c;
    double *D, *lastX, *lastD;
    long long *t;
    int *back, *dead, *lastdead;
    size_t bytes;
    JointStreamState(void *st, size_t S, size_t H, size_t J, size_t R)
        : c(st), D(c.take<double>(S * J * R * H)), lastX(c.take<double>(S * J * H * 3)), lastD(c.take<double>(S * J * H)),
          t(c.take<long long>(S)), back(c.take<int>(S * J * R * H)), dead(c.take<int>(S * J * R)), lastdead(c.take<int>(S * J)),
          bytes(c.bytes(8)) {}
};
size_t joint_stream_bytes(int S, int H, int J, int lag, int max_frames) {
    return JointStreamState(nullptr, S, H, J, (size_t)lag + max_frames).bytes;
}

// (clip_frames, stream_emit: zedo_chain.h - the fusion on live streams, zedo_joint_stream_marginal.hip, takes them and the reset, dead
// and advance kernels below as they are)
__global__ __launch_bounds__(256) void joint_stream_reset_kernel(const int *__restrict__ which, int S, long long *__restrict__ t) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && (!which || which[s] != 0)) t[s] = 0;
}

__global__ __launch_bounds__(256) void joint_stream_dead_kernel(const double *__restrict__ junary, const long long *__restrict__ t, int S,
                                                                int F, int H, int J, int R, int *__restrict__ dead) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;           // i = n J + j, n = s F + f: junary[(h N + n) J + j] = junary[h NJ + i]
    const int NJ = S * F * J;
    if (i >= NJ) return;
    const int n = i / J, j = i - n * J, s = n / F, f = n - s * F;
    int any = 0;
    for (int h = 0; h < H; ++h) any |= finite64(junary[(size_t)h * NJ + i]) ? 1 : 0;
    dead[((size_t)s * J + j) * R + (int)((clip_frames(t[s]) + f) % R)] = any ? 0 : 1;
}

// joint_temporal_scan_kernel on the F frames of stream s's chunk (rows n = s F + f of the call), continued from the state: frame t + f
// of the clip.  "Chain start" is t + f == 0 or the frame before is dead - for f = 0 that flag is the state's lastdead, not the ring's
// (with lag = 0 and F = max_frames the dead kernel has just reused that row).  The statements of a frame are the offline kernel's
// (zedo_chain.h: the first-order chain's frame step), on the same operands: the bits of D and back are its bits.  The arg-min at a
// chain's end is not taken here: emission does that.
template <int P, int K>
__global__ __launch_bounds__(CHAIN_T) void joint_stream_scan_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                    const float *__restrict__ Tr, int F, int H, int N, int J, int R,
                                                                    double lambda, const long long *__restrict__ tcount,
                                                                    double *__restrict__ D, int *__restrict__ back,
                                                                    const int *__restrict__ dead, double *__restrict__ lastX,
                                                                    double *__restrict__ lastD, int *__restrict__ lastdead) {
    using L = ChainLanes<P, K>;
    constexpr int SLOTS = L::SLOTS;
    __shared__ double sX[L::CAP * 3], sD[L::CAP];
    __shared__ double sPv[CHAIN_T];                                // the parts' minima (P > 1)
    __shared__ int sPi[CHAIN_T];
    const int tid = threadIdx.x;
    const L ln(tid, H);
    const int s = blockIdx.x / J, j = (int)blockIdx.x - s * J;
    const size_t sj = blockIdx.x;
    const long long t0 = clip_frames(tcount[s]);
    const int a = s * F, b = a + F;
    const double inf = __builtin_huge_val();
    double *const Dr = D + sj * R * H;
    int *const br = back + sj * R * H;
    const int *const dr = dead + sj * R;
    double *const lX = lastX + sj * H * 3, *const lD = lastD + sj * H;
    double xn[K][3], un[K];
    auto fetch = [&](int n) { ZEDO_CHAIN_STEP_FETCH(n) };
    fetch(a);
    int prev_dead = t0 > 0 ? lastdead[sj] : 1;                     // (workgroup-uniform)
    if (t0 > 0 && ln.part == 0) {                                  // X[t-1,.] and D[t-1,.] of the clip: visible after barrier A
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int h = ln.slot + k * SLOTS;
            if (h < H) {
                sD[h] = lD[h];
                sX[h * 3] = lX[h * 3]; sX[h * 3 + 1] = lX[h * 3 + 1]; sX[h * 3 + 2] = lX[h * 3 + 2];
            }
        }
    }
    int row = (int)(t0 % R);
    for (int n = a; n < b; ++n) {
        double xc[K][3], uc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uc[k] = un[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) xc[k][c] = xn[k][c];
        }
        fetch(min(n + 1, b - 1));                                  // unconditional: in flight over the barriers
        const bool is_dead = dr[row] != 0, start = prev_dead != 0;
        const bool chain = !is_dead && !start;                     // (workgroup-uniform)
        const bool last = n + 1 == b;
        double dn[K];
        int bn[K];
        __syncthreads();                                           // A: X[n-1,.] and D[n-1,.] are in the LDS
        ZEDO_CHAIN_STEP_WALK
        __syncthreads();                                           // B: frame n-1 has been read by every lane
        if (ln.part == 0) {
            ZEDO_CHAIN_STEP_COMBINE
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int h = ln.slot + k * SLOTS;
                if (h < H) {
                    ZEDO_CHAIN_STEP_VALUE(k)
                    Dr[(size_t)row * H + h] = d;
                    br[(size_t)row * H + h] = chain ? bn[k] : -1;
                    sD[h] = d;
                    sX[h * 3] = xc[k][0]; sX[h * 3 + 1] = xc[k][1]; sX[h * 3 + 2] = xc[k][2];
                    if (last) {                                    // (workgroup-uniform) the next push continues from here
                        lD[h] = d;
                        lX[h * 3] = xc[k][0]; lX[h * 3 + 1] = xc[k][1]; lX[h * 3 + 2] = xc[k][2];
                    }
                }
            }
        }
        if (last && tid == 0) lastdead[sj] = is_dead ? 1 : 0;
        prev_dead = is_dead ? 1 : 0;
        row = row + 1 == R ? 0 : row + 1;
    }
}

// One wave per (stream, output row r, joint): frame n = e0 + r of the clip, if the push emits it.  The horizon e = min(n + lag, the last
// frame of n's chain on the clip's t1 frames): 64 dead flags per step, by ballot.  Then the lowest arg-min of D[e,j,.] (wave_arg), the
// back pointers e .. n+1 - every lane walks the same addresses - and cost = D[n,j,h_n].  Every value read from the ring is clamped to
// 0 .. H-1 before it is an index.  Everything the wave branches on is wave-uniform.
__global__ __launch_bounds__(CHAIN_T) void joint_stream_emit_kernel(const long long *__restrict__ tcount, const int *__restrict__ flush,
                                                                    int S, int F, int H, int J, int R, int lag,
                                                                    const double *__restrict__ D, const int *__restrict__ back,
                                                                    const int *__restrict__ dead, int *__restrict__ path,
                                                                    double *__restrict__ cost) {
    const int lane = threadIdx.x & 63, rows = F + lag;
    const size_t w = (size_t)blockIdx.x * CHAIN_W + (threadIdx.x >> 6), total = (size_t)S * rows * J;
    if (w >= total) return;
    const int j = (int)(w % J), r = (int)(w / J % rows), s = (int)(w / J / rows);
    const StreamEmit em = stream_emit(tcount[s], F, lag, flush && flush[s] != 0);
    if (r >= em.cnt) return;
    const long long n = em.e0 + r;
    const size_t sj = (size_t)s * J + j;
    const double *const Dr = D + sj * R * H;
    const int *const br = back + sj * R * H, *const dr = dead + sj * R;
    const int rn = (int)(n % R);
    if (dr[rn] != 0) {
        if (lane == 0) { path[w] = 0; cost[w] = __builtin_huge_val(); }
        return;
    }
#ifdef ZEDO_MUT_JS_HORIZON   // tools/mutation_check.py only: the horizon is taken one frame short
    const long long hi = min(max(n + lag - 1, n), em.t1 - 1);
#else
    const long long hi = min(n + lag, em.t1 - 1);
#endif
    long long e = hi;
    for (long long m0 = n + 1; m0 <= hi; m0 += 64) {
        const long long m = m0 + lane;
        const int d = m <= hi ? dr[(int)(m % R)] : 0;
        const unsigned long long mask = __ballot(d != 0);
        if (mask) { e = m0 + (__ffsll((long long)mask) - 1) - 1; break; }
    }
    int re = (int)(e % R);
    double v = __builtin_huge_val();
    int vh = INT_MAX;
    for (int h = lane; h < H; h += 64) {
        const double d = Dr[(size_t)re * H + h];
        if (arg_better<false>(d, h, v, vh)) { v = d; vh = h; }
    }
    wave_arg<false>(v, vh);
    int h = clampi(vh, 0, H - 1);                                  // (INT_MAX: no entry compared - a row of NaN)
    for (long long m = e; m > n; --m) {
        h = clampi(br[(size_t)re * H + h], 0, H - 1);
        re = re == 0 ? R - 1 : re - 1;
    }
    if (lane == 0) { path[w] = h; cost[w] = Dr[(size_t)rn * H + h]; }
}

__global__ __launch_bounds__(256) void joint_stream_advance_kernel(const int *__restrict__ flush, int S, int F, int lag,
                                                                   long long *__restrict__ t, long long *__restrict__ emit) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const bool fl = flush && flush[s] != 0;
    const StreamEmit em = stream_emit(t[s], F, lag, fl);
    emit[2 * s] = em.e0;
    emit[2 * s + 1] = em.cnt;
    t[s] = fl ? 0 : em.t1;
}

hipError_t launch_joint_stream_reset(void *state, int S, int H, int J, int lag, int max_frames, const int *which, hipStream_t st) {
    const JointStreamState w(state, S, H, J, (size_t)lag + max_frames);
    hipLaunchKernelGGL(joint_stream_reset_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, which, S, w.t);
    return hipGetLastError();
}

hipError_t launch_joint_stream_push(const double *junary, const float *x, const float *T, int S, int F, int H, int J, int lag,
                                    int max_frames, double lambda, const int *flush, void *state, int *path, double *cost,
                                    long long *emit, hipStream_t st) {
    const int R = lag + max_frames;                                // R S J H <= INT_MAX
    const JointStreamState w(state, S, H, J, R);
    if (F > 0) {
        const int N = S * F;
        hipLaunchKernelGGL(joint_stream_dead_kernel, dim3((unsigned)(((size_t)N * J + 255) / 256)), dim3(256), 0, st, junary, w.t, S, F, H, J,
                           R, w.dead);
        dispatch_pk(H, [&](auto P, auto K) {
            hipLaunchKernelGGL((joint_stream_scan_kernel<P(), K()>), dim3((unsigned)S * (unsigned)J), dim3(CHAIN_T), 0, st, junary, x, T, F, H,
                               N, J, R, lambda, w.t, w.D, w.back, w.dead, w.lastX, w.lastD, w.lastdead);
        });
    }
    const size_t waves = (size_t)S * (F + lag) * J;
    if (waves)
        hipLaunchKernelGGL(joint_stream_emit_kernel, dim3((unsigned)((waves + CHAIN_W - 1) / CHAIN_W)), dim3(CHAIN_T), 0, st, w.t, flush, S, F,
                           H, J, R, lag, w.D, w.back, w.dead, path, cost);
    hipLaunchKernelGGL(joint_stream_advance_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, flush, S, F, lag, w.t, emit);
    return hipGetLastError();
}

}  // namespace zedo
