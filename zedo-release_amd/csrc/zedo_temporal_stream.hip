// Pose-level selection on a live video for gfx950 (zedo_temporal_stream_push): the chain of zedo_temporal.hip, fed in chunks, with the
// tables in caller-owned state and every frame decided `lag` frames after it went in.  Per push, in stream order:
//   joint_stream_dead_kernel           (zedo_joint_stream.hip, J = 1) the dead flag of every chunk frame, into the ring
//   temporal_stream_transition_kernel  the motion term m[n,h',h] of every chunk frame that has a predecessor - the tile of
//                                      temporal_transition_kernel; the predecessor of a chunk's first frame is the state's copy of x
//   temporal_stream_scan_kernel        the resident form of temporal_scan_kernel, one workgroup per stream: its first frame continues
//                                      from the state's D of the frame before, its rows of D and back go into the ring, its last
//                                      frame's D, dead flag and x back into the state
//   joint_stream_emit_kernel           (zedo_joint_stream.hip, J = 1) one wave per (emitted frame, stream): horizon, arg-min, back pointers
//   joint_stream_advance_kernel        (zedo_joint_stream.hip) d_emit and the clip's frame count (0 after a flush)
// The transition and the scan kernel take the statements of a tile and of a frame from zedo_temporal.h, on the same operands as the
// offline kernels: the bits of D and back are the offline call's.  The ring holds R = lag + max_frames frames as in zedo_joint_stream.hip:
// a push writes the rows of frames t .. t+F-1 and its emission reads frames >= max(0, t - lag) > t + F - 1 - R.  No atomics, no scratch.
#include "zedo_temporal.h"

#include <algorithm>

namespace zedo {

// The state of S streams, R = lag + max_frames - that of zedo_joint_stream.hip with J = 1 and without its X, plus M and lastx:
//   D f64 [S,R,H] | lastD f64 [S,H] | t i64 [S] | M f64 [S,max_frames,H,H] | back i32 [S,R,H] | dead i32 [S,R] | lastdead i32 [S] |
//   lastx f32 [S,H,J,3]   (padded to 8)
// M: the transition costs of the current push, [S F,H,H] at its head - scratch.  lastx: x of the clip's last frame as it arrived.
struct TemporalStreamState {
    Carve c;
    double *D, *lastD;
    long long *t;
    double *M;
    int *back, *dead, *lastdead;
    float *lastx;
    size_t bytes;
    TemporalStreamState(void *st, size_t S, size_t H, size_t J, size_t R, size_t mf)
        : c(st), D(c.take<double>(S * R * H)), lastD(c.take<double>(S * H)), t(c.take<long long>(S)), M(c.take<double>(S * mf * H * H)),
          back(c.take<int>(S * R * H)), dead(c.take<int>(S * R)), lastdead(c.take<int>(S)), lastx(c.take<float>(S * H * J * 3)),
          bytes(c.bytes(8)) {}
};
size_t temporal_stream_bytes(int S, int H, int J, int lag, int max_frames) {
    return TemporalStreamState(nullptr, S, H, J, (size_t)lag + max_frames, max_frames).bytes;
}

// m[n,h',h] of chunk frame n = s F + f (ZEDO_TEMPORAL_TILE): frame n - 1 is row n - 1 of the chunk, for f = 0 the state's lastx [S,H,J,3]
// - the clip's last frame before this push; with an empty clip the frame starts a chain and has no transition costs (the scan reads
// none of them).  Written as M[n][h'][h].
__global__ __launch_bounds__(TT_T) void temporal_stream_transition_kernel(const float *__restrict__ x, const float *__restrict__ lastx,
                                                                          const long long *__restrict__ tcount, int F, int H, int N, int J,
                                                                          double *__restrict__ M) {
    __shared__ float sc[TT_H * TT_LD];                             // frame n, hypotheses h0 ..
    __shared__ float sp[TT_P * TT_LD];                             // frame n-1, hypotheses p0 ..
    const int n = blockIdx.x, s = n / F, f = n - s * F;
    if (f == 0 && clip_frames(tcount[s]) == 0) return;             // the clip's first frame (workgroup-uniform)
    ZEDO_TEMPORAL_TILE_LANES
    const size_t hs = (size_t)N * J * 3, J3 = (size_t)J * 3;       // floats from one hypothesis of a frame to the next: chunk, state
    const float *const xp = f > 0 ? x + (size_t)(n - 1) * J3 : lastx + (size_t)s * H * J3;
    const size_t ps = f > 0 ? hs : J3;
    ZEDO_TEMPORAL_TILE(x[(size_t)(h0 + r) * hs + ((size_t)n * J + js) * 3 + e], xp[(size_t)(p0 + r) * ps + (size_t)js * 3 + e])
}

// temporal_scan_kernel<RESIDENT> on the F frames of stream s's chunk (rows n = s F + f of the call), continued from the state: frame
// t + f of the clip.  "Chain start" is t + f == 0 or the frame before is dead - for f = 0 that flag is the state's lastdead, not the
// ring's (with lag = 0 and F = max_frames the dead kernel has just reused that row).  D[t-1,.] comes from the state's lastD into the LDS
// and stays there, double buffered, one barrier per frame; u[n+1,h] and the first TS_PF transition costs of the lane's first h are
// fetched BEFORE the barrier that ends frame n.  The statements of a frame are the offline kernel's (zedo_temporal.h).  The arg-min at
// a chain's end is not taken here: emission does that.  After the last frame: D, the dead flag and x of that frame into the state - the
// transition kernel of this push has read the old x (stream order).
__global__ __launch_bounds__(256) void temporal_stream_scan_kernel(const double *__restrict__ unary, const float *__restrict__ x,
                                                                   const double *__restrict__ M, int F, int H, int N, int J, int R,
                                                                   double lambda, const long long *__restrict__ tcount,
                                                                   double *__restrict__ D, int *__restrict__ back,
                                                                   const int *__restrict__ dead, double *__restrict__ lastD,
                                                                   int *__restrict__ lastdead, float *__restrict__ lastx) {
    constexpr bool RESIDENT = true;
    __shared__ double sD[2 * TS_CAP];
    const int tid = threadIdx.x, T = blockDim.x;
    const int s = blockIdx.x, a = s * F, b = a + F;
    const long long t0 = clip_frames(tcount[s]);
    const double inf = __builtin_huge_val();
    const size_t HH = (size_t)H * H;
    double *const Dr = D + (size_t)s * R * H, *const lD = lastD + (size_t)s * H;
    int *const br = back + (size_t)s * R * H;
    const int *const dr = dead + (size_t)s * R;
    int cur = 0;
    if (t0 > 0)                                                    // D[t-1,.] of the clip: visible after the first frame's barrier
        for (int h = tid; h < H; h += T) sD[h] = lD[h];
    // this lane's first h: the next frame's unary and the head of its column of transition costs, one frame ahead
    const int hf = min(tid, H - 1);
    double un = unary[(size_t)hf * N + a], mn[TS_PF];
#pragma unroll
    for (int k = 0; k < TS_PF; ++k) mn[k] = M[(size_t)a * HH + (size_t)min(k, H - 1) * H + hf];
    int prev_dead = t0 > 0 ? lastdead[s] : 1;                      // (workgroup-uniform)
    int row = (int)(t0 % R);
    for (int n = a; n < b; ++n) {
        const double uc = un;
        double mc[TS_PF];
#pragma unroll
        for (int k = 0; k < TS_PF; ++k) mc[k] = mn[k];
        {   // unconditional loads: the last frame re-reads its own
            const int nn = min(n + 1, b - 1);
            un = unary[(size_t)hf * N + nn];
#pragma unroll
            for (int k = 0; k < TS_PF; ++k) mn[k] = M[(size_t)nn * HH + (size_t)min(k, H - 1) * H + hf];
        }
        const bool is_dead = dr[row] != 0, start = prev_dead != 0;
        __syncthreads();                                           // D[n-1,.] of every lane is in sD[cur]
        const double *Mn = M + (size_t)n * HH;
        if (is_dead || start) {
            ZEDO_TEMPORAL_FRAME_START(unary[(size_t)h * N + n], Dr[(size_t)row * H + h], br[(size_t)row * H + h])
        } else {
            ZEDO_TEMPORAL_FRAME_RESIDENT(unary[(size_t)h * N + n], Dr[(size_t)row * H + h], br[(size_t)row * H + h])
        }
        cur ^= 1;
        prev_dead = is_dead ? 1 : 0;
        row = row + 1 == R ? 0 : row + 1;
    }
    // the next push continues from here; a lane wrote the entries of sD[cur] it reads
    for (int h = tid; h < H; h += T) lD[h] = sD[cur * TS_CAP + h];
    if (tid == 0) lastdead[s] = prev_dead;
#ifndef ZEDO_MUT_TSTREAM_LASTX   // tools/mutation_check.py only: the state keeps the x of an earlier push
    const int J3 = J * 3;
    for (int q = tid; q < H * J3; q += T) {
        const int h = q / J3, e = q - h * J3;
        lastx[(size_t)s * H * J3 + q] = x[((size_t)h * N + (b - 1)) * J3 + e];
    }
#endif
}

hipError_t launch_temporal_stream_reset(void *state, int S, int H, int J, int lag, int max_frames, const int *which, hipStream_t st) {
    const TemporalStreamState w(state, S, H, J, (size_t)lag + max_frames, max_frames);
    hipLaunchKernelGGL(joint_stream_reset_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, which, S, w.t);
    return hipGetLastError();
}

hipError_t launch_temporal_stream_push(const double *unary, const float *x, int S, int F, int H, int J, int lag, int max_frames,
                                       double lambda, const int *flush, void *state, int *path, double *cost, long long *emit,
                                       hipStream_t st) {
    const int R = lag + max_frames;                                // R S H, S max_frames H H and 3 S H J <= INT_MAX
    const TemporalStreamState w(state, S, H, J, R, max_frames);
    if (F > 0) {
        const int N = S * F;
        hipLaunchKernelGGL(joint_stream_dead_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, unary, w.t, S, F, H, 1, R, w.dead);
        hipLaunchKernelGGL(temporal_stream_transition_kernel, dim3(N, (H + TT_H - 1) / TT_H, (H + TT_P - 1) / TT_P), dim3(TT_T), 0, st, x,
                           w.lastx, w.t, F, H, N, J, w.M);
        hipLaunchKernelGGL(temporal_stream_scan_kernel, dim3((unsigned)S), dim3(std::min(256, (H + 63) / 64 * 64)), 0, st, unary, x, w.M, F, H,
                           N, J, R, lambda, w.t, w.D, w.back, w.dead, w.lastD, w.lastdead, w.lastx);
    }
    const size_t waves = (size_t)S * (F + lag);
    if (waves)
        hipLaunchKernelGGL(joint_stream_emit_kernel, dim3((unsigned)((waves + CHAIN_W - 1) / CHAIN_W)), dim3(CHAIN_T), 0, st, w.t, flush, S, F,
                           H, 1, R, lag, w.D, w.back, w.dead, path, cost);
    hipLaunchKernelGGL(joint_stream_advance_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, flush, S, F, lag, w.t, emit);
    return hipGetLastError();
}

}  // namespace zedo
