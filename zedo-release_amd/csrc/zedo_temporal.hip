// Temporally consistent hypothesis selection for gfx950 (zedo_temporal_select): per frame of a clip the hypothesis that minimises its
// own unary cost plus lambda times the mean joint displacement to the previous frame's choice, solved exactly by dynamic programming
// (Viterbi) in fp64.  Four kernels:
//   temporal_dead_kernel        one lane per frame: does the frame have a hypothesis with a finite unary at all?
//   temporal_transition_kernel  the motion term m[n,h',h], the only part quadratic in H and independent of the recurrence: parallel over
//                               (frame, h', h), the two frames' poses staged through the LDS once per workgroup
//   temporal_scan_kernel        the forward recurrence, one workgroup per clip, one lane per hypothesis h (lanes loop beyond the workgroup)
//   temporal_backtrack_kernel   the backward pass, one workgroup per clip, runs of the back table staged through the LDS
// The host cuts the frames into chunks of C (whatever transition costs the caller's workspace holds) and launches the transition and the
// scan kernel per chunk; D and back live in the workspace for all frames, so the result does not depend on C.  No atomics.  The arg-min
// reduction and the workspace carving are zedo_chain.h's; the statements of a transition tile and of a frame of the resident scan are
// zedo_temporal.h's, where the call on live streams (zedo_temporal_stream.hip) takes them from as well.
#include "zedo_temporal.h"

#include <algorithm>

namespace zedo {

__global__ __launch_bounds__(256) void temporal_dead_kernel(const double *__restrict__ unary, int H, int N, int *__restrict__ dead) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int any = 0;
    for (int h = 0; h < H; ++h) any |= finite64(unary[(size_t)h * N + n]) ? 1 : 0;        // a wave reads 512 contiguous bytes per hypothesis
    dead[n] = any ? 0 : 1;
}

// m[n,h',h] of the frames of a chunk (ZEDO_TEMPORAL_TILE of zedo_temporal.h): frame n - 1 is row n - 1 of the same tensor.  Written as
// M[n - c0][h'][h].
__global__ __launch_bounds__(TT_T) void temporal_transition_kernel(const float *__restrict__ x, int H, int N, int J, int c0,
                                                                   double *__restrict__ M) {
    __shared__ float sc[TT_H * TT_LD];                             // frame n, hypotheses h0 ..
    __shared__ float sp[TT_P * TT_LD];                             // frame n-1, hypotheses p0 ..
    const int n = c0 + blockIdx.x;
    if (n < 1) return;                                             // frame 0 has no predecessor (workgroup-uniform)
    ZEDO_TEMPORAL_TILE_LANES
    const size_t hs = (size_t)N * J * 3;                           // floats from one hypothesis of a frame to the next
    ZEDO_TEMPORAL_TILE(x[(size_t)(h0 + r) * hs + ((size_t)n * J + js) * 3 + e], x[(size_t)(p0 + r) * hs + ((size_t)(n - 1) * J + js) * 3 + e])
}

// The forward recurrence.  One workgroup per clip s walks the frames of the chunk [c0, c0 + cnt) that fall inside
// [seq_start[s], seq_start[s+1]) (both clamped to 0 .. N: an offset is never an address).  Lane t owns h = t, t + T, ...
//   chain start (first frame of the clip, or frame n-1 dead):  D[n,h] = u[n,h], back = -1
//   otherwise:  D[n,h] = u[n,h] + min_h' (D[n-1,h'] + lambda m[n,h',h]), back = the lowest h' that attains it
//   dead frame: D[n,.] = +inf
// RESIDENT (H <= TS_CAP): D[n-1,.] stays in the LDS, double buffered - the lanes drop D[n,h] into the other buffer and ONE barrier
// per frame hands it over; the first frame of a chunk that continues a clip fetches it from the workspace table.  Otherwise D[n-1,.]
// comes from the table through the LDS TS_CAP entries at a time, behind barriers.  What does not depend on D - u[n+1,h] and the first
// TS_PF transition costs of the lane's first h - is fetched BEFORE the barrier that ends frame n.
// A frame that ends a chain (last of the clip, or frame n+1 dead) also gets the lowest arg-min of D[n,.] (endh[n]): the backward pass
// starts there and needs no reduction of its own.
template <bool RESIDENT>
__global__ __launch_bounds__(256) void temporal_scan_kernel(const double *__restrict__ unary, const double *__restrict__ M,
                                                            const int *__restrict__ seq_start, const int *__restrict__ dead, int H, int N,
                                                            double lambda, int c0, int cnt, double *D, int *__restrict__ back,
                                                            int *__restrict__ endh) {
    __shared__ double sD[RESIDENT ? 2 * TS_CAP : TS_CAP];
    __shared__ double rv[4];
    __shared__ int rh[4];
    const int tid = threadIdx.x, T = blockDim.x;
    const int a = clampi(seq_start[blockIdx.x], 0, N), b = clampi(seq_start[blockIdx.x + 1], 0, N);
    const int lo = max(a, c0), hi = min(b, c0 + cnt);
    if (lo >= hi) return;                                          // (workgroup-uniform)
    const double inf = __builtin_huge_val();
    const size_t HH = (size_t)H * H;
    int cur = 0;
    if (RESIDENT && lo > a)                                        // the clip began in an earlier chunk: D[lo-1,.] from the table
        for (int h = tid; h < H; h += T) sD[h] = D[(size_t)(lo - 1) * H + h];
    // this lane's first h: the next frame's unary and the head of its column of transition costs, one frame ahead
    const int hf = min(tid, H - 1);
    double un = unary[(size_t)hf * N + lo], mn[TS_PF];
#pragma unroll
    for (int k = 0; k < TS_PF; ++k) mn[k] = M[(size_t)(lo - c0) * HH + (size_t)min(k, H - 1) * H + hf];
    for (int n = lo; n < hi; ++n) {
        const double uc = un;
        double mc[TS_PF];
#pragma unroll
        for (int k = 0; k < TS_PF; ++k) mc[k] = mn[k];
        {   // unconditional loads (behind a branch the compiler would wait for them at the join): the last frame re-reads its own
            const int nn = min(n + 1, hi - 1);
            un = unary[(size_t)hf * N + nn];
#pragma unroll
            for (int k = 0; k < TS_PF; ++k) mn[k] = M[(size_t)(nn - c0) * HH + (size_t)min(k, H - 1) * H + hf];
        }
        const bool is_dead = dead[n] != 0, start = (n > a ? dead[n - 1] : 1) != 0;          // (dead[] is read inside 0 .. N-1 only)
        const bool ends = !is_dead && (n + 1 < b ? dead[n + 1] : 1) != 0;
        __syncthreads();                                           // D[n-1,.] of every lane is in sD[cur] (RESIDENT) / in the table
        const double *Mn = M + (size_t)(n - c0) * HH;
        if (is_dead || start) {
            ZEDO_TEMPORAL_FRAME_START(unary[(size_t)h * N + n], D[(size_t)n * H + h], back[(size_t)n * H + h])
        } else if (RESIDENT) {
            ZEDO_TEMPORAL_FRAME_RESIDENT(unary[(size_t)h * N + n], D[(size_t)n * H + h], back[(size_t)n * H + h])
        } else {
            // H above TS_CAP: every group of T hypotheses walks D[n-1,.] through the LDS in pieces of TS_CAP; all lanes take every barrier
            for (int g = 0; g < H; g += T) {
                const int h = g + tid;
                double best = inf;
                int bh = 0;
                for (int q0 = 0; q0 < H; q0 += TS_CAP) {
                    const int nq = min(TS_CAP, H - q0);
                    __syncthreads();                               // the previous piece has been read; D[n-1,.] is in the table
                    for (int q = tid; q < nq; q += T) sD[q] = D[(size_t)(n - 1) * H + q0 + q];
                    __syncthreads();
                    if (h < H)
#pragma unroll 8
                        for (int q = 0; q < nq; ++q) {
                            const double c = sD[q] + ZEDO_TEMPORAL_WEIGHTED(Mn[(size_t)(q0 + q) * H + h]);
                            if (q0 + q == 0 || c < best) { best = c; bh = q0 + q; }
                        }
                }
                if (h < H) {
                    const double u0 = unary[(size_t)h * N + n];
                    D[(size_t)n * H + h] = (finite64(u0) ? u0 : inf) + best;
                    back[(size_t)n * H + h] = bh;
                }
            }
        }
        cur ^= 1;
        if (ends) {                                                // (workgroup-uniform) the lowest arg-min of D[n,.]
            __syncthreads();                                       // D[n,.] of every lane is in sD[cur] / in the table
            double v = inf;
            int vh = INT_MAX;
            for (int h = tid; h < H; h += T) {
                const double d = RESIDENT ? sD[cur * TS_CAP + h] : D[(size_t)n * H + h];
                if (arg_better<false>(d, h, v, vh)) { v = d; vh = h; }
            }
            block_arg<false>(v, vh, rv, rh, tid, (T + 63) / 64);
            if (tid == 0) endh[n] = vh == INT_MAX ? 0 : vh;
        }
    }
}

// The backward pass.  One workgroup per clip, from its last frame: runs of up to TB_RUN frames - the rows back[n+1,.] the run needs,
// dead[n] and endh[n] - are staged into the LDS by all lanes, lane 0 walks the run there (one LDS read per frame where the table would
// cost one dependent HBM load per frame), then all lanes write path[n] and gather cost[n] = D[n, path[n]] for the run.  A value read
// from the tables is clamped to 0 .. H-1 before it is an index.  (H above TB_INTS: the walk reads the table itself.)
constexpr int TB_RUN = 256, TB_INTS = 8192;
__global__ __launch_bounds__(256) void temporal_backtrack_kernel(const int *__restrict__ seq_start, const int *__restrict__ dead,
                                                                 const int *__restrict__ endh, const int *__restrict__ back,
                                                                 const double *__restrict__ D, int H, int N, int *__restrict__ path,
                                                                 double *__restrict__ cost) {
    __shared__ int sb[TB_INTS], sdead[TB_RUN], send[TB_RUN], spath[TB_RUN];
    __shared__ int carry[2];                                       // lane 0's state between runs: have a successor in the chain, its h
    const int tid = threadIdx.x, T = blockDim.x;
    const int a = clampi(seq_start[blockIdx.x], 0, N), b = clampi(seq_start[blockIdx.x + 1], 0, N);
    if (a >= b) return;
    const bool staged = H <= TB_INTS;
    const int R = staged ? min(TB_RUN, TB_INTS / H) : TB_RUN;
    if (tid == 0) { carry[0] = 0; carry[1] = 0; }
    for (int r1 = b; r1 > a; r1 -= R) {                            // the run [r0, r1), walked downwards
        const int r0 = max(a, r1 - R), len = r1 - r0;
        __syncthreads();                                           // the previous run's LDS has been read
        for (int i = tid; i < len; i += T) { sdead[i] = dead[r0 + i]; send[i] = endh[r0 + i]; }
        if (staged) {                                              // rows r0+1 .. r1 of back (row b is never read: frame b-1 ends a chain)
            const int rows = min(r1, b - 1) - r0;
            for (int q = tid; q < rows * H; q += T) sb[q] = back[(size_t)(r0 + 1) * H + q];
        }
        __syncthreads();
        if (tid == 0) {
            int have = carry[0], p = carry[1];
            for (int i = len - 1; i >= 0; --i) {
                if (sdead[i]) { p = 0; have = 0; }
                else {
#ifdef ZEDO_MUT_TB_WALK   // tools/mutation_check.py only: the walk in memory reads the row of the frame itself (a row of the clip: <= b - 1)
                    p = have ? (staged ? sb[i * H + p] : back[(size_t)min(r0 + i, b - 1) * H + p]) : send[i];
#else
                    p = have ? (staged ? sb[i * H + p] : back[(size_t)(r0 + i + 1) * H + p]) : send[i];
#endif
                    p = clampi(p, 0, H - 1);
                    have = 1;
                }
                spath[i] = p;
            }
            carry[0] = have; carry[1] = p;
        }
        __syncthreads();
        for (int i = tid; i < len; i += T) {
            const int n = r0 + i, p = spath[i];
            path[n] = p;
            cost[n] = sdead[i] ? __builtin_huge_val() : D[(size_t)n * H + p];
        }
    }
}

// Workspace: D [N,H] f64 | back [N,H] i32, dead [N] i32, endh [N] i32 (padded to 8 bytes) | M [C,H,H] f64
struct TemporalWs {
    Carve c;
    double *D;
    int *back, *dead, *endh;
    double *M;
    size_t fixed_bytes;                                            // everything but M
    TemporalWs(void *ws, size_t N, size_t H)
        : c(ws), D(c.take<double>(N * H)), back(c.take<int>(N * H)), dead(c.take<int>(N)), endh(c.take<int>(N)), M(c.take<double>(0)),
          fixed_bytes(c.bytes()) {}
};
size_t temporal_fixed_bytes(int N, int H) { return TemporalWs(nullptr, N, H).fixed_bytes; }

hipError_t launch_temporal_select(const double *unary, const float *x, const int *seq_start, int n_seq, int H, int N, int J, double lambda,
                                  void *ws, int chunk, int *path, double *cost, hipStream_t st) {
    const TemporalWs w(ws, N, H);
    hipLaunchKernelGGL(temporal_dead_kernel, dim3((N + 255) / 256), dim3(256), 0, st, unary, H, N, w.dead);
    const int T = std::min(256, (H + 63) / 64 * 64);
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int cnt = std::min(chunk, N - c0);
        if (c0 + cnt > 1)
            hipLaunchKernelGGL(temporal_transition_kernel, dim3(cnt, (H + TT_H - 1) / TT_H, (H + TT_P - 1) / TT_P), dim3(TT_T), 0, st, x, H, N,
                               J, c0, w.M);
        if (H <= TS_CAP)
            hipLaunchKernelGGL(temporal_scan_kernel<true>, dim3(n_seq), dim3(T), 0, st, unary, w.M, seq_start, w.dead, H, N, lambda, c0, cnt,
                               w.D, w.back, w.endh);
        else
            hipLaunchKernelGGL(temporal_scan_kernel<false>, dim3(n_seq), dim3(T), 0, st, unary, w.M, seq_start, w.dead, H, N, lambda, c0, cnt,
                               w.D, w.back, w.endh);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(temporal_backtrack_kernel, dim3(n_seq), dim3(256), 0, st, seq_start, w.dead, w.endh, w.back, w.D, H, N, path, cost);
    return hipGetLastError();
}

}  // namespace zedo
