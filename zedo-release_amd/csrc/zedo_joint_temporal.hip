// Joint-wise selection along a video for gfx950 (zedo_joint_temporal_select): for every joint of every clip the hypothesis path that
// minimises that joint's unary cost plus lambda times that joint's displacement in the camera frame (x + T) to the previous frame's
// choice - J independent Viterbi chains per clip, fp64.  Three kernels:
//   joint_temporal_dead_kernel       one lane per (frame, joint): does it have a hypothesis with a finite unary at all?
//   joint_temporal_scan_kernel       the forward recurrence, one workgroup per (clip, joint); the transition cost of a pair (h', h) is one
//                                    square root of three terms and is computed where the recurrence consumes it - there is no H x H table
//   joint_temporal_backtrack_kernel  the backward pass, one workgroup per (clip, joint), runs of the back table staged through the LDS
// The (clip, joint) of a workgroup, the lane split, the reductions and the statements of the scan's frame step - shared with the
// streaming scan of zedo_joint_stream.hip - are zedo_chain.h's.  A chain reads 12 bytes of x per (frame, hypothesis), at a stride of
// N J 3 floats across h; the other joints of the same pose row sit in the same few 128-byte lines, and neighbours in the grid run at
// the same time, so a line fetched from HBM for one chain serves the others from the L2.  No atomics.
#include "zedo_chain.h"

namespace zedo {

__global__ __launch_bounds__(256) void joint_temporal_dead_kernel(const double *__restrict__ junary, int H, int NJ, int *__restrict__ dead) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;           // i = n J + j: junary[(h N + n) J + j] = junary[h NJ + i]
    if (i >= NJ) return;
    int any = 0;
    for (int h = 0; h < H; ++h) any |= finite64(junary[(size_t)h * NJ + i]) ? 1 : 0;      // a wave reads 512 contiguous bytes per hypothesis
    dead[i] = any ? 0 : 1;
}

// The forward recurrence of one (clip, joint), on ChainLanes<P, K>: the lane (part, slot) owns the hypotheses h = slot + k SLOTS of frame
// n and walks its part of the h' of frame n-1; with P > 1 part 0 combines the parts' minima with a strict comparison - the tie still
// goes to the lowest h'.  With P = 1 one LDS read of (X[n-1,h'], D[n-1,h']) serves the lane's every h.
// X[n-1,.] (fp64 triples) and D[n-1,.] sit in the LDS; every lane of a wave reads the same h' - a broadcast.  Two barriers per frame:
// A - frame n-1 is in the LDS; B - every lane has read it (and the parts' minima are in the LDS), the owners replace it with frame n,
// which they hold in registers.  What does not depend on D - x, T and junary of frame n+1 - is fetched BEFORE barrier A of frame n.
//   chain start (first frame of the clip, or (n-1, j) dead):  D[n,j,h] = u[n,j,h], back = -1
//   otherwise:  D[n,j,h] = u[n,j,h] + min_h' (D[n-1,j,h'] + lambda m[n,j,h',h]), back = the lowest h' that attains it
//   dead (n, j): D[n,j,.] = +inf
// A frame that ends a chain (last of the clip, or (n+1, j) dead) also gets the lowest arg-min of D[n,j,.] (endh): the backward pass
// starts there.
constexpr int JT_CAP = 4 * CHAIN_T;
template <int P, int K>
__global__ __launch_bounds__(CHAIN_T) void joint_temporal_scan_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                      const float *__restrict__ Tr, const int *__restrict__ seq_start,
                                                                      const int *__restrict__ dead, int H, int N, int J, double lambda,
                                                                      double *__restrict__ D, int *__restrict__ back, int *__restrict__ endh) {
    using L = ChainLanes<P, K>;
    constexpr int SLOTS = L::SLOTS;
    __shared__ double sX[L::CAP * 3], sD[L::CAP];
    __shared__ double sPv[CHAIN_T];                                // the parts' minima (P > 1)
    __shared__ int sPi[CHAIN_T];
    __shared__ double rv[CHAIN_W];
    __shared__ int rh[CHAIN_W];
    const int tid = threadIdx.x;
    const L ln(tid, H);
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;                                            // (workgroup-uniform)
    const double inf = __builtin_huge_val();
    double xn[K][3], un[K];                                        // X[n,h,j,.] and u[n,j,h] of this lane's h
    auto fetch = [&](int n) { ZEDO_CHAIN_STEP_FETCH(n) };
    fetch(a);
    for (int n = a; n < b; ++n) {
        double xc[K][3], uc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uc[k] = un[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) xc[k][c] = xn[k][c];
        }
        fetch(min(n + 1, b - 1));                                  // unconditional (the last frame re-reads its own): in flight over the barriers
        const size_t nj = (size_t)n * J + j;
        const bool is_dead = dead[nj] != 0, start = (n > a ? dead[nj - J] : 1) != 0;      // (dead[] is read inside the clip only)
        const bool ends = !is_dead && (n + 1 < b ? dead[nj + J] : 1) != 0;
        const bool chain = !is_dead && !start;                     // (workgroup-uniform)
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
                    dn[k] = d;
                    D[nj * H + h] = d;
                    back[nj * H + h] = chain ? bn[k] : -1;
                    sD[h] = d;
                    sX[h * 3] = xc[k][0]; sX[h * 3 + 1] = xc[k][1]; sX[h * 3 + 2] = xc[k][2];
                } else dn[k] = inf;
            }
        }
        if (ends) {                                                // (workgroup-uniform) the lowest arg-min of D[n,j,.], from the owners' registers
            double v = inf;
            int vh = INT_MAX;
            if (ln.part == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int h = ln.slot + k * SLOTS;
                    if (h < H && arg_better<false>(dn[k], h, v, vh)) { v = dn[k]; vh = h; }
                }
            }
            block_arg<false>(v, vh, rv, rh, tid);
            if (tid == 0) endh[nj] = vh == INT_MAX ? 0 : vh;
        }
    }
}

// The backward pass of one (clip, joint), from the clip's last frame: runs of up to JB_RUN frames - the rows back[n+1,j,.] the run needs,
// dead and endh - are staged into the LDS by all lanes, lane 0 walks the run there, then all lanes write path and gather cost =
// D[n,j,path] for the run.  A value read from the tables is clamped to 0 .. H-1 before it is an index.  H <= 1024: a run is at least
// JB_INTS / 1024 = 8 frames.
constexpr int JB_RUN = 256, JB_INTS = 8192;
static_assert(JB_INTS >= JT_CAP, "at least one staged row of back per run");
__global__ __launch_bounds__(256) void joint_temporal_backtrack_kernel(const int *__restrict__ seq_start, const int *__restrict__ dead,
                                                                       const int *__restrict__ endh, const int *__restrict__ back,
                                                                       const double *__restrict__ D, int H, int N, int J,
                                                                       int *__restrict__ path, double *__restrict__ cost) {
    __shared__ int sb[JB_INTS], sdead[JB_RUN], send[JB_RUN], spath[JB_RUN];
    __shared__ int carry[2];                                       // lane 0's state between runs: have a successor in the chain, its h
    const int tid = threadIdx.x, T = blockDim.x;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;
    const int R = min(JB_RUN, JB_INTS / H);
    if (tid == 0) { carry[0] = 0; carry[1] = 0; }
    for (int r1 = b; r1 > a; r1 -= R) {                            // the run [r0, r1), walked downwards
        const int r0 = max(a, r1 - R), len = r1 - r0;
        __syncthreads();                                           // the previous run's LDS has been read
        for (int i = tid; i < len; i += T) { sdead[i] = dead[(size_t)(r0 + i) * J + j]; send[i] = endh[(size_t)(r0 + i) * J + j]; }
        const int rows = min(r1, b - 1) - r0;                      // rows r0+1 .. of back (row b is never read: frame b-1 ends a chain)
        for (int q = tid; q < rows * H; q += T) {
            const int r = q / H, e = q - r * H;
            sb[q] = back[((size_t)(r0 + 1 + r) * J + j) * H + e];
        }
        __syncthreads();
        if (tid == 0) {
            int have = carry[0], p = carry[1];
            for (int i = len - 1; i >= 0; --i) {
                if (sdead[i]) { p = 0; have = 0; }
                else {
                    p = clampi(have ? sb[i * H + p] : send[i], 0, H - 1);
                    have = 1;
                }
                spath[i] = p;
            }
            carry[0] = have; carry[1] = p;
        }
        __syncthreads();
        for (int i = tid; i < len; i += T) {
            const size_t nj = (size_t)(r0 + i) * J + j;
            const int p = spath[i];
            path[nj] = p;
            cost[nj] = sdead[i] ? __builtin_huge_val() : D[nj * H + p];
        }
    }
}

// Workspace: D [N,J,H] f64 | back [N,J,H] i32, dead [N,J] i32, endh [N,J] i32 (padded to 8 bytes)
struct JointTemporalWs {
    Carve c;
    double *D;
    int *back, *dead, *endh;
    size_t bytes;
    JointTemporalWs(void *ws, size_t nj, size_t H)
        : c(ws), D(c.take<double>(nj * H)), back(c.take<int>(nj * H)), dead(c.take<int>(nj)), endh(c.take<int>(nj)), bytes(c.bytes(8)) {}
};
size_t joint_temporal_bytes(int N, int H, int J) { return JointTemporalWs(nullptr, (size_t)N * J, H).bytes; }

// the dead flags on their own, for the other chain models on the same unaries
hipError_t launch_joint_temporal_dead(const double *junary, int H, int NJ, int *dead, hipStream_t st) {
    hipLaunchKernelGGL(joint_temporal_dead_kernel, dim3((unsigned)(((size_t)NJ + 255) / 256)), dim3(256), 0, st, junary, H, NJ, dead);
    return hipGetLastError();
}

hipError_t launch_joint_temporal_select(const double *junary, const float *x, const float *T, const int *seq_start, int n_seq, int H, int N,
                                        int J, double lambda, void *ws, int *path, double *cost, hipStream_t st) {
    const JointTemporalWs w(ws, (size_t)N * J, H);
    const dim3 grid((unsigned)n_seq * (unsigned)J);                // n_seq <= N and N J H <= INT_MAX
    hipLaunchKernelGGL(joint_temporal_dead_kernel, dim3((unsigned)(((size_t)N * J + 255) / 256)), dim3(256), 0, st, junary, H, N * J, w.dead);
    dispatch_pk(H, [&](auto P, auto K) {
        hipLaunchKernelGGL((joint_temporal_scan_kernel<P(), K()>), grid, dim3(CHAIN_T), 0, st, junary, x, T, seq_start, w.dead, H, N, J, lambda,
                           w.D, w.back, w.endh);
    });
    hipLaunchKernelGGL(joint_temporal_backtrack_kernel, grid, dim3(256), 0, st, seq_start, w.dead, w.endh, w.back, w.D, H, N, J, path, cost);
    return hipGetLastError();
}

}  // namespace zedo
