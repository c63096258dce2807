// Joint-wise selection along a video for gfx950 (zedo_joint_temporal_select): for every joint of every clip the hypothesis path that
// minimises that joint's unary cost plus lambda times that joint's displacement in the camera frame (x + T) to the previous frame's
// choice - J independent Viterbi chains per clip, fp64.  Three kernels:
//   joint_temporal_dead_kernel       one lane per (frame, joint): does it have a hypothesis with a finite unary at all?
//   joint_temporal_scan_kernel       the forward recurrence, one workgroup per (clip, joint); the transition cost of a pair (h', h) is one
//                                    square root of three terms and is computed where the recurrence consumes it - there is no H x H table
//   joint_temporal_backtrack_kernel  the backward pass, one workgroup per (clip, joint), runs of the back table staged through the LDS
// Workgroup w serves clip w / J, joint w % J: the J chains of a clip are neighbours in the grid.  A chain reads 12 bytes of x per
// (frame, hypothesis), at a stride of N J 3 floats across h; the other joints of the same pose row sit in the same few 128-byte
// lines, and neighbours in the grid run at the same time, so a line fetched from HBM for one chain serves the others from the L2.
// No atomics.
#include "zedo_internal.h"

namespace zedo {

__device__ __forceinline__ bool jt_finite64(double v) { return fabs(v) < __builtin_huge_val(); }   // false for NaN and +-inf
__device__ __forceinline__ int jt_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void joint_temporal_dead_kernel(const double *__restrict__ junary, int H, int NJ, int *__restrict__ dead) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;           // i = n J + j: junary[(h N + n) J + j] = junary[h NJ + i]
    if (i >= NJ) return;
    int any = 0;
    for (int h = 0; h < H; ++h) any |= jt_finite64(junary[(size_t)h * NJ + i]) ? 1 : 0;   // a wave reads 512 contiguous bytes per hypothesis
    dead[i] = any ? 0 : 1;
}

// The forward recurrence of one (clip, joint).  256 lanes as P parts x 256 / P slots:
//   P = 4 (H <= 64) and P = 2 (H <= 128): lane (part, slot) owns h = slot and walks ONE part of the h' (ceil(H / P) consecutive ones);
//       the parts' minima meet in the LDS and part 0 combines them in ascending part order with a strict comparison - the tie still
//       goes to the lowest h';
//   P = 1 (H <= JT_CAP = 1024): lane t owns K hypotheses h = t, t + 256, .. and walks all h'; one LDS read of (X[n-1,h'], D[n-1,h'])
//       serves the lane's every h.  K = 1 (H <= 256), 2 (H <= 512) or 4: no lane evaluates square roots for a hypothesis nobody owns
//       beyond the last, partly filled group of 256.
// X[n-1,.] (fp64 triples) and D[n-1,.] sit in the LDS; every lane of a wave reads the same h' - a broadcast.  Two barriers per frame:
// A - frame n-1 is in the LDS; B - every lane has read it (and the parts' minima are in the LDS), the owners replace it with frame n,
// which they hold in registers.  What does not depend on D - x, T and junary of frame n+1 - is fetched BEFORE barrier A of frame n.
//   chain start (first frame of the clip, or (n-1, j) dead):  D[n,j,h] = u[n,j,h], back = -1
//   otherwise:  D[n,j,h] = u[n,j,h] + min_h' (D[n-1,j,h'] + lambda m[n,j,h',h]), back = the lowest h' that attains it
//   dead (n, j): D[n,j,.] = +inf
// A frame that ends a chain (last of the clip, or (n+1, j) dead) also gets the lowest arg-min of D[n,j,.] (endh): the backward pass
// starts there.
constexpr int JT_T = 256, JT_CAP = 1024;
template <int P, int K>
__global__ __launch_bounds__(JT_T) void joint_temporal_scan_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                   const float *__restrict__ Tr, const int *__restrict__ seq_start,
                                                                   const int *__restrict__ dead, int H, int N, int J, double lambda,
                                                                   double *__restrict__ D, int *__restrict__ back, int *__restrict__ endh) {
    constexpr int SLOTS = JT_T / P, CAP = K * SLOTS;
    static_assert(P == 1 || K == 1, "a lane owns several hypotheses only where the h' are not split");
    __shared__ double sX[CAP * 3], sD[CAP];
    __shared__ double sPv[JT_T];                                   // the parts' minima (P > 1)
    __shared__ int sPi[JT_T];
    __shared__ double rv[JT_T / 64];
    __shared__ int rh[JT_T / 64];
    const int tid = threadIdx.x, part = tid / SLOTS, slot = tid - part * SLOTS;
    const int s = blockIdx.x / J, j = blockIdx.x - s * J;
    const int a = jt_clampi(seq_start[s], 0, N), b = jt_clampi(seq_start[s + 1], 0, N);
    if (a >= b) return;                                            // (workgroup-uniform)
    const double inf = __builtin_huge_val();
    const int per = (H + P - 1) / P, q0 = min(H, part * per), q1 = min(H, q0 + per);      // this lane's h' (part 0 is never empty)
    // X[n,h,j,.] and u[n,j,h] of this lane's h (a lane past H reads hypothesis H-1 and stores nothing)
    double xn[K][3], un[K];
    auto fetch = [&](int n) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const size_t g = (size_t)min(slot + k * SLOTS, H - 1) * N + n;
            const float *px = x + (g * J + j) * 3;
#ifdef ZEDO_MUT_JT_NO_T   // tools/mutation_check.py only: the motion term is taken on x alone although T was given
            const float *pt = nullptr;
#else
            const float *pt = Tr ? Tr + g * 3 : nullptr;
#endif
#pragma unroll
            for (int c = 0; c < 3; ++c) xn[k][c] = (double)px[c] + (pt ? (double)pt[c] : 0.0);
            un[k] = junary[g * J + j];
        }
    };
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
        if (chain) {
#pragma unroll
            for (int k = 0; k < K; ++k) { dn[k] = inf; bn[k] = 0; }
#pragma unroll 4
            for (int hp = q0; hp < q1; ++hp) {
                const double p0 = sX[hp * 3], p1 = sX[hp * 3 + 1], p2 = sX[hp * 3 + 2], pd = sD[hp];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double d0 = xc[k][0] - p0, d1 = xc[k][1] - p1, d2 = xc[k][2] - p2;
                    const double c = pd + lambda * sqrt(d0 * d0 + d1 * d1 + d2 * d2);
                    if (hp == q0 || c < dn[k]) { dn[k] = c; bn[k] = hp; }   // strict: the lowest h' that attains the minimum
                }
            }
            if (P > 1) { sPv[tid] = dn[0]; sPi[tid] = bn[0]; }
        }
        __syncthreads();                                           // B: frame n-1 has been read by every lane
        if (part == 0) {
            if (chain && P > 1) {
                const int np = (H + per - 1) / per;                // the parts that are not empty
                for (int p = 1; p < np; ++p) {
                    const double c = sPv[p * SLOTS + slot];
                    if (c < dn[0]) { dn[0] = c; bn[0] = sPi[p * SLOTS + slot]; }
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int h = slot + k * SLOTS;
                if (h < H) {
                    const double u0 = jt_finite64(uc[k]) ? uc[k] : inf;
                    const double d = chain ? u0 + dn[k] : (is_dead ? inf : u0);
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
            int vh = 0x7fffffff;
            if (part == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int h = slot + k * SLOTS;
                    if (h < H && (dn[k] < v || (dn[k] == v && h < vh))) { v = dn[k]; vh = h; }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(v, off);
                const int oh = __shfl_xor(vh, off);
                if (ov < v || (ov == v && oh < vh)) { v = ov; vh = oh; }
            }
            if ((tid & 63) == 0) { rv[tid >> 6] = v; rh[tid >> 6] = vh; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < JT_T / 64; ++w)
                    if (rv[w] < v || (rv[w] == v && rh[w] < vh)) { v = rv[w]; vh = rh[w]; }
                endh[nj] = vh == 0x7fffffff ? 0 : vh;
            }
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
    const int s = blockIdx.x / J, j = blockIdx.x - s * J;
    const int a = jt_clampi(seq_start[s], 0, N), b = jt_clampi(seq_start[s + 1], 0, N);
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
                    p = jt_clampi(have ? sb[i * H + p] : send[i], 0, H - 1);
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
size_t joint_temporal_bytes(int N, int H, int J) {
    const size_t nj = (size_t)N * J, njh = nj * H;
    return njh * 8 + (((njh + 2 * nj) * 4 + 7) & ~(size_t)7);
}

// the dead flags on their own, for the other chain model on the same unaries (zedo_joint_marginal.hip)
hipError_t launch_joint_temporal_dead(const double *junary, int H, int NJ, int *dead, hipStream_t st) {
    hipLaunchKernelGGL(joint_temporal_dead_kernel, dim3((unsigned)(((size_t)NJ + 255) / 256)), dim3(256), 0, st, junary, H, NJ, dead);
    return hipGetLastError();
}

hipError_t launch_joint_temporal_select(const double *junary, const float *x, const float *T, const int *seq_start, int n_seq, int H, int N,
                                        int J, double lambda, void *ws, int *path, double *cost, hipStream_t st) {
    const size_t nj = (size_t)N * J, njh = nj * H;
    double *D = static_cast<double *>(ws);
    int *back = reinterpret_cast<int *>(D + njh), *dead = back + njh, *endh = dead + nj;
    const dim3 grid((unsigned)n_seq * (unsigned)J);                // n_seq <= N and N J H <= INT_MAX
    hipLaunchKernelGGL(joint_temporal_dead_kernel, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, st, junary, H, (int)nj, dead);
#define ZEDO_JT_SCAN(P, K)                                                                                                          \
    hipLaunchKernelGGL((joint_temporal_scan_kernel<P, K>), grid, dim3(JT_T), 0, st, junary, x, T, seq_start, dead, H, N, J, lambda, D, back, \
                       endh)
    if (H <= JT_T / 4) ZEDO_JT_SCAN(4, 1);
    else if (H <= JT_T / 2) ZEDO_JT_SCAN(2, 1);
    else if (H <= JT_T) ZEDO_JT_SCAN(1, 1);
    else if (H <= 2 * JT_T) ZEDO_JT_SCAN(1, 2);
    else ZEDO_JT_SCAN(1, 4);
#undef ZEDO_JT_SCAN
    hipLaunchKernelGGL(joint_temporal_backtrack_kernel, grid, dim3(256), 0, st, seq_start, dead, endh, back, D, H, N, J, path, cost);
    return hipGetLastError();
}

}  // namespace zedo
