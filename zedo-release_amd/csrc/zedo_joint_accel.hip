// Joint-wise selection along a video with a second-order motion model for gfx950 (zedo_joint_accel_select): for every joint of every clip
// the hypothesis path that minimises that joint's unary cost plus lambda_v times its displacement plus lambda_a times its SECOND
// difference X[n] - 2 X[n-1] + X[n-2] in the camera frame (x + T) - a term that is blind to a constant velocity.  The state of the chain
// is a PAIR of hypotheses: H^2 states and H^3 transitions per (frame, joint), fp64.  Four kernels:
//   joint_temporal_dead_kernel    (zedo_joint_temporal.hip) one lane per (frame, joint): does it have a finite unary at all?
//   joint_accel_scan_kernel       the forward recurrence over pairs, one workgroup per (clip, joint); the pair table E[n-1] stays in the LDS,
//                                 the arg-min h'' of every pair goes to the workspace as one byte (back2)
//   joint_accel_backtrack_kernel  the backward pass, one workgroup per (clip, joint), runs of back2 staged through the LDS
//   joint_accel_cost_kernel       the cost of the kept path re-accumulated along it, one workgroup per (clip, joint): the terms of a run of
//                                 frames in parallel, their sum by one lane in ascending frame order
// The (clip, joint) of a workgroup, the camera-frame load, the arg-min reduction and - shared with zedo_joint_accel_marginal.hip - a
// lane's pairs, their terms of frames n and n-1 and the factor 2 of the second difference (accel_lead) are zedo_chain.h's.  E is never
// stored for all frames.  No atomics.
#include "zedo_chain.h"

namespace zedo {

// The forward recurrence of one (clip, joint).  The H^2 pairs q = h' H + h are dealt to the 256 lanes round robin: lane t owns the KA
// pairs q = t, t + 256, ..; KA = 1 (H <= 16), 2 (H <= 22), 4 (H <= 32), 7 (H <= 42), 10 (H <= 50), 13 (H <= 57) or 16 (H <= JA_CAP = 64):
// seven instantiations, each the smallest with 256 KA >= H^2, so that the loops over a lane's pairs are straight-line code.
// In the LDS: the table E[n-1] as sE[h'' H + h'] (h''-major: what frame n-1 wrote at its own q), X of frames n, n-1 and n-2 (three
// rotating slots of H fp64 triples) and u of frames n and n-1 (two slots).  A lane keeps g_c = X[n,h,c] - 2 X[n-1,h',c] of its pairs in
// registers; all lanes walk h'' in lockstep: X[n-2,h''] is one broadcast read, and E[n-1][h'',h'] of neighbouring lanes is the same or
// the next double.  Two barriers per frame: A - E[n-1], X[n] and u[n] are in the LDS; B - every lane has read them; the owners then
// replace the table with E[n], which they hold in registers, and the first H lanes put X[n+1], u[n+1] into the slots of frame n-2.
// x, T and junary of frame n+2 are fetched BEFORE barrier A of frame n.
//   start (n first of its clip, or (n-1, j) dead):  nothing to scan; a chain of this one frame keeps the lowest arg-min of u[n,.]
//   second (n-1 is a start):  E[n][h',h] = u[n-1,h'] + (u[n,h] + lambda_v m[n,h',h])
//   otherwise:  E[n][h',h] = u[n,h] + (lambda_v m[n,h',h] + min_h'' (E[n-1][h'',h'] + lambda_a a[n,h'',h',h])), back2 = the lowest h''
// A frame that ends a chain also gets endq: the lowest q = h' H + h that minimises E[n] (of a one-frame chain: the lowest h).
constexpr int JA_CAP = 64;
template <int KA>
__global__ __launch_bounds__(CHAIN_T) void joint_accel_scan_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                const float *__restrict__ Tr, const int *__restrict__ seq_start,
                                                                const int *__restrict__ dead, int H, int N, int J, double lambda_v,
                                                                double lambda_a, unsigned char *__restrict__ back2, int *__restrict__ endq) {
    __shared__ double sE[JA_CAP * JA_CAP];
    __shared__ double sX[3][JA_CAP * 3], sU[2][JA_CAP];
    __shared__ double rv[CHAIN_W];
    __shared__ int rq[CHAIN_W];
    const int tid = threadIdx.x, HH = H * H;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;                                            // (workgroup-uniform)
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
        sU[a & 1][tid] = un;
    }
    fetch(min(a + 1, b - 1));
    unsigned char *const back_j = back2 + (size_t)j * N * HH;      // back2 [J,N,H,H]: the frames of one chain are contiguous
    for (int n = a; n < b; ++n) {
        const double xc[3] = {xn[0], xn[1], xn[2]}, uc = un;       // frame n+1
        fetch(min(n + 2, b - 1));                                  // unconditional: in flight over the barriers of this frame
        const size_t nj = (size_t)n * J + j;
        const bool is_dead = dead[nj] != 0, start = (n > a ? dead[nj - J] : 1) != 0;      // (dead[] is read inside the clip only)
        const bool second = !start && (n - 1 > a ? dead[nj - 2 * (size_t)J] : 1) != 0;
        const bool ends = !is_dead && (n + 1 < b ? dead[nj + J] : 1) != 0;
        const bool scan = !is_dead && !start;                      // (all workgroup-uniform)
        const double *X0 = sX[s0], *X1 = sX[s1], *X2 = sX[s2], *U0 = sU[n & 1], *U1 = sU[(n & 1) ^ 1];
        double en[KA];
        int bn[KA];
        __syncthreads();                                           // A: E[n-1], X[n], X[n-1], X[n-2], u[n], u[n-1] are in the LDS
        ZEDO_CHAIN_PAIR_STEP(KA)                                   // the frame's step (zedo_chain.h): E[n] into en, the lowest h'' into bn
        double v = inf;                                            // a chain of one frame: the candidates are u[n,.]
        int vq = INT_MAX;
        if (ends && start && tid < H) { v = U0[tid]; vq = tid; }
        __syncthreads();                                           // B: the LDS of frame n has been read by every lane
        if (scan) {
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                const int q = tid + k * CHAIN_T;
                if (q < HH) {
                    sE[q] = en[k];                                 // E[n][h',h] at h' H + h: the next frame reads it h''-major
                    if (!second) back_j[(size_t)n * HH + q] = (unsigned char)bn[k];
                    if (arg_better<false>(en[k], q, v, vq)) { v = en[k]; vq = q; }       // (q ascends with k)
                }
            }
        }
        if (tid < H) {
            sX[s2][tid * 3] = xc[0]; sX[s2][tid * 3 + 1] = xc[1]; sX[s2][tid * 3 + 2] = xc[2];
            sU[(n & 1) ^ 1][tid] = uc;
        }
        { const int t = s2; s2 = s1; s1 = s0; s0 = t; }
        if (ends) {                                                // (workgroup-uniform) the lowest arg-min, from the owners' registers
            block_arg<false>(v, vq, rv, rq, tid);
            if (tid == 0) endq[nj] = vq == INT_MAX ? 0 : vq;
        }
    }
}

// The backward pass of one (clip, joint), from the clip's last frame: runs of up to min(JAB_RUN, JAB_BYTES / H^2) frames - the tables
// back2[n+2] the run needs, dead and endq - are staged into the LDS by all lanes, lane 0 walks the run there, then all lanes write path.
// At the end of a chain of two frames or more endq is the pair (h', h) of its last two frames; below them
// path[n] = back2[n+2][path[n+1], path[n+2]].  A value read from the tables is clamped before it is an index.  H <= 64: a run is at
// least JAB_BYTES / 4096 = 8 frames.
constexpr int JAB_RUN = 256, JAB_BYTES = 32768;
static_assert(JAB_BYTES >= JA_CAP * JA_CAP, "at least one staged table of back2 per run");
__global__ __launch_bounds__(256) void joint_accel_backtrack_kernel(const int *__restrict__ seq_start, const int *__restrict__ dead,
                                                                    const int *__restrict__ endq, const unsigned char *__restrict__ back2,
                                                                    int H, int N, int J, int *__restrict__ path) {
    __shared__ unsigned char sb[JAB_BYTES];
    __shared__ int sdead[JAB_RUN + 1], send[JAB_RUN], spath[JAB_RUN];
    __shared__ int carry[4];                                       // lane 0's state between runs: known successors, path[n+1], path[n+2], h'
    const int tid = threadIdx.x, T = blockDim.x, HH = H * H;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;
    const int R = min(JAB_RUN, JAB_BYTES / HH);
    const unsigned char *const back_j = back2 + (size_t)j * N * HH;
    if (tid == 0) { carry[0] = 0; carry[1] = 0; carry[2] = 0; carry[3] = 0; }
    for (int r1 = b; r1 > a; r1 -= R) {                            // the run [r0, r1), walked downwards
        const int r0 = max(a, r1 - R), len = r1 - r0;
        __syncthreads();                                           // the previous run's LDS has been read
        for (int i = tid; i <= len; i += T)                        // sdead[i + 1]: frame r0 + i; sdead[0]: the frame below the run
            sdead[i] = r0 + i - 1 >= a ? dead[(size_t)(r0 + i - 1) * J + j] : 1;
        for (int i = tid; i < len; i += T) send[i] = endq[(size_t)(r0 + i) * J + j];
        const int rows = min(r1 + 2, b) - (r0 + 2);                // the tables of frames r0+2 .. : frame r0 + i reads table i
        if (rows > 0) {
            const unsigned char *src = back_j + (size_t)(r0 + 2) * HH;
            for (int q = tid; q < rows * HH; q += T) sb[q] = src[q];
        }
        __syncthreads();
        if (tid == 0) {
            int have = carry[0], pa = carry[1], pb = carry[2], pend = carry[3];
            for (int i = len - 1; i >= 0; --i) {
                int p = 0;
                if (sdead[i + 1]) have = 0;
                else {
                    if (have == 0) {                               // the last frame of a chain
                        if (sdead[i]) p = clampi(send[i], 0, H - 1);          // .. of one frame
                        else {
                            const int q = clampi(send[i], 0, HH - 1);
                            pend = q / H;
                            p = q - pend * H;
                            have = 1;
                        }
                    } else if (have == 1) { p = pend; have = 2; }
                    else p = clampi(sb[i * HH + pa * H + pb], 0, H - 1);
                    pb = pa;
                    pa = p;
                }
                spath[i] = p;
            }
            carry[0] = have; carry[1] = pa; carry[2] = pb; carry[3] = pend;
        }
        __syncthreads();
        for (int i = tid; i < len; i += T) path[(size_t)(r0 + i) * J + j] = spath[i];
    }
}

// The cost of the kept path, re-accumulated along it, one workgroup per (clip, joint), runs of 256 frames upwards: lane i forms the term
// of frame r0 + i - u[n,p_n] at a start, u[n,p_n] + lambda_v m at the second frame of a chain, u[n,p_n] + (lambda_v m + lambda_a a)
// beyond - and lane 0 adds the terms of the run in ascending frame order, cost[n] = cost[n-1] + term[n].  A dead (frame, joint): +inf.
__global__ __launch_bounds__(256) void joint_accel_cost_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                               const float *__restrict__ Tr, const int *__restrict__ seq_start,
                                                               const int *__restrict__ dead, const int *__restrict__ path, int H, int N,
                                                               int J, double lambda_v, double lambda_a, double *__restrict__ cost) {
    __shared__ double st[256];
    __shared__ int sk[256];                                        // 0 dead, 1 start, 2 inside a chain
    const int tid = threadIdx.x;
    const ClipJoint cj = clip_joint(seq_start, N, J);
    const int j = cj.j, a = cj.a, b = cj.b;
    if (a >= b) return;
    const double inf = __builtin_huge_val();
    double acc = 0.0;                                              // lane 0: cost[n-1]
    for (int r0 = a; r0 < b; r0 += 256) {
        const int len = min(256, b - r0), n = r0 + tid;
        __syncthreads();                                           // the previous run's LDS has been read
        if (tid < len) {
            const size_t nj = (size_t)n * J + j;
            int kind = 0;
            double t = 0.0;
            if (!dead[nj]) {
                const bool start = (n > a ? dead[nj - J] : 1) != 0;
                const bool second = !start && (n - 1 > a ? dead[nj - 2 * (size_t)J] : 1) != 0;
                const int p0 = clampi(path[nj], 0, H - 1);
                const double u0 = junary[((size_t)p0 * N + n) * J + j];
                t = finite64(u0) ? u0 : inf;
                kind = 1;
                if (!start) {
                    const int p1 = clampi(path[nj - J], 0, H - 1);
                    double X0[3], X1[3];
                    load_cam(x, Tr, (size_t)p0 * N + n, J, j, X0);
                    load_cam(x, Tr, (size_t)p1 * N + n - 1, J, j, X1);
                    const double d0 = X0[0] - X1[0], d1 = X0[1] - X1[1], d2 = X0[2] - X1[2];
                    double w = lambda_v * sqrt(d0 * d0 + d1 * d1 + d2 * d2);
                    if (!second) {
                        const int p2 = clampi(path[nj - 2 * (size_t)J], 0, H - 1);
                        double X2[3];
                        load_cam(x, Tr, (size_t)p2 * N + n - 2, J, j, X2);
                        const double e0 = accel_lead(X0[0], X1[0]) + X2[0], e1 = accel_lead(X0[1], X1[1]) + X2[1],
                                     e2 = accel_lead(X0[2], X1[2]) + X2[2];
                        w = w + lambda_a * sqrt(e0 * e0 + e1 * e1 + e2 * e2);
                    }
                    t = t + w;
                    kind = 2;
                }
            }
            st[tid] = t;
            sk[tid] = kind;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < len; ++i) {
                const int kind = sk[i];
                acc = kind == 2 ? acc + st[i] : st[i];
                st[i] = kind ? acc : inf;
            }
        }
        __syncthreads();
        if (tid < len) cost[(size_t)n * J + j] = st[tid];
    }
}

// Workspace: back2 [J,N,H,H] u8 (padded to 4 bytes) | dead [N,J] i32, endq [N,J] i32
struct JointAccelWs {
    Carve c;
    unsigned char *back2;
    int *dead, *endq;
    size_t bytes;
    JointAccelWs(void *ws, size_t nj, size_t H)
        : c(ws), back2(c.take<unsigned char>(nj * H * H)), dead(c.take<int>(nj)), endq(c.take<int>(nj)), bytes(c.bytes()) {}
};
size_t joint_accel_bytes(int N, int H, int J) { return JointAccelWs(nullptr, (size_t)N * J, H).bytes; }

hipError_t launch_joint_accel_select(const double *junary, const float *x, const float *T, const int *seq_start, int n_seq, int H, int N,
                                     int J, double lambda_v, double lambda_a, void *ws, int *path, double *cost, hipStream_t st) {
    const JointAccelWs w(ws, (size_t)N * J, H);
    const dim3 grid((unsigned)n_seq * (unsigned)J);                // n_seq <= N and N J H <= INT_MAX
    const hipError_t e = launch_joint_temporal_dead(junary, H, N * J, w.dead, st);
    if (e != hipSuccess) return e;
    dispatch_pairs(H, [&](auto KA) {
        hipLaunchKernelGGL((joint_accel_scan_kernel<KA()>), grid, dim3(CHAIN_T), 0, st, junary, x, T, seq_start, w.dead, H, N, J, lambda_v,
                           lambda_a, w.back2, w.endq);
    });
    hipLaunchKernelGGL(joint_accel_backtrack_kernel, grid, dim3(256), 0, st, seq_start, w.dead, w.endq, w.back2, H, N, J, path);
    hipLaunchKernelGGL(joint_accel_cost_kernel, grid, dim3(256), 0, st, junary, x, T, seq_start, w.dead, path, H, N, J, lambda_v, lambda_a,
                       cost);
    return hipGetLastError();
}

}  // namespace zedo
