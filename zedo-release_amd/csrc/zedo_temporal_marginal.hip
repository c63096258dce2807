// Pose-level fusion along a video for gfx950 (zedo_temporal_marginal): the sum-product twin of zedo_temporal.hip, as zedo_joint_marginal.hip
// is the twin of zedo_joint_temporal.hip.  Per clip the posterior marginals of the WHOLE hypotheses under the chain model the Viterbi
// recurrence of zedo_temporal_select optimises, at a temperature tau - forward-backward in the log domain, fp64 - and from them the
// posterior mean pose, the covariance of every joint and the most probable hypothesis of every frame.  Kernels, in stream order:
//   temporal_dead_kernel                      (zedo_temporal.hip) one lane per frame: does it have a finite unary at all?
//   per chunk of C frames, ascending:
//     temporal_transition_kernel              (zedo_temporal.hip) m[n,h',h] as M[n - c0][h'][h]
//     temporal_marginal_forward_kernel        A[n,.], temporal_scan_kernel<true>'s layout with (min, +) replaced by (LSE, +); log Z at a chain's end
//   per chunk, DESCENDING:
//     temporal_marginal_transition_back_kernel  the same tile with the two frames' roles swapped: m[n+1,h,h'] as Mt[n - c0][h'][h] - the
//                                             transposed table, the same bits ((a - b)^2 = (b - a)^2 exactly, the joint order is unchanged)
//     temporal_marginal_backward_kernel       B[n,.] from the chunk's last frame down, log Z handed down the chain
//   temporal_marginal_weight_kernel           one wave per frame: w = exp(A + B - log Z) over the B table, d_w, the arg-max, log Z
//   temporal_marginal_moments_kernel          one lane per (frame, joint): the mean, then the centred covariance; the only pass over d_x
// A, B, log Z and the dead flags live in the workspace for all frames and everything that crosses a chunk boundary goes through them, so
// the result does not depend on C.  The transition costs of a chunk are computed twice, once in each layout: the workspace holds one chunk
// of them.  No atomics, no scratch.  Every log-sum-exp takes two walks over its terms, shifted by their TRUE maximum.
#include "zedo_temporal.h"

#include <algorithm>

namespace zedo {

// LSE_h' (V[h'] - c Mn[h' H + h]), h' ascending in both walks: the largest term, then the sum of exp(term - largest) (shifted by 0 where
// no term is above -inf: every exp is 0 and the result -inf).  V [H] sits in the LDS; `first`: h is the lane's first hypothesis, whose
// TS_PF leading costs mc were fetched a frame ahead.
__device__ __forceinline__ double tm_lse(const double *V, const double *__restrict__ Mn, int H, int h, bool first, const double (&mc)[TS_PF],
                                         double c) {
    const double ninf = -__builtin_huge_val();
    const int h0 = first ? min(TS_PF, H) : 0;
    double mx = ninf;
    if (first) {
#pragma unroll
        for (int k = 0; k < TS_PF; ++k)
            if (k < H) {
                const double t = V[k] - c * mc[k];
                if (t > mx) mx = t;
            }
    }
#pragma unroll 8
    for (int hp = h0; hp < H; ++hp) {
        const double t = V[hp] - c * Mn[(size_t)hp * H + h];
        if (t > mx) mx = t;
    }
    const double sh = mx > ninf ? mx : 0.0;
    double sm = 0.0;
    if (first) {
#pragma unroll
        for (int k = 0; k < TS_PF; ++k)
            if (k < H) sm += exp((V[k] - c * mc[k]) - sh);
    }
#pragma unroll 4
    for (int hp = h0; hp < H; ++hp) sm += exp((V[hp] - c * Mn[(size_t)hp * H + h]) - sh);
    return mx + log(sm);
}

// The forward recurrence: temporal_scan_kernel<true> with (min, +) replaced by (LSE, +).  One workgroup per clip s walks the frames of
// the chunk [c0, c0 + cnt) inside [seq_start[s], seq_start[s+1]) (clamped to 0 .. N); lane t owns h = t, t + T, ..; A[n-1,.] stays in
// the LDS, double buffered, ONE barrier per frame; a chunk that continues a clip takes A[lo-1,.] from the table; u[n+1,h] and the first
// TS_PF transition costs of the lane's first h are fetched BEFORE the barrier that ends frame n.
//   l[n,h] = -u[n,h] / tau, -inf where the unary is not finite
//   chain start (first frame of the clip, or frame n-1 dead):  A[n,h] = l[n,h]
//   otherwise:  A[n,h] = l[n,h] + LSE_h' (A[n-1,h'] - c m[n,h',h])
//   dead frame: A[n,.] = -inf
// A frame that ends a chain (last of the clip, or frame n+1 dead) also gets log Z = LSE_h A[n,h] (lz[n]): shifted by the largest A, the
// lane's h ascending, a butterfly inside each wave, then the waves ascending.
__global__ __launch_bounds__(256) void temporal_marginal_forward_kernel(const double *__restrict__ unary, const double *__restrict__ M,
                                                                        const int *__restrict__ seq_start, const int *__restrict__ dead,
                                                                        int H, int N, double c, double tau, int c0, int cnt,
                                                                        double *A, double *__restrict__ lz) {
    __shared__ double sA[2 * TS_CAP];
    __shared__ double rv[4];
    const int tid = threadIdx.x, T = blockDim.x, nw = T >> 6;
    const int a = clampi(seq_start[blockIdx.x], 0, N), b = clampi(seq_start[blockIdx.x + 1], 0, N);
    const int lo = max(a, c0), hi = min(b, c0 + cnt);
    if (lo >= hi) return;                                          // (workgroup-uniform)
    const double ninf = -__builtin_huge_val();
    const size_t HH = (size_t)H * H;
    int cur = 0;
    if (lo > a)                                                    // the clip began in an earlier chunk: A[lo-1,.] from the table
        for (int h = tid; h < H; h += T) sA[h] = A[(size_t)(lo - 1) * H + h];
    const int hf = min(tid, H - 1);
    double un = unary[(size_t)hf * N + lo], mn[TS_PF];
#pragma unroll
    for (int k = 0; k < TS_PF; ++k) mn[k] = M[(size_t)(lo - c0) * HH + (size_t)min(k, H - 1) * H + hf];
    // (frame 0 has no transition costs - its slot of M, which always exists, is read unwritten - and is a chain start: they are not used)
    for (int n = lo; n < hi; ++n) {
        const double uc = un;
        double mc[TS_PF];
#pragma unroll
        for (int k = 0; k < TS_PF; ++k) mc[k] = mn[k];
        {   // unconditional loads: the last frame re-reads its own
            const int nn = min(n + 1, hi - 1);
            un = unary[(size_t)hf * N + nn];
#pragma unroll
            for (int k = 0; k < TS_PF; ++k) mn[k] = M[(size_t)(nn - c0) * HH + (size_t)min(k, H - 1) * H + hf];
        }
        const bool is_dead = dead[n] != 0, start = (n > a ? dead[n - 1] : 1) != 0;          // (dead[] is read inside 0 .. N-1 only)
        const bool ends = !is_dead && (n + 1 < b ? dead[n + 1] : 1) != 0;
        __syncthreads();                                           // A[n-1,.] of every lane is in sA[cur]
        const double *Mn = M + (size_t)(n - c0) * HH;
        const double *prev = sA + cur * TS_CAP;
        for (int h = tid; h < H; h += T) {
            const bool first = h == tid;
            const double u0 = first ? uc : unary[(size_t)h * N + n];
            const double l = finite64(u0) ? -u0 / tau : ninf;
            double v = is_dead ? ninf : l;
            if (!is_dead && !start) v = l + tm_lse(prev, Mn, H, h, first, mc, c);
            A[(size_t)n * H + h] = v;
            sA[(cur ^ 1) * TS_CAP + h] = v;
        }
        cur ^= 1;
        if (ends) {                                                // (workgroup-uniform) log Z of the chain that ends here
            __syncthreads();                                       // A[n,.] of every lane is in sA[cur]
            double v = ninf;
            for (int h = tid; h < H; h += T) v = fmax(v, sA[cur * TS_CAP + h]);
            v = wave_max(v);
            if ((tid & 63) == 0) rv[tid >> 6] = v;
            __syncthreads();
            v = rv[0];
            for (int w = 1; w < nw; ++w) v = fmax(v, rv[w]);
            __syncthreads();                                       // rv takes the sums next
            double e = 0.0;
            for (int h = tid; h < H; h += T) e += exp(sA[cur * TS_CAP + h] - v);
            e = wave_sum(e);
            if ((tid & 63) == 0) rv[tid >> 6] = e;
            __syncthreads();                                       // (the next write to rv is behind the next frame's barrier)
            if (tid == 0) {
                double s = rv[0];
                for (int w = 1; w < nw; ++w) s += rv[w];
                lz[n] = v + log(s);
            }
        }
    }
}

// m[n+1,h,h'] of the frames n = c0 + i of a chunk, for the backward walk: ZEDO_TEMPORAL_TILE with the two frames' roles swapped - the
// 64-wide side is h of frame n, the 16-wide side h' of frame n+1 - written as Mt[i][h'][h], so that the lanes of the backward scan (one
// per h) read a row of it coalesced.  The bits are those of temporal_transition_kernel's m[n+1][h][h'].
__global__ __launch_bounds__(TT_T) void temporal_marginal_transition_back_kernel(const float *__restrict__ x, int H, int N, int J, int c0,
                                                                                 double *__restrict__ M) {
    __shared__ float sc[TT_H * TT_LD];                             // frame n, hypotheses h0 ..
    __shared__ float sp[TT_P * TT_LD];                             // frame n+1, hypotheses p0 ..
    const int n = c0 + blockIdx.x;
    if (n + 1 >= N) return;                                        // the last frame has no successor (workgroup-uniform)
    ZEDO_TEMPORAL_TILE_LANES
    const size_t hs = (size_t)N * J * 3;                           // floats from one hypothesis of a frame to the next
    ZEDO_TEMPORAL_TILE(x[(size_t)(h0 + r) * hs + ((size_t)n * J + js) * 3 + e], x[(size_t)(p0 + r) * hs + ((size_t)(n + 1) * J + js) * 3 + e])
}

// The backward recurrence on the frames of the chunk [c0, c0 + cnt) inside the clip, from the last down.  The LDS holds V[n+1,.] =
// l[n+1,.] + B[n+1,.], double buffered, ONE barrier per frame; the lane that owns h walks the h' of frame n+1 along row h' of Mt.  The
// chunks run in DESCENDING order: a clip that goes on past the chunk takes B[hi,.] and the chain's log Z from the tables.
//   chain end (last frame of the clip, or frame n+1 dead):  B[n,h] = 0; log Z is the forward kernel's lz[n]
//   otherwise:  B[n,h] = LSE_h' (l[n+1,h'] + B[n+1,h'] - c m[n+1,h,h']), lz[n] = lz[n+1]
//   dead frame: B[n,.] = 0 (nothing reads it), lz[n] = -inf
__global__ __launch_bounds__(256) void temporal_marginal_backward_kernel(const double *__restrict__ unary, const double *__restrict__ Mt,
                                                                         const int *__restrict__ seq_start, const int *__restrict__ dead,
                                                                         int H, int N, double c, double tau, int c0, int cnt, double *B,
                                                                         double *lz) {
    __shared__ double sV[2 * TS_CAP];
    const int tid = threadIdx.x, T = blockDim.x;
    const int a = clampi(seq_start[blockIdx.x], 0, N), b = clampi(seq_start[blockIdx.x + 1], 0, N);
    const int lo = max(a, c0), hi = min(b, c0 + cnt);
    if (lo >= hi) return;                                          // (workgroup-uniform)
    const double ninf = -__builtin_huge_val();
    const size_t HH = (size_t)H * H;
    int cur = 0;
    double lzc = ninf;                                             // log Z of the chain the walk is in (workgroup-uniform)
    if (hi < b && dead[hi] == 0) {                                 // the clip goes on in a later chunk, which has been walked
        for (int h = tid; h < H; h += T) {
            const double u1 = unary[(size_t)h * N + hi];
            sV[h] = (finite64(u1) ? -u1 / tau : ninf) + B[(size_t)hi * H + h];
        }
        lzc = lz[hi];
    }
    const int hf = min(tid, H - 1);
    double un = unary[(size_t)hf * N + (hi - 1)], mn[TS_PF];
#pragma unroll
    for (int k = 0; k < TS_PF; ++k) mn[k] = Mt[(size_t)(hi - 1 - c0) * HH + (size_t)min(k, H - 1) * H + hf];
    // (frame N-1 has no successor - its slot of Mt is read as the forward pass left it - and ends a chain: the costs are not used)
    for (int n = hi - 1; n >= lo; --n) {
        const double uc = un;
        double mc[TS_PF];
#pragma unroll
        for (int k = 0; k < TS_PF; ++k) mc[k] = mn[k];
        {   // unconditional loads: the first frame re-reads its own
            const int nn = max(n - 1, lo);
            un = unary[(size_t)hf * N + nn];
#pragma unroll
            for (int k = 0; k < TS_PF; ++k) mn[k] = Mt[(size_t)(nn - c0) * HH + (size_t)min(k, H - 1) * H + hf];
        }
        const bool is_dead = dead[n] != 0, ends = (n + 1 < b ? dead[n + 1] : 1) != 0;       // (dead[] is read inside 0 .. N-1 only)
        const bool chain = !is_dead && !ends;                      // (workgroup-uniform) frame n+1 continues this chain
        if (is_dead) lzc = ninf;
        else if (ends) lzc = lz[n];                                // written by the forward kernel, by no lane of this one
        __syncthreads();                                           // V[n+1,.] of every lane is in sV[cur]
        const double *Mn = Mt + (size_t)(n - c0) * HH;
        const double *next = sV + cur * TS_CAP;
        for (int h = tid; h < H; h += T) {
            const bool first = h == tid;
            const double u0 = first ? uc : unary[(size_t)h * N + n];
            const double l = finite64(u0) ? -u0 / tau : ninf;
            double Bv = 0.0;
#ifndef ZEDO_MUT_TM_NO_BACKWARD   // tools/mutation_check.py only: B = 0 on every frame - the filtering marginals, not the smoothed ones
            if (chain) Bv = tm_lse(next, Mn, H, h, first, mc, c);
#endif
            B[(size_t)n * H + h] = Bv;
            sV[(cur ^ 1) * TS_CAP + h] = is_dead ? ninf : l + Bv;
        }
        cur ^= 1;
        if (tid == 0 && !(ends && !is_dead)) lz[n] = lzc;
    }
}

// One wave per frame: w[n,h] = exp(A[n,h] + B[n,h] - log Z) - exactly 0 for an excluded hypothesis (A = -inf) - written over B[n,.] for
// the moments kernel and to d_w if given; the lowest h with the largest marginal (the lane's h ascending, strict; then the wave's
// butterfly with the tie to the lowest h), that marginal, log Z.  A dead frame: a row of zeros, hypothesis 0, 0, -inf.
__global__ __launch_bounds__(CHAIN_T) void temporal_marginal_weight_kernel(const double *__restrict__ A, double *__restrict__ W,
                                                                           const double *__restrict__ lz, const int *__restrict__ dead,
                                                                           int H, int N, int *__restrict__ hmax, double *__restrict__ wmax,
                                                                           double *__restrict__ logz, double *__restrict__ wout) {
    const int n = blockIdx.x * CHAIN_W + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;                                            // (wave-uniform)
    const double ninf = -__builtin_huge_val();
    const bool is_dead = dead[n] != 0;
    const double z = lz[n];
    double bw = ninf;
    int bh = INT_MAX;
    for (int h = lane; h < H; h += 64) {
        const size_t q = (size_t)n * H + h;
        const double w = is_dead ? 0.0 : exp((A[q] + W[q]) - z);
        W[q] = w;
        if (wout) wout[q] = w;
        if (!is_dead && w > bw) { bw = w; bh = h; }
    }
    wave_arg<true>(bw, bh);
    if (lane == 0) {
        hmax[n] = bh == INT_MAX ? 0 : bh;
        wmax[n] = bh == INT_MAX ? 0.0 : bw;
        logz[n] = is_dead ? ninf : z;
    }
}

// One lane per (frame, joint), q = n J + j: the lanes of a wave read 768 contiguous bytes of a hypothesis' row of d_x (any alignment).
//   X[h,n,j,c] = (double)x + (T ? (double)T : 0);  mean = sum_h w X, h ascending;  cov = sum_h w (X - mean)(X - mean)^T from the
//   centred differences, h ascending, in the order xx, xy, xz, yy, yz, zz.  The second walk reads the rows again.
// A dead frame reports NaN in both.
__global__ __launch_bounds__(CHAIN_T) void temporal_marginal_moments_kernel(const float *__restrict__ x, const float *__restrict__ Tr,
                                                                            const double *__restrict__ W, const int *__restrict__ dead,
                                                                            int H, int N, int J, double *__restrict__ mean,
                                                                            double *__restrict__ cov) {
    const size_t q = (size_t)blockIdx.x * CHAIN_T + threadIdx.x, NJ = (size_t)N * J;
    if (q >= NJ) return;
    const size_t n = q / J;
    if (dead[n]) {
        const double qnan = __builtin_nan("");
#pragma unroll
        for (int i = 0; i < 3; ++i) mean[q * 3 + i] = qnan;
#pragma unroll
        for (int i = 0; i < 6; ++i) cov[q * 6 + i] = qnan;
        return;
    }
    const double *w = W + n * H;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
#pragma unroll 4
    for (int h = 0; h < H; ++h) {
        const float *px = x + ((size_t)h * NJ + q) * 3;
        const float *pt = Tr ? Tr + ((size_t)h * N + n) * 3 : nullptr;
        const double wh = w[h];
        m0 += wh * ((double)px[0] + (pt ? (double)pt[0] : 0.0));
        m1 += wh * ((double)px[1] + (pt ? (double)pt[1] : 0.0));
        m2 += wh * ((double)px[2] + (pt ? (double)pt[2] : 0.0));
    }
    double c6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int h = 0; h < H; ++h) {
        const float *px = x + ((size_t)h * NJ + q) * 3;
        const float *pt = Tr ? Tr + ((size_t)h * N + n) * 3 : nullptr;
        const double wh = w[h];
        const double d0 = ((double)px[0] + (pt ? (double)pt[0] : 0.0)) - m0, d1 = ((double)px[1] + (pt ? (double)pt[1] : 0.0)) - m1,
                     d2 = ((double)px[2] + (pt ? (double)pt[2] : 0.0)) - m2;
        c6[0] += wh * (d0 * d0); c6[1] += wh * (d0 * d1); c6[2] += wh * (d0 * d2);
        c6[3] += wh * (d1 * d1); c6[4] += wh * (d1 * d2); c6[5] += wh * (d2 * d2);
    }
    mean[q * 3] = m0; mean[q * 3 + 1] = m1; mean[q * 3 + 2] = m2;
#pragma unroll
    for (int i = 0; i < 6; ++i) cov[q * 6 + i] = c6[i];
}

// Workspace: A [N,H] f64 | B [N,H] f64 (the marginals in the end) | lz [N] f64 | dead [N] i32 (padded to 8 bytes) | M [C,H,H] f64
struct TemporalMarginalWs {
    Carve c;
    double *A, *B, *lz;
    int *dead;
    double *M;
    size_t fixed_bytes;                                            // everything but M
    TemporalMarginalWs(void *ws, size_t N, size_t H)
        : c(ws), A(c.take<double>(N * H)), B(c.take<double>(N * H)), lz(c.take<double>(N)), dead(c.take<int>(N)), M(c.take<double>(0)),
          fixed_bytes(c.bytes()) {}
};
size_t temporal_marginal_fixed_bytes(int N, int H) { return TemporalMarginalWs(nullptr, N, H).fixed_bytes; }

hipError_t launch_temporal_marginal(const double *unary, const float *x, const float *Tr, const int *seq_start, int n_seq, int H, int N, int J,
                                    double c, double tau, void *ws, int chunk, double *mean, double *cov, int *hmax, double *wmax,
                                    double *logz, double *wout, hipStream_t st) {
    const TemporalMarginalWs w(ws, N, H);
    hipLaunchKernelGGL(temporal_dead_kernel, dim3((N + 255) / 256), dim3(256), 0, st, unary, H, N, w.dead);
    const int T = std::min(256, (H + 63) / 64 * 64);
    const int ty = (H + TT_H - 1) / TT_H, tz = (H + TT_P - 1) / TT_P;          // the tiles of a frame's H x H transition costs
    int last = 0;
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int cnt = std::min(chunk, N - c0);
        last = c0;
        if (c0 + cnt > 1)
            hipLaunchKernelGGL(temporal_transition_kernel, dim3(cnt, ty, tz), dim3(TT_T), 0, st, x, H, N, J, c0, w.M);
        hipLaunchKernelGGL(temporal_marginal_forward_kernel, dim3(n_seq), dim3(T), 0, st, unary, w.M, seq_start, w.dead, H, N, c, tau, c0, cnt,
                           w.A, w.lz);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (int c0 = last; c0 >= 0; c0 -= chunk) {
        const int cnt = std::min(chunk, N - c0);
        if (c0 + 1 < N)
            hipLaunchKernelGGL(temporal_marginal_transition_back_kernel, dim3(cnt, ty, tz), dim3(TT_T), 0, st, x, H, N, J, c0,
                               w.M);
        hipLaunchKernelGGL(temporal_marginal_backward_kernel, dim3(n_seq), dim3(T), 0, st, unary, w.M, seq_start, w.dead, H, N, c, tau, c0, cnt,
                           w.B, w.lz);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(temporal_marginal_weight_kernel, dim3((N + CHAIN_W - 1) / CHAIN_W), dim3(CHAIN_T), 0, st, w.A, w.B, w.lz, w.dead, H, N,
                       hmax, wmax, logz, wout);
    const size_t NJ = (size_t)N * J;
    hipLaunchKernelGGL(temporal_marginal_moments_kernel, dim3((unsigned)((NJ + CHAIN_T - 1) / CHAIN_T)), dim3(CHAIN_T), 0, st, x, Tr, w.B,
                       w.dead, H, N, J, mean, cov);
    return hipGetLastError();
}

}  // namespace zedo
