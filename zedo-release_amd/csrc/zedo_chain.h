// What the label-free selection and fusion kernels share (zedo_temporal.hip, zedo_temporal_stream.hip, zedo_joint_temporal.hip, zedo_joint_stream.hip,
// zedo_joint_stream_marginal.hip, zedo_joint_marginal.hip, zedo_joint_accel.hip, zedo_joint_accel_stream.hip, zedo_joint_accel_marginal.hip, zedo_joint_accel_stream_marginal.hip, zedo_joint_tree.hip, zedo_joint_tree_marginal.hip): the one
// copy of their lane layout, their reductions and their staging.  The rules every user relies on live here and nowhere else:
//   - a tie goes to the lowest index (strict comparisons, parts and waves combined in ascending order);
//   - a sum is a butterfly inside each wave, then the waves in ascending order: a fixed order, no atomics;
//   - a lane past H reads row H-1 and stores nothing;
//   - an offset read from seq_start is clamped to 0 .. N before it is an address.
// The recurrences themselves - what is minimised or summed - stay in their own files; the four that two files run, the first-order
// chain's frame step, its sum-product twin, the second-order chain's frame step and its sum-product twin, are here.
#pragma once
#include "zedo_internal.h"

#include <climits>
#include <cstdint>
#include <type_traits>

namespace zedo {

constexpr int CHAIN_T = 256, CHAIN_W = CHAIN_T / 64;               // the workgroup of every kernel of this family: four waves

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < __builtin_huge_val(); }   // false for NaN and +-inf
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// X[n,h,j,.] in the camera frame: (double)x + (T ? (double)T : 0) of row g = h N + n
__device__ __forceinline__ void load_cam(const float *__restrict__ x, const float *__restrict__ T, size_t g, int J, int j, double out[3]) {
    const float *px = x + (g * J + j) * 3;
    const float *pt = T ? T + g * 3 : nullptr;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (double)px[c] + (pt ? (double)pt[c] : 0.0);
}

// Workgroup w of a grid of n_seq J serves clip s = w / J, joint j = w % J (the J chains of a clip are neighbours in the grid), frames
// a .. b-1.  An empty clip (a >= b) is workgroup-uniform: the kernel returns.
struct ClipJoint { int s, j, a, b; };
__device__ __forceinline__ ClipJoint clip_joint(const int *__restrict__ seq_start, int N, int J) {
    const int s = blockIdx.x / J;
    return {s, (int)blockIdx.x - s * J, clampi(seq_start[s], 0, N), clampi(seq_start[s + 1], 0, N)};
}

// ---- the lane split: CHAIN_T lanes as P parts x CHAIN_T / P slots ----
// The lane (part, slot) owns the outer index slot (+ SLOTS, .. : K of them) and walks ONE part of the inner index, q0 .. q1-1 of
// 0 .. H-1 (ceil(H / P) consecutive ones; part 0 is never empty, np parts are not).  The parts' results meet in the LDS and part 0
// combines them in ascending part order.  H -> P: 4 (H <= 64), 2 (H <= 128), else 1, and then K = 1 (H <= 256), 2 (H <= 512) or 4 (H <=
// 1024): no lane walks for an index nobody owns beyond the last, partly filled group.  chain_parts and dispatch_pk are the only places
// that know these numbers.
__host__ __device__ constexpr int chain_parts(int H) { return H <= CHAIN_T / 4 ? 4 : (H <= CHAIN_T / 2 ? 2 : 1); }

struct Lanes {
    int slots, part, slot, q0, q1, np;
    __device__ __forceinline__ Lanes(int tid, int H, int P) : slots(CHAIN_T / P), part(tid / slots), slot(tid - part * slots) {
        const int per = (H + P - 1) / P;
        q0 = min(H, part * per);
        q1 = min(H, q0 + per);
        np = (H + per - 1) / per;
    }
};
// P fixed by the instantiation; a kernel whose H is only known at run time (the tree kernels) uses Lanes(tid, H, chain_parts(H))
template <int P, int K>
struct ChainLanes : Lanes {
    static_assert(P == 1 || K == 1, "a lane owns several hypotheses only where the inner index is not split");
    static constexpr int SLOTS = CHAIN_T / P, CAP = K * SLOTS;     // CAP: the hypotheses the instantiation holds in the LDS
    __device__ __forceinline__ ChainLanes(int tid, int H) : Lanes(tid, H, P) {}
};

// f(integral_constant<int, P>, integral_constant<int, K>) of the instantiation that serves H <= 4 CHAIN_T
template <int V>
using IntC = std::integral_constant<int, V>;
template <class F>
inline void dispatch_pk(int H, F &&f) {
    const int P = chain_parts(H);
    if (P == 4) f(IntC<4>(), IntC<1>());
    else if (P == 2) f(IntC<2>(), IntC<1>());
    else if (H <= CHAIN_T) f(IntC<1>(), IntC<1>());
    else if (H <= 2 * CHAIN_T) f(IntC<1>(), IntC<2>());
    else f(IntC<1>(), IntC<4>());
}

// ---- reductions ----
// The best v (MAX: the largest, otherwise the smallest) and the lowest h that holds it; h = INT_MAX: no entry.  Every lane gets both.
template <bool MAX>
__device__ __forceinline__ bool arg_better(double ov, int oh, double v, int h) {
    return (MAX ? ov > v : ov < v) || (ov == v && oh < h);
}
template <bool MAX>
__device__ __forceinline__ void wave_arg(double &v, int &h) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oh = __shfl_xor(h, off);
        if (arg_better<MAX>(ov, oh, v, h)) { v = ov; h = oh; }
    }
}
// over the workgroup's nw waves, in ascending wave order; sred, sredi: nw entries of the LDS.  One barrier; the caller puts another
// between this and its next write to sred / sredi (the barriers of the next frame do where a kernel reduces once per frame).
template <bool MAX>
__device__ __forceinline__ void block_arg(double &v, int &h, double *sred, int *sredi, int tid, int nw = CHAIN_W) {
    wave_arg<MAX>(v, h);
    if ((tid & 63) == 0) { sred[tid >> 6] = v; sredi[tid >> 6] = h; }
    __syncthreads();
    v = sred[0];
    h = sredi[0];
    for (int w = 1; w < nw; ++w)
        if (arg_better<MAX>(sred[w], sredi[w], v, h)) { v = sred[w]; h = sredi[w]; }
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
// the sum of v over the wave, a butterfly: every lane gets it
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// sums of NV values over the CHAIN_W waves of the workgroup: a butterfly inside each wave, then the waves ascending; every lane gets
// the sums.  sred: CHAIN_W NV doubles of the LDS, free again on return.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *sred, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) sred[(tid >> 6) * NV + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = sred[i];
        for (int w = 1; w < CHAIN_W; ++w) s += sred[w * NV + i];
        v[i] = s;
    }
    __syncthreads();
}

// ---- the first-order chain's frame step (joint_temporal_scan_kernel on a whole clip, joint_stream_scan_kernel on a chunk of it) ----
// Everything that decides a bit of D or back, as statements in the kernel's own scope: the streaming call promises the offline call's
// bits, and the same walk as a __forceinline__ function template changes the register assignment of the offline kernel from its first
// block on.  A kernel keeps what is its own: where a frame's rows live, where "chain start" comes from, what a chain's end leaves behind.
// In scope: P, K, SLOTS and ln of ChainLanes<P, K>; tid, H, N, J, j, junary, x, Tr, lambda, inf; xn [K][3], un [K] - the frame that is
// being fetched - and xc [K][3], uc [K] - the frame in hand; dn [K], bn [K]; chain (n continues a chain) and is_dead, workgroup-uniform;
// sX [CAP][3], sD [CAP] - frame n-1 - and sPv, sPi [CHAIN_T] of the LDS.
#ifdef ZEDO_MUT_JT_NO_T   // tools/mutation_check.py only: the motion term is taken on x alone although T was given
#define ZEDO_CHAIN_STEP_T(G) nullptr
#else
#define ZEDO_CHAIN_STEP_T(G) (Tr ? Tr + (G) * 3 : nullptr)
#endif
// X[FRAME,h,j,.] and u[FRAME,j,h] of this lane's h into xn, un.  load_cam's statements in place, not a call of it: through the function
// the compiler joins the three loads of x into one and converts it before the branch on T, i.e. waits for the prefetch ahead of barrier
// A - an offline call without T on one clip of 1 015 frames (J = 17, H = 50) measured 2 875 us against 2 778 us.
#define ZEDO_CHAIN_STEP_FETCH(FRAME)                                                                                                   \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                                \
            const size_t g = (size_t)min(ln.slot + k * SLOTS, H - 1) * N + (FRAME);                                                    \
            const float *px = x + (g * J + j) * 3;                                                                                     \
            const float *pt = ZEDO_CHAIN_STEP_T(g);                                                                                    \
            _Pragma("unroll") for (int c = 0; c < 3; ++c) xn[k][c] = (double)px[c] + (pt ? (double)pt[c] : 0.0);                       \
            un[k] = junary[g * J + j];                                                                                                 \
        }
// between barriers A and B: min_h' (D[n-1,h'] + lambda |X[n,h] - X[n-1,h']|) over the lane's part q0 .. q1-1 into dn, the lowest h' that
// attains it into bn; with P > 1 both go to the LDS
#define ZEDO_CHAIN_STEP_WALK                                                                                                           \
        if (chain) {                                                                                                                   \
            _Pragma("unroll") for (int k = 0; k < K; ++k) { dn[k] = inf; bn[k] = 0; }                                                  \
            _Pragma("unroll 4") for (int hp = ln.q0; hp < ln.q1; ++hp) {                                                               \
                const double p0 = sX[hp * 3], p1 = sX[hp * 3 + 1], p2 = sX[hp * 3 + 2], pd = sD[hp];                                   \
                _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                        \
                    const double d0 = xc[k][0] - p0, d1 = xc[k][1] - p1, d2 = xc[k][2] - p2;                                           \
                    const double c = pd + lambda * sqrt(d0 * d0 + d1 * d1 + d2 * d2);                                                  \
                    if (hp == ln.q0 || c < dn[k]) { dn[k] = c; bn[k] = hp; }   /* strict: the lowest h' that attains the minimum */    \
                }                                                                                                                      \
            }                                                                                                                          \
            if (P > 1) { sPv[tid] = dn[0]; sPi[tid] = bn[0]; }                                                                         \
        }
// after barrier B, by part 0: the parts' minima in ascending part order, strict - the tie still goes to the lowest h'
#define ZEDO_CHAIN_STEP_COMBINE                                                                                                        \
            if (chain && P > 1) {                                                                                                      \
                for (int p = 1; p < ln.np; ++p) {                                                                                      \
                    const double c = sPv[p * SLOTS + ln.slot];                                                                         \
                    if (c < dn[0]) { dn[0] = c; bn[0] = sPi[p * SLOTS + ln.slot]; }                                                    \
                }                                                                                                                      \
            }
// d = D[n,j,h] of the owner of h = slot + K_ SLOTS: u + the minimum inside a chain, u at a chain's start, +inf where the unary is not
// finite or (n, j) is dead.  Declares u0 and d.  (A function of the same text changes joint_stream_scan_kernel's code.)
#define ZEDO_CHAIN_STEP_VALUE(K_)                                                                                                      \
                    const double u0 = finite64(uc[K_]) ? uc[K_] : inf;                                                                 \
                    const double d = chain ? u0 + dn[K_] : (is_dead ? inf : u0);

// ---- the live streams of the first-order chain (zedo_joint_stream.hip, zedo_joint_stream_marginal.hip) ----
// The frame count as the kernels take it: a state that was never reset may hold anything, and a row t % R is an address
__device__ __forceinline__ long long clip_frames(long long t) { return t < 0 ? 0 : (t > (1ll << 62) ? (1ll << 62) : t); }
// What a push emits for stream s, from the clip's frame count before it: frames e0 .. e0 + cnt - 1; t1: the clip's frames after it
struct StreamEmit { long long t1, e0, cnt; };
__device__ __forceinline__ StreamEmit stream_emit(long long t0, int F, int lag, bool flush) {
    t0 = clip_frames(t0);
    const long long t1 = t0 + F, e0 = t0 > lag ? t0 - lag : 0, e1 = flush ? t1 : (t1 > lag ? t1 - lag : 0);
    return {t1, e0, e1 - e0};
}
// The kernels of zedo_joint_stream.hip that do not know what a stream's tables hold - the frame count [S], the dead flags [SJ,R] - and
// serve both streaming calls: reset (t = 0 where which is null or set), the dead flags of a chunk into the ring, and the advance
// (d_emit and the frame count, 0 after a flush).
__global__ __launch_bounds__(256) void joint_stream_reset_kernel(const int *__restrict__ which, int S, long long *__restrict__ t);
__global__ __launch_bounds__(256) void joint_stream_dead_kernel(const double *__restrict__ junary, const long long *__restrict__ t, int S, int F, int H, int J,
                                         int R, int *__restrict__ dead);
__global__ __launch_bounds__(256) void joint_stream_advance_kernel(const int *__restrict__ flush, int S, int F, int lag, long long *__restrict__ t,
                                            long long *__restrict__ emit);
// and the decision of the first-order chains, whatever a chain is made of - J chains per stream, tables D [SJ,R,H], back [SJ,R,H], dead
// [SJ,R]: one wave per (stream, output row, joint).  The pose-level stream (zedo_temporal_stream.hip) takes it with J = 1.
__global__ __launch_bounds__(CHAIN_T) void joint_stream_emit_kernel(const long long *__restrict__ tcount, const int *__restrict__ flush, int S, int F,
                                                  int H, int J, int R, int lag, const double *__restrict__ D, const int *__restrict__ back,
                                                  const int *__restrict__ dead, int *__restrict__ path, double *__restrict__ cost);

// ---- the first-order chain's sum-product step (zedo_joint_marginal.hip on a whole clip, zedo_joint_stream_marginal.hip on a chunk of
// it and on the lag window): a Viterbi step with (min, +) replaced by (log-sum-exp, +) ----
// One lane's share of LSE_h' (sV[h'] - c |xc[k] - sX[h']|) over h' = q0 .. q1-1, for each of its K hypotheses: mx = the largest term
// (-inf if the share has none above -inf), sm = sum exp(term - mx) ascending in h' (shifted by 0 where mx is -inf: every exp is 0).
template <int K>
__device__ __forceinline__ void jm_walk(const double *sX, const double *sV, int q0, int q1, const double (&xc)[K][3], double c,
                                        double (&mx)[K], double (&sm)[K]) {
    const double ninf = -__builtin_huge_val();
#pragma unroll
    for (int k = 0; k < K; ++k) mx[k] = ninf;
#pragma unroll 4
    for (int hp = q0; hp < q1; ++hp) {
        const double p0 = sX[hp * 3], p1 = sX[hp * 3 + 1], p2 = sX[hp * 3 + 2], pv = sV[hp];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double d0 = xc[k][0] - p0, d1 = xc[k][1] - p1, d2 = xc[k][2] - p2;
            const double t = pv - c * sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            if (t > mx[k]) mx[k] = t;
        }
    }
    double sh[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { sh[k] = mx[k] > ninf ? mx[k] : 0.0; sm[k] = 0.0; }
#pragma unroll 2
    for (int hp = q0; hp < q1; ++hp) {
        const double p0 = sX[hp * 3], p1 = sX[hp * 3 + 1], p2 = sX[hp * 3 + 2], pv = sV[hp];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double d0 = xc[k][0] - p0, d1 = xc[k][1] - p1, d2 = xc[k][2] - p2;
            const double t = pv - c * sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            sm[k] += exp(t - sh[k]);
        }
    }
}

// Part 0's end of a log-sum-exp: (mx, sm) of its own share and, with P > 1, those of the other parts from the LDS, in ascending part order.
template <int P>
__device__ __forceinline__ double jm_combine(double mx, double sm, const double *sPm, const double *sPs, int slots, int slot, int np) {
    const double ninf = -__builtin_huge_val();
    if (P > 1) {
        double M = mx;
        for (int p = 1; p < np; ++p) {
            const double v = sPm[p * slots + slot];
            if (v > M) M = v;
        }
        double S = mx == M ? sm : (mx > ninf ? sm * exp(mx - M) : 0.0);
        for (int p = 1; p < np; ++p) {
            const double v = sPm[p * slots + slot], q = sPs[p * slots + slot];
            S += v == M ? q : (v > ninf ? q * exp(v - M) : 0.0);
        }
        mx = M;
        sm = S;
    }
    return mx + log(sm);
}
// l = l[n,j,h] and v = A[n,j,h] of the owner of h = slot + K_ SLOTS, after barrier B: l = -u / tau (-inf where the unary is not finite);
// v = l + the log-sum-exp inside a chain, l at a chain's start, -inf where (n, j) is dead.  Declares l and v.  In scope: P, SLOTS, slot
// and ln of ChainLanes<P, K>; uc [K], mx [K], sm [K]; tau, ninf; chain and is_dead, workgroup-uniform; sPm, sPs [CHAIN_T] of the LDS.
#define ZEDO_CHAIN_FORWARD_VALUE(K_)                                                                                                   \
                    const double l = finite64(uc[K_]) ? -uc[K_] / tau : ninf;                                                          \
                    const double v = is_dead ? ninf : (chain ? l + jm_combine<P>(mx[K_], sm[K_], sPm, sPs, SLOTS, slot, ln.np) : l);

// ---- what a fusion kernel along a video reads off the marginals of one (frame, joint) (zedo_joint_marginal.hip, zedo_joint_accel_marginal.hip) ----
// The tail of a backward kernel's frame, as statements in the kernel's own scope: a function of the same text changes the register
// allocation of joint_marginal_backward_kernel, and that kernel's instruction stream is pinned.  A lane holds K hypotheses h = H0 + k HSTEP
// with their X in XC [K][3]; OWN (an expression in h) says whether the lane owns h, WEIGHT (an expression in k) is its marginal.  Written:
// d_w (wout, if not null), the lowest h with the largest marginal, the mean sum_h w X and the covariance sum_h w (X - mean)(X - mean)^T
// from the centred differences - block_arg and block_sum: a fixed order - and log Z of the chain.  Reached by the whole workgroup.  In
// scope: H, tid, lz, mean, cov, hmax, wmax, logz, wout, ninf and sred (6 CHAIN_W doubles), sredi (CHAIN_W ints) of the LDS, free on entry
// and again afterwards.  Declares wk, m3, bw, bh, c6.
#define ZEDO_CHAIN_MOMENTS(K, H0, HSTEP, OWN, WEIGHT, XC, NJ)                                                                          \
        double wk[K], m3[3] = {0.0, 0.0, 0.0}, bw = ninf;                                                                              \
        int bh = INT_MAX;                                                                                                              \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                                \
            const int h = (H0) + k * (HSTEP);                                                                                          \
            const bool own = OWN;                                                                                                      \
            wk[k] = own ? (WEIGHT) : 0.0;                                                                                              \
            if (own) {                                                                                                                 \
                if (wout) wout[(NJ) * H + h] = wk[k];                                                                                  \
                if (wk[k] > bw) { bw = wk[k]; bh = h; }            /* ascending h, strict: the lowest h of the lane */                 \
                _Pragma("unroll") for (int cc = 0; cc < 3; ++cc) m3[cc] += wk[k] * XC[k][cc];                                          \
            }                                                                                                                          \
        }                                                                                                                              \
        block_arg<true>(bw, bh, sred, sredi, tid);                                                                                     \
        __syncthreads();                                                                                                               \
        block_sum<3>(m3, sred, tid);                                                                                                   \
        double c6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                                                                                 \
        _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                                \
            const double d0 = XC[k][0] - m3[0], d1 = XC[k][1] - m3[1], d2 = XC[k][2] - m3[2];                                          \
            c6[0] += wk[k] * (d0 * d0); c6[1] += wk[k] * (d0 * d1); c6[2] += wk[k] * (d0 * d2);                                        \
            c6[3] += wk[k] * (d1 * d1); c6[4] += wk[k] * (d1 * d2); c6[5] += wk[k] * (d2 * d2);                                        \
        }                                                                                                                              \
        block_sum<6>(c6, sred, tid);                                                                                                   \
        if (tid < 3) mean[(NJ) * 3 + tid] = m3[tid];                                                                                   \
        if (tid < 6) cov[(NJ) * 6 + tid] = c6[tid];                                                                                    \
        if (tid == 0) { hmax[NJ] = bh == INT_MAX ? 0 : bh; wmax[NJ] = bh == INT_MAX ? 0.0 : bw; logz[NJ] = lz; }
// a dead (frame, joint): NaN, hypothesis 0, weight 0, log Z = -inf, a row of zeros; OWNER: does the lane own its h = H0 + k HSTEP below H.
// In scope as above, and qnan.
#define ZEDO_CHAIN_DEAD_OUTPUTS(K, H0, HSTEP, OWNER, NJ)                                                                               \
            if (tid < 3) mean[(NJ) * 3 + tid] = qnan;                                                                                  \
            if (tid < 6) cov[(NJ) * 6 + tid] = qnan;                                                                                   \
            if (tid == 0) { hmax[NJ] = 0; wmax[NJ] = 0.0; logz[NJ] = ninf; }                                                           \
            if (wout && (OWNER))                                                                                                       \
                _Pragma("unroll") for (int k = 0; k < K; ++k)                                                                          \
                    if ((H0) + k * (HSTEP) < H) wout[(NJ) * H + (H0) + k * (HSTEP)] = 0.0;

// ---- the pairs of the second-order chain models (zedo_joint_accel.hip, zedo_joint_accel_marginal.hip) ----
// The H^2 pairs q = h' H + h of a (frame, joint) are dealt to the CHAIN_T lanes round robin, KA to a lane: f(integral_constant<int, KA>)
// of the smallest of the seven instantiations - KA = 1 (H <= 16), 2 (H <= 22), 4 (H <= 32), 7 (H <= 42), 10 (H <= 50), 13 (H <= 57) or 16
// (H <= 64) - with CHAIN_T KA >= H^2.
template <class F>
inline void dispatch_pairs(int H, F &&f) {
    const int HH = H * H;
    if (HH <= CHAIN_T) f(IntC<1>());
    else if (HH <= 2 * CHAIN_T) f(IntC<2>());
    else if (HH <= 4 * CHAIN_T) f(IntC<4>());
    else if (HH <= 7 * CHAIN_T) f(IntC<7>());
    else if (HH <= 10 * CHAIN_T) f(IntC<10>());
    else if (HH <= 13 * CHAIN_T) f(IntC<13>());
    else f(IntC<16>());
}
// qh1 [KA], qh0 [KA]: h' and h of the KA pairs q = tid, tid + 256, .. of a lane (a pair past H^2 is computed as pair H^2 - 1 and stored
// nowhere).  One text in the two forms the pinned kernels need: joint_accel_scan_kernel's code changes when this is a function, that of
// the fusion kernels when it is not.  The statements take tid, H and HH = H^2 from the scope they stand in.
#define ZEDO_CHAIN_LANE_PAIRS(KA)                                                                                                      \
    _Pragma("unroll") for (int k = 0; k < KA; ++k) {                                                                                   \
        const int q = min(tid + k * CHAIN_T, HH - 1);                                                                                  \
        qh1[k] = q / H;                                                                                                                \
        qh0[k] = q - qh1[k] * H;                                                                                                       \
    }
template <int KA>
__device__ __forceinline__ void lane_pairs(int tid, int H, int (&qh1)[KA], int (&qh0)[KA]) {
    const int HH = H * H;
    ZEDO_CHAIN_LANE_PAIRS(KA)
}
// The leading part a - 2 p of the second difference a - 2 p + b; the caller adds b, and chooses which of the three frames a, p and b are
__device__ __forceinline__ double accel_lead(double a, double p) {
#ifdef ZEDO_MUT_JA_FIRST_DIFF   // tools/mutation_check.py only: the factor 2 is dropped, a - p + b
    return a - p;
#else
    return a - 2.0 * p;
#endif
}
// What a forward kernel keeps of frames n and n-1 for the lane's pairs, between its barriers A and B: g [KA][3], g_c = X[n,h,c] -
// 2 X[n-1,h',c], and lm [KA] = W |X[n,h] - X[n-1,h']| (the squares, then their sum ascending in c).  INIT: the kernel's own statements
// for pair k, if any.  In scope: qh1, qh0, X0 = X[n], X1 = X[n-1] of the LDS.
#define ZEDO_CHAIN_PAIR_TERMS(KA, W, INIT)                                                                                             \
            double g[KA][3], lm[KA];                                                                                                   \
            _Pragma("unroll") for (int k = 0; k < KA; ++k) {                                                                           \
                const int h1 = qh1[k], h0 = qh0[k];                                                                                    \
                double d[3];                                                                                                           \
                _Pragma("unroll") for (int c = 0; c < 3; ++c) {                                                                        \
                    const double p = X1[h1 * 3 + c];                                                                                   \
                    d[c] = X0[h0 * 3 + c] - p;                                                                                         \
                    g[k][c] = accel_lead(X0[h0 * 3 + c], p);                                                                           \
                }                                                                                                                      \
                lm[k] = (W) * sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);                                                           \
                INIT                                                                                                                   \
            }
// ---- the second-order chain's frame step (joint_accel_scan_kernel on a whole clip, joint_accel_stream_scan_kernel on a chunk of it) ----
// Everything that decides a bit of E or back2, between a kernel's barriers A and B, as statements in the kernel's own scope - the
// streaming call promises the offline call's bits: the second-frame rule, the H^3 walk with its strict comparison, the final additions.
// Leaves E[n] of the lane's pairs in en [KA] and the lowest h'' in bn [KA] (not at a second frame).  A kernel keeps what is its own:
// where back2 lives, where "start" and "second" come from, what a frame's arg-min is for.  In scope: H, inf, lambda_v, lambda_a; qh1,
// qh0 [KA]; scan (n continues a chain) and second, workgroup-uniform; of the LDS: sE = E[n-1] h''-major, X0, X1, X2 = X of frames n, n-1,
// n-2, U0, U1 = u of frames n, n-1.
#define ZEDO_CHAIN_PAIR_STEP(KA)                                                                                                       \
        if (scan) {                                                                                                                    \
            ZEDO_CHAIN_PAIR_TERMS(KA, lambda_v, en[k] = inf; bn[k] = 0;)      /* g_c = X[n,h,c] - 2 X[n-1,h',c];  lm = lambda_v m */    \
            if (second) {                                                                                                              \
                _Pragma("unroll") for (int k = 0; k < KA; ++k) en[k] = U1[qh1[k]] + (U0[qh0[k]] + lm[k]);                              \
            } else {                                                                                                                   \
                for (int h2 = 0; h2 < H; ++h2) {                                                                                       \
                    const double p0 = X2[h2 * 3], p1 = X2[h2 * 3 + 1], p2 = X2[h2 * 3 + 2];   /* broadcast */                          \
                    const double *row = sE + h2 * H;                                                                                   \
                    _Pragma("unroll") for (int k = 0; k < KA; ++k) {                                                                   \
                        const double e0 = g[k][0] + p0, e1 = g[k][1] + p1, e2 = g[k][2] + p2;                                          \
                        const double c = row[qh1[k]] + lambda_a * sqrt(e0 * e0 + e1 * e1 + e2 * e2);                                   \
                        if (h2 == 0 || c < en[k]) { en[k] = c; bn[k] = h2; }  /* strict: the lowest h'' that attains the minimum */    \
                    }                                                                                                                  \
                }                                                                                                                      \
                _Pragma("unroll") for (int k = 0; k < KA; ++k) en[k] = U0[qh0[k]] + (lm[k] + en[k]);                                   \
            }                                                                                                                          \
        }
// The horizon of frame n on a live stream, by one wave: the last frame of n's chain among n .. hi - the first m whose successor's flag in
// the ring dr [R] is set, or hi.  64 flags per step, by ballot; wave-uniform.
__device__ __forceinline__ long long stream_horizon(const int *__restrict__ dr, long long n, long long hi, int R, int lane) {
    for (long long m0 = n + 1; m0 <= hi; m0 += 64) {
        const long long m = m0 + lane;
        const int d = m <= hi ? dr[(int)(m % R)] : 0;
        const unsigned long long mask = __ballot(d != 0);
        if (mask) return m0 + (__ffsll((long long)mask) - 1) - 1;
    }
    return hi;
}

// ---- the second-order chain's sum-product step (zedo_joint_accel_marginal.hip on a whole clip, zedo_joint_accel_stream_marginal.hip on a
// chunk of it and on the lag window): the step above with (min, +) replaced by (log-sum-exp, +) ----
constexpr int JAM_CAP = 64;                                        // the pair tables of a (frame, joint) stay in the LDS

// lse[k] = LSE_i (tab[i H + col[k]] - c_a |g[k] + Xb[i]|), i = 0 .. H-1, for the KA pairs of a lane: all lanes walk i in lockstep, Xb[i]
// is a broadcast read and tab[i H + col] of neighbouring lanes is the same or the next double.  First walk: the largest term; second:
// the sum of exp(term - largest), ascending in i (shifted by 0 where no term is above -inf: every exp is 0 and the result -inf).
// |e| = sqrt(e0^2 + e1^2 + e2^2): the squares, then their sum ascending in c.
template <int KA>
__device__ __forceinline__ void jam_walk(const double *tab, const double *Xb, int H, const int (&col)[KA], const double (&g)[KA][3],
                                         double c_a, double (&lse)[KA]) {
    const double ninf = -__builtin_huge_val();
    double sh[KA], sm[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) sh[k] = ninf;
    for (int i = 0; i < H; ++i) {
        const double p0 = Xb[i * 3], p1 = Xb[i * 3 + 1], p2 = Xb[i * 3 + 2];
        const double *row = tab + i * H;
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const double e0 = g[k][0] + p0, e1 = g[k][1] + p1, e2 = g[k][2] + p2;
            const double t = row[col[k]] - c_a * sqrt(e0 * e0 + e1 * e1 + e2 * e2);
            if (t > sh[k]) sh[k] = t;
        }
    }
#pragma unroll
    for (int k = 0; k < KA; ++k) { sh[k] = sh[k] > ninf ? sh[k] : 0.0; sm[k] = 0.0; }
    for (int i = 0; i < H; ++i) {
        const double p0 = Xb[i * 3], p1 = Xb[i * 3 + 1], p2 = Xb[i * 3 + 2];
        const double *row = tab + i * H;
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const double e0 = g[k][0] + p0, e1 = g[k][1] + p1, e2 = g[k][2] + p2;
            const double t = row[col[k]] - c_a * sqrt(e0 * e0 + e1 * e1 + e2 * e2);
            sm[k] += exp(t - sh[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < KA; ++k) lse[k] = sh[k] + log(sm[k]);
}

// LSE over the workgroup of the KA terms of every lane (-inf: no term), shifted by their largest: the lane's terms ascending in k, then
// block_sum's fixed order.  At least one term is above -inf.  sred: CHAIN_W doubles of the LDS, free on entry and on return.
template <int KA>
__device__ __forceinline__ double jam_block_lse(const double (&t)[KA], double *sred, int tid) {
    double v = t[0];
#pragma unroll
    for (int k = 1; k < KA; ++k) v = fmax(v, t[k]);
    v = wave_max(v);
    if ((tid & 63) == 0) sred[tid >> 6] = v;
    __syncthreads();
    v = sred[0];
    for (int w = 1; w < CHAIN_W; ++w) v = fmax(v, sred[w]);
    __syncthreads();                                               // sred is block_sum's next
    double e[1] = {0.0};
#pragma unroll
    for (int k = 0; k < KA; ++k) e[0] += exp(t[k] - v);             // exp(-inf) = 0 where there is no term
    block_sum<1>(e, sred, tid);
    return v + log(e[0]);
}

// The forward value of a frame, between a kernel's barriers A and B, as statements in the kernel's own scope: A2[n] of the lane's pairs
// into an [KA].  In scope: H, c_v, c_a; qh1, qh0 [KA]; scan (n continues a chain) and second, workgroup-uniform; of the LDS: sA = A2[n-1]
// h''-major, X0, X1, X2 = X of frames n, n-1, n-2, L0, L1 = l of frames n, n-1.
//   second (n-1 is a start):  A2[n][h',h] = l[n-1,h'] + (l[n,h] - c_v m[n,h',h])
//   otherwise:  A2[n][h',h] = l[n,h] + (-c_v m[n,h',h] + LSE_h'' (A2[n-1][h'',h'] - c_a a[n,h'',h',h]))
#define ZEDO_CHAIN_PAIR_FORWARD(KA)                                                                                                    \
        if (scan) {                                                                                                                    \
            ZEDO_CHAIN_PAIR_TERMS(KA, c_v, )                       /* g_c = X[n,h,c] - 2 X[n-1,h',c];  lm = c_v m[n,h',h] */           \
            if (second) {                                                                                                              \
                _Pragma("unroll") for (int k = 0; k < KA; ++k) an[k] = L1[qh1[k]] + (L0[qh0[k]] - lm[k]);                              \
            } else {                                                                                                                   \
                jam_walk<KA>(sA, X2, H, qh1, g, c_a, an);                                                                              \
                _Pragma("unroll") for (int k = 0; k < KA; ++k) an[k] = L0[qh0[k]] + (an[k] - lm[k]);                                   \
            }                                                                                                                          \
        }

// The backward body of a frame n, from barrier A to the outputs, as statements in the kernel's own scope: B2[n] into sB, the pair
// marginals into sP, and everything that is read off them (ZEDO_CHAIN_MOMENTS) into the output row NJ of frame n - if EMIT - and, where
// n is the second frame of its chain, into the row NJ - J of the chain's first frame, from the row sums of the same table.
//   chain of one frame:  log Z = LSE_h l[n,h],  w[n,h] = exp(l[n,h] - log Z)
//   chain end (n has pairs and `ends`):  B2[n] = 0,  log Z = LSE over all pairs of A2[n]
//   otherwise, once per frame:  M[h+][h] = (l[n+1,h+] - c_v m[n+1,h,h+]) + B2[n+1][h,h+], stored h+-major: the walk's lanes of consecutive h
//              read consecutive doubles; then  B2[n][h',h] = LSE_h+ (M[h+][h] - c_a a[n+1,h',h,h+]) - one square root per transition.  A lane
//              keeps X[n-1,h'] - 2 X[n,h] and adds X[n+1,h+]: the second difference in ANOTHER association than the forward pass
//   pi[n][h',h] = exp((A2[n][h',h] + B2[n][h',h]) - log Z) into the LDS;  w[n,h] = sum_h' pi[n][h',h], ascending, by lane h; the first
//              frame c0 of a chain has no table: w[c0,h'] = sum_h pi[c0+1][h',h], ascending, formed at frame c0+1
// In scope: H, HH, J, tid, hx, c_v, c_a_back, ninf, qnan; qh1, qh0, ac [KA] = A2[n] of the lane's pairs; is_dead, start, second, ends and
// pairs = !is_dead && !start, workgroup-uniform; lz, carried from frame to frame; the outputs; of the LDS: sB = B2[n+1] at h H + h+, sM,
// sP, Xp, X0, X1 = X of frames n+1, n, n-1, Lp, L0 = l of frames n+1, n, sred (6 CHAIN_W doubles) and sredi (CHAIN_W ints).
#define ZEDO_CHAIN_PAIR_BACKWARD(KA, NJ, EMIT)                                                                                         \
        double bn[KA];                                             /* B2[n] of this lane's pairs */                                    \
        _Pragma("unroll") for (int k = 0; k < KA; ++k) bn[k] = 0.0;                                                                    \
        __syncthreads();                                           /* A: B2[n+1], X and l of frames n+1, n, n-1 are in the LDS */      \
        if (pairs && !ends) {                                                                                                          \
            _Pragma("unroll") for (int k = 0; k < KA; ++k) {       /* the pair (h, h+) of frame n+1 at this lane's q */                \
                const int q = tid + k * CHAIN_T, h = qh1[k], hp = qh0[k];                                                              \
                if (q < HH) {                                                                                                          \
                    const double d0 = Xp[hp * 3] - X0[h * 3], d1 = Xp[hp * 3 + 1] - X0[h * 3 + 1], d2 = Xp[hp * 3 + 2] - X0[h * 3 + 2]; \
                    sM[hp * H + h] = (Lp[hp] - c_v * sqrt(d0 * d0 + d1 * d1 + d2 * d2)) + sB[q];                                       \
                }                                                                                                                      \
            }                                                                                                                          \
            __syncthreads();                                       /* M is in the LDS; B2[n+1] has been read by every lane */          \
            double g[KA][3];                                       /* g_c = X[n-1,h',c] - 2 X[n,h,c] */                                \
            _Pragma("unroll") for (int k = 0; k < KA; ++k)                                                                             \
                _Pragma("unroll") for (int c = 0; c < 3; ++c) g[k][c] = accel_lead(X1[qh1[k] * 3 + c], X0[qh0[k] * 3 + c]);            \
            jam_walk<KA>(sM, Xp, H, qh0, g, c_a_back, bn);                                                                             \
        }                                                                                                                              \
        if (!is_dead && ends) {                                    /* (workgroup-uniform) log Z of the chain that ends here */         \
            double t[KA];                                                                                                              \
            _Pragma("unroll") for (int k = 0; k < KA; ++k)                                                                             \
                t[k] = start ? (k == 0 && tid < H ? L0[tid] : ninf) : (tid + k * CHAIN_T < HH ? ac[k] : ninf);                         \
            lz = jam_block_lse<KA>(t, sred, tid);                                                                                      \
        }                                                                                                                              \
        if (pairs) {                                                                                                                   \
            _Pragma("unroll") for (int k = 0; k < KA; ++k) {                                                                           \
                const int q = tid + k * CHAIN_T;                                                                                       \
                if (q < HH) {                                                                                                          \
                    sB[q] = bn[k];                                 /* B2[n][h',h] at h' H + h: frame n-1 reads it as B2[n+1][h,h+] */  \
                    sP[q] = exp((ac[k] + bn[k]) - lz);                                                                                 \
                }                                                                                                                      \
            }                                                                                                                          \
        }                                                                                                                              \
        __syncthreads();                                           /* C: the pair marginals of frame n are in the LDS */               \
        if (is_dead) {                                                                                                                 \
            ZEDO_CHAIN_DEAD_OUTPUTS(1, tid, 0, true, NJ)                                                                               \
        } else if (pairs || ends) {                                /* (a start with a successor is served by that successor, below) */ \
            const int passes = pairs && second ? 2 : 1;            /* pass 1: frame n-1, the first of its chain, from the same table */ \
            for (int p = (EMIT) ? 0 : 1; p < passes; ++p) {                                                                            \
                const double *Xm = p ? X1 : X0;                                                                                        \
                const double xm[1][3] = {{Xm[hx * 3], Xm[hx * 3 + 1], Xm[hx * 3 + 2]}};                                                \
                double wv = 0.0;                                                                                                       \
                if (tid < H) {                                                                                                         \
                    if (!pairs) wv = exp(L0[tid] - lz);                                                                                \
                    else if (p == 0)                                                                                                   \
                        for (int h1 = 0; h1 < H; ++h1) wv += sP[h1 * H + tid];                                                         \
                    else                                                                                                               \
                        for (int h0 = 0; h0 < H; ++h0) wv += sP[tid * H + h0];                                                         \
                }                                                                                                                      \
                const size_t mj = (NJ) - (size_t)p * J;                                                                                \
                ZEDO_CHAIN_MOMENTS(1, tid, 0, h < H, wv, xm, mj)                                                                       \
            }                                                                                                                          \
        }

// ---- the bone tree: one workgroup per pose, everything in the LDS ----
// sqrt(d0^2 + d1^2 + d2^2), d = a - b: products, then the sum ascending in c
__device__ __forceinline__ double tr_dist(const double *a, double b0, double b1, double b2) {
    const double d0 = a[0] - b0, d1 = a[1] - b1, d2 = a[2] - b2;
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}
// the bone term of one pair, in metres: exactly 0 when both ends come from one hypothesis (mix and both own are then the same bits)
__device__ __forceinline__ double tr_bone(double mix, double own_c, double own_p) {
#ifdef ZEDO_MUT_TREE_NO_HALF   // tools/mutation_check.py only: the two hypotheses' lengths are summed, not averaged
    return fabs(mix - (own_c + own_p));
#else
    return fabs(mix - 0.5 * (own_c + own_p));
#endif
}
// Pose n's tables, staged once.  sX [J][H][3]: the camera-frame positions - H runs of 12 J bytes at a stride of N J 3 floats, consecutive
// lanes read consecutive floats of a row.  Joint-major, so the lanes of a wave read X[j][h] of consecutive h - fp64 triples at a stride of
// 6 dwords, which 32 lanes spread over the 64 banks without a conflict (ds_read_b64 is served in groups of 32 lanes, bank = dword address
// mod 64) - or all the same h: a broadcast.  sS [J][H]: score(w u) of the unary u weighted by the confidence w (the clamp of
// zedo_min_reproj, taken in fp32: NaN stays NaN), `excluded` where w u is not finite.  sLive [J]: does the joint have a hypothesis that
// is not excluded - a wave per joint, by ballot.  sZero (may be null): a table [J][H] zeroed in the same pass.  Ends WITHOUT a barrier:
// sLive is visible after the caller's next one.
template <class Score>
__device__ __forceinline__ void tree_stage(const double *__restrict__ junary, const float *__restrict__ x, const float *__restrict__ Tr,
                                           const float *__restrict__ weight, size_t n, int H, int N, int J, double excluded, Score score,
                                           double *sX, double *sS, int *sLive, double *sZero = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, JH = J * H, J3 = 3 * J;
    for (int e = tid; e < 3 * JH; e += CHAIN_T) {
        const int h = e / J3, r = e - h * J3, j = r / 3, c = r - 3 * j;
        const size_t row = (size_t)h * N + n;
        sX[(j * H + h) * 3 + c] = (double)x[row * J3 + r] + (Tr ? (double)Tr[row * 3 + c] : 0.0);
    }
    for (int e = tid; e < JH; e += CHAIN_T) {
        const int h = e / J, j = e - h * J;
        double w = 1.0;
        if (weight) {
            float c = weight[n * J + j];
            if (c > 1.0f) c = 1.0f;
            if (c < 1e-4f) c = 1e-4f;
            w = (double)c;
        }
        const double u = w * junary[((size_t)h * N + n) * J + j];
        sS[j * H + h] = finite64(u) ? score(u) : excluded;
        if (sZero) sZero[j * H + h] = 0.0;
    }
    __syncthreads();
    for (int j = wave; j < J; j += CHAIN_W) {
        int any = 0;
        for (int h = lane; h < H; h += 64) any |= sS[j * H + h] != excluded ? 1 : 0;
        const bool live = __ballot(any) != 0;
        if (lane == 0) sLive[j] = live ? 1 : 0;
    }
}

// ---- the workspace of an entry point, carved in ONE place: its size is where the carving ends ----
// take<T>(n): n elements of T at the next offset aligned for T.  With ws = nullptr only bytes() means anything.  A layout struct holds
// a Carve as its FIRST member and initialises its tables from it in the order they are declared.
class Carve {
    uintptr_t base_;
    size_t off_ = 0;

public:
    explicit Carve(void *ws) : base_(reinterpret_cast<uintptr_t>(ws)) {}
    template <class T>
    T *take(size_t n) {
        off_ = (off_ + alignof(T) - 1) & ~(alignof(T) - 1);
        T *const p = reinterpret_cast<T *>(base_ + off_);
        off_ += n * sizeof(T);
        return p;
    }
    size_t bytes(size_t align = 1) const { return (off_ + align - 1) & ~(align - 1); }
};

}  // namespace zedo
