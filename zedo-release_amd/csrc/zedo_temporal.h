// What the pose-level temporal selection on a whole clip (zedo_temporal.hip) and on live streams (zedo_temporal_stream.hip) share: the
// statements of a transition tile and of a frame of the resident scan, once.  They are statements in the kernel's own scope, not
// functions, for the reason zedo_chain.h gives for the joint chains' frame step: the streaming call promises the offline call's bits,
// and the offline kernels' instruction streams are pinned.  A kernel keeps what is its own: where a frame's poses, unaries and rows
// of D and back live, where "chain start" comes from, what a chain's end leaves behind.
#pragma once
#include "zedo_chain.h"

namespace zedo {

// ---- the transition tile: m[n,h',h] = (1/J) sum_j || x[h,n,j] - x[h',n-1,j] ||, sums ascending in c, then in j ----
// One workgroup per (frame n, tile of TT_H hypotheses h of frame n, tile of TT_P hypotheses h' of frame n-1): the tiles' poses arrive
// in the LDS TT_J joints at a time (coalesced along a pose's coordinates, any alignment, any J), each of the 256 lanes keeps the running
// sums of its TT_P / 4 pairs in registers across the joint pieces - the order of the additions is that of one loop over j.
// [hyp][TT_LD] with an odd TT_LD: the 64 lanes of a wave read 64 different h at an odd word stride (no bank conflict) and one h' (a
// broadcast).  Written as M[workgroup x][h'][h]: the scan's lanes (one per h) read a row of it coalesced, and a wave of the tile
// writes 512 contiguous bytes.
constexpr int TT_H = 64, TT_P = 16, TT_J = 32, TT_LD = TT_J * 3 + 1, TT_T = 256, TT_K = TT_P / (TT_T / TT_H);
static_assert(TT_T == 4 * TT_H && TT_K * 4 == TT_P && (TT_LD & 1), "four h' rows per pass over the 64 h lanes, odd LDS row stride");
#ifdef ZEDO_MUT_TT_PIECE   // tools/mutation_check.py only: every piece stages joints 0 .. of the pose again (valid addresses: ne <= 3 J)
#define ZEDO_TEMPORAL_TILE_PIECE(J0) 0
#else
#define ZEDO_TEMPORAL_TILE_PIECE(J0) (J0)
#endif
// In scope: H, J, M; sc [TT_H TT_LD], sp [TT_P TT_LD] of the LDS.  XC, XP: the float e of joint js .. of hypothesis h0 + r of frame
// n, and of hypothesis p0 + r of frame n-1 - expressions in r, js and e (and h0, p0).  ZEDO_TEMPORAL_TILE_LANES declares tid, h0, p0,
// nh, np, lh, lp - what a kernel's own addresses may need; ZEDO_TEMPORAL_TILE follows it and declares acc.
#define ZEDO_TEMPORAL_TILE_LANES                                                                                                       \
    const int tid = threadIdx.x, h0 = blockIdx.y * TT_H, p0 = blockIdx.z * TT_P;                                                       \
    const int nh = min(TT_H, H - h0), np = min(TT_P, H - p0);                                                                          \
    const int lh = tid & (TT_H - 1), lp = tid / TT_H;             /* this lane's h and the first of its h' (then every fourth) */
#define ZEDO_TEMPORAL_TILE(XC, XP)                                                                                                     \
    double acc[TT_K];                                                                                                                  \
    _Pragma("unroll") for (int k = 0; k < TT_K; ++k) acc[k] = 0.0;                                                                     \
    for (int j0 = 0; j0 < J; j0 += TT_J) {                                                                                             \
        const int ne = min(TT_J, J - j0) * 3;                      /* floats of this piece per pose */                                 \
        const int js = ZEDO_TEMPORAL_TILE_PIECE(j0);                                                                                   \
        __syncthreads();                                           /* the previous piece has been read by every lane */                \
        for (int q = tid; q < nh * ne; q += TT_T) {                                                                                    \
            const int r = q / ne, e = q - r * ne;                                                                                      \
            sc[r * TT_LD + e] = XC;                                                                                                    \
        }                                                                                                                              \
        for (int q = tid; q < np * ne; q += TT_T) {                                                                                    \
            const int r = q / ne, e = q - r * ne;                                                                                      \
            sp[r * TT_LD + e] = XP;                                                                                                    \
        }                                                                                                                              \
        __syncthreads();                                           /* the lanes read what other lanes have staged */                   \
        if (lh < nh) {                                                                                                                 \
            const float *a = sc + lh * TT_LD;                                                                                          \
            for (int e = 0; e < ne; e += 3) {                                                                                          \
                const double a0 = (double)a[e], a1 = (double)a[e + 1], a2 = (double)a[e + 2];                                          \
                _Pragma("unroll") for (int k = 0; k < TT_K; ++k) {                                                                     \
                    const float *b = sp + min(lp + 4 * k, np - 1) * TT_LD;          /* (a row past the tile is computed and not stored) */ \
                    const double d0 = a0 - (double)b[e], d1 = a1 - (double)b[e + 1], d2 = a2 - (double)b[e + 2];                       \
                    acc[k] += sqrt(d0 * d0 + d1 * d1 + d2 * d2);                                                                       \
                }                                                                                                                      \
            }                                                                                                                          \
        }                                                                                                                              \
    }                                                                                                                                  \
    if (lh < nh) {                                                                                                                     \
        _Pragma("unroll") for (int k = 0; k < TT_K; ++k) {                                                                             \
            const int p = lp + 4 * k;                                                                                                  \
            if (p < np) M[((size_t)blockIdx.x * H + (p0 + p)) * H + (h0 + lh)] = acc[k] / (double)J;                                   \
        }                                                                                                                              \
    }

// The two kernels of zedo_temporal.hip that do not know what a chain does with its costs and serve the fusion call
// (zedo_temporal_marginal.hip) as well: the dead flag of every frame, and the tile above on the frames c0 .. of a chunk, as M[n - c0][h'][h].
__global__ __launch_bounds__(256) void temporal_dead_kernel(const double *__restrict__ unary, int H, int N, int *__restrict__ dead);
__global__ __launch_bounds__(TT_T) void temporal_transition_kernel(const float *__restrict__ x, int H, int N, int J, int c0,
                                                                   double *__restrict__ M);

// ---- a frame of the forward recurrence with D[n-1,.] resident in the LDS (H <= TS_CAP) ----
// Lane t owns h = t, t + T, ..; D[n-1,.] is in sD[cur TS_CAP ..], the lanes drop D[n,h] into the other half and ONE barrier per frame
// hands it over.  TS_PF: the transition costs of the lane's first h that were fetched a frame ahead.
constexpr int TS_CAP = 1024, TS_PF = 16;
#ifdef ZEDO_MUT_TEMPORAL_LAMBDA   // tools/mutation_check.py only: the motion term is not weighted
#define ZEDO_TEMPORAL_WEIGHTED(M_) (M_)
#else
#define ZEDO_TEMPORAL_WEIGHTED(M_) (lambda * (M_))
#endif
// In scope: tid, T, H, inf, lambda; uc = u[n, tid] and mc [TS_PF] = m[n, 0 .. TS_PF-1, tid], fetched ahead; is_dead, workgroup-uniform;
// RESIDENT; sD, cur; Mn = m[n] [H',H].  U_AT, D_AT, B_AT: u[n,h], D[n,h] and back[n,h] where the kernel keeps them - expressions in h.
//   a dead frame or a chain's start:  D[n,h] = u[n,h] (+inf: dead, or the unary is not finite), back = -1
#define ZEDO_TEMPORAL_FRAME_START(U_AT, D_AT, B_AT)                                                                                    \
            for (int h = tid; h < H; h += T) {                                                                                         \
                const double u0 = h == tid ? uc : U_AT;                                                                                \
                const double d = (!is_dead && finite64(u0)) ? u0 : inf;                                                                \
                D_AT = d;                                                                                                              \
                B_AT = -1;                                                                                                             \
                if (RESIDENT) sD[(cur ^ 1) * TS_CAP + h] = d;                                                                          \
            }
//   inside a chain:  D[n,h] = u[n,h] + min_h' (D[n-1,h'] + lambda m[n,h',h]), back = the lowest h' that attains it
#define ZEDO_TEMPORAL_FRAME_RESIDENT(U_AT, D_AT, B_AT)                                                                                 \
            const double *prev = sD + cur * TS_CAP;                                                                                    \
            for (int h = tid; h < H; h += T) {                                                                                         \
                const bool first = h == tid;                                                                                           \
                const double u0 = first ? uc : U_AT;                                                                                   \
                double best = inf;                                                                                                     \
                int bh = 0;                                                                                                            \
                auto take = [&](int hp, double m) {                                                                                    \
                    const double c = prev[hp] + ZEDO_TEMPORAL_WEIGHTED(m);                                                             \
                    if (hp == 0 || c < best) { best = c; bh = hp; }      /* strict: the lowest h' that attains the minimum */          \
                };                                                                                                                     \
                int hp = 0;                                                                                                            \
                if (first) {                                                                                                           \
                    _Pragma("unroll") for (int k = 0; k < TS_PF; ++k) if (k < H) take(k, mc[k]);                                       \
                    hp = min(TS_PF, H);                                                                                                \
                }                                                                                                                      \
                _Pragma("unroll 8") for (; hp < H; ++hp) take(hp, Mn[(size_t)hp * H + h]);                                             \
                const double d = (finite64(u0) ? u0 : inf) + best;                                                                     \
                D_AT = d;                                                                                                              \
                B_AT = bh;                                                                                                             \
                sD[(cur ^ 1) * TS_CAP + h] = d;                                                                                        \
            }

}  // namespace zedo
