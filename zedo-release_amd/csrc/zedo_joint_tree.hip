// Skeleton-coupled joint-wise aggregation for gfx950 (zedo_joint_tree_select): per pose the assignment of one hypothesis to every joint
// that minimises the joints' unary costs plus mu times, for every bone, the mismatch between the assembled bone's length and the length
// the two hypotheses that supply its ends give that bone - exact min-sum dynamic programming over the bone tree, fp64, one launch.
// One workgroup of 256 lanes serves one pose; everything lives in the LDS, sized to the case:
//   X    [J][H][3] f64   the pose's camera-frame positions, joint-major (tree_stage of zedo_chain.h stages X, S and the live flags;
//                        neighbouring poses are neighbours in memory, and neighbours in the grid run at the same time)
//   S    [J][H]    f64   u, then u plus the messages of the children
//   back [J][H]    u16   the arg-min of a bone's message
//   own  [2][H]    f64   the bone's own length in every hypothesis, formed once per bone, double-buffered over consecutive bones
// 34 J H + 16 H + 4096 bytes in all (the parts' minima, the roots and the flags are the 4096).
// The bones are walked in the host's post-order (children before parents, siblings ascending), handed over by value.  For one bone the
// H^2 pairs are dealt by the lane split of zedo_chain.h with P = chain_parts(H): the lane (part, slot) owns hp = slot (+ 256, .. when
// P = 1 and H > 256) and walks one part of the hc in lockstep with its wave, so
// S[g][hc], own[hc] and X[g][hc] are broadcast reads; the parts' minima meet in the LDS and part 0 combines them in ascending part
// order with a strict comparison - the lowest hc still wins.  S[p][.] takes its children's messages in the order of the walk, i.e. in
// ascending child index whatever the launch shape.  One barrier per bone (two where the hc are split).  The roots' minima, the downward
// pass and bone[n,.] end the same launch.  No atomics, no scratch.
#include "zedo_chain.h"

namespace zedo {

__global__ __launch_bounds__(CHAIN_T) void joint_tree_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                          const float *__restrict__ Tr, const float *__restrict__ weight, const TreeOrder tr,
                                                          int H, int N, int J, double mu, int *__restrict__ joint_h, double *__restrict__ cost,
                                                          double *__restrict__ bone) {
    extern __shared__ double tr_lds[];
    const int JH = J * H;
    double *const sX = tr_lds, *const sS = sX + 3 * JH, *const sOwn = sS + JH, *const sPv = sOwn + 2 * H, *const sRmin = sPv + CHAIN_T;
    int *const sPi = reinterpret_cast<int *>(sRmin + TR_JMAX), *const sSel = sPi + CHAIN_T, *const sLive = sSel + TR_JMAX;
    unsigned short *const sBack = reinterpret_cast<unsigned short *>(sLive + TR_JMAX);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = blockIdx.x;
    const double inf = __builtin_huge_val();

    tree_stage(junary, x, Tr, weight, n, H, N, J, inf, [](double u) { return u; }, sX, sS, sLive);
    __syncthreads();

    // upwards: the message of every live bone with a live parent, in the host's order
    const int P = chain_parts(H);
    const Lanes ln(tid, H, P);
    const int SLOTS = ln.slots, part = ln.part, slot = ln.slot, q0 = ln.q0, q1 = ln.q1;   // q0 .. q1-1: this lane's hc
    int nb = 0;
    for (int i = 0; i < J; ++i) {
        const int g = tr.order[i], p = tr.parent[g];
        if (p < 0 || !sLive[g] || !sLive[p]) continue;             // (workgroup-uniform) a root, dead, or cut off by a dead parent
        double *const own = sOwn + (nb & 1) * H;
        ++nb;
        const double *const Xg = sX + (size_t)g * H * 3, *const Xp = sX + (size_t)p * H * 3, *const Sg = sS + g * H;
        for (int h = tid; h < H; h += CHAIN_T) own[h] = tr_dist(Xg + h * 3, Xp[h * 3], Xp[h * 3 + 1], Xp[h * 3 + 2]);
        __syncthreads();                                           // A: own[] is there; the previous bone's sums are in S
        for (int hp = slot; hp < H; hp += SLOTS) {
            const double p0 = Xp[hp * 3], p1 = Xp[hp * 3 + 1], p2 = Xp[hp * 3 + 2], op = own[hp];
            double best = inf;
            int bi = q0;
#pragma unroll 2
            for (int hc = q0; hc < q1; ++hc) {
                const double c = Sg[hc] + mu * tr_bone(tr_dist(Xg + hc * 3, p0, p1, p2), own[hc], op);
                if (c < best) { best = c; bi = hc; }               // strict: the lowest hc that attains the minimum
            }
            if (P == 1) {
                sBack[g * H + hp] = (unsigned short)bi;
                sS[p * H + hp] += best;
            } else {
                sPv[tid] = best;
                sPi[tid] = bi;
            }
        }
        if (P > 1) {
            __syncthreads();                                       // B: the parts' minima are in the LDS
            if (part == 0 && slot < H) {
                double best = sPv[slot];
                int bi = sPi[slot];
                for (int q = 1; q < ln.np; ++q) {
                    const double c = sPv[q * SLOTS + slot];
                    if (c < best) { best = c; bi = sPi[q * SLOTS + slot]; }
                }
                sBack[g * H + slot] = (unsigned short)bi;
                sS[p * H + slot] += best;
            }
        }
    }
    __syncthreads();

    // the roots: a live joint without a live parent; a wave per root takes the lowest arg-min of S[root][.]
    for (int j = wave; j < J; j += CHAIN_T / 64) {
        const int p = tr.parent[j];
        if (!sLive[j] || (p >= 0 && sLive[p])) continue;           // (wave-uniform)
        double v = inf;
        int vh = INT_MAX;
        for (int h = lane; h < H; h += 64) {
            const double c = sS[j * H + h];
            if (c < v) { v = c; vh = h; }
        }
        wave_arg<false>(v, vh);
        if (lane == 0) { sRmin[j] = v; sSel[j] = vh == INT_MAX ? 0 : vh; }
    }
    __syncthreads();
    if (tid == 0) {
        double c = 0.0;
        int roots = 0;
        for (int j = 0; j < J; ++j) {                              // ascending root index
            const int p = tr.parent[j];
            if (sLive[j] && !(p >= 0 && sLive[p])) { c += sRmin[j]; ++roots; }
        }
        cost[n] = roots ? c : inf;
        for (int i = J - 1; i >= 0; --i) {                         // downwards: parents before children
            const int g = tr.order[i], p = tr.parent[g];
            if (!sLive[g]) sSel[g] = 0;
            else if (p >= 0 && sLive[p]) sSel[g] = sBack[g * H + sSel[p]];
        }
    }
    __syncthreads();
    for (int j = tid; j < J; j += CHAIN_T) {
        const int p = tr.parent[j], hc = sSel[j];
        double b = 0.0;
        if (sLive[j] && p >= 0 && sLive[p]) {
            const int hp = sSel[p];
            const double *const Xj = sX + (size_t)j * H * 3, *const Xp = sX + (size_t)p * H * 3;
            const double own_c = tr_dist(Xj + hc * 3, Xp[hc * 3], Xp[hc * 3 + 1], Xp[hc * 3 + 2]);
            const double own_p = tr_dist(Xj + hp * 3, Xp[hp * 3], Xp[hp * 3 + 1], Xp[hp * 3 + 2]);
            b = tr_bone(tr_dist(Xj + hc * 3, Xp[hp * 3], Xp[hp * 3 + 1], Xp[hp * 3 + 2]), own_c, own_p);
        }
        joint_h[n * J + j] = hc;
        bone[n * J + j] = b;
    }
}

size_t joint_tree_lds_bytes(int H, int J) { return (size_t)34 * J * H + (size_t)16 * H + 4096; }

// parent [J] -> the post-order with children in ascending index; false for anything that is not a forest
bool joint_tree_order(const int *parent, int J, TreeOrder *out) {
    if (J < 1 || J > TR_JMAX) return false;
    int first[TR_JMAX], next[TR_JMAX], stack[TR_JMAX], roots = 0;
    for (int j = 0; j < J; ++j) {
        if (parent[j] < -1 || parent[j] >= J || parent[j] == j) return false;
        first[j] = next[j] = -1;
        roots += parent[j] < 0;
    }
    if (!roots) return false;
    for (int j = J - 1; j >= 0; --j)                                // prepend in descending index: the lists come out ascending
        if (parent[j] >= 0) { next[j] = first[parent[j]]; first[parent[j]] = j; }
    int cnt = 0;
    for (int r = 0; r < J; ++r) {
        if (parent[r] >= 0) continue;
        int sp = 0;
        stack[sp++] = r;
        while (sp) {
            const int v = stack[sp - 1];
            if (first[v] >= 0) {                                   // descend into the next child, consuming it
                const int c = first[v];
                first[v] = next[c];
                stack[sp++] = c;
            } else {
                out->order[cnt++] = (unsigned char)v;
                --sp;
            }
        }
    }
    if (cnt != J) return false;                                    // what no root reaches sits on a cycle
    for (int j = 0; j < J; ++j) out->parent[j] = (signed char)parent[j];
    for (int j = J; j < TR_JMAX; ++j) { out->parent[j] = -1; out->order[j] = 0; }
    return true;
}

hipError_t launch_joint_tree_select(const double *junary, const float *x, const float *T, const float *weight, const TreeOrder &tr, int H,
                                    int N, int J, double mu, int *joint_h, double *cost, double *bone, hipStream_t st) {
    static std::atomic<bool> lds_ok[MAX_DEVICES];
    hipError_t e = allow_lds(reinterpret_cast<const void *>(joint_tree_kernel), TR_LDS, lds_ok);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(joint_tree_kernel, dim3((unsigned)N), dim3(CHAIN_T), joint_tree_lds_bytes(H, J), st, junary, x, T, weight, tr, H, N, J, mu,
                       joint_h, cost, bone);
    return hipGetLastError();
}

}  // namespace zedo
