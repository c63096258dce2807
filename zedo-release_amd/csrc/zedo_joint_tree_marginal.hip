// Skeleton-coupled fusion per pose for gfx950 (zedo_joint_tree_marginal): the sum-product twin of zedo_joint_tree.hip.  The energy of
// zedo_joint_tree_select read as a probability at a temperature tau; the skeleton is a tree, so one pass from the leaves to the roots and
// one back give every joint's exact marginals over its hypotheses - in the log domain, fp64 - and from them the posterior mean position,
// its covariance, the most probable hypothesis, the log-partition value and every bone's expected mismatch.  One launch, one workgroup
// of 256 lanes per pose, everything in the LDS, sized to the case:
//   X    [J][H][3] f64   the pose's camera-frame positions, joint-major (tree_stage of zedo_chain.h stages X, S and the live flags)
//   S    [J][H]    f64   l = -u / tau, then l plus the messages of the children
//   M    [J][H]    f64   M_g[hp], the message bone g sends up (the downward pass needs it); once Dn[g] is formed, the slot holds
//                        sum_hp pi[g,hp,hc] b[g,hp,hc] of every hc instead: the terms of bone[n,g]
//   Dn   [J][H]    f64   the message from above; at the end the marginal w[j,h] itself
//   own  [H], E [H] f64  the bone's own length in every hypothesis, and E_g[hp] = S[p,hp] - M_g[hp] + Dn[p,hp] of the downward pass
// 48 J H + 16 H + 8192 bytes in all (the parts' maxima, sums and bone sums, log Z of every joint and the flags are the 8192).
// The bones are walked in the host's post-order upwards and in its reverse downwards.  For one bone the H^2 pairs are dealt by the lane
// split of zedo_chain.h with P = chain_parts(H); a lane owns the OUTER index (hp upwards, hc downwards;
// + 256, .. when P = 1 and H > 256) and walks one part of the inner index in lockstep with its wave, so the inner index's value, own
// length and position are broadcast reads in both roles, and the owner's position is read once, at the conflict-free stride above.  A
// log-sum-exp takes two walks: the first finds the largest term, the second adds exp(term - largest) in ascending inner index; the bone
// term is recomputed in the second walk (one square root and one exp per pair per walk at most).  With P > 1 every part shifts by its
// own maximum and part 0 combines the parts in ascending order, shifted by the largest.  Downwards the second walk also adds
// exp(term - largest) b: the pair marginals are consumed where they are formed.  The roots' log Z, the marginals, the mean, the
// covariance, the arg-max and bone[n,.] end the same launch, a wave per joint.  No atomics, no scratch, every sum in a fixed order.
#include "zedo_chain.h"

namespace zedo {

// One lane's share of LSE_q (V[q] - c b(q)) over the inner index q = q0 .. q1-1 for one outer index.  UP: the outer index is hp (xo =
// X[p][hp], oo = own[hp]) and q runs over hc (Xin = X[g], V = S[g]); otherwise the outer index is hc (xo = X[g][hc], oo = own[hc]) and q
// runs over hp (Xin = X[p], V = E).  mx = the largest term (-inf if the share has none above -inf), sm = sum exp(term - mx) ascending in
// q (shifted by 0 where mx is -inf: every exp is 0), and downwards sb = sum exp(term - mx) b.
template <bool UP>
__device__ __forceinline__ void tm_walk(const double *Xin, const double *V, const double *own, int q0, int q1, const double (&xo)[3],
                                        double oo, double c, double &mx, double &sm, double &sb) {
    const double ninf = -__builtin_huge_val();
    mx = ninf;
#pragma unroll 2
    for (int q = q0; q < q1; ++q) {
        const double mix = UP ? tr_dist(Xin + q * 3, xo[0], xo[1], xo[2]) : tr_dist(xo, Xin[q * 3], Xin[q * 3 + 1], Xin[q * 3 + 2]);
        const double t = V[q] - c * (UP ? tr_bone(mix, own[q], oo) : tr_bone(mix, oo, own[q]));
        if (t > mx) mx = t;
    }
    const double sh = mx > ninf ? mx : 0.0;
    sm = 0.0;
    sb = 0.0;
#pragma unroll 2
    for (int q = q0; q < q1; ++q) {
        const double mix = UP ? tr_dist(Xin + q * 3, xo[0], xo[1], xo[2]) : tr_dist(xo, Xin[q * 3], Xin[q * 3 + 1], Xin[q * 3 + 2]);
        const double b = UP ? tr_bone(mix, own[q], oo) : tr_bone(mix, oo, own[q]);
        const double e = exp(V[q] - c * b - sh);
        sm += e;
        if (!UP) sb += e * b;
    }
}

// Part 0's end of a split log-sum-exp: (mx, sm, sb) of its own share and those of the other parts from the LDS, in ascending part order,
// every part's sums scaled to the largest maximum.
__device__ __forceinline__ void tm_combine(double &mx, double &sm, double &sb, const double *sPm, const double *sPs, const double *sPb,
                                           int slots, int slot, int np) {
    const double ninf = -__builtin_huge_val();
    double M = mx;
    for (int p = 1; p < np; ++p) {
        const double v = sPm[p * slots + slot];
        if (v > M) M = v;
    }
    const double f0 = mx == M ? 1.0 : (mx > ninf ? exp(mx - M) : 0.0);
    double S = mx == M ? sm : sm * f0, B = mx == M ? sb : sb * f0;
    for (int p = 1; p < np; ++p) {
        const double v = sPm[p * slots + slot], q = sPs[p * slots + slot], r = sPb[p * slots + slot];
        if (v == M) { S += q; B += r; }
        else if (v > ninf) { const double f = exp(v - M); S += q * f; B += r * f; }
    }
    mx = M;
    sm = S;
    sb = B;
}

__global__ __launch_bounds__(CHAIN_T) void joint_tree_marginal_kernel(const double *__restrict__ junary, const float *__restrict__ x,
                                                                   const float *__restrict__ Tr, const float *__restrict__ weight,
                                                                   const TreeOrder tr, int H, int N, int J, double c, double tau,
                                                                   double *__restrict__ mean, double *__restrict__ cov, int *__restrict__ hmax,
                                                                   double *__restrict__ wmax, double *__restrict__ logz,
                                                                   double *__restrict__ bone, double *__restrict__ wout) {
    extern __shared__ double tm_lds[];
    const int JH = J * H;
    double *const sX = tm_lds, *const sS = sX + 3 * JH, *const sM = sS + JH, *const sD = sM + JH, *const sOwn = sD + JH, *const sE = sOwn + H;
    double *const sPm = sE + H, *const sPs = sPm + CHAIN_T, *const sPb = sPs + CHAIN_T, *const sLz = sPb + CHAIN_T;
    int *const sLive = reinterpret_cast<int *>(sLz + TR_JMAX);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = blockIdx.x;
    const double ninf = -__builtin_huge_val(), qnan = __builtin_nan("");

    // l = -u / tau; sD = 0: Dn of a root - every other live joint's is written on the way down
    tree_stage(junary, x, Tr, weight, n, H, N, J, ninf, [tau](double u) { return -u / tau; }, sX, sS, sLive, sD);

    const int P = chain_parts(H);
    const Lanes ln(tid, H, P);
    const int SLOTS = ln.slots, part = ln.part, slot = ln.slot, q0 = ln.q0, q1 = ln.q1, np = ln.np;       // q0 .. q1-1: this lane's inner indices

    // upwards: the message of every live bone with a live parent, in the host's order
    for (int i = 0; i < J; ++i) {
        __syncthreads();                                           // T: the flags; the previous bone's sums are in S, own[] is free
        const int g = tr.order[i], p = tr.parent[g];
        if (p < 0 || !sLive[g] || !sLive[p]) continue;             // (workgroup-uniform) a root, dead, or cut off by a dead parent
        const double *const Xg = sX + (size_t)g * H * 3, *const Xp = sX + (size_t)p * H * 3;
        for (int h = tid; h < H; h += CHAIN_T) sOwn[h] = tr_dist(Xg + h * 3, Xp[h * 3], Xp[h * 3 + 1], Xp[h * 3 + 2]);
        __syncthreads();                                           // A: own[] is there
        for (int hp = slot; hp < H; hp += SLOTS) {
            const double xo[3] = {Xp[hp * 3], Xp[hp * 3 + 1], Xp[hp * 3 + 2]};
            double mx, sm, sb;
            tm_walk<true>(Xg, sS + g * H, sOwn, q0, q1, xo, sOwn[hp], c, mx, sm, sb);
            if (P == 1) {
                const double m = mx + log(sm);
                sM[g * H + hp] = m;
                sS[p * H + hp] += m;
            } else {
                sPm[tid] = mx;
                sPs[tid] = sm;
            }
        }
        if (P > 1) {
            __syncthreads();                                       // B: the parts' maxima and sums are in the LDS
            if (part == 0 && slot < H) {
                double mx = sPm[slot], sm = sPs[slot], sb = 0.0;
                tm_combine(mx, sm, sb, sPm, sPs, sPs, SLOTS, slot, np);
                const double m = mx + log(sm);
                sM[g * H + slot] = m;
                sS[p * H + slot] += m;
            }
        }
    }
    __syncthreads();

    // the roots: a live joint without a live parent; a wave per root takes log Z = LSE_h S[root,h], shifted by the largest
    for (int j = wave; j < J; j += CHAIN_T / 64) {
        const int p = tr.parent[j];
        if (!sLive[j] || (p >= 0 && sLive[p])) continue;           // (wave-uniform)
        double v = ninf;
        for (int h = lane; h < H; h += 64) v = fmax(v, sS[j * H + h]);
        v = wave_max(v);
        double e = 0.0;
        for (int h = lane; h < H; h += 64) e += exp(sS[j * H + h] - v);
        e = wave_sum(e);
        if (lane == 0) sLz[j] = v + log(e);
    }
    __syncthreads();
    if (tid == 0)
        for (int i = J - 1; i >= 0; --i) {                         // parents before children: a joint takes its component's log Z
            const int g = tr.order[i], p = tr.parent[g];
            if (!sLive[g]) sLz[g] = ninf;
            else if (p >= 0 && sLive[p]) sLz[g] = sLz[p];
        }

    // downwards: Dn of every live bone with a live parent, and with it the terms of the bone's expected mismatch
    for (int i = J - 1; i >= 0; --i) {
        __syncthreads();                                           // T: log Z; Dn of the parent is there, own[] and E[] are free
        const int g = tr.order[i], p = tr.parent[g];
        if (p < 0 || !sLive[g] || !sLive[p]) continue;             // (workgroup-uniform)
        const double *const Xg = sX + (size_t)g * H * 3, *const Xp = sX + (size_t)p * H * 3;
        for (int h = tid; h < H; h += CHAIN_T) {
            sOwn[h] = tr_dist(Xg + h * 3, Xp[h * 3], Xp[h * 3 + 1], Xp[h * 3 + 2]);
            sE[h] = sS[p * H + h] - sM[g * H + h] + sD[p * H + h];
        }
        __syncthreads();                                           // A: own[] and E[] are there; M_g has been read
        const double lz = sLz[g];
        auto finish = [&](int hc, double mx, double sm, double sb) {
#ifndef ZEDO_MUT_TREEMARG_NO_DOWN   // tools/mutation_check.py only: Dn stays 0 - the downward pass is dropped
            sD[g * H + hc] = mx + log(sm);
#endif
            sM[g * H + hc] = sb * exp((mx > ninf ? mx : 0.0) + sS[g * H + hc] - lz);      // sum_hp pi[g,hp,hc] b[g,hp,hc]
        };
        for (int hc = slot; hc < H; hc += SLOTS) {
            const double xo[3] = {Xg[hc * 3], Xg[hc * 3 + 1], Xg[hc * 3 + 2]};
            double mx, sm, sb;
            tm_walk<false>(Xp, sE, sOwn, q0, q1, xo, sOwn[hc], c, mx, sm, sb);
            if (P == 1) {
                finish(hc, mx, sm, sb);
            } else {
                sPm[tid] = mx;
                sPs[tid] = sm;
                sPb[tid] = sb;
            }
        }
        if (P > 1) {
            __syncthreads();                                       // B: the parts' maxima and sums are in the LDS
            if (part == 0 && slot < H) {
                double mx = sPm[slot], sm = sPs[slot], sb = sPb[slot];
                tm_combine(mx, sm, sb, sPm, sPs, sPb, SLOTS, slot, np);
                finish(slot, mx, sm, sb);
            }
        }
    }
    __syncthreads();

    // what is read off the marginals, a wave per joint: every sum lane by lane in ascending h, then a butterfly over the wave
    for (int j = wave; j < J; j += CHAIN_T / 64) {
        const size_t nj = n * J + j;
        if (!sLive[j]) {                                           // (wave-uniform) NaN, hypothesis 0, weight 0, log Z = -inf, bone 0, a row of zeros
            if (lane < 3) mean[nj * 3 + lane] = qnan;
            if (lane < 6) cov[nj * 6 + lane] = qnan;
            if (lane == 0) { hmax[nj] = 0; wmax[nj] = 0.0; logz[nj] = ninf; bone[nj] = 0.0; }
            if (wout)
                for (int h = lane; h < H; h += 64) wout[nj * H + h] = 0.0;
            continue;
        }
        const int p = tr.parent[j];
        const bool coupled = p >= 0 && sLive[p];
        const double lz = sLz[j];
        const double *const Xj = sX + (size_t)j * H * 3;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, bs = 0.0, bw = ninf;
        int bh = INT_MAX;
        for (int h = lane; h < H; h += 64) {
            const double w = exp(sS[j * H + h] + sD[j * H + h] - lz);                     // exactly 0 for an excluded hypothesis (S = -inf)
            sD[j * H + h] = w;                                     // (read back by this lane only)
            if (wout) wout[nj * H + h] = w;
            if (w > bw) { bw = w; bh = h; }                        // ascending h, strict: the lowest h of the lane
            m0 += w * Xj[h * 3]; m1 += w * Xj[h * 3 + 1]; m2 += w * Xj[h * 3 + 2];
            if (coupled) bs += sM[j * H + h];
        }
        wave_arg<true>(bw, bh);
        m0 = wave_sum(m0); m1 = wave_sum(m1); m2 = wave_sum(m2); bs = wave_sum(bs);
        double c6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int h = lane; h < H; h += 64) {
            const double w = sD[j * H + h], d0 = Xj[h * 3] - m0, d1 = Xj[h * 3 + 1] - m1, d2 = Xj[h * 3 + 2] - m2;
            c6[0] += w * (d0 * d0); c6[1] += w * (d0 * d1); c6[2] += w * (d0 * d2);
            c6[3] += w * (d1 * d1); c6[4] += w * (d1 * d2); c6[5] += w * (d2 * d2);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) c6[k] = wave_sum(c6[k]);
        if (lane == 0) {
            mean[nj * 3] = m0; mean[nj * 3 + 1] = m1; mean[nj * 3 + 2] = m2;
#pragma unroll
            for (int k = 0; k < 6; ++k) cov[nj * 6 + k] = c6[k];
            hmax[nj] = bh == INT_MAX ? 0 : bh;
            wmax[nj] = bh == INT_MAX ? 0.0 : bw;
            logz[nj] = lz;
            bone[nj] = bs;
        }
    }
}

constexpr size_t TM_FIXED = 8192;                                  // 3 x 256 doubles of the parts, 64 of log Z, 64 flags: 6912 bytes
size_t joint_tree_marginal_lds_bytes(int H, int J) { return (size_t)48 * J * H + (size_t)16 * H + TM_FIXED; }

int joint_tree_marginal_max_h(int J) {
    if (J < 1 || J > TR_JMAX) return 0;
    const size_t h = (TR_LDS - TM_FIXED) / ((size_t)48 * J + 16);
    return h > (size_t)TR_HMAX ? TR_HMAX : (int)h;
}

hipError_t launch_joint_tree_marginal(const double *junary, const float *x, const float *T, const float *weight, const TreeOrder &tr, int H,
                                      int N, int J, double c, double tau, double *mean, double *cov, int *hmax, double *wmax, double *logz,
                                      double *bone, double *w, hipStream_t st) {
    static std::atomic<bool> lds_ok[MAX_DEVICES];
    hipError_t e = allow_lds(reinterpret_cast<const void *>(joint_tree_marginal_kernel), TR_LDS, lds_ok);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(joint_tree_marginal_kernel, dim3((unsigned)N), dim3(CHAIN_T), joint_tree_marginal_lds_bytes(H, J), st, junary, x, T, weight,
                       tr, H, N, J, c, tau, mean, cov, hmax, wmax, logz, bone, w);
    return hipGetLastError();
}

}  // namespace zedo
