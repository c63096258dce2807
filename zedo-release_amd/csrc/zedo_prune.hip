// Hypothesis pruning between two stages of the OIL loop for gfx950 (zedo_prune_rank, zedo_prune_gather): per pose the K slots with the
// smallest error are kept and the rows of x, T and the hypothesis ids are compacted to K x N, slots in ascending order.  Two kernels:
//   prune_rank_kernel    a workgroup takes a tile of P consecutive poses and stages their H errors slot-major in the LDS; a lane owns one
//                        pose and every G-th slot (G = 256 / P), counts the slots that precede each of its own (H^2 compares per pose),
//                        publishes "kept" flags in the LDS and takes the output position of a kept slot as the number of kept lower slots
//   prune_gather_kernel  a streaming copy indexed by the table: one wavefront per output row, the lanes along the row's 3 J + 4 words
// Integer logic on the errors as given: the table does not depend on P or on the launch.  No atomics, no workspace.
#include "zedo_internal.h"

#include <algorithm>

namespace zedo {

// finite ascending, then +inf, then NaN: a NaN is behind everything that is not a NaN
__device__ __forceinline__ bool prune_less(double a, double b) { return a < b || (a == a && b != b); }

// slot b with error vb comes before slot a with error va: the strict order above, ties (equal values, -0.0 and 0.0, two NaNs) to the
// lower slot
__device__ __forceinline__ bool prune_precedes(double vb, int b, double va, int a) {
#ifdef ZEDO_MUT_PRUNE_TIE
    return prune_less(vb, va) || (!prune_less(va, vb) && b <= a);
#else
    return prune_less(vb, va) || (!prune_less(va, vb) && b < a);
#endif
}

// LDS: err [H][P] float64, kept [H][P] bytes.  Lanes over consecutive poses read consecutive words; the lanes of a wave that share a pose
// (P < 64) read the same word (a broadcast).  CAP: the bytes of the instantiation, P * H * 9 <= CAP.
constexpr int PR_T = 256, PR_MAXP = 64, PR_CAP_SMALL = 32 * 1024, PR_CAP_LARGE = 144 * 1024, PR_MAXH = 1024;
static_assert(PR_MAXH * 9 * 16 <= PR_CAP_LARGE, "H = 1024 runs with tiles of 16 poses");

template <int CAP>
__global__ __launch_bounds__(PR_T) void prune_rank_kernel(const double *__restrict__ err, int H, int N, int K, int P, int *__restrict__ keep) {
    __shared__ double lds[CAP / 8];
    double *serr = lds;
    unsigned char *skept = reinterpret_cast<unsigned char *>(lds + (size_t)H * P);
    const int tid = threadIdx.x, n0 = blockIdx.x * P;
    for (int q = tid; q < H * P; q += PR_T) {                    // P consecutive poses of one slot: one coalesced run of 8 P bytes
        const int b = q / P, p = q - b * P;
        serr[q] = n0 + p < N ? err[(size_t)b * N + n0 + p] : 0.0;
    }
    __syncthreads();
    const int p = tid % P, g = tid / P, G = PR_T / P, n = n0 + p;
    for (int a = g; a < H; a += G) {
        const double va = serr[a * P + p];
        int before = 0;
        for (int b = 0; b < H; ++b) before += prune_precedes(serr[b * P + p], b, va, a) ? 1 : 0;
        skept[a * P + p] = before < K ? 1 : 0;
    }
    __syncthreads();
    if (n >= N) return;
    for (int a = g; a < H; a += G) {
        if (!skept[a * P + p]) continue;
        int r = 0;
#ifdef ZEDO_MUT_PR_P32   // tools/mutation_check.py only: tiles of 32 poses count the kept slots below a - 1 (r stays within 0 .. K-1)
        for (int b = 0; b < (P == 32 ? a - 1 : a); ++b) r += skept[b * P + p];
#else
        for (int b = 0; b < a; ++b) r += skept[b * P + p];
#endif
        keep[(size_t)r * N + n] = a;                              // r < K: exactly K slots of a pose are kept
    }
}

// poses per tile: the largest power of two up to 64 whose tile fits the instantiation
static int prune_tile(int H, int cap) {
    int P = PR_MAXP;
    while (P > 1 && (long long)H * P * 9 > cap) P >>= 1;
    return P;
}

hipError_t launch_prune_rank(const double *err, int H, int N, int K, int *keep, hipStream_t st) {
    if ((long long)H * PR_MAXP * 9 <= PR_CAP_SMALL) {
        const int P = PR_MAXP;
        hipLaunchKernelGGL(prune_rank_kernel<PR_CAP_SMALL>, dim3((N + P - 1) / P), dim3(PR_T), 0, st, err, H, N, K, P, keep);
    } else {
        const int P = prune_tile(H, PR_CAP_LARGE);
        hipLaunchKernelGGL(prune_rank_kernel<PR_CAP_LARGE>, dim3((N + P - 1) / P), dim3(PR_T), 0, st, err, H, N, K, P, keep);
    }
    return hipGetLastError();
}

// Output row (r, n) = input row keep[r,n] * N + n.  One wavefront per output row, four per workgroup, rows walked with the grid's stride:
// lane c < 3 J copies x, the next three T, the next one the id - 4-byte accesses, contiguous per row (204 + 12 + 4 bytes at J = 17).
// A table entry outside 0 .. H-1 is never an address: the row becomes NaN, its id -1.
constexpr int PG_T = 256, PG_ROWS = PG_T / 64, PG_MAXGRID = 1 << 20;
__global__ __launch_bounds__(PG_T) void prune_gather_kernel(const int *__restrict__ keep, int H, int K, int N, int J3, const float *__restrict__ x,
                                                            const float *__restrict__ T, const int *__restrict__ hyp,
                                                            float *__restrict__ x_out, float *__restrict__ T_out, int *__restrict__ hyp_out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, C = J3 + 4;
    const long long rows = (long long)K * N;
    for (long long row = (long long)blockIdx.x * PG_ROWS + w; row < rows; row += (long long)gridDim.x * PG_ROWS) {
        const int h = keep[row], n = (int)(row % N);
        const bool ok = h >= 0 && h < H;
        const size_t g = ok ? (size_t)h * N + n : 0;
        const float nan = __builtin_nanf("");
        for (int c = lane; c < C; c += 64) {
            if (c < J3) x_out[(size_t)row * J3 + c] = ok ? x[g * J3 + c] : nan;
            else if (c < J3 + 3) T_out[(size_t)row * 3 + (c - J3)] = ok ? T[g * 3 + (c - J3)] : nan;
            else hyp_out[row] = !ok ? -1 : (hyp ? hyp[g] : h);
        }
#ifdef ZEDO_MUT_PG_TRIP   // tools/mutation_check.py only: the rows behind the grid's first trip are never written
        break;
#endif
    }
}

hipError_t launch_prune_gather(const int *keep, int H, int K, int N, int J, const float *x, const float *T, const int *hyp, float *x_out,
                               float *T_out, int *hyp_out, hipStream_t st) {
    const long long blocks = ((long long)K * N + PG_ROWS - 1) / PG_ROWS;
    hipLaunchKernelGGL(prune_gather_kernel, dim3((unsigned)std::min<long long>(blocks, PG_MAXGRID)), dim3(PG_T), 0, st, keep, H, K, N, J * 3, x,
                       T, hyp, x_out, T_out, hyp_out);
    return hipGetLastError();
}

}  // namespace zedo
