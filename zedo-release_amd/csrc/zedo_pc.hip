// Streaming kernels of zedo_pc_step (include/zedo_hip.h): what one predictor-corrector call of the generic sampler does
// beside the score network (reference advanced/sampling.py:180-331, 400-529).  The affine part of every update,
// x_mean = a x + c eps(x), is the EPI_SDE epilogue of post_dense with other scalars (zedo_capi.hip); here are
//   pc_noise_kernel     x += coef z on the padded state              (ALD corrector step; z is the caller's [B][D] draw)
//   pc_finish_kernel    x_mean -> d_x_mean, x_mean + C z -> d_x      (the predictor's noise term, fused with the unpack)
//   pc_norms_kernel / pc_lvn_scalars_kernel / pc_lvn_update_kernel   the Langevin corrector, whose step size needs the
//                       batch means of ||score|| and ||z|| (:281-283): row norms, ONE workgroup that sums them in a fixed
//                       order and writes s and sqrt(2 s) to device memory, and the update that reads the two floats.
// No float atomics, no data-dependent value on the host: results are bit-identical from run to run and every launch is
// legal under stream capture.  Plain C++ with vector stores only; -ffp-contract=off, the unfused x + (k * v) is what the
// reference's torch expressions compute.  No kernel here uses scratch memory (-Rpass-analysis=kernel-resource-usage: 0
// bytes/lane, at most 16 VGPRs).
#include "zedo_internal.h"

namespace zedo {

__global__ void pc_noise_kernel(float *__restrict__ xpad, const float *__restrict__ z, float coef, int B, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * D) return;
    const int r = (int)(i / D), c = (int)(i % D);
    float *p = xpad + (size_t)r * XLD + c;
    *p = *p + coef * z[i];
}

__global__ void pc_finish_kernel(const float *__restrict__ xpad, const float *__restrict__ z, float coef,
                                 float *__restrict__ x, float *__restrict__ x_mean, int B, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * D) return;
    const int r = (int)(i / D), c = (int)(i % D);
    const float m = xpad[(size_t)r * XLD + c];
    if (x_mean) x_mean[i] = m;
    x[i] = z ? m + coef * z[i] : m;
}

// ||eps_b|| over the D real columns of the padded eps rows and ||z_b|| of the unpadded draw: 16 lanes per row (4 rows per
// wave64), 4 columns per lane summed left to right, then an xor-shuffle tree over the 16 lanes - one fixed order per row.
constexpr int NORM_LANES = 16;
__global__ void pc_norms_kernel(const float *__restrict__ eps, const float *__restrict__ z, float *__restrict__ n_eps,
                                float *__restrict__ n_z, int B, int D) {
    const int lane = threadIdx.x % NORM_LANES;
    const long long row = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / NORM_LANES;
    const bool live = row < B;             // dead lanes keep shuffling: a 16-lane group is all live or all dead
    float se = 0.f, sz = 0.f;
#pragma unroll
    for (int q = 0; q < XLD / NORM_LANES; ++q) {
        const int c = lane * (XLD / NORM_LANES) + q;
        if (live && c < D) {
            const float e = eps[(size_t)row * XLD + c], v = z[(size_t)row * D + c];
            se = se + e * e;
            sz = sz + v * v;
        }
    }
#pragma unroll
    for (int o = NORM_LANES / 2; o > 0; o >>= 1) {
        se = se + __shfl_xor(se, o, NORM_LANES);
        sz = sz + __shfl_xor(sz, o, NORM_LANES);
    }
    if (live && lane == 0) {
        n_eps[row] = sqrtf(se);
        n_z[row] = sqrtf(sz);
    }
}

// One workgroup: thread t sums rows t, t + 256, ... in that order, then a binary tree over the 256 partial sums.  n = the
// B REAL rows of the call (the padding rows of the workspace hold eps of whatever the padded state carries and must not
// enter the mean).  s = factor (mean||z|| / (|net_scale| mean||eps||))^2  == (snr mean||z|| / mean||score||)^2 2 alpha
// (reference :281-284); out[0] = s, out[1] = sqrt(2 s).
constexpr int SUM_THREADS = 256;
__global__ void __launch_bounds__(SUM_THREADS) pc_lvn_scalars_kernel(const float *__restrict__ n_eps, const float *__restrict__ n_z,
                                                                     int n, float factor, float abs_net_scale, float *__restrict__ out) {
    __shared__ float sh_e[SUM_THREADS], sh_z[SUM_THREADS];
    const int t = threadIdx.x;
    float se = 0.f, sz = 0.f;
    for (int i = t; i < n; i += SUM_THREADS) {
        se = se + n_eps[i];
        sz = sz + n_z[i];
    }
    sh_e[t] = se; sh_z[t] = sz;
    __syncthreads();
    for (int o = SUM_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) {
            sh_e[t] = sh_e[t] + sh_e[t + o];
            sh_z[t] = sh_z[t] + sh_z[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
#ifdef ZEDO_MUT_PC_MEAN     // tools/mutation_check.py only: the eps mean divided by the padded row count
        const float me = sh_e[0] / (float)((n + BATCH_PAD - 1) / BATCH_PAD * BATCH_PAD), mz = sh_z[0] / (float)n;
#else
        const float me = sh_e[0] / (float)n, mz = sh_z[0] / (float)n;
#endif
        const float r = mz / (abs_net_scale * me);
        const float s = factor * (r * r);
        out[0] = s;
        out[1] = sqrtf(s * 2.0f);
    }
}

// x_mean = x + (s net_scale) eps;  x = x_mean + sqrt(2 s) z   on the B real rows of the padded state (:284-285)
__global__ void pc_lvn_update_kernel(float *__restrict__ xpad, const float *__restrict__ eps, const float *__restrict__ z,
                                     const float *__restrict__ scal, float net_scale, int B, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * D) return;
    const int r = (int)(i / D), c = (int)(i % D);
    const float k = scal[0] * net_scale, sq = scal[1];
    const size_t j = (size_t)r * XLD + c;
    const float m = xpad[j] + k * eps[j];
    xpad[j] = m + sq * z[i];
}

static inline dim3 grid_for(size_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

hipError_t launch_pc_noise(float *xpad, const float *z, float coef, int B, int D, hipStream_t st) {
    hipLaunchKernelGGL(pc_noise_kernel, grid_for((size_t)B * D, 256), dim3(256), 0, st, xpad, z, coef, B, D);
    return hipGetLastError();
}

hipError_t launch_pc_finish(const float *xpad, const float *z, float coef, float *x, float *x_mean, int B, int D, hipStream_t st) {
    hipLaunchKernelGGL(pc_finish_kernel, grid_for((size_t)B * D, 256), dim3(256), 0, st, xpad, z, coef, x, x_mean, B, D);
    return hipGetLastError();
}

hipError_t launch_pc_langevin(float *xpad, const float *eps, const float *z, float factor, float net_scale, float *n_eps,
                              float *n_z, float *scal, int B, int D, hipStream_t st) {
    hipLaunchKernelGGL(pc_norms_kernel, grid_for((size_t)B * NORM_LANES, 256), dim3(256), 0, st, eps, z, n_eps, n_z, B, D);
    hipLaunchKernelGGL(pc_lvn_scalars_kernel, dim3(1), dim3(SUM_THREADS), 0, st, n_eps, n_z, B, factor, fabsf(net_scale), scal);
    hipLaunchKernelGGL(pc_lvn_update_kernel, grid_for((size_t)B * D, 256), dim3(256), 0, st, xpad, eps, z, scal, net_scale, B, D);
    return hipGetLastError();
}

}  // namespace zedo
