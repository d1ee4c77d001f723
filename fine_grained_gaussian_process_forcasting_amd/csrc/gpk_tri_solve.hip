// Batched triangular solve with one right-hand side per matrix for gfx950: R w = d (trans = 0) or
// R^T w = d (trans = 1), R (B, n, n) lower triangular, n <= 256.
//
// Replaces torch.linalg.solve_triangular in upstream MultivariateNormal.log_prob
// (distributions/multivariate_normal.py: the whitening R^{-1}(value - mean) against the Cholesky
// root of the covariance) and, with trans = 1, the solve of its autograd backward.
//
// One workgroup of 256 threads per matrix, thread i owns x_i. Sixteen columns at a time: the
// diagonal 16 x 16 block goes through LDS and is solved by 16 lanes of wave 0 (column-oriented
// substitution, the pivot's value broadcast by a shuffle), then every remaining thread subtracts
// its 16 products in ascending k (trans = 0: 64 contiguous bytes of its own row; trans = 1: one
// element of 16 rows, coalesced across the threads). fp32 FMA, fixed order, no atomics. The strict
// upper triangle of R is never read.
#include "gpk_common.h"
#include "gpk_posterior_cov.h"

namespace {

__global__ __launch_bounds__(256) void gpk_tri_solve_kernel(const float* __restrict__ R, const float* __restrict__ d,
                                                            int n, int trans, float* __restrict__ w) {
  __shared__ float x[256];
  __shared__ float dg[16 * 17];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const float* Rb = R + b * (size_t)n * n;
  x[tid] = tid < n ? d[b * n + tid] : 0.f;
  const int NB = (n + 15) >> 4;
  for (int step = 0; step < NB; ++step) {
    const int kb = trans ? NB - 1 - step : step;
    {
      const int r = tid >> 4, c = tid & 15;
      const int row = 16 * kb + r, col = 16 * kb + c;
      float v = (r == c) ? 1.f : 0.f;   // identity on padded rows
      if (row < n && col <= row) v = Rb[(size_t)row * n + col];
      dg[r * 17 + c] = v;
    }
    __syncthreads();
    if (tid < 16) {
      float xv = x[16 * kb + tid];
      if (!trans) {
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          const float wm = __shfl(xv, m, 64) / dg[m * 17 + m];
          if (tid == m) xv = wm;
          else if (tid > m) xv = __builtin_fmaf(-dg[tid * 17 + m], wm, xv);
        }
      } else {
#pragma unroll
        for (int m = 15; m >= 0; --m) {
          const float wm = __shfl(xv, m, 64) / dg[m * 17 + m];
          if (tid == m) xv = wm;
          else if (tid < m) xv = __builtin_fmaf(-dg[m * 17 + tid], wm, xv);
        }
      }
      x[16 * kb + tid] = xv;
    }
    __syncthreads();
    if (!trans) {
      if (tid >= 16 * kb + 16 && tid < n) {
        float s = x[tid];
        const float* rr = Rb + (size_t)tid * n + 16 * kb;   // columns 16 kb .. 16 kb + 15 < tid < n
#pragma unroll
        for (int k = 0; k < 16; ++k) s = __builtin_fmaf(-rr[k], x[16 * kb + k], s);
        x[tid] = s;
      }
    } else {
      if (tid < 16 * kb) {
        float s = x[tid];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int kk = 16 * kb + k;
          if (kk < n) s = __builtin_fmaf(-Rb[(size_t)kk * n + tid], x[kk], s);
        }
        x[tid] = s;
      }
    }
    __syncthreads();
  }
  if (tid < n) w[b * n + tid] = x[tid];
}

}  // namespace

int gpk_launch_tri_solve(const float* R, const float* d, int B, int n, int trans, float* w, hipStream_t stream) {
  hipLaunchKernelGGL(gpk_tri_solve_kernel, dim3((unsigned)B), dim3(256), 0, stream, R, d, n, trans, w);
  return (int)hipGetLastError();
}
