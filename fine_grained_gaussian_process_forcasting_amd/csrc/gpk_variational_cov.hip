// Dense covariance of a variational q(f) (eval mode) for gfx950, phase 1.
//
// Replaces, per window b, the dense evaluation of upstream variational/variational_strategy.py
// (whitened) predictive_covar, which MultivariateNormal.rsample / covariance_matrix of a DeepGP
// layer output materialise (reference denoising_model/DeepGP.py:62-64):
//   K_ZX = s2 exp(-0.5 |(z_m - x_i) / l|^2)        fp32, the arithmetic of gpk_variational_f32
//   A    = L^{-1} K_ZX                             fp64, cast to fp32
//   cov  = K_XX + jitter I + A^T diag(vstd^2 - 1) A
// This file keeps A for phase 2 (the variational mode of gpk_post_cov_kernel,
// gpk_posterior_cov.hip): row-major (B, M, as) with the row stride as = N rounded up to 64
// (columns >= N hold zeros), followed by the window's own mean of x / l (B x 64 floats), which
// centres phase 2's K_XX Gram as upstream _sq_dist does for x1 == x2; phase 2 never walks the
// inputs of a window again.
//
// Design: one workgroup of 4 waves per (window, 64-point column block), output o on grid y.
//   The column means of Z / l, the staging of the block's points and the constants are
//     gpk_var_dense.h's (vd_col_means, vd_stage_points), which describes them once for the four
//     units that run them.
//   K_ZX block (M x 64): the forward's Gram. z / l and x / l centred by the column means of
//     Z / l, squared norms by fma over the padded D, the cross term on fp32 MFMA, d2 = |z|^2 +
//     |x|^2 - 2 z.x clamped at 0, k = s2 exp2(-0.5 log2(e) d2). The inducing points go through
//     LDS 64 rows at a time (row stride: padded D + 4); the block stays in LDS with the row
//     stride kKS. In line here and in gpk_vchol_fwd_kernel, gpk_vcc_fwd_kernel and
//     gpk_vcg_q_kernel: as a function it moves the register figures of the other three
//     (DESIGN.md §8.9); the four copies are the same text.
//   A = L^{-1} K_ZX: wave w owns the 16 columns w of the block and walks the row tiles; row
//     tile rt contracts the k blocks kb <= rt only (L^{-1} is lower triangular, its zero blocks
//     are skipped) with mfma_f64_16x16x4_f64, L^{-1} read from global memory (L2-resident: all
//     workgroups read the same M x M matrix), four k blocks' operands in flight at a time and
//     the next four loaded under these MFMAs. The cast to fp32 happens on the store. In line here
//     and in the two Cholesky forward kernels, which walk the row tiles down and write over K:
//     as a function the row-tile product took 14 SGPRs off this kernel (106 -> 92, §8.9).
// No atomics, fixed summation order: deterministic. Output o of a batched launch runs the
// single-output body on its own slices: bit-identical to a single-output call.
#include "gpk_common.h"
#include "gpk_posterior_cov.h"
#include "gpk_var_dense.h"

#include <mutex>

namespace {

struct VarCovP1Args {
  const float* X;
  const float* Z;
  const double* Linv;
  const float* hyp;
  float* ws;
  int B, N, M, D, as;
  long long x_stride, ws_stride;
};

__global__ __launch_bounds__(256) void gpk_var_cov_a_kernel(VarCovP1Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.N, M = a.M, D = a.D;
  const int MP = (M + 15) & ~15;
  const int Dq = vd_dq(D);
  const int lgq = vd_lgq(Dq);
  const int ds = Dq + 4;                 // LDS row stride of the staged z / x rows
  float* Kl = lds;                       // MP x kKS
  float* zs = Kl + (size_t)MP * kKS;     // 64 x ds
  float* xs = zs + 64 * ds;              // 64 x ds
  float* zn = xs + 64 * ds;              // 64
  float* xn = zn + 64;                   // 64
  float* cm = xn + 64;                   // 64
  float* lsc = cm + 64;                  // 64
  float* scr = lsc + 64;                 // 512

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int ncb = (N + kCB - 1) / kCB;
  const int b = blockIdx.x / ncb, cb = blockIdx.x - b * ncb;
  const size_t o = blockIdx.y;

  const float* hyp = a.hyp + o * (size_t)(4 + 2 * D);
  const float* Xb = a.X + o * (size_t)a.x_stride + (size_t)b * N * D;
  const float* Z = a.Z + o * (size_t)M * D;
  const double* Linv = a.Linv + o * (size_t)M * M;
  float* Aw = a.ws + o * (size_t)a.ws_stride + (size_t)b * M * a.as;
  float* muw = a.ws + o * (size_t)a.ws_stride + (size_t)a.B * M * a.as + (size_t)b * 64;
  const float s2 = hyp[0];

  if (tid < 64) lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
  lds_barrier();

  vd_col_means(Z, M, D, Dq, lsc, scr, cm, tid);
  // ---- the window's own mean of x / l for phase 2 (one workgroup per window writes it; the
  //      same text in gpk_vcc_fwd_kernel, gpk_var_chol_cov.hip):
  //      P = 256 / Dq partial sums per column over rows i = k mod P, ascending, then k = 0..P-1
  if (cb == 0) {
    const int d = tid & (Dq - 1), k = tid >> lgq, P = 256 >> lgq;
    float s = 0.f;
    if (d < D) {
      const float l = lsc[d];
#pragma unroll 4
      for (int i = k; i < N; i += P) s += Xb[(size_t)i * D + d] / l;
    }
    scr[tid] = s;   // = scr[k * Dq + d]
    lds_barrier();
    if (tid < 64) {
      float t = 0.f;
      if (tid < D)
        for (int q = 0; q < P; ++q) t += scr[q * Dq + tid];
      muw[tid] = tid < D ? t / (float)N : 0.f;
    }
    lds_barrier();
  }
  vd_stage_points(Xb, N, D, Dq, cb, lsc, cm, xs, xn, tid);

  // ---- K_ZX block, 64 inducing rows at a time (in line in four kernels, see the file head)
  for (int r0 = 0; r0 < MP; r0 += 64) {
    lds_barrier();   // the previous chunk's Gram reads are done (first pass: xn is written)
#pragma unroll 4
    for (int e = tid; e < 64 * Dq; e += 256) {
      const int r = e >> lgq, d = e & (Dq - 1);
      const int m = r0 + r;
      const bool ok = d < D && m < M;
      const float v = Z[ok ? (size_t)m * D + d : 0];
      zs[r * ds + d] = ok ? v / lsc[d] - cm[d] : 0.f;
    }
    lds_barrier();
    if (tid < 64) {
      float s = 0.f;
      for (int d = 0; d < Dq; ++d) s = __builtin_fmaf(zs[tid * ds + d], zs[tid * ds + d], s);
      zn[tid] = s;
    }
    lds_barrier();
    const int nrt = (MP - r0) >= 64 ? 4 : (MP - r0) / 16;
    const float* xb = xs + (16 * w + c) * ds + g;
    const int col = 16 * w + c;
    const float xnc = xn[col];
    const bool okc = kCB * cb + col < N;
    for (int rt = 0; rt < nrt; ++rt) {
      const float* za = zs + (16 * rt + c) * ds + g;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < Dq / 4; ++k)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(za[4 * k], xb[4 * k], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 16 * rt + 4 * g + r;
        float dist = zn[p] + xnc - 2.f * acc[r];
        dist = dist < 0.f ? 0.f : dist;
        Kl[(size_t)(r0 + p) * kKS + col] =
            (r0 + p < M && okc) ? s2 * __builtin_amdgcn_exp2f(kNHalfLog2e * dist) : 0.f;
      }
    }
  }
  lds_barrier();

  // ---- A = L^{-1} K_ZX for this wave's 16 columns: lane (g, c) feeds the A operand
  //      L^{-1}[16 rt + c][16 kb + 4 g + u] and the B operand K[16 kb + 4 g + u][16 w + c] in
  //      MFMA step u; acc[r] = A[16 rt + g + 4 r][16 w + c]
  const int MB = MP / 16;
  const float* Kc = Kl + 16 * w + c;
  for (int rt = 0; rt < MB; ++rt) {
    const int m = 16 * rt + c;
    const double* row = Linv + (size_t)(m < M ? m : 0) * M;
    // four k blocks' operands (16 loads per lane) are in flight together: with one workgroup
    // per CU at M = 256 nothing else hides the L2 latency of a dependent load per block
    auto load_a = [&](int kb0, double (&dst)[4][4]) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int p = 16 * (kb0 + q) + 4 * g + u;
          const bool ok = m < M && p < M && kb0 + q <= rt;
          const double v = row[ok ? p : 0];
          dst[q][u] = ok ? v : 0.0;
        }
    };
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    double an[4][4];
    load_a(0, an);
    for (int kb0 = 0; kb0 <= rt; kb0 += 4) {
      double av[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int u = 0; u < 4; ++u) av[q][u] = an[q][u];
      if (kb0 + 4 <= rt) load_a(kb0 + 4, an);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (kb0 + q > rt) break;   // ascending kb, u: the order of the block-at-a-time loop
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(
              av[q][u], (double)Kc[(size_t)(16 * (kb0 + q) + 4 * g + u) * kKS], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = 16 * rt + g + 4 * r;
      if (mr < M) Aw[(size_t)mr * a.as + kCB * cb + 16 * w + c] = (float)acc[r];
    }
  }
}

size_t var_cov_p1_lds(int M, int D) {
  const int MP = (M + 15) & ~15;
  return ((size_t)MP * kKS + 2 * 64 * (vd_dq(D) + 4) + 4 * 64 + 512) * sizeof(float);
}

}  // namespace

size_t gpk_var_cov_ws_floats(int B, int N, int M) {
  return (size_t)B * M * gpk_post_cov_vstride(N) + (size_t)B * 64;
}

int gpk_launch_variational_cov_phase1(const GpkVarCovArgs& a, float* ws, const float* Z, const double* Linv,
                                      int O, hipStream_t stream) {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)gpk_var_cov_a_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipGetLastError();
  });
  const long long grid = (long long)a.B * ((a.N + kCB - 1) / kCB);
  if (grid > 0x7fffffff) return -9;
  VarCovP1Args p{a.X, Z, Linv, a.hyp, ws, a.B, a.N, a.M, a.D, a.as, a.x_stride, a.ws_stride};
  hipLaunchKernelGGL(gpk_var_cov_a_kernel, dim3((unsigned)grid, O), dim3(256), var_cov_p1_lds(a.M, a.D), stream, p);
  return (int)hipGetLastError();
}
