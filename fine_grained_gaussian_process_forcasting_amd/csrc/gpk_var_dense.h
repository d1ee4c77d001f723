// Dense-covariance and Cholesky q(u) kernels of the variational GP: the device blocks that more
// than one of their units runs, once. The units:
//   gpk_variational_cov.hip       phase 1 of the dense Sigma of q(f): A = L^{-1} K_ZX
//   gpk_variational_cov_grad.hip  its adjoint (t, q, dlinv, kxx, reduce, finish)
//   gpk_var_chol.hip              Cholesky q(u): mean / variance, adjoint, KL
//   gpk_var_chol_cov.hip          dense Sigma of a Cholesky q(u), both ways
// Everything here is unit-local (anonymous namespace) and forced inline: a kernel is still one
// instruction stream. A change to a block here re-canonicalises the device code of every kernel
// that calls it: prove such a change with scripts/isa_diff.py (equal register, spill, LDS and
// scratch figures per kernel) and scripts/var_dense_ab.py (equal bits), DESIGN.md §8.9. The
// batched-equals-single and diagonal-L_q-equals-mean-field tests rest on every caller running the
// same arithmetic in the same order, which is what one copy gives.
//
// NOT here, although more than one kernel runs them, because as functions they move a caller's
// register figures (§8.9 has the figures): the K_ZX block builder and the A = L^{-1} K_ZX row
// tile (in line in gpk_var_cov_a_kernel, gpk_vchol_fwd_kernel, gpk_vcc_fwd_kernel; the former
// also in gpk_vcg_q_kernel), the H-chunk staging and T accumulation of the two t kernels, the W
// pass inside gpk_vcc_fwd_kernel (a copy of vd_w_pass), and the SYRK tile of
// gpk_post_cov_kernel / gpk_vcc_syrk_kernel. gpk_vcc_fwd_kernel is the parent's text throughout:
// it also keeps its own copy of vd_col_means and vd_stage_points (with the calls it timed 0.4 %
// slower), which leaves the window's own mean of x / l with two in-line copies (there and in
// gpk_var_cov_a_kernel). Edit those copies together.
//
// The mean-field forward and adjoint units (gpk_var_common.h: col_means, stage_inducing) sum in
// the same orders from their own copy; this header is not combined with that one.
//
// Conventions: a workgroup is 256 threads = 4 waves; tid = threadIdx.x, w = the wave, lane =
// (g, c) with c = lane & 15, g = lane >> 4; MFMA operands follow gpk_common.h's acc layout.
// Functions that every thread of the workgroup must call say so.
#pragma once
#include "gpk_common.h"

namespace {

constexpr int kCB = 64;        // points per column block
constexpr int kKS = 68;        // LDS row stride of a 64-column panel (the four k rows of an MFMA
                               // step land 16 banks apart)
constexpr int kHS = 273;       // LDS row stride of a 16-row chunk of H (N <= 256)
constexpr float kNHalfLog2e = -0.72134752044448170f;  // -0.5 * log2(e)

// D padded to a power of two >= 16 (<= 64): MFMA k steps and d tiles, and 256 % Dq == 0.
__host__ __device__ constexpr int vd_dq(int D) { return D <= 16 ? 16 : (D <= 32 ? 32 : 64); }
__host__ __device__ constexpr int vd_lgq(int Dq) { return Dq == 16 ? 4 : (Dq == 32 ? 5 : 6); }
__host__ __device__ constexpr int vd_max(int a, int b) { return a > b ? a : b; }

// Column means of Z / l in the forward's order: 8 partial sums per column over rows m = k mod 8,
// then k ascending. Every thread of the workgroup calls it; scr holds 8 * Dq floats.
GPK_DEVICE void vd_col_means(const float* Z, int M, int D, int Dq, const float* lsc, float* scr, float* cm,
                             int tid) {
  for (int e = tid; e < 8 * Dq; e += 256) {
    const int d = e % Dq, k = e / Dq;
    float s = 0.f;
    if (d < D) {
      const float l = lsc[d];
#pragma unroll 4
      for (int m = k; m < M; m += 8) s += Z[(size_t)m * D + d] / l;
    }
    scr[e] = s;
  }
  lds_barrier();
  if (tid < 64) {
    float s = 0.f;
    if (tid < Dq) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s += scr[k * Dq + tid];
    }
    cm[tid] = tid < D ? s / (float)M : 0.f;
  }
  lds_barrier();
}

// Column block cb's 64 points of a window, scaled, centred by the inducing mean cm, zero padded
// -> xs (64 x ds, ds = Dq + 4), and their squared norms by fma over the padded D -> xn. Every
// thread calls it; the caller's next barrier publishes xn.
GPK_DEVICE void vd_stage_points(const float* Xb, int N, int D, int Dq, int cb, const float* lsc, const float* cm,
                                float* xs, float* xn, int tid) {
  const int lgq = vd_lgq(Dq), ds = Dq + 4;
#pragma unroll 4
  for (int e = tid; e < kCB * Dq; e += 256) {
    const int j = e >> lgq, d = e & (Dq - 1);
    const int col = kCB * cb + j;
    const bool ok = d < D && col < N;
    const float v = Xb[ok ? (size_t)col * D + d : 0];
    xs[j * ds + d] = ok ? v / lsc[d] - cm[d] : 0.f;
  }
  lds_barrier();
  if (tid < 64) {
    float s = 0.f;
    for (int d = 0; d < Dq; ++d) s = __builtin_fmaf(xs[tid * ds + d], xs[tid * ds + d], s);
    xn[tid] = s;
  }
}

// Stage rows 16 kb .. 16 kb + 15 of L_q = tril(C), columns 0 .. 16 kb + 15, into Lp (row
// stride LS); entries above the diagonal and rows >= M are zeros. Every thread calls it.
GPK_DEVICE void vd_stage_panel(const float* C, int M, int kb, float* Lp, int LS, int tid) {
  const int nc = 16 * (kb + 1);
  for (int e = tid; e < 16 * nc; e += 256) {
    const int kk = e / nc, m = e - kk * nc;
    const int k = 16 * kb + kk;
    const bool ok = k < M && m <= k;
    const float v = C[ok ? (size_t)k * M + m : 0];
    Lp[kk * LS + m] = ok ? v : 0.f;
  }
}

// W = L_q^T A for this wave's 16 columns: acc[mt][r] = W[16 mt + 4 g + r][16 w + c]. Al holds A
// (MP x kKS, rows >= M zero); L_q goes through Lp in 16-row panels, panel kb feeds the row tiles
// mt <= kb (the structurally zero tiles are never touched). Lane (g, c) feeds, in MFMA step u of
// panel kb, the A operand L_q[16 kb + 4 g + u][16 mt + c] and the B operand
// A[16 kb + 4 g + u][16 w + c]. Every thread calls it; it opens with a barrier (A is complete,
// whatever lay under Lp is free).
GPK_DEVICE void vd_w_pass(f32x4 (&acc)[16], const float* Al, float* Lp, const float* C, int M, int MB,
                          int LS, int tid, int w, int c, int g) {
#pragma unroll
  for (int mt = 0; mt < 16; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < MB; ++kb) {
    lds_barrier();   // the previous panel's reads are done
    vd_stage_panel(C, M, kb, Lp, LS, tid);
    lds_barrier();
    float bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) bv[u] = Al[(size_t)(16 * kb + 4 * g + u) * kKS + 16 * w + c];
#pragma unroll
    for (int mt = 0; mt < 16; ++mt) {
      if (mt > kb) continue;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Lp[(4 * g + u) * LS + 16 * mt + c], bv[u], acc[mt], 0, 0, 0);
    }
  }
}

// Row tile mt of Y = L_q P for this wave's 16 columns, P (MP x kKS) in LDS: stages panel mt of
// L_q into Lp (between two barriers: the previous panel's reads are done, first pass: P is
// written), which feeds the tiles kb <= mt of P. Lane (g, c) feeds the A operand
// L_q[16 mt + c][16 kb + 4 g + u] and the B operand P[16 kb + 4 g + u][16 w + c]; returns
// y[r] = Y[16 mt + 4 g + r][16 w + c]. Every thread calls it, mt ascending; the epilogue is
// the caller's.
GPK_DEVICE f32x4 vd_lq_row_tile(const float* C, int M, int mt, float* Lp, int LS, const float* Pl, int tid,
                                int w, int c, int g) {
  lds_barrier();
  vd_stage_panel(C, M, mt, Lp, LS, tid);
  lds_barrier();
  f32x4 y = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb <= mt; ++kb) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      y = __builtin_amdgcn_mfma_f32_16x16x4f32(Lp[c * LS + 16 * kb + 4 * g + u],
                                               Pl[(size_t)(16 * kb + 4 * g + u) * kKS + 16 * w + c], y, 0, 0, 0);
  }
  return y;
}

// One 64 x 64 block of the lower triangle of sum_b P_b Q_b^T in fp64 (mfma_f64_16x16x4f64 from
// two LDS panels), one partial per split of the windows: workgroup blockIdx.x = (split sp, block
// pair (bi, bj), bj <= bi), windows sp WS .. min(B, (sp + 1) WS) - 1 ascending, the N columns 64
// at a time. P / Q: window 0's panel (M rows used, row stride as, columns >= N masked), pstride /
// qstride floats to the next window's. Cp: the first split's M x M partial (the splits follow
// each other); entries outside the lower blocks are not written.
GPK_DEVICE void vd_lower_gram(const float* P, size_t pstride, const float* Q, size_t qstride, int as, int N,
                              int M, int B, int WS, int npairs, double* Cp) {
  __shared__ float LA[64 * kKS];
  __shared__ float LB[64 * kKS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int sp = blockIdx.x / npairs;
  int pr = blockIdx.x - sp * npairs;
  int bi = 0;
  while (pr > bi) { pr -= bi + 1; ++bi; }
  const int bj = pr;   // bj <= bi
  const int b0 = sp * WS;
  const int b1 = b0 + WS < B ? b0 + WS : B;
  Cp += (size_t)sp * M * M;

  f64x4 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int b = b0; b < b1; ++b) {
    const float* Ab = P + (size_t)b * pstride;
    const float* Wb = Q + (size_t)b * qstride;
    for (int i0 = 0; i0 < N; i0 += 64) {
      lds_barrier();
#pragma unroll 4
      for (int e = tid; e < 64 * 64; e += 256) {
        const int r = e >> 6, j = e & 63;
        const int col = i0 + j, ma = 64 * bi + r, mb = 64 * bj + r;
        const bool oka = ma < M && col < N, okb = mb < M && col < N;
        const float va = Ab[oka ? (size_t)ma * as + col : 0];
        const float vb = Wb[okb ? (size_t)mb * as + col : 0];
        LA[r * kKS + j] = oka ? va : 0.f;
        LB[r * kKS + j] = okb ? vb : 0.f;
      }
      lds_barrier();
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const double av = (double)LA[(16 * w + c) * kKS + 4 * kk + g];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, (double)LB[(16 * ct + c) * kKS + 4 * kk + g],
                                                         acc[ct], 0, 0, 0);
      }
    }
  }
  // acc[ct][r] = block[16 w + g + 4 r][16 ct + c]
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 64 * bi + 16 * w + g + 4 * r, col = 64 * bj + 16 * ct + c;
      if (row < M && col < M) Cp[(size_t)row * M + col] = acc[ct][r];
    }
}

}  // namespace
