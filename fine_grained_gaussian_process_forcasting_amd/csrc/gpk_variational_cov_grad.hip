// Adjoint of the dense covariance of a variational q(f) (gpk_variational_cov.hip) for gfx950.
//
// Replaces the torch autograd backward of the dense restatement of upstream
// variational/variational_strategy.py predictive_covar, which train.py:166 runs through the
// skip-input draw of denoising_model/DeepGP.py:62-64 (x.rsample() of a multi-output layer).
//
// Per window b, from g = dObjective / dcov (any N x N matrix), H = g + g^T, w_m = vstd_m^2 - 1 and
// the forward's A = L^{-1} K_ZX (fp32, kept by the caller: the forward's workspace):
//   T = A H            dw_m = 1/2 sum_i T_mi A_mi        dA = diag(w) T
//   dLinv = tril(sum_b dA K_ZX^T)                        Q = (L^{-T} dA) o K_ZX
//   U_md = sum_{b,i} Q_mi (zt_md - xt_id)                V_id = sum_m Q_mi (zt_md - xt_id)
//   P = H o K_XX (diagonal apart: K_ii = s2)             W_id = sum_j P_ij (xh_id - xh_jd)
//   dZ = -U / l     dX = (V - W) / l     dl_d = (sum zt U - sum xt V + sum xh W)_d / l_d
//   ds2 = (sum Q + sum_ij g_ij K_ij) / s2                dvstd_m = 2 vstd_m sum_b dw_m
// zt, xt: z / l and x / l centred by the column means of Z / l, xh: x / l centred by the window's
// own mean (the forward's centring: the differences never see the offset of the inputs). The
// jitter has no gradient; the clamp of d2 at 0 has none either (its factor x_i - x_j vanishes).
//
// Kernels (output o on grid y of each; all MFMA operands follow gpk_common.h's acc layout):
//   t    one workgroup per (window, 64 rows of A): T on mfma_f32_16x16x4f32 over 16-row chunks of
//        H staged in LDS from g and g^T; dw row partials; dA -> workspace.
//   q    one workgroup per (chunk of windows, 64-point column block): K_ZX block with the
//        forward's fp32 Gram arithmetic (-> workspace for dlinv), dK = L^{-T} dA on the fp32
//        MFMA (L^{-1} cast on load, its zero blocks skipped), Q in place over K in LDS, then
//        Q x, Q^T z and the row / column sums of Q (a ones operand) on the MFMA; writes this
//        part of dX and per-workgroup partials of U, sum Q and sum xt V.
//   dlinv one workgroup per (64 x 64 block of the lower triangle, split of the windows):
//        vd_lower_gram on dA and K_ZX, fp64 partial per split.
//   kxx  one workgroup per (chunk of windows, 64-row tile row of cov): K_XX tile by tile as the
//        forward's phase 2 computes it, P in LDS, P x and the row sums on the MFMA; subtracts its
//        part from dX (this launch follows q on the stream) and writes partials of dl and ds2.
//   reduce / finish: every partial summed in fp64 in a fixed order.
// No atomics, no host synchronisation, fixed summation orders: two launches give the same bits;
// a window's dX comes from that window's data alone; the chunking depends on (B, N, M, D) only,
// so output o of a batched launch has the bits of a single-output call.
// The blocks this unit runs together with the forward and the Cholesky units -- constants,
// column means, point staging, the fp64 lower-block Gram of dlinv -- are gpk_var_dense.h's and are
// described there.
#include "gpk_common.h"
#include "gpk_variational_cov_grad.h"
#include "gpk_var_dense.h"

#include <mutex>

namespace {

constexpr int kMaxN = 256;

// Workspace slice of one output (byte offsets, each a multiple of 16) and the work split.
struct VcgPlan {
  int as, MP, Dq, ncb;
  int WC, nchunk;        // windows per workgroup of q / kxx, number of such chunks
  int WS, nsplit;        // windows per split of dlinv, number of splits
  int npairs;            // 64 x 64 blocks in the lower triangle of dLinv
  size_t off_dp, off_uz, off_qt, off_dA, off_K, off_dw, off_up, off_qr, off_xv, off_cp, total;
};

__host__ VcgPlan vcg_plan(int B, int N, int M, int D) {
  VcgPlan p;
  p.as = (N + 63) / 64 * 64;
  p.MP = (M + 15) & ~15;
  p.Dq = vd_dq(D);
  p.ncb = (N + kCB - 1) / kCB;
  p.WC = B > 64 ? (B + 63) / 64 : 1;
  p.nchunk = B > 0 ? (B + p.WC - 1) / p.WC : 0;
  const GpkVarGramSplit sp = gpk_var_gram_split(B, M);
  p.WS = sp.WS;
  p.nsplit = sp.nsplit;
  p.npairs = sp.npairs;
  size_t off = 0;
  p.off_dp = off; off = gpk_up16(off + (size_t)p.nsplit * M * M * sizeof(double));
  p.off_uz = off; off = gpk_up16(off + (size_t)M * 64 * sizeof(double));
  p.off_qt = off; off = gpk_up16(off + (size_t)M * sizeof(double));
  p.off_dA = off; off = gpk_up16(off + (size_t)B * M * p.as * sizeof(float));
  p.off_K = off;  off = gpk_up16(off + (size_t)B * M * p.as * sizeof(float));
  p.off_dw = off; off = gpk_up16(off + (size_t)B * M * sizeof(float));
  const size_t nwg = (size_t)p.nchunk * p.ncb;
  p.off_up = off; off = gpk_up16(off + nwg * p.MP * p.Dq * sizeof(float));
  p.off_qr = off; off = gpk_up16(off + nwg * p.MP * sizeof(float));
  p.off_xv = off; off = gpk_up16(off + nwg * 64 * sizeof(float));
  p.off_cp = off; off = gpk_up16(off + nwg * 128 * sizeof(float));
  p.total = off;
  return p;
}

struct VcgArgs {
  GpkVarCovGradArgs a;
  VcgPlan p;
  long long state_stride;   // floats between two outputs' forward workspaces
  size_t ws_stride;         // bytes between two outputs' workspace slices (>= p.total)
  int dpar_stride;          // floats between two outputs' dpar rows (>= M + 1 + D)
};

template <typename T>
GPK_DEVICE T* vcg_ws(const VcgArgs& k, size_t o, size_t off) {
  return (T*)((char*)k.a.ws + o * k.ws_stride + off);
}

// Row tile of the mi-th tile a wave owns: 0 1 2 3 3 2 1 0 0 1 2 3 3 2 1 0 over the waves (the
// triangular dK product of tile row mt costs MB - mt tile products).
GPK_DEVICE int vcg_row_tile(int mi, int w) { return 8 * (mi >> 1) + ((mi & 1) ? 7 - w : w); }

// ------------------------------------------------------------------------------------------------
// t: T = A H, dw, dA. The H-chunk staging and the accumulation are the text of gpk_vcc_t_kernel
// (gpk_var_chol_cov.hip, R = 2 M rows): as one function that kernel spills 21 SGPRs instead of
// 22, so both stay in line; edit them together.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcg_t_kernel(VcgArgs k) {
  __shared__ float Hs[16 * kHS];
  const int N = k.a.N, M = k.a.M, as = k.p.as;
  const int NP = (N + 15) & ~15, nct = NP >> 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int nrb = (M + 63) / 64;
  const int b = blockIdx.x / nrb, rb = blockIdx.x - b * nrb;
  const size_t o = blockIdx.y;

  const float* A = k.a.state + o * (size_t)k.state_stride + (size_t)b * M * as;
  const float* G = k.a.gcov + (o * (size_t)k.a.B + b) * (size_t)N * N;
  const float* vstd = k.a.vstd + o * (size_t)M;
  float* dA = vcg_ws<float>(k, o, k.p.off_dA) + (size_t)b * M * as;
  float* dwp = vcg_ws<float>(k, o, k.p.off_dw) + (size_t)b * M;

  const int m = 64 * rb + 16 * w + c;   // the A operand's row
  const float* Arow = A + (size_t)(m < M ? m : 0) * as;
  f32x4 acc[16];
#pragma unroll
  for (int ct = 0; ct < 16; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < N; j0 += 16) {
    lds_barrier();   // the previous chunk's reads are done
    for (int e = tid; e < 16 * NP; e += 256) {   // g[j][i], rows of g
      const int jj = e / NP, i = e - jj * NP;
      const int j = j0 + jj;
      const bool ok = j < N && i < N;
      const float v = G[ok ? (size_t)j * N + i : 0];
      Hs[jj * kHS + i] = ok ? v : 0.f;
    }
    lds_barrier();
    for (int e = tid; e < 16 * NP; e += 256) {   // + g[i][j], 16 consecutive floats of a row of g
      const int jj = e & 15, i = e >> 4;
      const int j = j0 + jj;
      if (j < N && i < N) Hs[jj * kHS + i] += G[(size_t)i * N + j];
    }
    lds_barrier();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int j = j0 + 4 * kk + g;
      const bool ok = m < M && j < N;
      const float ld = Arow[ok ? j : 0];
      const float av = ok ? ld : 0.f;
      const float* hb = Hs + (4 * kk + g) * kHS + c;
#pragma unroll
      for (int ct = 0; ct < 16; ++ct)
        if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, hb[16 * ct], acc[ct], 0, 0, 0);
    }
  }

  // acc[ct][r] = T[64 rb + 16 w + 4 g + r][16 ct + c]
  float dwr[4] = {0.f, 0.f, 0.f, 0.f};
  float wv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int mr = 64 * rb + 16 * w + 4 * g + r;
    const float s = vstd[mr < M ? mr : 0];
    wv[r] = s * s - 1.f;
  }
#pragma unroll
  for (int ct = 0; ct < 16; ++ct) {
    if (ct >= nct) continue;
    const int col = 16 * ct + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = 64 * rb + 16 * w + 4 * g + r;
      if (mr < M && col < N) {
        dwr[r] = __builtin_fmaf(acc[ct][r], A[(size_t)mr * as + col], dwr[r]);
        dA[(size_t)mr * as + col] = wv[r] * acc[ct][r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = dwr[r];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
    const int mr = 64 * rb + 16 * w + 4 * g + r;
    if (c == 0 && mr < M) dwp[mr] = 0.5f * v;
  }
}

// ------------------------------------------------------------------------------------------------
// q: K_ZX, dK, Q and its contractions with the inputs
// ------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void gpk_vcg_q_kernel(VcgArgs k) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int Dq = 16 * DT, ds = Dq + 4, lgq = DT == 1 ? 4 : (DT == 2 ? 5 : 6);
  const int N = k.a.N, M = k.a.M, D = k.a.D, B = k.a.B, as = k.p.as;
  const int MP = k.p.MP, MB = MP >> 4;
  float* Kl = lds;                       // MP x kKS
  float* zs = Kl + (size_t)MP * kKS;     // 64 x ds
  float* xs = zs + 64 * ds;              // 64 x ds
  float* zn = xs + 64 * ds;              // 64
  float* xn = zn + 64;                   // 64
  float* cm = xn + 64;                   // 64
  float* lsc = cm + 64;                  // 64
  float* scr = lsc + 64;                 // 512

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int ncb = k.p.ncb;
  const int chunk = blockIdx.x / ncb, cb = blockIdx.x - chunk * ncb;
  const size_t o = blockIdx.y;
  const int b0 = chunk * k.p.WC;
  const int b1 = b0 + k.p.WC < B ? b0 + k.p.WC : B;

  const float* hyp = k.a.hyp + o * (size_t)(4 + 2 * D);
  const float* Z = k.a.Z + o * (size_t)M * D;
  const double* Linv = k.a.Linv + o * (size_t)M * M;
  const float s2 = hyp[0];

  if (tid < 64) lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
  lds_barrier();
  vd_col_means(Z, M, D, Dq, lsc, scr, cm, tid);

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 accU[4][DT], accQr[4];
  float accXV[DT];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    accQr[mi] = zero4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) accU[mi][dt] = zero4;
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) accXV[dt] = 0.f;

  for (int b = b0; b < b1; ++b) {
    const float* Xb = k.a.X + o * (size_t)k.a.x_stride + (size_t)b * N * D;
    const float* dAb = vcg_ws<float>(k, o, k.p.off_dA) + (size_t)b * M * as;
    float* Kb = vcg_ws<float>(k, o, k.p.off_K) + (size_t)b * M * as;
    float* dXb = k.a.dX + (o * (size_t)B + b) * (size_t)N * D;

    lds_barrier();   // the previous window's reads of xs and Kl are done
    vd_stage_points(Xb, N, D, Dq, cb, lsc, cm, xs, xn, tid);
    // ---- K_ZX block, 64 inducing rows at a time (the forward's arithmetic): in line (the text of
    //      gpk_var_cov_a_kernel's with Dq at compile time), as a function it moves q<2>'s VGPR count
    //      264 -> 268 and SGPR spills
    for (int r0 = 0; r0 < MP; r0 += 64) {
      lds_barrier();
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
        f32x4 acc = zero4;
#pragma unroll
        for (int kk = 0; kk < Dq / 4; ++kk)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(za[4 * kk], xb[4 * kk], acc, 0, 0, 0);
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

    // ---- K_ZX -> workspace (dlinv reads it); columns >= N hold zeros
    for (int e = tid; e < M * kCB; e += 256) {
      const int m = e >> 6, j = e & 63;
      Kb[(size_t)m * as + kCB * cb + j] = Kl[(size_t)m * kKS + j];
    }
    lds_barrier();   // before Q overwrites K

    // ---- dK = L^{-T} dA for the row tiles this wave owns, Q = dK o K in place
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int mt = vcg_row_tile(mi, w);
      if (mt >= MB) continue;
      f32x4 dk[4] = {zero4, zero4, zero4, zero4};
      const int mcol = 16 * mt + c;
      for (int kb = mt; kb < MB; ++kb) {
        float av[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kr = 16 * kb + 4 * g + u;
          const bool ok = kr < M && mcol < M;
          const double v = Linv[ok ? (size_t)kr * M + mcol : 0];
          av[u] = ok ? (float)v : 0.f;
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int col = kCB * cb + 16 * ct + c;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int kr = 16 * kb + 4 * g + u;
            const bool ok = kr < M && col < N;
            const float v = dAb[ok ? (size_t)kr * as + col : 0];
            dk[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], ok ? v : 0.f, dk[ct], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t idx = (size_t)(16 * mt + 4 * g + r) * kKS + 16 * ct + c;
          Kl[idx] = dk[ct][r] * Kl[idx];
        }
    }
    lds_barrier();

    // ---- U: Q x and the row sums of Q for the same row tiles, summed over the chunk's windows
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int mt = vcg_row_tile(mi, w);
      if (mt >= MB) continue;
      const float* qa = Kl + (size_t)(16 * mt + c) * kKS + g;
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const float av = qa[4 * kk];
        accQr[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accQr[mi], 0, 0, 0);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          accU[mi][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xs[(4 * kk + g) * ds + 16 * dt + c],
                                                              accU[mi][dt], 0, 0, 0);
      }
    }

    // ---- V: Q^T z and the column sums of Q for this wave's 16 points
    f32x4 accV[DT], accQs = zero4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) accV[dt] = zero4;
    for (int r0 = 0; r0 < MP; r0 += 64) {
      lds_barrier();   // the previous chunk's reads of zs are done
#pragma unroll 4
      for (int e = tid; e < 64 * Dq; e += 256) {
        const int r = e >> lgq, d = e & (Dq - 1);
        const int m = r0 + r;
        const bool ok = d < D && m < M;
        const float v = Z[ok ? (size_t)m * D + d : 0];
        zs[r * ds + d] = ok ? v / lsc[d] - cm[d] : 0.f;
      }
      lds_barrier();
      const int nk = ((MP - r0) >= 64 ? 64 : (MP - r0)) / 4;
      for (int kk = 0; kk < nk; ++kk) {
        const float av = Kl[(size_t)(r0 + 4 * kk + g) * kKS + 16 * w + c];
        accQs = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accQs, 0, 0, 0);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          accV[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, zs[(4 * kk + g) * ds + 16 * dt + c], accV[dt],
                                                          0, 0, 0);
      }
    }
    // accV[dt][r] = (Q^T zt)[16 w + 4 g + r][16 dt + c]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int d = 16 * dt + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * w + 4 * g + r;
        const int gi = kCB * cb + i;
        const float xv = xs[i * ds + d];
        const float v = accV[dt][r] - accQs[r] * xv;
        if (gi < N && d < D) dXb[(size_t)gi * D + d] = v / lsc[d];
        accXV[dt] = __builtin_fmaf(xv, v, accXV[dt]);
      }
    }
  }

  // ---- this workgroup's partials
  const size_t wg = blockIdx.x;
  float* Up = vcg_ws<float>(k, o, k.p.off_up) + wg * (size_t)MP * Dq;
  float* qrp = vcg_ws<float>(k, o, k.p.off_qr) + wg * (size_t)MP;
  float* xvp = vcg_ws<float>(k, o, k.p.off_xv) + wg * 64;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mt = vcg_row_tile(mi, w);
    if (mt >= MB) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = 16 * mt + 4 * g + r;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) Up[(size_t)mr * Dq + 16 * dt + c] = accU[mi][dt][r];
      if (c == 0) qrp[mr] = accQr[mi][r];
    }
  }
  lds_barrier();
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    float v = accXV[dt];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (g == 0) scr[w * 64 + 16 * dt + c] = v;
  }
  lds_barrier();
  if (tid < Dq) xvp[tid] = scr[tid] + scr[64 + tid] + scr[128 + tid] + scr[192 + tid];
}

size_t vcg_q_lds(int MP, int Dq) {
  return ((size_t)MP * kKS + 2 * 64 * (Dq + 4) + 4 * 64 + 512) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
// dlinv: fp64 partials of sum_b dA K_ZX^T
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcg_dlinv_kernel(VcgArgs k) {
  const int M = k.a.M, as = k.p.as;
  const size_t o = blockIdx.y;
  const size_t ws = (size_t)M * as;   // floats between two windows' panels
  vd_lower_gram(vcg_ws<float>(k, o, k.p.off_dA), ws, vcg_ws<float>(k, o, k.p.off_K), ws, as, k.a.N, M, k.a.B,
                k.p.WS, k.p.npairs, vcg_ws<double>(k, o, k.p.off_dp));
}

// ------------------------------------------------------------------------------------------------
// kxx: the K_XX part
// ------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void gpk_vcg_kxx_kernel(VcgArgs k) {
  constexpr int Dq = 16 * DT, ds = Dq + 4, lgq = DT == 1 ? 4 : (DT == 2 ? 5 : 6);
  __shared__ float xi[64 * ds];
  __shared__ float xj[64 * ds];
  __shared__ float Pl[64 * kKS];
  __shared__ float ni[64], nj[64], mu[64], lsc[64];
  __shared__ float scr[4 * 64 + 4];
  const int N = k.a.N, M = k.a.M, D = k.a.D, B = k.a.B, as = k.p.as;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int ncb = k.p.ncb;
  const int chunk = blockIdx.x / ncb, rt = blockIdx.x - chunk * ncb;
  const size_t o = blockIdx.y;
  const int b0 = chunk * k.p.WC;
  const int b1 = b0 + k.p.WC < B ? b0 + k.p.WC : B;
  const float* hyp = k.a.hyp + o * (size_t)(4 + 2 * D);
  const float s2 = hyp[0];
  const float* mus = k.a.state + o * (size_t)k.state_stride + (size_t)B * M * as;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  if (tid < 64) lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
  float accDl[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) accDl[dt] = 0.f;
  float accS = 0.f;

  for (int b = b0; b < b1; ++b) {
    const float* Xb = k.a.X + o * (size_t)k.a.x_stride + (size_t)b * N * D;
    const float* Gb = k.a.gcov + (o * (size_t)B + b) * (size_t)N * N;
    float* dXb = k.a.dX + (o * (size_t)B + b) * (size_t)N * D;
    lds_barrier();   // the previous window's reads are done (first pass: lsc is written)
    if (tid < 64) mu[tid] = tid < D ? mus[(size_t)b * 64 + tid] : 0.f;
    lds_barrier();
#pragma unroll 4
    for (int e = tid; e < 64 * Dq; e += 256) {
      const int r = e >> lgq, d = e & (Dq - 1);
      const int row = 64 * rt + r;
      const bool ok = d < D && row < N;
      const float v = Xb[ok ? (size_t)row * D + d : 0];
      xi[r * ds + d] = ok ? v / lsc[d] - mu[d] : 0.f;
    }
    lds_barrier();
    if (tid < 64) {
      float s = 0.f;
      for (int d = 0; d < Dq; ++d) s = __builtin_fmaf(xi[tid * ds + d], xi[tid * ds + d], s);
      ni[tid] = s;
    }
    f32x4 accPX[DT], accRs = zero4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) accPX[dt] = zero4;
    float diag = 0.f;

    for (int jb = 0; jb < ncb; ++jb) {
      lds_barrier();   // the previous block's reads of xj and Pl are done
#pragma unroll 4
      for (int e = tid; e < 64 * Dq; e += 256) {
        const int r = e >> lgq, d = e & (Dq - 1);
        const int row = 64 * jb + r;
        const bool ok = d < D && row < N;
        const float v = Xb[ok ? (size_t)row * D + d : 0];
        xj[r * ds + d] = ok ? v / lsc[d] - mu[d] : 0.f;
      }
      lds_barrier();
      if (tid < 64) {
        float s = 0.f;
        for (int d = 0; d < Dq; ++d) s = __builtin_fmaf(xj[tid * ds + d], xj[tid * ds + d], s);
        nj[tid] = s;
      }
      lds_barrier();
      // ---- P = H o K_XX for this wave's 16 columns of the block, the diagonal apart
      {
        const int jl = 16 * w + c, gj = 64 * jb + jl;
        const float njc = nj[jl];
        const float* xb = xj + jl * ds + g;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const float* xa = xi + (16 * it + c) * ds + g;
          f32x4 G = zero4;
#pragma unroll
          for (int kk = 0; kk < Dq / 4; ++kk)
            G = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[4 * kk], xb[4 * kk], G, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int il = 16 * it + 4 * g + r, gi = 64 * rt + il;
            const float d2 = __builtin_fmaxf(ni[il] + njc - 2.f * G[r], 0.f);
            const float kv = s2 * __builtin_amdgcn_exp2f(d2 * kNHalfLog2e);
            float p = 0.f;
            if (gi < N && gj < N) {
              const float h = Gb[(size_t)gi * N + gj] + Gb[(size_t)gj * N + gi];
              if (gi == gj) diag = __builtin_fmaf(0.5f * h, s2, diag);
              else p = h * kv;
            }
            Pl[il * kKS + jl] = p;
          }
        }
      }
      lds_barrier();
      // ---- P x and the row sums for this wave's 16 rows
      {
        const float* pa = Pl + (16 * w + c) * kKS + g;
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
          const float av = pa[4 * kk];
          accRs = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accRs, 0, 0, 0);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
            accPX[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xj[(4 * kk + g) * ds + 16 * dt + c],
                                                             accPX[dt], 0, 0, 0);
        }
      }
    }
    // ---- W = rowsum(P) o x - P x; dX -= W / l
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int d = 16 * dt + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = 16 * w + 4 * g + r, gi = 64 * rt + il;
        const float xv = xi[il * ds + d];
        const float wv = accRs[r] * xv - accPX[dt][r];
        if (gi < N && d < D) dXb[(size_t)gi * D + d] -= wv / lsc[d];
        accDl[dt] = __builtin_fmaf(xv, wv, accDl[dt]);
      }
    }
    if (c == 0) accS += 0.5f * (accRs[0] + accRs[1] + accRs[2] + accRs[3]);
    accS += diag;
  }

  // ---- this workgroup's partials: dl (Dq values) and ds2 * s2
  float* cp = vcg_ws<float>(k, o, k.p.off_cp) + (size_t)blockIdx.x * 128;
  lds_barrier();
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    float v = accDl[dt];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (g == 0) scr[w * 64 + 16 * dt + c] = v;
  }
  const float sw = wave_sum(accS);
  if (lane == 0) scr[256 + w] = sw;
  lds_barrier();
  if (tid < Dq) cp[tid] = scr[tid] + scr[64 + tid] + scr[128 + tid] + scr[192 + tid];
  if (tid == 64) cp[64] = scr[256] + scr[257] + scr[258] + scr[259];
}

// ------------------------------------------------------------------------------------------------
// reduce: dLinv, dZ, dvstd from the partials; finish: dl and ds2
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcg_reduce_kernel(VcgArgs k) {
  __shared__ float lsc[64], cm[64], scr[512];
  const int M = k.a.M, D = k.a.D, B = k.a.B;
  const int MP = k.p.MP, Dq = k.p.Dq;
  const int tid = threadIdx.x;
  const size_t o = blockIdx.y;
  const float* hyp = k.a.hyp + o * (size_t)(4 + 2 * D);
  const float* Z = k.a.Z + o * (size_t)M * D;
  if (tid < 64) lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
  lds_barrier();
  vd_col_means(Z, M, D, Dq, lsc, scr, cm, tid);

  const long long e = (long long)blockIdx.x * 256 + tid;
  const long long mm = (long long)M * M;
  if (e < mm) {
    const int m = (int)(e / M), kc = (int)(e - (long long)m * M);
    double s = 0.0;
    if (kc <= m) {
      const double* Dp = vcg_ws<double>(k, o, k.p.off_dp);
      for (int sp = 0; sp < k.p.nsplit; ++sp) s += Dp[(size_t)sp * mm + e];
    }
    k.a.dLinv[o * (size_t)mm + e] = s;
    return;
  }
  const long long e2 = e - mm;
  if (e2 >= (long long)MP * Dq) return;
  const int m = (int)(e2 / Dq), d = (int)(e2 - (long long)m * Dq);
  if (m >= M || d >= D) return;
  const int nwg = k.p.nchunk * k.p.ncb;
  const float* Up = vcg_ws<float>(k, o, k.p.off_up);
  const float* qrp = vcg_ws<float>(k, o, k.p.off_qr);
  double qx = 0.0, qr = 0.0;
  for (int wg = 0; wg < nwg; ++wg) {
    qx += Up[(size_t)wg * MP * Dq + e2];
    qr += qrp[(size_t)wg * MP + m];
  }
  const float l = lsc[d];
  const float zt = Z[(size_t)m * D + d] / l - cm[d];
  const double U = qr * (double)zt - qx;
  k.a.dZ[o * (size_t)M * D + (size_t)m * D + d] = (float)(-U / (double)l);
  vcg_ws<double>(k, o, k.p.off_uz)[(size_t)m * 64 + d] = (double)zt * U / (double)l;
  if (d == 0) {
    vcg_ws<double>(k, o, k.p.off_qt)[m] = qr;
    const float* dwp = vcg_ws<float>(k, o, k.p.off_dw);
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += dwp[(size_t)b * M + m];
    k.a.dpar[o * (size_t)k.dpar_stride + m] = (float)(2.0 * (double)k.a.vstd[o * (size_t)M + m] * s);
  }
}

__global__ __launch_bounds__(256) void gpk_vcg_finish_kernel(VcgArgs k) {
  __shared__ double sh[256];
  const int M = k.a.M, D = k.a.D;
  const int tid = threadIdx.x;
  const size_t o = blockIdx.y;
  const float* hyp = k.a.hyp + o * (size_t)(4 + 2 * D);
  const int nwg = k.p.nchunk * k.p.ncb;
  const double* uz = vcg_ws<double>(k, o, k.p.off_uz);
  const double* qt = vcg_ws<double>(k, o, k.p.off_qt);
  const float* xvp = vcg_ws<float>(k, o, k.p.off_xv);
  const float* cp = vcg_ws<float>(k, o, k.p.off_cp);
  float* dpar = k.a.dpar + o * (size_t)k.dpar_stride;

  // dl_d: four interleaved partial sums per dimension, then q ascending
  {
    const int d = tid & 63, q = tid >> 6;
    double s = 0.0;
    if (d < D) {
      for (int m = q; m < M; m += 4) s += uz[(size_t)m * 64 + d];
      double t = 0.0;
      for (int wg = q; wg < nwg; wg += 4) t += (double)cp[(size_t)wg * 128 + d] - (double)xvp[(size_t)wg * 64 + d];
      s += t / (double)hyp[4 + D + d];
    }
    sh[tid] = s;
    __syncthreads();
    if (tid < D) dpar[M + 1 + tid] = (float)(sh[tid] + sh[64 + tid] + sh[128 + tid] + sh[192 + tid]);
    __syncthreads();
  }
  // ds2: strided partial sums, then a fixed tree
  {
    double s = 0.0;
    for (int m = tid; m < M; m += 256) s += qt[m];
    for (int wg = tid; wg < nwg; wg += 256) s += (double)cp[(size_t)wg * 128 + 64];
    sh[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) sh[tid] += sh[tid + off];
      __syncthreads();
    }
    if (tid == 0) dpar[M] = (float)(sh[0] / (double)hyp[0]);
  }
}

bool vcg_shape_ok(int B, int N, int M, int D) {
  return B >= 0 && N >= 1 && N <= kMaxN && M >= 1 && M <= 256 && D >= 1 && D <= 64 &&
         (long long)B * 4 <= 0x7fffffffLL;   // t: B * ceil(M / 64) workgroups on grid x
}

}  // namespace

size_t gpk_var_cov_grad_ws_bytes(int B, int N, int M, int D) {
  if (!vcg_shape_ok(B, N, M, D)) return 0;
  return vcg_plan(B, N, M, D).total;
}

static void vcg_set_lds_once() {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)gpk_vcg_q_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)gpk_vcg_q_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)gpk_vcg_q_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipGetLastError();
  });
}

size_t gpk_var_cov_grad_tail_plan(int B, int N, int M, int D, size_t* off_dA, int* as) {
  if (!vcg_shape_ok(B, N, M, D)) return 0;
  const VcgPlan p = vcg_plan(B, N, M, D);
  if (off_dA != nullptr) *off_dA = p.off_dA;
  if (as != nullptr) *as = p.as;
  return p.total;
}

int gpk_launch_var_cov_grad_from_dA(const GpkVarCovGradArgs& a, size_t ws_stride, int dpar_stride,
                                    hipStream_t stream) {
  vcg_set_lds_once();
  if (!vcg_shape_ok(a.B, a.N, a.M, a.D) || a.O < 1 || a.O > 65535) return -9;
  VcgArgs k{a, vcg_plan(a.B, a.N, a.M, a.D), 0, ws_stride, dpar_stride};
  if (ws_stride < k.p.total || (ws_stride & 15) != 0 || dpar_stride < a.M + 1 + a.D) return -9;
  const unsigned O = (unsigned)a.O;
  const unsigned gq = (unsigned)(k.p.nchunk * k.p.ncb);
  const size_t lds = vcg_q_lds(k.p.MP, k.p.Dq);
  const long long nred = ((long long)a.M * a.M + (long long)k.p.MP * k.p.Dq + 255) / 256;
  // what t and kxx would have written: no dw, no K_XX partials. One strided fill each for all
  // the outputs' slices (the slice stride is the pitch), so the launch count does not grow with O.
  const size_t ndw = (size_t)a.B * a.M * sizeof(float), ncp = (size_t)gq * 128 * sizeof(float);
  hipError_t e;
  if (O == 1) {
    e = hipMemsetAsync((char*)a.ws + k.p.off_dw, 0, ndw, stream);
    if (e == hipSuccess) e = hipMemsetAsync((char*)a.ws + k.p.off_cp, 0, ncp, stream);
  } else {
    e = hipMemset2DAsync((char*)a.ws + k.p.off_dw, ws_stride, 0, ndw, O, stream);
    if (e == hipSuccess) e = hipMemset2DAsync((char*)a.ws + k.p.off_cp, ws_stride, 0, ncp, O, stream);
  }
  if (e != hipSuccess) return (int)e;
  if (k.p.Dq == 16) hipLaunchKernelGGL(gpk_vcg_q_kernel<1>, dim3(gq, O), dim3(256), lds, stream, k);
  else if (k.p.Dq == 32) hipLaunchKernelGGL(gpk_vcg_q_kernel<2>, dim3(gq, O), dim3(256), lds, stream, k);
  else hipLaunchKernelGGL(gpk_vcg_q_kernel<4>, dim3(gq, O), dim3(256), lds, stream, k);
  hipLaunchKernelGGL(gpk_vcg_dlinv_kernel, dim3((unsigned)(k.p.npairs * k.p.nsplit), O), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(gpk_vcg_reduce_kernel, dim3((unsigned)nred, O), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(gpk_vcg_finish_kernel, dim3(1, O), dim3(256), 0, stream, k);
  return (int)hipGetLastError();
}

int gpk_launch_var_cov_grad_from_dA_kxx(const GpkVarCovGradArgs& a, size_t ws_stride, int dpar_stride,
                                        long long state_stride, long long mu_offset, hipStream_t stream) {
  vcg_set_lds_once();
  if (!vcg_shape_ok(a.B, a.N, a.M, a.D) || a.O < 1 || a.O > 65535) return -9;
  VcgArgs k{a, vcg_plan(a.B, a.N, a.M, a.D), state_stride, ws_stride, dpar_stride};
  if (ws_stride < k.p.total || (ws_stride & 15) != 0 || dpar_stride < a.M + 1 + a.D) return -9;
  // kxx finds a window's means B * M * as floats into an output's state: hand it the base that
  // puts them at the caller's offset (it reads nothing else of the state)
  const long long own = (long long)a.B * a.M * k.p.as;
  if (a.state == nullptr || a.gcov == nullptr || mu_offset < own || state_stride < mu_offset + (long long)a.B * 64)
    return -9;
  k.a.state = a.state + (mu_offset - own);
  const unsigned O = (unsigned)a.O;
  const unsigned gq = (unsigned)(k.p.nchunk * k.p.ncb);
  const size_t lds = vcg_q_lds(k.p.MP, k.p.Dq);
  const long long nred = ((long long)a.M * a.M + (long long)k.p.MP * k.p.Dq + 255) / 256;
  // what t would have written: no dw (kxx writes every K_XX partial itself)
  const size_t ndw = (size_t)a.B * a.M * sizeof(float);
  const hipError_t e = O == 1 ? hipMemsetAsync((char*)a.ws + k.p.off_dw, 0, ndw, stream)
                              : hipMemset2DAsync((char*)a.ws + k.p.off_dw, ws_stride, 0, ndw, O, stream);
  if (e != hipSuccess) return (int)e;
  if (k.p.Dq == 16) hipLaunchKernelGGL(gpk_vcg_q_kernel<1>, dim3(gq, O), dim3(256), lds, stream, k);
  else if (k.p.Dq == 32) hipLaunchKernelGGL(gpk_vcg_q_kernel<2>, dim3(gq, O), dim3(256), lds, stream, k);
  else hipLaunchKernelGGL(gpk_vcg_q_kernel<4>, dim3(gq, O), dim3(256), lds, stream, k);
  hipLaunchKernelGGL(gpk_vcg_dlinv_kernel, dim3((unsigned)(k.p.npairs * k.p.nsplit), O), dim3(256), 0, stream, k);
  if (k.p.Dq == 16) hipLaunchKernelGGL(gpk_vcg_kxx_kernel<1>, dim3(gq, O), dim3(256), 0, stream, k);
  else if (k.p.Dq == 32) hipLaunchKernelGGL(gpk_vcg_kxx_kernel<2>, dim3(gq, O), dim3(256), 0, stream, k);
  else hipLaunchKernelGGL(gpk_vcg_kxx_kernel<4>, dim3(gq, O), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(gpk_vcg_reduce_kernel, dim3((unsigned)nred, O), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(gpk_vcg_finish_kernel, dim3(1, O), dim3(256), 0, stream, k);
  return (int)hipGetLastError();
}

int gpk_launch_var_cov_grad(const GpkVarCovGradArgs& a, hipStream_t stream) {
  vcg_set_lds_once();
  if (!vcg_shape_ok(a.B, a.N, a.M, a.D)) return -9;
  VcgArgs k{a, vcg_plan(a.B, a.N, a.M, a.D), 0, 0, a.M + 1 + a.D};
  k.ws_stride = k.p.total;
  k.state_stride = (long long)a.B * a.M * k.p.as + (long long)a.B * 64;
  const unsigned O = (unsigned)a.O;
  const int nrb = (a.M + 63) / 64;
  const unsigned gq = (unsigned)(k.p.nchunk * k.p.ncb);
  const size_t lds = vcg_q_lds(k.p.MP, k.p.Dq);
  const long long nred = ((long long)a.M * a.M + (long long)k.p.MP * k.p.Dq + 255) / 256;

  hipLaunchKernelGGL(gpk_vcg_t_kernel, dim3((unsigned)(a.B * nrb), O), dim3(256), 0, stream, k);
  if (k.p.Dq == 16) hipLaunchKernelGGL(gpk_vcg_q_kernel<1>, dim3(gq, O), dim3(256), lds, stream, k);
  else if (k.p.Dq == 32) hipLaunchKernelGGL(gpk_vcg_q_kernel<2>, dim3(gq, O), dim3(256), lds, stream, k);
  else hipLaunchKernelGGL(gpk_vcg_q_kernel<4>, dim3(gq, O), dim3(256), lds, stream, k);
  hipLaunchKernelGGL(gpk_vcg_dlinv_kernel, dim3((unsigned)(k.p.npairs * k.p.nsplit), O), dim3(256), 0, stream, k);
  if (k.p.Dq == 16) hipLaunchKernelGGL(gpk_vcg_kxx_kernel<1>, dim3(gq, O), dim3(256), 0, stream, k);
  else if (k.p.Dq == 32) hipLaunchKernelGGL(gpk_vcg_kxx_kernel<2>, dim3(gq, O), dim3(256), 0, stream, k);
  else hipLaunchKernelGGL(gpk_vcg_kxx_kernel<4>, dim3(gq, O), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(gpk_vcg_reduce_kernel, dim3((unsigned)nred, O), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(gpk_vcg_finish_kernel, dim3(1, O), dim3(256), 0, stream, k);
  return (int)hipGetLastError();
}
