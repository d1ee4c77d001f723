// Cholesky (full-covariance) q(u) = N(m, L_q L_q^T) of the whitened variational GP for gfx950:
// predictive mean / variance, their adjoint, and KL(q || N(0, I)).
//
// Replaces upstream variational/cholesky_variational_distribution.py (q(u) with
// chol_variational_covar, L_q = tril(C)) inside variational/variational_strategy.py forward and
// _variational_strategy.py::kl_divergence, reached from denoising_model/DeepGP.py:28-38 when the
// distribution class is swapped, and the autograd backward through them.
//
// Per window b, with A = L^{-1} K_ZX (fp64 solve, fp32 result) as gpk_variational_f32 forms it:
//   W = L_q^T A          mean_i = a_i^T m + x_i.w + b0
//   var_i = s2 + jitter - sum_m A_mi^2 + sum_m W_mi^2     (clamped at 1e-6, flag bit 0)
// and for the objective sum gmean mean + sum gvar var (gvar zeroed where the clamp fired):
//   dA = gmean_i m + 2 gvar_i (L_q w_i - a_i)      dm = sum gmean_i a_i
//   dC = 2 tril(sum gvar_i a_i w_i^T)              ds2 += sum gvar
// From dA on the adjoint is the pipeline of gpk_variational_cov_grad.hip (q, dlinv, reduce,
// finish), which this unit launches on the dA it writes into that pipeline's workspace.
//
// Kernels (all MFMA operands follow gpk_common.h's acc layout):
//   fwd   one workgroup of 4 waves per (window, 64-point column block), shaped like phase 1 of
//         gpk_variational_cov.hip: the K_ZX block with the forward's fp32 Gram arithmetic and
//         centring, A = L^{-1} K_ZX on mfma_f64_16x16x4f64 written over K in LDS (row tiles
//         descending: tile rt reads the K tiles <= rt only), W = L_q^T A on mfma_f32_16x16x4f32
//         with L_q staged through LDS in 16-row panels (panel kb feeds the row tiles mt <= kb:
//         the structurally zero tiles are never touched), W kept in registers; the column sums
//         of A^2, W^2 and A^T m finish the 64 points. With `saved`: A (B, M, as) and the mask.
//   da    one workgroup per (window, 64-point block): reads the saved A, recomputes W (same
//         panel loop), writes W diag(gvar) for the Gram kernel, forms Y = L_q W row tile by row
//         tile (panel mt feeds the W tiles kb <= mt) and dA into the shared pipeline's
//         workspace; row partials of dm, sum gvar, sum gmean and X^T gmean.
//   gram  one workgroup per (64 x 64 block of the lower triangle, split of the windows):
//         vd_lower_gram on A and W diag(gvar), fp64 partials.
//   finish  every partial summed in fp64 in a fixed order; dX += gmean_i w.
//   kl    one launch each way, the M^2 sum in a fixed order.
// O outputs of a multi-output layer run with the output index on grid y of every launch: a
// workgroup offsets its base pointers (X by x_stride, 0 when the inputs are shared; Z, Linv, m, C,
// hyp, the saved state, the workspace slice and every output array by their dense leading O) and
// is otherwise the single-output workgroup, so output o has the bits of a single-output call.
// No atomics in any sum, fixed summation orders: two launches give the same bits; a window's
// mean / var / dX come from that window's data alone.
// The blocks this unit runs together with the dense-covariance units -- constants, column means,
// point staging, the L_q panel staging, the W pass, the Y row tile, the fp64 lower-block Gram --
// are gpk_var_dense.h's and are described there.
#include "gpk_common.h"
#include "gpk_var_chol.h"
#include "gpk_var_dense.h"
#include "gpk_variational_cov_grad.h"

#include <mutex>

namespace {

constexpr float kMinVar = 1e-6f;

// ------------------------------------------------------------------------------------------------
// fwd
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vchol_fwd_kernel(GpkVarCholArgs a, int as) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.N, M = a.M, D = a.D;
  const int MP = (M + 15) & ~15, MB = MP >> 4;
  const int Dq = vd_dq(D);
  const int lgq = vd_lgq(Dq);
  const int ds = Dq + 4;                 // LDS row stride of the staged z / x rows
  const int LS = MP + 4;                 // LDS row stride of an L_q panel
  const int nst = vd_max(2 * 64 * ds, 16 * LS);
  float* Kl = lds;                       // MP x kKS: K_ZX, then A
  float* zs = Kl + (size_t)MP * kKS;     // 64 x ds   } the L_q panel (16 x LS) lies over
  float* xs = zs + 64 * ds;              // 64 x ds   } these two once K_ZX is formed
  float* Lp = zs;
  float* zn = zs + nst;                  // 64
  float* xn = zn + 64;                   // 64
  float* cm = xn + 64;                   // 64
  float* lsc = cm + 64;                  // 64
  float* lin = lsc + 64;                 // 64: x_i . w
  float* w2 = lin + 64;                  // 64: column sums of W^2
  float* scr = w2 + 64;                  // 512
  float* vm = scr + 512;                 // MP

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int ncb = (N + kCB - 1) / kCB;
  const int b = blockIdx.x / ncb, cb = blockIdx.x - b * ncb;

  // output o: only the base pointers move, the workgroup's body is the single-output one
  const size_t o = blockIdx.y;
  const float* hyp = a.hyp + o * (size_t)(4 + 2 * D);
  const float* Xb = a.X + o * (size_t)a.x_stride + (size_t)b * N * D;
  const float* Z = a.Z + o * (size_t)M * D;
  const double* Linv = a.Linv + o * (size_t)M * M;
  const float* vmean = a.vmean + o * (size_t)M;
  const float* vchol = a.vchol + o * (size_t)M * M;
  float* saved = a.saved != nullptr ? a.saved + o * ((size_t)a.B * M * as + (size_t)a.B * as) : nullptr;
  float* meanb = a.mean + (o * (size_t)a.B + b) * (size_t)N;
  float* varb = a.var + (o * (size_t)a.B + b) * (size_t)N;
  const float s2 = hyp[0], jit = hyp[2], b0 = hyp[3];

  if (tid < 64) lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
  for (int m = tid; m < MP; m += 256) vm[m] = m < M ? vmean[m] : 0.f;
  if (tid >= 64 && tid < 128) {   // the linear mean of this block's points
    const int j = tid - 64, col = kCB * cb + j;
    float s = 0.f;
    if (col < N)
      for (int d = 0; d < D; ++d) s = __builtin_fmaf(Xb[(size_t)col * D + d], hyp[4 + d], s);
    lin[j] = s;
  }
  lds_barrier();

  vd_col_means(Z, M, D, Dq, lsc, scr, cm, tid);
  vd_stage_points(Xb, N, D, Dq, cb, lsc, cm, xs, xn, tid);
  // ---- K_ZX block, 64 inducing rows at a time: in line (the text of gpk_var_cov_a_kernel's), as a
  //      function it moves this kernel's VGPR count 188 -> 180
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

  // ---- A = L^{-1} K_ZX for this wave's 16 columns (in line in the three forward kernels, see
  //      gpk_variational_cov.hip's head), written over K: row tile rt contracts the
  //      K tiles kb <= rt, so the tiles go in descending order and a finished tile of A is never
  //      read as K again
  float* Aw = saved != nullptr ? saved + (size_t)b * M * as : nullptr;
  float* Kc = Kl + 16 * w + c;
  for (int rt = MB - 1; rt >= 0; --rt) {
    const int m = 16 * rt + c;
    const double* row = Linv + (size_t)(m < M ? m : 0) * M;
    // four k blocks' operands (16 loads per lane) are in flight together and the next four are
    // loaded under these MFMAs: with one workgroup per CU at M = 256 nothing else hides the L2
    // latency of a dependent load per block
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
      const float v = (float)acc[r];
      Kc[(size_t)mr * kKS] = v;   // rows >= M: L^{-1}'s row was masked, v = 0
      if (Aw != nullptr && mr < M) Aw[(size_t)mr * as + kCB * cb + 16 * w + c] = v;
    }
  }

  // ---- W = L_q^T A (the pass opens with a barrier: A is complete, zs / xs are free)
  f32x4 accW[16];
  vd_w_pass(accW, Kl, Lp, vchol, M, MB, LS, tid, w, c, g);
  {
    float s = 0.f;
#pragma unroll
    for (int mt = 0; mt < 16; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) s = __builtin_fmaf(accW[mt][r], accW[mt][r], s);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (g == 0) w2[16 * w + c] = s;
  }

  // ---- column sums of A^2 and A^T m: four interleaved partial sums per column, then q ascending
  {
    const int j = lane, q = w;
    float sa = 0.f, sm = 0.f;
    for (int m = q; m < M; m += 4) {
      const float v = Kl[(size_t)m * kKS + j];
      sa = __builtin_fmaf(v, v, sa);
      sm = __builtin_fmaf(v, vm[m], sm);
    }
    scr[q * 64 + j] = sa;
    scr[256 + q * 64 + j] = sm;
  }
  lds_barrier();
  int clamped = 0;
  if (tid < 64) {
    const int col = kCB * cb + tid;
    const float sa = (scr[tid] + scr[64 + tid]) + (scr[128 + tid] + scr[192 + tid]);
    const float sm = (scr[256 + tid] + scr[320 + tid]) + (scr[384 + tid] + scr[448 + tid]);
    float var_i = (s2 + jit) - sa + w2[tid];
    const bool clamp = var_i < kMinVar;
    if (col < N) {
      if (clamp) { var_i = kMinVar; clamped = 1; }   // MVN.variance clamp (fp32)
      meanb[col] = sm + (lin[tid] + b0);
      varb[col] = var_i;
    }
    // the clamp passes no gradient: the adjoint masks gvar with this (padding: 0)
    if (saved != nullptr)
      saved[(size_t)a.B * M * as + (size_t)b * as + col] = (col < N && !clamp) ? 1.f : 0.f;
  }
  if (a.flags != nullptr && clamped)
    (void)__hip_atomic_fetch_or(a.flags, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

size_t vch_fwd_lds(int M, int D) {
  const int MP = (M + 15) & ~15;
  const int nst = vd_max(2 * 64 * (vd_dq(D) + 4), 16 * (MP + 4));
  return ((size_t)MP * kKS + nst + 6 * 64 + 512 + MP) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
// Adjoint: workspace plan (byte offsets, each a multiple of 16)
// ------------------------------------------------------------------------------------------------
struct VchPlan {
  int as, MP, ncb;
  int WS, nsplit, npairs;   // windows per split of gram, number of splits, 64 x 64 lower blocks
  size_t off_dA;            // inside the shared pipeline's slice (which starts at byte 0)
  size_t off_wg, off_dm, off_xg, off_sc, off_cp, total;
};

__host__ VchPlan vch_plan(int B, int N, int M, int D) {
  VchPlan p;
  size_t off_dA = 0;
  int as = 0;
  const size_t tail = gpk_var_cov_grad_tail_plan(B, N, M, D, &off_dA, &as);
  p.as = as;
  p.off_dA = off_dA;
  p.MP = (M + 15) & ~15;
  p.ncb = (N + kCB - 1) / kCB;
  const GpkVarGramSplit sp = gpk_var_gram_split(B, M);
  p.WS = sp.WS;
  p.nsplit = sp.nsplit;
  p.npairs = sp.npairs;
  const size_t nwg = (size_t)B * p.ncb;
  size_t off = gpk_up16(tail);
  p.off_wg = off; off = gpk_up16(off + (size_t)B * M * p.as * sizeof(float));   // W diag(gvar)
  p.off_dm = off; off = gpk_up16(off + nwg * M * sizeof(float));                // sum_i gmean_i A_mi
  p.off_xg = off; off = gpk_up16(off + nwg * 64 * sizeof(float));               // X^T gmean
  p.off_sc = off; off = gpk_up16(off + nwg * 2 * sizeof(float));                // sum gvar, sum gmean
  p.off_cp = off; off = gpk_up16(off + (size_t)p.nsplit * M * M * sizeof(double));
  p.total = tail == 0 ? 0 : off;
  return p;
}

struct VchAdjArgs {
  GpkVarCholAdjArgs a;
  VchPlan p;
};

template <typename T>
GPK_DEVICE T* vch_ws(const VchAdjArgs& k, size_t o, size_t off) {
  return (T*)((char*)k.a.ws + o * k.p.total + off);
}

// Output o's slice of the forward's state: A (B, M, as), then the clamp mask (B, as).
GPK_DEVICE const float* vch_saved(const VchAdjArgs& k, size_t o) {
  return k.a.saved + o * ((size_t)k.a.B * k.a.M * k.p.as + (size_t)k.a.B * k.p.as);
}

// ------------------------------------------------------------------------------------------------
// da: W, Y = L_q W, dA, the row partials
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vchol_da_kernel(VchAdjArgs k) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = k.a.N, M = k.a.M, D = k.a.D, as = k.p.as;
  const int MP = k.p.MP, MB = MP >> 4, LS = MP + 4;
  float* Al = lds;                       // MP x kKS
  float* Wl = Al + (size_t)MP * kKS;     // MP x kKS
  float* Lp = Wl + (size_t)MP * kKS;     // 16 x LS
  float* gm = Lp + 16 * LS;              // 64
  float* gv = gm + 64;                   // 64
  float* vm = gv + 64;                   // MP

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int ncb = k.p.ncb;
  const int b = blockIdx.x / ncb, cb = blockIdx.x - b * ncb;
  const size_t o = blockIdx.y;
  const float* sv0 = vch_saved(k, o);
  const float* As = sv0 + (size_t)b * M * as;
  const float* mask = sv0 + (size_t)k.a.B * M * as + (size_t)b * as;
  const float* gmean = k.a.gmean + (o * (size_t)k.a.B + b) * (size_t)N;
  const float* gvar = k.a.gvar + (o * (size_t)k.a.B + b) * (size_t)N;
  const float* vmean = k.a.vmean + o * (size_t)M;
  const float* vchol = k.a.vchol + o * (size_t)M * M;
  float* dAb = vch_ws<float>(k, o, k.p.off_dA) + (size_t)b * M * as;
  float* Wgb = vch_ws<float>(k, o, k.p.off_wg) + (size_t)b * M * as;

  for (int e = tid; e < MP * kCB; e += 256) {
    const int m = e >> 6, j = e & 63;
    const float v = As[m < M ? (size_t)m * as + kCB * cb + j : 0];
    Al[(size_t)m * kKS + j] = m < M ? v : 0.f;
  }
  if (tid < 64) {
    const int col = kCB * cb + tid;
    const bool ok = col < N;
    const float gmv = gmean[ok ? col : 0];
    const float gvv = gvar[ok ? col : 0];
    gm[tid] = ok ? gmv : 0.f;
    gv[tid] = (ok && mask[col] != 0.f) ? gvv : 0.f;
  }
  for (int m = tid; m < MP; m += 256) vm[m] = m < M ? vmean[m] : 0.f;

  // ---- W = L_q^T A (the pass opens with a barrier), kept in LDS; W diag(gvar) -> workspace
  f32x4 accW[16];
  vd_w_pass(accW, Al, Lp, vchol, M, MB, LS, tid, w, c, g);
  {
    const int col = 16 * w + c;
    const float gvc = gv[col];
#pragma unroll
    for (int mt = 0; mt < 16; ++mt) {
      if (mt >= MB) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mr = 16 * mt + 4 * g + r;
        Wl[(size_t)mr * kKS + col] = accW[mt][r];
        if (mr < M) Wgb[(size_t)mr * as + kCB * cb + col] = accW[mt][r] * gvc;
      }
    }
  }

  // ---- Y = L_q W row tile by row tile (panel mt feeds the W tiles kb <= mt),
  //      dA = gmean m + 2 gvar (Y - A)
  for (int mt = 0; mt < MB; ++mt) {
    const f32x4 y = vd_lq_row_tile(vchol, M, mt, Lp, LS, Wl, tid, w, c, g);
    const int col = 16 * w + c;
    const float gmc = gm[col], gvc2 = 2.f * gv[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = 16 * mt + 4 * g + r;
      if (mr < M)
        dAb[(size_t)mr * as + kCB * cb + col] =
            __builtin_fmaf(gvc2, y[r] - Al[(size_t)mr * kKS + col], gmc * vm[mr]);
    }
  }

  // ---- this workgroup's partials (columns ascending)
  const size_t wg = blockIdx.x;
  if (tid < M) {
    float s = 0.f;
    for (int j = 0; j < kCB; ++j) s = __builtin_fmaf(gm[j], Al[(size_t)tid * kKS + j], s);
    vch_ws<float>(k, o, k.p.off_dm)[wg * M + tid] = s;
  }
  if (tid < 64) {
    float s = 0.f;
    if (tid < D) {
      const float* Xb = k.a.X + o * (size_t)k.a.x_stride + (size_t)b * N * D;
      const int nv = N - kCB * cb < kCB ? N - kCB * cb : kCB;
      for (int j = 0; j < nv; ++j) s = __builtin_fmaf(gm[j], Xb[(size_t)(kCB * cb + j) * D + tid], s);
    }
    vch_ws<float>(k, o, k.p.off_xg)[wg * 64 + tid] = s;
  }
  if (w == 1) {
    const float sv = wave_sum(gv[lane]), sg = wave_sum(gm[lane]);
    if (lane == 0) {
      vch_ws<float>(k, o, k.p.off_sc)[wg * 2] = sv;
      vch_ws<float>(k, o, k.p.off_sc)[wg * 2 + 1] = sg;
    }
  }
}

size_t vch_da_lds(int MP) {
  return ((size_t)2 * MP * kKS + 16 * (MP + 4) + 2 * 64 + MP) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
// gram: fp64 partials of sum_b A (W diag gvar)^T, the lower 64 x 64 blocks
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vchol_gram_kernel(VchAdjArgs k) {
  const int M = k.a.M, as = k.p.as;
  const size_t o = blockIdx.y;
  const size_t ws = (size_t)M * as;   // floats between two windows' panels
  vd_lower_gram(vch_saved(k, o), ws, vch_ws<float>(k, o, k.p.off_wg), ws, as, k.a.N, M, k.a.B, k.p.WS,
                k.p.npairs, vch_ws<double>(k, o, k.p.off_cp));
}

// ------------------------------------------------------------------------------------------------
// finish: dC, dm, dweights, dbias, ds2 += sum gvar, dX += gmean_i w. Follows the shared
// pipeline's finish on the stream (ds2 and dX are read-modify-write).
//   blocks [0, nC): dC     [nC, nC + nV): dm and dweights     nC + nV: dbias, ds2     then dX
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vchol_finish_kernel(VchAdjArgs k, int nC, int nV) {
  __shared__ double sh[2][256];
  const int N = k.a.N, M = k.a.M, D = k.a.D, B = k.a.B;
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  const size_t o = blockIdx.y;
  float* dpar = k.a.dpar + o * (size_t)(M + 2 * D + 2);
  const long long nwg = (long long)B * k.p.ncb;
  if (blk < nC) {
    const long long e = (long long)blk * 256 + tid, mm = (long long)M * M;
    if (e >= mm) return;
    const int m = (int)(e / M), kc = (int)(e - (long long)m * M);
    double s = 0.0;
    if (kc <= m) {
      const double* Cp = vch_ws<double>(k, o, k.p.off_cp);
      for (int sp = 0; sp < k.p.nsplit; ++sp) s += Cp[(size_t)sp * mm + e];
    }
    k.a.dchol[o * (size_t)mm + e] = (float)(2.0 * s);
    return;
  }
  if (blk < nC + nV) {
    const int e = (blk - nC) * 256 + tid;
    if (e < M) {
      const float* dmp = vch_ws<float>(k, o, k.p.off_dm);
      double s = 0.0;
      for (long long wg = 0; wg < nwg; ++wg) s += dmp[wg * M + e];
      dpar[e] = (float)s;
    } else if (e < M + D) {
      const int d = e - M;
      const float* xg = vch_ws<float>(k, o, k.p.off_xg);
      double s = 0.0;
      for (long long wg = 0; wg < nwg; ++wg) s += xg[wg * 64 + d];
      dpar[M + 1 + D + d] = (float)s;
    }
    return;
  }
  if (blk == nC + nV) {
    const float* sc = vch_ws<float>(k, o, k.p.off_sc);
    double sv = 0.0, sg = 0.0;
    for (long long wg = tid; wg < nwg; wg += 256) {
      sv += sc[2 * wg];
      sg += sc[2 * wg + 1];
    }
    sh[0][tid] = sv;
    sh[1][tid] = sg;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) {
        sh[0][tid] += sh[0][tid + off];
        sh[1][tid] += sh[1][tid + off];
      }
      __syncthreads();
    }
    if (tid == 0) {
      dpar[M] = (float)((double)dpar[M] + sh[0][0]);
      dpar[M + 1 + 2 * D] = (float)sh[1][0];
    }
    return;
  }
  const long long e = (long long)(blk - nC - nV - 1) * 256 + tid;
  if (e >= (long long)B * N * D) return;
  const long long pt = e / D;
  const int d = (int)(e - pt * D);
  const size_t eo = o * (size_t)B * N * D + e;
  k.a.dX[eo] = __builtin_fmaf(k.a.gmean[o * (size_t)B * N + pt], k.a.hyp[o * (size_t)(4 + 2 * D) + 4 + d], k.a.dX[eo]);
}

// ------------------------------------------------------------------------------------------------
// kl
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_chol_kl_fwd_kernel(const float* __restrict__ m,
                                                              const float* __restrict__ C, int M,
                                                              float* __restrict__ kl) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  const size_t o = blockIdx.y;
  m += o * (size_t)M;
  C += o * (size_t)M * M;
  double s = 0.0;
  for (int e = tid; e < M * M; e += 256) {
    const int r = e / M, kc = e - r * M;
    if (kc > r) continue;
    const double v = (double)C[e];
    s += v * v;
    if (kc == r) s -= log(v * v);
  }
  for (int e = tid; e < M; e += 256) s += (double)m[e] * (double)m[e];
  sh[tid] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) sh[tid] += sh[tid + off];
    __syncthreads();
  }
  if (tid == 0) kl[o] = (float)(0.5 * (sh[0] - (double)M));
}

__global__ __launch_bounds__(256) void gpk_chol_kl_bwd_kernel(const float* __restrict__ m,
                                                              const float* __restrict__ C, int M,
                                                              const float* __restrict__ gkl,
                                                              float* __restrict__ dm, float* __restrict__ dC) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const size_t o = blockIdx.y;
  const float g = gkl[o];
  m += o * (size_t)M;
  C += o * (size_t)M * M;
  dm += o * (size_t)M;
  dC += o * (size_t)M * M;
  if (e < M * M) {
    const int r = e / M, kc = e - r * M;
    const float v = C[e];
    dC[e] = kc > r ? 0.f : (kc == r ? g * (v - 1.f / v) : g * v);
  } else if (e < M * M + M) {
    dm[e - M * M] = g * m[e - M * M];
  }
}

bool vch_fwd_shape_ok(int B, int N, int M, int D) {
  return B >= 0 && N >= 1 && M >= 1 && M <= 256 && D >= 1 && D <= 64 &&
         (long long)B * ((N + kCB - 1) / kCB) <= 0x7fffffffLL;
}

void vch_set_lds_once() {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)gpk_vchol_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute((const void*)gpk_vchol_da_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipGetLastError();
  });
}

}  // namespace

size_t gpk_var_chol_saved_bytes(int B, int N, int M, int D) {
  if (B < 1 || !vch_fwd_shape_ok(B, N, M, D)) return 0;
  const size_t as = (size_t)(N + 63) / 64 * 64;
  return ((size_t)B * M * as + (size_t)B * as) * sizeof(float);   // A, then the clamp mask
}

size_t gpk_var_chol_adjoint_ws_bytes(int B, int N, int M, int D) {
  if (B < 1 || N < 1 || M < 1 || D < 1) return 0;
  if (gpk_var_cov_grad_tail_plan(B, N, M, D, nullptr, nullptr) == 0) return 0;
  return vch_plan(B, N, M, D).total;
}

int gpk_launch_var_chol(const GpkVarCholArgs& a, hipStream_t stream) {
  if (!vch_fwd_shape_ok(a.B, a.N, a.M, a.D) || a.O < 1 || a.O > 65535) return -7;
  vch_set_lds_once();
  const size_t lds = vch_fwd_lds(a.M, a.D);
  if (lds > 160 * 1024) return -9;
  const int ncb = (a.N + kCB - 1) / kCB;
  const int as = ncb * kCB;
  if (a.flags != nullptr) {
    const hipError_t e = hipMemsetAsync(a.flags, 0, sizeof(int), stream);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(gpk_vchol_fwd_kernel, dim3((unsigned)(a.B * ncb), (unsigned)a.O), dim3(256), lds, stream, a, as);
  return (int)hipGetLastError();
}

int gpk_launch_var_chol_adjoint(const GpkVarCholAdjArgs& a, hipStream_t stream) {
  if (gpk_var_chol_adjoint_ws_bytes(a.B, a.N, a.M, a.D) == 0 || a.O < 1 || a.O > 65535) return -10;
  vch_set_lds_once();
  const unsigned O = (unsigned)a.O;
  VchAdjArgs k{a, vch_plan(a.B, a.N, a.M, a.D)};
  const size_t lds = vch_da_lds(k.p.MP);
  if (lds > 160 * 1024) return -12;
  hipLaunchKernelGGL(gpk_vchol_da_kernel, dim3((unsigned)(a.B * k.p.ncb), O), dim3(256), lds, stream, k);
  hipLaunchKernelGGL(gpk_vchol_gram_kernel, dim3((unsigned)(k.p.npairs * k.p.nsplit), O), dim3(256), 0, stream, k);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  // from dA on: the shared pipeline on our slices (its plan is the head of each) and our dpar
  // rows (its {0[M], ds2, dl[D]} is the head of each)
  GpkVarCovGradArgs t{};
  t.X = a.X; t.Z = a.Z; t.Linv = a.Linv; t.vstd = a.vmean; t.hyp = a.hyp;
  t.state = nullptr; t.gcov = nullptr;
  t.B = a.B; t.N = a.N; t.M = a.M; t.D = a.D; t.O = a.O;
  t.x_stride = a.x_stride;
  t.ws = a.ws; t.dX = a.dX; t.dLinv = a.dLinv; t.dZ = a.dZ; t.dpar = a.dpar;
  const int rc = gpk_launch_var_cov_grad_from_dA(t, k.p.total, a.M + 2 * a.D + 2, stream);
  if (rc != 0) return rc;
  const int nC = (int)(((long long)a.M * a.M + 255) / 256);
  const int nV = (a.M + a.D + 255) / 256;
  const long long nX = ((long long)a.B * a.N * a.D + 255) / 256;
  if (nC + nV + 1 + nX > 0x7fffffffLL) return -10;
  hipLaunchKernelGGL(gpk_vchol_finish_kernel, dim3((unsigned)(nC + nV + 1 + nX), O), dim3(256), 0, stream, k, nC, nV);
  return (int)hipGetLastError();
}

int gpk_launch_chol_kl(const float* m, const float* chol, int O, int M, float* kl, const float* gkl,
                       float* dm, float* dchol, hipStream_t stream) {
  if (O < 1 || O > 65535) return -3;
  if (gkl == nullptr) {
    hipLaunchKernelGGL(gpk_chol_kl_fwd_kernel, dim3(1, (unsigned)O), dim3(256), 0, stream, m, chol, M, kl);
  } else {
    const int nb = (M * M + M + 255) / 256;
    hipLaunchKernelGGL(gpk_chol_kl_bwd_kernel, dim3(nb, (unsigned)O), dim3(256), 0, stream, m, chol, M, gkl, dm,
                       dchol);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
