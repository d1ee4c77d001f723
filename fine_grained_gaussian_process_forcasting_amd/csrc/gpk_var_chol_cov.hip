// Dense covariance of q(f) for a Cholesky (full-covariance) q(u) = N(m, L_q L_q^T) of the
// whitened variational GP, and its adjoint, for gfx950.
//
// Replaces the dense evaluation of upstream variational/variational_strategy.py (whitened)
// predictive_covar with variational/cholesky_variational_distribution.py's q(u), which
// MultivariateNormal.rsample / covariance_matrix of a DeepGP layer output materialise (reference
// denoising_model/DeepGP.py:62-64), and the torch autograd backward through it.
//
// Per window b, with A = L^{-1} K_ZX (fp64 solve, fp32 result) as gpk_variational_cov_f32 and
// gpk_variational_chol_f32 form it and L_q = tril(C):
//   W = L_q^T A        cov = K_XX + jitter I + W^T W - A^T A = K_XX + jitter I + S^T diag(+1, -1) S
// with the stacked panel S = [W; A] (2 M rows), which is also the adjoint's saved state. From
// g = dObjective / dcov (any matrix), H = g + g^T:
//   T = S H = [T_W; T_A]        dA = L_q T_W - T_A        dC = tril(sum_b A T_W^T)
// and from dA on the adjoint is the pipeline of gpk_variational_cov_grad.hip with its K_XX part
// (q, dlinv, kxx, reduce, finish), launched on the dA this unit writes into that pipeline's
// workspace. The jitter has no gradient.
//
// Kernels (all MFMA operands follow gpk_common.h's acc layout; output o on grid y of each):
//   fwd   one workgroup of 4 waves per (window, 64-point column block): the K_ZX block with the
//         forward's fp32 Gram arithmetic and centring, A on mfma_f64_16x16x4f64 written over K
//         in LDS (row tiles descending), W = L_q^T A on mfma_f32_16x16x4f32 with L_q staged in
//         16-row panels (zeros above the diagonal filled in at staging, structurally zero tiles
//         skipped); A and W -> S, and the window's own mean of x / l after the panels.
//   syrk  one workgroup per (window, 64 x 64 tile with tile row <= tile column), the SYRK of
//         gpk_posterior_cov.hip over the 2 M rows of S with the +-1 weight folded into the
//         I-side panel as a chunk is staged; tile and mirror from the same registers, the
//         diagonal from the same accumulators.
//   t     one workgroup per (window, 64 rows of S): T = S H, the t kernel of
//         gpk_variational_cov_grad.hip over the stacked rows.
//   da    one workgroup per (window, 64-point block): T_W block in LDS, Y = L_q T_W row tile by
//         row tile (panel mt feeds the tiles kb <= mt), dA = Y - T_A -> the shared workspace.
//   gram  one workgroup per (64 x 64 block of the lower triangle, split of the windows):
//         vd_lower_gram on the A rows of S and T_W, fp64 partial per split.
//   finish  dC = tril(sum of the partials) in fp64, fixed order; {ds2, dl} out of the pipeline's row.
// No atomics in any sum, fixed summation orders: two launches give the same bits; a window's cov
// and dX come from that window's data alone; output o of a batched launch offsets its base
// pointers only and has the bits of a single-output call.
// The blocks this unit runs together with the other dense-covariance and Cholesky units --
// constants, the L_q panel staging, the Y row tile, the fp64 lower-block Gram -- are
// gpk_var_dense.h's and are described there; fwd keeps every block in line (see there). syrk stays
// a copy of gpk_post_cov_kernel (a shared tile body moves the SGPR count of all three kernels, §8.9).
#include "gpk_common.h"
#include "gpk_posterior_cov.h"
#include "gpk_var_chol_cov.h"
#include "gpk_var_dense.h"
#include "gpk_variational_cov_grad.h"

#include <mutex>

namespace {

constexpr int kTile = 64;      // output tile edge of syrk
constexpr int kKC = 32;        // rows of S per LDS chunk of syrk
constexpr int kVS = kTile + 16;  // LDS row stride of such a chunk (the half's two k rows 16 banks apart)
constexpr int kXS = 64 + 4;    // LDS row stride of syrk's staged inputs

struct VccFwdArgs {
  GpkVarCholCovArgs a;
  int as;
  long long state_stride;   // floats between two outputs' states
};

// ------------------------------------------------------------------------------------------------
// fwd: S = [W; A] and the window means. Every block in line: the column means and point staging
// mirror vd_col_means and vd_stage_points, the W pass vd_w_pass (gpk_var_dense.h), the window
// mean, the K_ZX block and the A row tile those of gpk_var_cov_a_kernel. As calls they move
// this kernel's register figures, or (means and staging alone) its time at O = 2,
// B = 256, N = 192, M = 256, D = 32: 1.952 - 1.958 ms against 1.943 - 1.951.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcc_fwd_kernel(VccFwdArgs k) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = k.a.N, M = k.a.M, D = k.a.D, as = k.as;
  const int MP = (M + 15) & ~15, MB = MP >> 4;
  const int Dq = vd_dq(D);
  const int lgq = Dq == 16 ? 4 : (Dq == 32 ? 5 : 6);   // not vd_lgq: the call moves this kernel off the parent's bytes
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
  float* scr = lsc + 64;                 // 512

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int ncb = (N + kCB - 1) / kCB;
  const int b = blockIdx.x / ncb, cb = blockIdx.x - b * ncb;
  const size_t o = blockIdx.y;

  const float* hyp = k.a.hyp + o * (size_t)(4 + 2 * D);
  const float* Xb = k.a.X + o * (size_t)k.a.x_stride + (size_t)b * N * D;
  const float* Z = k.a.Z + o * (size_t)M * D;
  const double* Linv = k.a.Linv + o * (size_t)M * M;
  const float* vchol = k.a.vchol + o * (size_t)M * M;
  float* st = k.a.state + o * (size_t)k.state_stride;
  float* Ww = st + (size_t)b * 2 * M * as;         // rows 0 .. M - 1 of the window's panel
  float* Aw = Ww + (size_t)M * as;                 // rows M .. 2 M - 1
  float* muw = st + (size_t)k.a.B * 2 * M * as + (size_t)b * 64;
  const float s2 = hyp[0];

  if (tid < 64) lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
  lds_barrier();

  // ---- column means of Z / l, the forward's order
  for (int e = tid; e < 8 * Dq; e += 256) {
    const int d = e % Dq, q = e / Dq;
    float s = 0.f;
    if (d < D) {
      const float l = lsc[d];
#pragma unroll 4
      for (int m = q; m < M; m += 8) s += Z[(size_t)m * D + d] / l;
    }
    scr[e] = s;
  }
  lds_barrier();
  if (tid < 64) {
    float s = 0.f;
    if (tid < Dq) {
#pragma unroll
      for (int q = 0; q < 8; ++q) s += scr[q * Dq + tid];
    }
    cm[tid] = tid < D ? s / (float)M : 0.f;
  }
  lds_barrier();

  // ---- the window's own mean of x / l for syrk and kxx (one workgroup per window writes it):
  //      P = 256 / Dq partial sums per column over rows i = q mod P, ascending, then q = 0..P-1
  if (cb == 0) {
    const int d = tid & (Dq - 1), q = tid >> lgq, P = 256 >> lgq;
    float s = 0.f;
    if (d < D) {
      const float l = lsc[d];
#pragma unroll 4
      for (int i = q; i < N; i += P) s += Xb[(size_t)i * D + d] / l;
    }
    scr[tid] = s;   // = scr[q * Dq + d]
    lds_barrier();
    if (tid < 64) {
      float t = 0.f;
      if (tid < D)
        for (int q2 = 0; q2 < P; ++q2) t += scr[q2 * Dq + tid];
      muw[tid] = tid < D ? t / (float)N : 0.f;
    }
    lds_barrier();
  }

  // ---- this block's points, scaled, centred by the inducing mean, zero padded
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

  // ---- K_ZX block, 64 inducing rows at a time
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

  // ---- A = L^{-1} K_ZX for this wave's 16 columns, written over K: row tile rt contracts the
  //      K tiles kb <= rt, so the tiles go in descending order and a finished tile of A is never
  //      read as K again. Lane (g, c) feeds the A operand L^{-1}[16 rt + c][16 kb + 4 g + u] and
  //      the B operand K[16 kb + 4 g + u][16 w + c]; acc[r] = A[16 rt + g + 4 r][16 w + c].
  float* Kc = Kl + 16 * w + c;
  const int gcol = kCB * cb + 16 * w + c;   // < as
  for (int rt = MB - 1; rt >= 0; --rt) {
    const int m = 16 * rt + c;
    const double* row = Linv + (size_t)(m < M ? m : 0) * M;
    // four k blocks' operands (16 loads per lane) in flight together, the next four loaded
    // under these MFMAs: with one workgroup per CU at M = 256 nothing else hides the L2 latency
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
        if (kb0 + q > rt) break;
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
      if (mr < M) Aw[(size_t)mr * as + gcol] = v;
    }
  }

  // ---- W = L_q^T A: acc[mt][r] = W[16 mt + 4 g + r][16 w + c]. Lane (g, c) feeds, in MFMA step u
  //      of panel kb, the A operand L_q[16 kb + 4 g + u][16 mt + c] and the B operand
  //      A[16 kb + 4 g + u][16 w + c]; panel kb feeds the row tiles mt <= kb only.
  f32x4 accW[16];
#pragma unroll
  for (int mt = 0; mt < 16; ++mt) accW[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < MB; ++kb) {
    lds_barrier();   // the previous panel's reads are done (first pass: A is complete, zs / xs free)
    vd_stage_panel(vchol, M, kb, Lp, LS, tid);
    lds_barrier();
    float bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) bv[u] = Kl[(size_t)(16 * kb + 4 * g + u) * kKS + 16 * w + c];
#pragma unroll
    for (int mt = 0; mt < 16; ++mt) {
      if (mt > kb) continue;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        accW[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Lp[(4 * g + u) * LS + 16 * mt + c], bv[u], accW[mt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int mt = 0; mt < 16; ++mt) {
    if (mt >= MB) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = 16 * mt + 4 * g + r;
      if (mr < M) Ww[(size_t)mr * as + gcol] = accW[mt][r];
    }
  }
}

size_t vcc_fwd_lds(int M, int D) {
  const int MP = (M + 15) & ~15;
  const int nst = vd_max(2 * 64 * (vd_dq(D) + 4), 16 * (MP + 4));
  return ((size_t)MP * kKS + nst + 4 * 64 + 512) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
// syrk: cov = K_XX + jitter I + S^T diag(+1, -1) S
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcc_syrk_kernel(VccFwdArgs k) {
  __shared__ float mu[64];
  __shared__ float lsc[64];
  __shared__ float nI[kTile];
  __shared__ float nJ[kTile];
  // the staged inputs of both tile sides; after the Gram, the two chunks of S
  __shared__ __attribute__((aligned(16))) float buf[2 * kTile * kXS];
  static_assert(2 * kKC * kVS <= 2 * kTile * kXS, "S chunks must fit the input staging");
  float* xI = buf;
  float* xJ = buf + kTile * kXS;
  float* vI = buf;
  float* vJ = buf + kKC * kVS;

  const int M = k.a.M, R = 2 * k.a.M, Ns = k.a.N, D = k.a.D, vs = k.as;
  const int T = (Ns + kTile - 1) / kTile;
  const int P = T * (T + 1) / 2;
  // XCD-aware order: the tile pairs of one window go to the same XCD (shared L2 for S)
  const int total = k.a.B * P;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  const int b = id / P;
  int ti, tj;
  tile_of(id - b * P, T, ti, tj);   // ti <= tj
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int D4 = (D + 3) & ~3;

  const size_t o = blockIdx.y;
  const float* hyp = k.a.hyp + o * (size_t)(4 + 2 * D);
  const float* Xs = k.a.X + o * (size_t)k.a.x_stride + (size_t)b * Ns * D;
  const float* st = k.a.state + o * (size_t)k.state_stride;
  const float* Vb = st + (size_t)b * R * vs;
  const float* mup = st + (size_t)k.a.B * R * vs;
  const float s2 = hyp[0];

  // ---- the first chunk's loads go out before anything else (one f32x4 per panel, thread and
  //      16-row half chunk: row = 16 h + tid / 16, columns 4 (tid % 16) ..)
  const int vr = tid >> 4, vc = 4 * (tid & 15);
  f32x4 ra[2], rb[2];
  float rw[2];
  auto vload = [&](int k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = k0 + 16 * h + vr;
      const size_t off = (size_t)(row < R ? row : 0) * vs;
      rw[h] = row < M ? 1.f : -1.f;   // W rows add, A rows subtract
      ra[h] = *(const f32x4*)&Vb[off + kTile * ti + vc];
      rb[h] = *(const f32x4*)&Vb[off + kTile * tj + vc];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (row >= R || kTile * ti + vc + t >= Ns) ra[h][t] = 0.f;
        if (row >= R || kTile * tj + vc + t >= Ns) rb[h][t] = 0.f;
      }
    }
  };
  vload(0);

  if (tid < 64) {
    mu[tid] = tid < D ? mup[(size_t)b * 64 + tid] : 0.f;
    lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
  }
  lds_barrier();
  // ---- both sides' inputs, scaled, centred by the window's own mean, zero padded
  for (int e = tid; e < kTile * 64; e += 256) {
    const int r = e >> 6, d = e & 63;
    const int ci = kTile * ti + r, cj = kTile * tj + r;
    const bool okd = d < D;
    const float vi = Xs[(okd && ci < Ns) ? (size_t)ci * D + d : 0];
    const float vj = Xs[(okd && cj < Ns) ? (size_t)cj * D + d : 0];
    const float l = lsc[d], m = mu[d];
    xI[r * kXS + d] = (okd && ci < Ns) ? vi / l - m : 0.f;
    xJ[r * kXS + d] = (okd && cj < Ns) ? vj / l - m : 0.f;
  }
  lds_barrier();
  if (tid < 2 * kTile) {
    const float* x = (tid < kTile ? xI : xJ) + (tid & 63) * kXS;
    float s = 0.f;
    for (int d = 0; d < D4; ++d) s = __builtin_fmaf(x[d], x[d], s);
    (tid < kTile ? nI : nJ)[tid & 63] = s;
  }
  lds_barrier();

  // ---- K(x_I, x_J) for this wave's strip: reg r = tile row 16 it + 4 g + r, column 16 w + c
  f32x4 Kt[4];
  {
    f32x4 G[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) G[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D4; d0 += 4) {
      const float bj = xJ[(16 * w + c) * kXS + d0 + g];
#pragma unroll
      for (int it = 0; it < 4; ++it)
        G[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(xI[(16 * it + c) * kXS + d0 + g], bj, G[it], 0, 0, 0);
    }
    const float nj = nJ[16 * w + c];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d2 = __builtin_fmaxf(nI[16 * it + 4 * g + r] + nj - 2.f * G[it][r], 0.f);
        Kt[it][r] = s2 * __builtin_amdgcn_exp2f(d2 * kNHalfLog2e);
      }
  }

  // ---- S_I^T diag(+-1) S_J over the 2 M rows, 32 at a time, ascending k
  f32x4 acc[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) acc[it] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < R; k0 += kKC) {
    lds_barrier();   // the previous chunk's reads are done
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *(f32x4*)&vI[(16 * h + vr) * kVS + vc] = ra[h] * rw[h];
      *(f32x4*)&vJ[(16 * h + vr) * kVS + vc] = rb[h];
    }
    lds_barrier();
    if (k0 + kKC < R) vload(k0 + kKC);
#pragma unroll
    for (int kk = 0; kk < kKC; kk += 4) {
      const float bj = vJ[(kk + g) * kVS + 16 * w + c];
#pragma unroll
      for (int it = 0; it < 4; ++it)
        acc[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(vI[(kk + g) * kVS + 16 * it + c], bj, acc[it], 0, 0, 0);
    }
  }

  // ---- the tile and its mirror from the same registers; diagonal: s2 + jitter + the tile's own sum
  float* Cb = k.a.cov + ((size_t)o * k.a.B + b) * (size_t)Ns * Ns;
  const float dg = s2 + hyp[2];
  const int col = kTile * tj + 16 * w + c;
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = kTile * ti + 16 * it + 4 * g + r;
      if (row >= Ns || col >= Ns) continue;
      if (row < col) {
        const float v = Kt[it][r] + acc[it][r];
        Cb[(size_t)row * Ns + col] = v;
        Cb[(size_t)col * Ns + row] = v;
      } else if (row == col) {
        Cb[(size_t)row * Ns + col] = dg + acc[it][r];
      }
    }
}

// ------------------------------------------------------------------------------------------------
// Adjoint: workspace plan (byte offsets, each a multiple of 16)
// ------------------------------------------------------------------------------------------------
struct VccPlan {
  int as, MP, ncb;
  int WS, nsplit, npairs;   // windows per split of gram, number of splits, 64 x 64 lower blocks
  size_t off_dA;            // inside the shared pipeline's slice (which starts at byte 0)
  size_t off_T, off_cp, off_dp, total;
  int dps;                  // floats of the pipeline's dpar row
};

__host__ VccPlan vcc_plan(int B, int N, int M, int D) {
  VccPlan p;
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
  p.dps = M + 1 + D;
  size_t off = gpk_up16(tail);
  p.off_T = off;  off = gpk_up16(off + (size_t)B * 2 * M * p.as * sizeof(float));    // T = S H
  p.off_cp = off; off = gpk_up16(off + (size_t)p.nsplit * M * M * sizeof(double));   // dC partials
  p.off_dp = off; off = gpk_up16(off + (size_t)p.dps * sizeof(float));               // the pipeline's dpar row
  p.total = tail == 0 ? 0 : off;
  return p;
}

struct VccAdjArgs {
  GpkVarCholCovGradArgs a;
  VccPlan p;
  long long state_stride;
};

template <typename T>
GPK_DEVICE T* vcc_ws(const VccAdjArgs& k, size_t o, size_t off) {
  return (T*)((char*)k.a.ws + o * k.p.total + off);
}

// ------------------------------------------------------------------------------------------------
// t: T = S H over the stacked rows. The H-chunk staging and the accumulation are the text of
// gpk_vcg_t_kernel (gpk_variational_cov_grad.hip) with R = 2 M rows; as one function this kernel
// spills 21 SGPRs instead of 22, so both stay in line.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcc_t_kernel(VccAdjArgs k) {
  __shared__ float Hs[16 * kHS];
  const int N = k.a.N, R = 2 * k.a.M, as = k.p.as;
  const int NP = (N + 15) & ~15, nct = NP >> 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int nrb = (R + 63) / 64;
  const int b = blockIdx.x / nrb, rb = blockIdx.x - b * nrb;
  const size_t o = blockIdx.y;

  const float* S = k.a.state + o * (size_t)k.state_stride + (size_t)b * R * as;
  const float* G = k.a.gcov + (o * (size_t)k.a.B + b) * (size_t)N * N;
  float* Tw = vcc_ws<float>(k, o, k.p.off_T) + (size_t)b * R * as;

  const int m = 64 * rb + 16 * w + c;   // the A operand's row
  const float* Srow = S + (size_t)(m < R ? m : 0) * as;
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
      const bool ok = m < R && j < N;
      const float ld = Srow[ok ? j : 0];
      const float av = ok ? ld : 0.f;
      const float* hb = Hs + (4 * kk + g) * kHS + c;
#pragma unroll
      for (int ct = 0; ct < 16; ++ct)
        if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, hb[16 * ct], acc[ct], 0, 0, 0);
    }
  }

  // acc[ct][r] = T[64 rb + 16 w + 4 g + r][16 ct + c]
#pragma unroll
  for (int ct = 0; ct < 16; ++ct) {
    if (ct >= nct) continue;
    const int col = 16 * ct + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = 64 * rb + 16 * w + 4 * g + r;
      if (mr < R && col < N) Tw[(size_t)mr * as + col] = acc[ct][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// da: dA = L_q T_W - T_A
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcc_da_kernel(VccAdjArgs k) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = k.a.N, M = k.a.M, as = k.p.as;
  const int MP = k.p.MP, MB = MP >> 4, LS = MP + 4;
  float* Tl = lds;                       // MP x kKS: this block's columns of T_W
  float* Lp = Tl + (size_t)MP * kKS;     // 16 x LS

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int ncb = k.p.ncb;
  const int b = blockIdx.x / ncb, cb = blockIdx.x - b * ncb;
  const size_t o = blockIdx.y;
  const float* TWb = vcc_ws<float>(k, o, k.p.off_T) + (size_t)b * 2 * M * as;
  const float* TAb = TWb + (size_t)M * as;
  const float* vchol = k.a.vchol + o * (size_t)M * M;
  float* dAb = vcc_ws<float>(k, o, k.p.off_dA) + (size_t)b * M * as;

  // columns >= N of T were never written: masked here
  for (int e = tid; e < MP * kCB; e += 256) {
    const int m = e >> 6, j = e & 63;
    const bool ok = m < M && kCB * cb + j < N;
    const float v = TWb[ok ? (size_t)m * as + kCB * cb + j : 0];
    Tl[(size_t)m * kKS + j] = ok ? v : 0.f;
  }

  // ---- Y = L_q T_W row tile by row tile (panel mt feeds the tiles kb <= mt), dA = Y - T_A
  const int col = 16 * w + c, gcol = kCB * cb + col;
  for (int mt = 0; mt < MB; ++mt) {
    const f32x4 y = vd_lq_row_tile(vchol, M, mt, Lp, LS, Tl, tid, w, c, g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = 16 * mt + 4 * g + r;
      if (mr < M) {
        const bool ok = gcol < N;
        const float ta = TAb[ok ? (size_t)mr * as + gcol : 0];
        dAb[(size_t)mr * as + gcol] = ok ? y[r] - ta : 0.f;
      }
    }
  }
}

size_t vcc_da_lds(int MP) { return ((size_t)MP * kKS + 16 * (MP + 4)) * sizeof(float); }

// ------------------------------------------------------------------------------------------------
// gram: fp64 partials of sum_b A T_W^T, the lower 64 x 64 blocks
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcc_gram_kernel(VccAdjArgs k) {
  const int M = k.a.M, as = k.p.as;
  const size_t o = blockIdx.y;
  const size_t ws = (size_t)2 * M * as;   // floats between two windows' stacked panels
  // the A rows of the windows' panels of S against T_W
  vd_lower_gram(k.a.state + o * (size_t)k.state_stride + (size_t)M * as, ws, vcc_ws<float>(k, o, k.p.off_T), ws,
                as, k.a.N, M, k.a.B, k.p.WS, k.p.npairs, vcc_ws<double>(k, o, k.p.off_cp));
}

// ------------------------------------------------------------------------------------------------
// finish: dC = tril(sum of the partials); {ds2, dl} from the pipeline's dpar row. Follows the
// shared pipeline's finish on the stream.   blocks [0, nC): dC     nC: dpar
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_vcc_finish_kernel(VccAdjArgs k, int nC) {
  const int M = k.a.M, D = k.a.D;
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  const size_t o = blockIdx.y;
  if (blk < nC) {
    const long long e = (long long)blk * 256 + tid, mm = (long long)M * M;
    if (e >= mm) return;
    const int m = (int)(e / M), kc = (int)(e - (long long)m * M);
    double s = 0.0;
    if (kc <= m) {
      const double* Cp = vcc_ws<double>(k, o, k.p.off_cp);
      for (int sp = 0; sp < k.p.nsplit; ++sp) s += Cp[(size_t)sp * mm + e];
    }
    k.a.dchol[o * (size_t)mm + e] = (float)s;
    return;
  }
  if (tid < 1 + D) k.a.dpar[o * (size_t)(1 + D) + tid] = vcc_ws<float>(k, o, k.p.off_dp)[M + tid];
}

void vcc_set_lds_once() {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)gpk_vcc_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute((const void*)gpk_vcc_da_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipGetLastError();
  });
}

long long vcc_state_floats(int B, int N, int M) {
  const long long as = ((long long)N + 63) / 64 * 64;
  return (long long)B * 2 * M * as + (long long)B * 64;
}

}  // namespace

size_t gpk_var_chol_cov_state_bytes(int B, int N, int M) {
  if (!gpk_var_cov_tile_grid_ok(B, N, M)) return 0;
  return (size_t)vcc_state_floats(B, N, M) * sizeof(float);
}

size_t gpk_var_chol_cov_grad_ws_bytes(int B, int N, int M, int D) {
  if (B < 0 || N < 1 || M < 1 || D < 1) return 0;
  if (gpk_var_cov_grad_tail_plan(B, N, M, D, nullptr, nullptr) == 0) return 0;
  if ((long long)B * 8 > 0x7fffffffLL) return 0;   // t: B * ceil(2 M / 64) workgroups on grid x
  const size_t total = vcc_plan(B, N, M, D).total;
  return total / sizeof(float) > 0x7fffffffULL ? 0 : total;   // the slice stride is the pipeline's dpar stride

}

int gpk_launch_var_chol_cov(const GpkVarCholCovArgs& a, hipStream_t stream) {
  if (!gpk_var_cov_tile_grid_ok(a.B, a.N, a.M) || a.D < 1 || a.D > 64 || a.O < 1 || a.O > 65535) return -7;
  if (a.B == 0) return 0;
  vcc_set_lds_once();
  const size_t lds = vcc_fwd_lds(a.M, a.D);
  if (lds > 160 * 1024) return -9;
  const int ncb = (a.N + kCB - 1) / kCB;
  VccFwdArgs k{a, ncb * kCB, vcc_state_floats(a.B, a.N, a.M)};
  const long long T = ncb;
  const long long grid2 = (long long)a.B * (T * (T + 1) / 2);
  hipLaunchKernelGGL(gpk_vcc_fwd_kernel, dim3((unsigned)(a.B * ncb), (unsigned)a.O), dim3(256), lds, stream, k);
  hipLaunchKernelGGL(gpk_vcc_syrk_kernel, dim3((unsigned)grid2, (unsigned)a.O), dim3(256), 0, stream, k);
  return (int)hipGetLastError();
}

int gpk_launch_var_chol_cov_grad(const GpkVarCholCovGradArgs& a, hipStream_t stream) {
  if (a.O < 1 || a.O > 65535) return -10;
  if (a.B == 0) return 0;
  if (gpk_var_chol_cov_grad_ws_bytes(a.B, a.N, a.M, a.D) == 0) return -10;
  vcc_set_lds_once();
  const unsigned O = (unsigned)a.O;
  VccAdjArgs k{a, vcc_plan(a.B, a.N, a.M, a.D), vcc_state_floats(a.B, a.N, a.M)};
  const size_t lds = vcc_da_lds(k.p.MP);
  if (lds > 160 * 1024) return -12;
  const int nrb = (2 * a.M + 63) / 64;
  hipLaunchKernelGGL(gpk_vcc_t_kernel, dim3((unsigned)(a.B * nrb), O), dim3(256), 0, stream, k);
  hipLaunchKernelGGL(gpk_vcc_da_kernel, dim3((unsigned)(a.B * k.p.ncb), O), dim3(256), lds, stream, k);
  hipLaunchKernelGGL(gpk_vcc_gram_kernel, dim3((unsigned)(k.p.npairs * k.p.nsplit), O), dim3(256), 0, stream, k);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  // from dA on: the shared pipeline, K_XX part included, on our slices (its plan is the head of
  // each); its dpar row {0[M], ds2, dl[D]} lands in the slice and finish copies the tail out
  GpkVarCovGradArgs t{};
  t.X = a.X; t.Z = a.Z; t.Linv = a.Linv; t.vstd = a.vchol; t.hyp = a.hyp;
  t.state = a.state; t.gcov = a.gcov;
  t.B = a.B; t.N = a.N; t.M = a.M; t.D = a.D; t.O = a.O;
  t.x_stride = a.x_stride;
  t.ws = a.ws; t.dX = a.dX; t.dLinv = a.dLinv; t.dZ = a.dZ;
  t.dpar = (float*)((char*)a.ws + k.p.off_dp);
  const int rc = gpk_launch_var_cov_grad_from_dA_kxx(t, k.p.total, (int)(k.p.total / sizeof(float)),
                                                     k.state_stride, (long long)a.B * 2 * a.M * k.p.as, stream);
  if (rc != 0) return rc;
  const int nC = (int)(((long long)a.M * a.M + 255) / 256);
  hipLaunchKernelGGL(gpk_vcc_finish_kernel, dim3((unsigned)(nC + 1), O), dim3(256), 0, stream, k, nC);
  return (int)hipGetLastError();
}
