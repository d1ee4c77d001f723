// Adjoint of the exact-GP posterior (gpk_posterior.hip + gpk_posterior_cov.hip) for gfx950.
//
// Replaces torch autograd through the dense restatement of upstream
// models/exact_prediction_strategies.py (exact_predictive_mean / exact_predictive_covar): the
// backward of model(x).mean / .variance / .covariance_matrix, of rsample and of log_prob in eval
// mode when a gradient flows to the test inputs, the training data or a hyper-parameter.
//
// Per window, with K_hat = s2 E(X, X) + noise I (+ the ladder's jitter) = L L^T, z = L^{-1}(y - c),
// K* = s2 E(X, Xs), K** = s2 E(Xs, Xs), V = L^{-1} K* (the forward's workspace), mean = c + V^T z,
// Sigma = K** - V^T V, var = diag Sigma, and the incoming gmean, gvar, gcov (any matrix):
//   G = gcov + diag(gvar)    H = G + G^T    W = L^{-T} V    alpha = L^{-T} z    u = W gmean
//   dK*  = -W H + alpha gmean^T          dK_hat = 1/2 W H W^T - 1/2 (u alpha^T + alpha u^T)
//   dK** = 1/2 H      dy = u      dc = sum gmean - sum u      dnoise = tr dK_hat
// No Cholesky adjoint. For each block K = s2 E(a, b) in coordinates a = x / l (centred by the
// forward's training mean of x / l, read from its workspace), Q = dK o K (the diagonal of the two
// square blocks apart: it is s2 (+ noise) exactly):
//   da_i = (Q b)_i - rowsum(Q)_i a_i     db_j = (Q^T a)_j - colsum(Q)_j b_j
//   dl_d = -sum (a o da + b o db)_d / l_d      ds2 = sum Q / s2 + tr dK_hat + 1/2 tr H
// The two square blocks are symmetric, so their db equals their da.
//
// Kernels (all MFMA operands follow gpk_common.h's acc layout, fp32 products only):
//   backsub one workgroup per (window, 64 columns of [V | z]): W and alpha by blocked back
//        substitution up L's block rows, the wave's tiles in registers, the 16 diagonal-block
//        inverses in LDS.
//   u    one workgroup per window: u = W gmean.
//   ks   one workgroup per (window, 64 test points): H's column block in LDS from gcov, gcov^T
//        and gvar; T = W H (-> workspace); K* with the forward's Gram arithmetic; Q* in LDS over
//        H; Q* xs and Q*^T x with the row / column sums on a ones operand. Writes the K* part of
//        the test side and one partial of the training side per column block.
//   kh   one workgroup per (window, 64 training rows): dK_hat tile by tile, 1/2 T W^T contracted
//        over Ns from the two workspace panels, minus the rank-2 term; Q_hat in LDS, Q_hat x and
//        the row sums; adds the column blocks' K* partials in ascending order.
//   kss  one workgroup per (window, 64 test rows): 1/2 H o K** likewise; follows ks on the stream.
//   finish one workgroup per window: dX, dXs, dy, dhyp from the window's sums.
// Without gvar and gcov, H = 0: T and the Ns-contraction are skipped and kss is not launched.
// No atomics, no host synchronisation, fixed summation orders: two launches give the same bits,
// and every output of a window comes from that window alone.
#include "gpk_common.h"
#include "gpk_posterior_cov.h"
#include "gpk_posterior_grad.h"

#include <mutex>

namespace {

constexpr int kKS = 68;        // LDS row stride of a 64-column panel
constexpr int kMaxN = 256;
constexpr float kNHalfLog2e = -0.72134752044448170f;  // -0.5 * log2(e)
constexpr int kCpStride = 32;  // per-window partial sums: 8 slots of 4 (see the kernels)

__host__ __device__ constexpr int pg_dq(int D) { return D <= 16 ? 16 : (D <= 32 ? 32 : 64); }

// Workspace (float offsets, each a multiple of 4) and the work split.
struct PgPlan {
  int vs, Dq, ncb, nrt;
  size_t off_W, off_T, off_al, off_u, off_dap, off_dxa, off_dxs, off_cp, total;
};

__host__ PgPlan pg_plan(int B, int N, int Ns, int D) {
  PgPlan p;
  p.vs = (Ns + 63) / 64 * 64;
  p.Dq = pg_dq(D);
  p.ncb = (Ns + 63) / 64;
  p.nrt = (N + 63) / 64;
  auto up = [](size_t v) { return (v + 3) & ~(size_t)3; };
  size_t off = 0;
  p.off_W = off;   off = up(off + (size_t)B * N * p.vs);
  p.off_T = off;   off = up(off + (size_t)B * N * p.vs);
  p.off_al = off;  off = up(off + (size_t)B * kMaxN);
  p.off_u = off;   off = up(off + (size_t)B * kMaxN);
  p.off_dap = off; off = up(off + (size_t)B * p.ncb * N * p.Dq);
  p.off_dxa = off; off = up(off + (size_t)B * N * p.Dq);
  p.off_dxs = off; off = up(off + (size_t)B * Ns * p.Dq);
  p.off_cp = off;  off = up(off + (size_t)B * kCpStride);
  p.total = off;
  return p;
}

struct PgArgs {
  GpkPostGradArgs a;
  PgPlan p;
  int tca;   // column tiles of backsub: [V | z] when gmean is present
};

GPK_DEVICE float* pg_ws(const PgArgs& k, size_t off) { return (float*)k.a.ws + off; }

// ------------------------------------------------------------------------------------------------
// backsub: W = L^{-T} V, alpha = L^{-T} z
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_pg_backsub_kernel(PgArgs k) {
  __shared__ __attribute__((aligned(16))) float dinv[16 * 256];
  __shared__ __attribute__((aligned(16))) float ltmp[16 * 256];
  const int N = k.a.N, Ns = k.a.Ns, vs = k.p.vs;
  const int NB = (N + 15) >> 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / k.tca, tile = blockIdx.x - b * k.tca;
  const float* Lb = k.a.L + (size_t)b * N * N;
  const float* Vb = k.a.state + (size_t)b * N * vs;
  const float* zb = k.a.z + (size_t)b * N;
  float* Wb = pg_ws(k, k.p.off_W) + (size_t)b * N * vs;
  float* alb = pg_ws(k, k.p.off_al) + (size_t)b * kMaxN;

  // ---- the diagonal blocks of L (identity on padded rows) and their inverses, as gpk_post_kernel
  {
    const int bi = tid >> 4, m = tid & 15;
    if (bi < NB) {
      const int row = 16 * bi + m;
      float lv[16];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const bool ok = kk <= m && row < N;
        lv[kk] = Lb[ok ? (size_t)row * N + 16 * bi + kk : 0];
      }
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        float v = (kk == m) ? 1.f : 0.f;
        if (kk <= m && row < N) v = lv[kk];
        ltmp[bi * 256 + m * 16 + kk] = v;
      }
    }
  }
  lds_barrier();
  {
    const int bi = tid >> 4, cc = tid & 15;
    if (bi < NB) {
      const float* Lt = ltmp + bi * 256;
      float x[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        float s = (m == cc) ? 1.f : 0.f;
#pragma unroll
        for (int kk = 0; kk < m; ++kk) s = __builtin_fmaf(-Lt[m * 16 + kk], x[kk], s);
        x[m] = (m < cc) ? 0.f : s / Lt[m * 16 + m];
      }
#pragma unroll
      for (int m = 0; m < 16; ++m) dinv[bi * 256 + m * 16 + cc] = x[m];   // inv[m][cc]
    }
  }
  lds_barrier();

  // ---- this lane's column of [V | z]; columns in (Ns, vs) and past the last one carry zeros
  if (tile * 64 + 16 * w >= (vs > Ns + 1 ? vs : Ns + 1)) return;   // nothing in this wave's strip
  const int col = tile * 64 + 16 * w + c;
  const bool isV = col < Ns;
  const bool isZ = k.a.gmean != nullptr && col == Ns;
  const float* sp = isV ? Vb + col : zb;
  const size_t sst = isV ? (size_t)vs : 1;
  const bool live = isV || isZ;

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 Wt[16];
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) {
    const int i = 15 - ii;
    if (i >= NB) continue;
    f32x4 C;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * i + 4 * g + r;
      const bool ok = live && row < N;
      const float v = sp[ok ? (size_t)row * sst : 0];
      C[r] = ok ? v : 0.f;
    }
    // - sum_{j > i} L_ji^T W_j (two accumulators: halves the dependent MFMA chain)
    f32x4 U0 = zero4, U1 = zero4;
#pragma unroll
    for (int j = i + 1; j < 16; ++j) {
      if (j >= NB) continue;
      f32x4 lt;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * j + 4 * g + r, cc = 16 * i + c;
        const bool ok = rr < N && cc < N;
        const float v = Lb[ok ? (size_t)rr * N + cc : 0];
        lt[r] = ok ? v : 0.f;
      }
      if (j & 1) U1 = mma_tn(lt, Wt[j], U1);
      else U0 = mma_tn(lt, Wt[j], U0);
    }
    C = C - U0 - U1;
    f32x4 di;
#pragma unroll
    for (int r = 0; r < 4; ++r) di[r] = dinv[i * 256 + (4 * g + r) * 16 + c];
    Wt[i] = mma_tn(di, C, zero4);   // (L_ii)^{-T} C
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * i + 4 * g + r;
      if (row < N) {
        if (col < vs) Wb[(size_t)row * vs + col] = isV ? Wt[i][r] : 0.f;
        if (isZ) alb[row] = Wt[i][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// u = W gmean
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_pg_u_kernel(PgArgs k) {
  __shared__ __attribute__((aligned(16))) float gm[kMaxN];
  const int N = k.a.N, Ns = k.a.Ns, vs = k.p.vs;
  const int tid = threadIdx.x, b = blockIdx.x;
  gm[tid] = tid < Ns ? k.a.gmean[(size_t)b * Ns + tid] : 0.f;
  lds_barrier();
  if (tid >= N) return;
  const float* Wr = pg_ws(k, k.p.off_W) + ((size_t)b * N + tid) * vs;
  float s = 0.f;
  for (int j = 0; j < vs; j += 4) {   // W's columns >= Ns hold zeros
    const f32x4 wv = *(const f32x4*)&Wr[j];
#pragma unroll
    for (int t = 0; t < 4; ++t) s = __builtin_fmaf(wv[t], gm[j + t], s);
  }
  pg_ws(k, k.p.off_u)[(size_t)b * kMaxN + tid] = s;
}

// Inputs of 64 points starting at row r0 of Xp (n rows), scaled, centred, zero padded.
template <int DT>
GPK_DEVICE void pg_stage(float* dst, const float* Xp, int r0, int rows, int n, int D, const float* lsc,
                         const float* mu, int tid) {
  constexpr int Dq = 16 * DT, ds = Dq + 4, lgq = DT == 1 ? 4 : (DT == 2 ? 5 : 6);
#pragma unroll 4
  for (int e = tid; e < rows * Dq; e += 256) {
    const int r = e >> lgq, d = e & (Dq - 1);
    const int row = r0 + r;
    const bool ok = d < D && row < n;
    const float v = Xp[ok ? (size_t)row * D + d : 0];
    dst[r * ds + d] = ok ? v / lsc[d] - mu[d] : 0.f;
  }
}

template <int DT>
GPK_DEVICE void pg_norms(float* dst, const float* src, int rows, int tid) {
  constexpr int Dq = 16 * DT, ds = Dq + 4;
  for (int n = tid; n < rows; n += 256) {
    float s = 0.f;
#pragma unroll 8
    for (int d = 0; d < Dq; ++d) s = __builtin_fmaf(src[n * ds + d], src[n * ds + d], s);
    dst[n] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// ks: T = W H, dK* = -T + alpha gmean^T, Q* and its contractions with the inputs
// ------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void gpk_pg_ks_kernel(PgArgs k) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int Dq = 16 * DT, ds = Dq + 4;
  const int N = k.a.N, Ns = k.a.Ns, D = k.a.D, vs = k.p.vs;
  const int NP = (N + 15) & ~15, NB = NP >> 4, NsP = (Ns + 15) & ~15;
  const int HR = NP > NsP ? NP : NsP;
  float* Hs = lds;                       // HR x kKS: H's column block, then Q*
  float* xtr = Hs + (size_t)HR * kKS;    // NP x ds
  float* xs = xtr + (size_t)NP * ds;     // 64 x ds
  float* ntr = xs + 64 * ds;             // 256
  float* nxs = ntr + 256;                // 64
  float* mu = nxs + 64;                  // 64
  float* lsc = mu + 64;                  // 64
  float* al = lsc + 64;                  // 256
  float* gm = al + 256;                  // 64
  float* scr = gm + 64;                  // 4

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int ncb = k.p.ncb;
  const int b = blockIdx.x / ncb, cb = blockIdx.x - b * ncb;
  const int J = 64 * cb;
  const bool hasH = k.a.gvar != nullptr || k.a.gcov != nullptr;
  const bool hasM = k.a.gmean != nullptr;
  const float* hyp = k.a.hyp + (long long)b * k.a.hyp_stride;  // this window's hyper vector (stride 0: shared)
  const float s2 = hyp[0];
  const float* Xb = k.a.X + (size_t)b * N * D;
  const float* Xsb = k.a.Xs + (size_t)b * Ns * D;
  const float* mup = k.a.state + (size_t)k.a.B * N * vs + (size_t)b * 64;
  const float* Wb = pg_ws(k, k.p.off_W) + (size_t)b * N * vs;
  float* Tb = pg_ws(k, k.p.off_T) + (size_t)b * N * vs;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  if (tid < 64) {
    mu[tid] = tid < D ? mup[tid] : 0.f;
    lsc[tid] = tid < D ? hyp[3 + (k.a.n_ls > 1 ? tid : 0)] : 1.f;
    const bool ok = hasM && J + tid < Ns;
    const float v = hasM ? k.a.gmean[(size_t)b * Ns + (ok ? J + tid : 0)] : 0.f;
    gm[tid] = ok ? v : 0.f;
  }
  al[tid] = 0.f;   // without gmean, alpha was never computed and is not read
  if (hasM && tid < N) al[tid] = pg_ws(k, k.p.off_al)[(size_t)b * kMaxN + tid];
  // ---- H[:, J .. J + 64) = g + g^T + 2 diag(gvar): rows of g, then 16-byte runs of its columns
  if (hasH) {
    const float* Gb = k.a.gcov ? k.a.gcov + (size_t)b * Ns * Ns : nullptr;
    const float* gvb = k.a.gvar ? k.a.gvar + (size_t)b * Ns : nullptr;
    for (int e = tid; e < NsP * 64; e += 256) {
      const int kk = e >> 6, j = e & 63;
      const bool ok = kk < Ns && J + j < Ns;
      float v = 0.f;
      if (ok && Gb) v = Gb[(size_t)kk * Ns + J + j];
      if (ok && gvb && kk == J + j) v += gvb[kk];
      Hs[kk * kKS + j] = v;
    }
    lds_barrier();
    for (int e = tid; e < NsP * 64; e += 256) {
      const int j = e / NsP, kk = e - j * NsP;
      const bool ok = kk < Ns && J + j < Ns;
      float v = 0.f;
      if (ok && Gb) v = Gb[(size_t)(J + j) * Ns + kk];
      if (ok && gvb && kk == J + j) v += gvb[kk];
      Hs[kk * kKS + j] += v;
    }
  }
  lds_barrier();   // mu, lsc
  pg_stage<DT>(xtr, Xb, 0, NP, N, D, lsc, mu, tid);
  pg_stage<DT>(xs, Xsb, J, 64, Ns, D, lsc, mu, tid);
  lds_barrier();
  pg_norms<DT>(ntr, xtr, NP, tid);
  pg_norms<DT>(nxs, xs, 64, tid);

  // ---- T = W H for the row tiles w, w + 4, .. of this wave, all four column tiles
  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[mi][ct] = zero4;
  if (hasH) {
    for (int k0 = 0; k0 < NsP; k0 += 16) {
      f32x4 bb[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int s = 0; s < 4; ++s) bb[ct][s] = Hs[(k0 + 4 * g + s) * kKS + 16 * ct + c];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int mt = w + 4 * mi;
        if (mt >= NB) continue;
        const int row = 16 * mt + c;
        f32x4 av = *(const f32x4*)&Wb[(size_t)(row < N ? row : 0) * vs + k0 + 4 * g];
        if (row >= N) av = zero4;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
          for (int s = 0; s < 4; ++s)
            acc[mi][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bb[ct][s], acc[mi][ct], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int mt = w + 4 * mi;
      if (mt >= NB) continue;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * mt + 4 * g + r;
          if (row < N) Tb[(size_t)row * vs + J + 16 * ct + c] = acc[mi][ct][r];
        }
    }
  }
  lds_barrier();   // H is read, the norms are written

  // ---- Q* = (alpha gmean^T - T) o K* over H in LDS
  float sq = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mt = w + 4 * mi;
    if (mt >= NB) continue;
    const float* xa = xtr + (16 * mt + c) * ds + g;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const float* xb = xs + (16 * ct + c) * ds + g;
      f32x4 G = zero4;
#pragma unroll
      for (int kk = 0; kk < Dq / 4; ++kk)
        G = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[4 * kk], xb[4 * kk], G, 0, 0, 0);
      const int j = 16 * ct + c;
      const float nj = nxs[j], gj = gm[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * mt + 4 * g + r;
        const float d2 = __builtin_fmaxf(ntr[i] + nj - 2.f * G[r], 0.f);
        const float kv = s2 * __builtin_amdgcn_exp2f(d2 * kNHalfLog2e);
        const float dk = al[i] * gj - acc[mi][ct][r];
        const float q = (i < N && J + j < Ns) ? dk * kv : 0.f;
        Hs[i * kKS + j] = q;
        sq += q;
      }
    }
  }
  lds_barrier();

  // ---- training side: Q* xs and the row sums, one partial per column block
  float* dap = pg_ws(k, k.p.off_dap) + ((size_t)b * ncb + cb) * N * Dq;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int mt = w + 4 * mi;
    if (mt >= NB) continue;
    f32x4 accQ[DT], rs = zero4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) accQ[dt] = zero4;
    const float* qa = Hs + (16 * mt + c) * kKS + g;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      const float av = qa[4 * kk];
      rs = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, rs, 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        accQ[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xs[(4 * kk + g) * ds + 16 * dt + c], accQ[dt], 0, 0, 0);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * mt + 4 * g + r, d = 16 * dt + c;
        if (i < N) dap[(size_t)i * Dq + d] = accQ[dt][r] - rs[r] * xtr[i * ds + d];
      }
  }
  // ---- test side: Q*^T x and the column sums for this wave's 16 points
  {
    f32x4 accV[DT], cs = zero4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) accV[dt] = zero4;
    for (int kk = 0; kk < NP / 4; ++kk) {
      const float av = Hs[(4 * kk + g) * kKS + 16 * w + c];
      cs = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, cs, 0, 0, 0);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        accV[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xtr[(4 * kk + g) * ds + 16 * dt + c], accV[dt], 0, 0, 0);
    }
    float* dxs = pg_ws(k, k.p.off_dxs) + (size_t)b * Ns * Dq;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * w + 4 * g + r, d = 16 * dt + c;
        if (J + j < Ns) dxs[(size_t)(J + j) * Dq + d] = accV[dt][r] - cs[r] * xs[j * ds + d];
      }
  }
  const float sw = wave_sum(sq);
  if (lane == 0) scr[w] = sw;
  lds_barrier();
  if (tid == 0) pg_ws(k, k.p.off_cp)[(size_t)b * kCpStride + cb] = scr[0] + scr[1] + scr[2] + scr[3];
}

size_t pg_ks_lds(int N, int Ns, int Dq) {
  const int NP = (N + 15) & ~15, NsP = (Ns + 15) & ~15;
  const int HR = NP > NsP ? NP : NsP;
  return ((size_t)HR * kKS + (size_t)(NP + 64) * (Dq + 4) + 256 + 3 * 64 + 256 + 64 + 4) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
// kh (HAT) and kss (!HAT): the two square blocks. HAT: points = training inputs, dK = 1/2 T W^T -
// 1/2 (u alpha^T + alpha u^T); !HAT: points = test inputs, dK = 1/2 H.
// ------------------------------------------------------------------------------------------------
template <int DT, bool HAT>
__global__ __launch_bounds__(256) void gpk_pg_sq_kernel(PgArgs k) {
  constexpr int Dq = 16 * DT, ds = Dq + 4;
  __shared__ __attribute__((aligned(16))) float xi[64 * ds];
  __shared__ __attribute__((aligned(16))) float xj[64 * ds];
  __shared__ __attribute__((aligned(16))) float Pl[64 * kKS];
  __shared__ float ni[64], nj[64], mu[64], lsc[64];
  __shared__ float ui[64], ai[64], uj[64], aj[64];
  __shared__ float scr[8];
  const int N = k.a.N, Ns = k.a.Ns, D = k.a.D, vs = k.p.vs;
  const int n = HAT ? N : Ns;                 // points of this block
  const int nt = HAT ? k.p.nrt : k.p.ncb;     // 64-point tiles
  const int NsP = (Ns + 15) & ~15;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / nt, rt = blockIdx.x - b * nt;
  const int I = 64 * rt;
  const bool hasH = k.a.gvar != nullptr || k.a.gcov != nullptr;
  const bool hasM = k.a.gmean != nullptr;
  const float* hyp = k.a.hyp + (long long)b * k.a.hyp_stride;  // this window's hyper vector (stride 0: shared)
  const float s2 = hyp[0];
  const float* Pb = HAT ? k.a.X + (size_t)b * N * D : k.a.Xs + (size_t)b * Ns * D;
  const float* mup = k.a.state + (size_t)k.a.B * N * vs + (size_t)b * 64;
  const float* Wb = pg_ws(k, k.p.off_W) + (size_t)b * N * vs;
  const float* Tb = pg_ws(k, k.p.off_T) + (size_t)b * N * vs;
  const float* ub = pg_ws(k, k.p.off_u) + (size_t)b * kMaxN;
  const float* alb = pg_ws(k, k.p.off_al) + (size_t)b * kMaxN;
  const float* Gb = (!HAT && k.a.gcov) ? k.a.gcov + (size_t)b * Ns * Ns : nullptr;
  const float* gvb = (!HAT && k.a.gvar) ? k.a.gvar + (size_t)b * Ns : nullptr;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  if (tid < 64) {
    mu[tid] = tid < D ? mup[tid] : 0.f;
    lsc[tid] = tid < D ? hyp[3 + (k.a.n_ls > 1 ? tid : 0)] : 1.f;
    if constexpr (HAT) {   // without gmean, u and alpha were never computed and are not read
      ui[tid] = 0.f;
      ai[tid] = 0.f;
      if (hasM && I + tid < N) {
        ui[tid] = ub[I + tid];
        ai[tid] = alb[I + tid];
      }
    }
  }
  lds_barrier();
  pg_stage<DT>(xi, Pb, I, 64, n, D, lsc, mu, tid);
  lds_barrier();
  pg_norms<DT>(ni, xi, 64, tid);

  f32x4 accPX[DT], accRs = zero4;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) accPX[dt] = zero4;
  float tr = 0.f;

  for (int jb = 0; jb < nt; ++jb) {
    const int J = 64 * jb;
    lds_barrier();   // the previous block's reads of xj and Pl are done
    pg_stage<DT>(xj, Pb, J, 64, n, D, lsc, mu, tid);
    if constexpr (HAT) {
      if (tid < 64) {
        uj[tid] = 0.f;
        aj[tid] = 0.f;
        if (hasM && J + tid < N) {
          uj[tid] = ub[J + tid];
          aj[tid] = alb[J + tid];
        }
      }
    }
    lds_barrier();
    pg_norms<DT>(nj, xj, 64, tid);
    lds_barrier();

    // ---- this wave's 16 columns of the block: dK, then P = dK o K with the diagonal apart
    const int jl = 16 * w + c, gj = J + jl;
    f32x4 acc[4] = {zero4, zero4, zero4, zero4};
    if constexpr (HAT) {
      if (hasH) {
        const float* wr = Wb + (size_t)(gj < N ? gj : 0) * vs + 4 * g;
        for (int k0 = 0; k0 < NsP; k0 += 16) {
          f32x4 bv = *(const f32x4*)&wr[k0];
          if (gj >= N) bv = zero4;
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            const int ir = I + 16 * it + c;
            f32x4 av = *(const f32x4*)&Tb[(size_t)(ir < N ? ir : 0) * vs + k0 + 4 * g];
            if (ir >= N) av = zero4;
#pragma unroll
            for (int s = 0; s < 4; ++s)
              acc[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc[it], 0, 0, 0);
          }
        }
      }
    }
    {
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
          const int il = 16 * it + 4 * g + r, gi = I + il;
          const float d2 = __builtin_fmaxf(ni[il] + njc - 2.f * G[r], 0.f);
          const float kv = s2 * __builtin_amdgcn_exp2f(d2 * kNHalfLog2e);
          float p = 0.f;
          if (gi < n && gj < n) {
            float dk;
            if constexpr (HAT) {
              dk = 0.5f * acc[it][r] - 0.5f * (ui[il] * aj[jl] + ai[il] * uj[jl]);
            } else {
              float h = 0.f;
              if (Gb) h = Gb[(size_t)gi * Ns + gj] + Gb[(size_t)gj * Ns + gi];
              if (gvb && gi == gj) h += 2.f * gvb[gi];
              dk = 0.5f * h;
            }
            if (gi == gj) tr += dk;
            else p = dk * kv;
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
          accPX[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xj[(4 * kk + g) * ds + 16 * dt + c], accPX[dt], 0, 0, 0);
      }
    }
  }

  // ---- da = P x - rowsum(P) o x, twice (db == da); the K* part is added here
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int il = 16 * w + 4 * g + r, gi = I + il, d = 16 * dt + c;
      if (gi >= n) continue;
      float v = 2.f * (accPX[dt][r] - accRs[r] * xi[il * ds + d]);
      if constexpr (HAT) {
        const float* dap = pg_ws(k, k.p.off_dap) + (size_t)b * k.p.ncb * N * Dq + (size_t)gi * Dq + d;
        for (int cb = 0; cb < k.p.ncb; ++cb) v += dap[(size_t)cb * N * Dq];
        pg_ws(k, k.p.off_dxa)[((size_t)b * N + gi) * Dq + d] = v;
      } else {
        pg_ws(k, k.p.off_dxs)[((size_t)b * Ns + gi) * Dq + d] += v;
      }
    }
  float sp = c == 0 ? accRs[0] + accRs[1] + accRs[2] + accRs[3] : 0.f;
  sp = wave_sum(sp);
  const float st = wave_sum(tr);
  if (lane == 0) { scr[w] = sp; scr[4 + w] = st; }
  lds_barrier();
  if (tid == 0) {
    float* cp = pg_ws(k, k.p.off_cp) + (size_t)b * kCpStride + (HAT ? 4 : 12);
    cp[rt] = scr[0] + scr[1] + scr[2] + scr[3];           // sum of Q, the diagonal apart
    cp[4 + rt] = scr[4] + scr[5] + scr[6] + scr[7];       // tr dK
  }
}

// ------------------------------------------------------------------------------------------------
// finish: dX, dXs, dy and dhyp of one window
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpk_pg_finish_kernel(PgArgs k) {
  __shared__ double sh[256];
  __shared__ float lsc[64], mu[64];
  const int N = k.a.N, Ns = k.a.Ns, D = k.a.D, Dq = k.p.Dq, vs = k.p.vs, n_ls = k.a.n_ls;
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* hyp = k.a.hyp + (long long)b * k.a.hyp_stride;  // this window's hyper vector (stride 0: shared)
  const bool hasH = k.a.gvar != nullptr || k.a.gcov != nullptr;
  const bool hasM = k.a.gmean != nullptr;
  const float* Xb = k.a.X + (size_t)b * N * D;
  const float* Xsb = k.a.Xs + (size_t)b * Ns * D;
  const float* dxa = pg_ws(k, k.p.off_dxa) + (size_t)b * N * Dq;
  const float* dxs = pg_ws(k, k.p.off_dxs) + (size_t)b * Ns * Dq;
  const float* ub = pg_ws(k, k.p.off_u) + (size_t)b * kMaxN;
  const float* cp = pg_ws(k, k.p.off_cp) + (size_t)b * kCpStride;
  float* dh = k.a.dhyp + (size_t)b * (3 + n_ls);
  if (tid < 64) {
    mu[tid] = tid < D ? k.a.state[(size_t)k.a.B * N * vs + (size_t)b * 64 + tid] : 0.f;
    lsc[tid] = tid < D ? hyp[3 + (n_ls > 1 ? tid : 0)] : 1.f;
  }
  __syncthreads();
  if (k.a.dX)
    for (int e = tid; e < N * D; e += 256) {
      const int i = e / D, d = e - i * D;
      k.a.dX[(size_t)b * N * D + e] = dxa[(size_t)i * Dq + d] / lsc[d];
    }
  if (k.a.dXs)
    for (int e = tid; e < Ns * D; e += 256) {
      const int i = e / D, d = e - i * D;
      k.a.dXs[(size_t)b * Ns * D + e] = dxs[(size_t)i * Dq + d] / lsc[d];
    }
  if (k.a.dy)
    for (int i = tid; i < N; i += 256) k.a.dy[(size_t)b * N + i] = hasM ? ub[i] : 0.f;

  // dl_d: four interleaved partial sums per dimension, then q ascending
  {
    const int d = tid & 63, q = tid >> 6;
    double s = 0.0;
    if (d < D) {
      const float l = lsc[d], m = mu[d];
      for (int i = q; i < N; i += 4) s += (double)(Xb[(size_t)i * D + d] / l - m) * (double)dxa[(size_t)i * Dq + d];
      for (int j = q; j < Ns; j += 4) s += (double)(Xsb[(size_t)j * D + d] / l - m) * (double)dxs[(size_t)j * Dq + d];
      s = -s / (double)l;
    }
    sh[tid] = s;
    __syncthreads();
    if (tid < 64) sh[tid] = sh[tid] + sh[64 + tid] + sh[128 + tid] + sh[192 + tid];
    __syncthreads();
    if (n_ls > 1) {
      if (tid < D) dh[3 + tid] = (float)sh[tid];
    } else if (tid == 0) {
      double t = 0.0;
      for (int dd = 0; dd < D; ++dd) t += sh[dd];
      dh[3] = (float)t;
    }
    __syncthreads();
  }
  // dc = sum gmean - sum u: strided partial sums, then a fixed tree
  {
    double s = 0.0;
    if (hasM) {
      for (int j = tid; j < Ns; j += 256) s += (double)k.a.gmean[(size_t)b * Ns + j];
      for (int i = tid; i < N; i += 256) s -= (double)ub[i];
    }
    sh[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) sh[tid] += sh[tid + off];
      __syncthreads();
    }
  }
  if (tid == 0) {
    double sq = 0.0, tr = 0.0, trh = 0.0;
    for (int cb = 0; cb < k.p.ncb; ++cb) sq += (double)cp[cb];
    for (int rt = 0; rt < k.p.nrt; ++rt) { sq += (double)cp[4 + rt]; tr += (double)cp[8 + rt]; }
    if (hasH)
      for (int cb = 0; cb < k.p.ncb; ++cb) { sq += (double)cp[12 + cb]; trh += (double)cp[16 + cb]; }
    dh[0] = (float)(sq / (double)hyp[0] + tr + trh);
    dh[1] = (float)tr;
    dh[2] = (float)sh[0];
  }
}

bool pg_shape_ok(int B, int N, int Ns, int D) {
  return B >= 0 && N >= 1 && N <= kMaxN && Ns >= 1 && Ns <= kGpkMvnRootMaxN && D >= 1 && D <= 64 &&
         (long long)B * 5 <= 0x7fffffffLL;   // backsub: up to 5 column tiles per window on grid x
}

}  // namespace

size_t gpk_post_grad_ws_bytes(int B, int N, int Ns, int D) {
  if (!pg_shape_ok(B, N, Ns, D)) return 0;
  return pg_plan(B, N, Ns, D).total * sizeof(float);
}

int gpk_launch_exact_posterior_grad(const GpkPostGradArgs& a, hipStream_t stream) {
  if (!pg_shape_ok(a.B, a.N, a.Ns, a.D)) return -11;
  // ks opts in to more than the default 64 KB of dynamic LDS: once per device (the attribute
  // belongs to the current device's copy of the kernel), and a refusal is this call's error
  // (-12: the shape needs more LDS than the device grants), not a failed launch further down.
  {
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return -12; }
    std::lock_guard<std::mutex> lock(mu);
    if (!done[dev]) {
      const hipFuncAttribute at = hipFuncAttributeMaxDynamicSharedMemorySize;
      if (hipFuncSetAttribute((const void*)gpk_pg_ks_kernel<1>, at, 160 * 1024) != hipSuccess ||
          hipFuncSetAttribute((const void*)gpk_pg_ks_kernel<2>, at, 160 * 1024) != hipSuccess ||
          hipFuncSetAttribute((const void*)gpk_pg_ks_kernel<4>, at, 160 * 1024) != hipSuccess) {
        (void)hipGetLastError();
        return -12;
      }
      done[dev] = true;
    }
  }
  PgArgs k{a, pg_plan(a.B, a.N, a.Ns, a.D), 0};
  const bool hasH = a.gvar != nullptr || a.gcov != nullptr;
  const bool hasM = a.gmean != nullptr;
  k.tca = hasM ? (a.Ns + 1 + 63) / 64 : k.p.ncb;
  const unsigned B = (unsigned)a.B;
  const size_t lds = pg_ks_lds(a.N, a.Ns, k.p.Dq);
  if (lds > 160 * 1024) return -11;

  hipLaunchKernelGGL(gpk_pg_backsub_kernel, dim3(B * k.tca), dim3(256), 0, stream, k);
  if (hasM) hipLaunchKernelGGL(gpk_pg_u_kernel, dim3(B), dim3(256), 0, stream, k);
  if (k.p.Dq == 16) {
    hipLaunchKernelGGL(gpk_pg_ks_kernel<1>, dim3(B * k.p.ncb), dim3(256), lds, stream, k);
    hipLaunchKernelGGL((gpk_pg_sq_kernel<1, true>), dim3(B * k.p.nrt), dim3(256), 0, stream, k);
    if (hasH) hipLaunchKernelGGL((gpk_pg_sq_kernel<1, false>), dim3(B * k.p.ncb), dim3(256), 0, stream, k);
  } else if (k.p.Dq == 32) {
    hipLaunchKernelGGL(gpk_pg_ks_kernel<2>, dim3(B * k.p.ncb), dim3(256), lds, stream, k);
    hipLaunchKernelGGL((gpk_pg_sq_kernel<2, true>), dim3(B * k.p.nrt), dim3(256), 0, stream, k);
    if (hasH) hipLaunchKernelGGL((gpk_pg_sq_kernel<2, false>), dim3(B * k.p.ncb), dim3(256), 0, stream, k);
  } else {
    hipLaunchKernelGGL(gpk_pg_ks_kernel<4>, dim3(B * k.p.ncb), dim3(256), lds, stream, k);
    hipLaunchKernelGGL((gpk_pg_sq_kernel<4, true>), dim3(B * k.p.nrt), dim3(256), 0, stream, k);
    if (hasH) hipLaunchKernelGGL((gpk_pg_sq_kernel<4, false>), dim3(B * k.p.ncb), dim3(256), 0, stream, k);
  }
  hipLaunchKernelGGL(gpk_pg_finish_kernel, dim3(B), dim3(256), 0, stream, k);
  return (int)hipGetLastError();
}
