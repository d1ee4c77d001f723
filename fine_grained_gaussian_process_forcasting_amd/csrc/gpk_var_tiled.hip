// Variational hot path, LDS-tiled unit (today only the fallback): gpk_var_fwd_kernel and
// gpk_var_adj_kernel. Shapes: M <= 64 with D in (32, 64], and the M > 64 adjoints the
// L^{-1}-in-registers path leaves over (its LDS plan does not fit, or the dA / K_ZX workspace
// reaches 2 GB); with GPK_VAR_REG=0 / GPK_VAR_LREG=0 (A/B builds) every shape of those paths.
//   gpk_var_fwd_kernel  the per-point work as ONE column-tiled GEMM A = L^{-1} [K_ZX(b=0) | ...]:
//                       a workgroup owns a chunk of TW points of one window and all M rows of A;
//                       K_ZX chunk from an f32-MFMA Gram (GPyTorch's centred _sq_dist form) in
//                       LDS, A in fp64 MFMA accumulators (v_mfma_f64_16x16x4f64, triangular
//                       k-range per row tile), mean / variance reduced in the epilogue.
//   gpk_var_adj_kernel  adjoint, same tiling: recomputes K_ZX, A; dA; dK = L^{-T} dA (fp64 MFMA);
//                       Q = dK o K_ZX; dX per point, and per-workgroup partials of
//                       Q X (M x D), sum_i Q, dvmean, dvstd, ds2, dl (deterministic, no atomics);
//                       dA and K_ZX (fp32, as the reference's fp32 dA) go to the workspace for
//                       gpk_dlinv_kernel (gpk_var_tail.hip).
#include "gpk_var_common.h"
#include "gpk_var_launch.h"

// Timing experiments only (A/B builds of the adjoint; results are wrong when set): bit 1
// skips A = L^-1 K_ZX, 2 dK = L^-T dA, 4 the dA / K_ZX workspace stores, 8 the Q / Q^T zs /
// QX section, 16 the q column sums, 32 the dX loop.
#ifndef GPK_VAR_SKIP
#define GPK_VAR_SKIP 0
#endif


namespace {

// Stage the chunk's points xs = x/l - cm (invalid columns zero) and their norms.
GPK_DEVICE void stage_points(const float* __restrict__ Xw, const float* __restrict__ ls, int nvalid,
                             int D, int TW, int Dq, int ds, const float* cm, float* xs, float* xn) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int base = 0; base < TW * Dq; base += 4 * T) {   // loads in flight together (stage_inducing)
    float v[4], l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * T + tid, j = e / Dq, d = e - j * Dq;
      const bool ok = e < TW * Dq && j < nvalid && d < D;
      v[u] = Xw[ok ? (size_t)j * D + d : 0];
      l[u] = ls[ok ? d : 0];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * T + tid, j = e / Dq, d = e - j * Dq;
      if (e < TW * Dq) xs[j * ds + d] = (j < nvalid && d < D) ? v[u] / l[u] - cm[d] : 0.f;
    }
  }
  lds_barrier();
  for (int j = tid; j < TW; j += T) {
    float s = 0.f;
    for (int d = 0; d < Dq; ++d) s = __builtin_fmaf(xs[j * ds + d], xs[j * ds + d], s);
    xn[j] = s;
  }
}

// K_ZX chunk (MP x TW, LDS) = s2 exp(-0.5 clamp(|zs|^2 + |xs|^2 - 2 zs.xs, 0)) on f32 MFMA.
template <int MB, int TW>
GPK_DEVICE void build_kzx(const float* zs, const float* xs, const float* zn, const float* xn,
                          int M, int nvalid, int Dq, int ds, float s2, float* Kl) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = threadIdx.x >> 6;
  constexpr int NCT = TW / 16;
  for (int t = wave; t < MB * NCT; t += 4) {
    const int rt = t / NCT, ct = t - rt * NCT;
    const float* za = zs + (16 * rt + c) * ds + g;
    const float* xb = xs + (16 * ct + c) * ds + g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Dq / 4; ++k) acc = mfma32(za[4 * k], xb[4 * k], acc);
    const int col = 16 * ct + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = 16 * rt + 4 * g + r;
      float dist = zn[p] + xn[col] - 2.f * acc[r];
      dist = dist < 0.f ? 0.f : dist;
      Kl[p * TW + col] = (p < M && col < nvalid) ? s2 * __builtin_amdgcn_exp2f(kNHalfLog2e * dist) : 0.f;
    }
  }
}

// A = L^{-1} K_ZX for the wave's row tiles (fp64 MFMA). acc[j][q][r] = A[16 rt_j + g + 4r][16 ct_q + c].
// The contraction runs in k-blocks of 16 inducing points; inside a block MFMA step u
// takes p = 16 kb + 4 g + u on lane group g (any consistent k-order is legal), so a
// lane's four A operands of a block are 4 consecutive doubles of one L^{-1} row. The
// whole next block's A operands are loaded while the current block's MFMAs run (row
// tile rt only needs blocks kb <= rt: L^{-1} is lower triangular).
template <int MB>
GPK_DEVICE void gemm_linv_k(const double* __restrict__ Linv, const float* Kl, int M,
                            f64x4 (&acc)[VarGeo<MB>::RT][VarGeo<MB>::CT]) {
  using G = VarGeo<MB>;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / G::WC, wc = wave - wr * G::WC;
#pragma unroll
  for (int j = 0; j < G::RT; ++j)
#pragma unroll
    for (int q = 0; q < G::CT; ++q) acc[j][q] = f64x4{0.0, 0.0, 0.0, 0.0};
  int last = 0;
#pragma unroll
  for (int j = 0; j < G::RT; ++j)
    if (wr + G::WR * j < MB) last = wr + G::WR * j;
  double an[G::RT][4];
  auto load_blk = [&](int kb, double (&dst)[G::RT][4]) {
#pragma unroll
    for (int j = 0; j < G::RT; ++j) {
      const int rt = wr + G::WR * j;
      const int m = 16 * rt + c;
      const bool ok = rt < MB && kb <= rt && m < M;
      const double* row = Linv + (size_t)(ok ? m : 0) * M;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = 16 * kb + 4 * g + u;
        dst[j][u] = (ok && p < M) ? row[p] : 0.0;
      }
    }
  };
  load_blk(0, an);
  for (int kb = 0; kb <= last; ++kb) {
    double a[G::RT][4];
#pragma unroll
    for (int j = 0; j < G::RT; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) a[j][u] = an[j][u];
    if (kb < last) load_blk(kb + 1, an);
    float bf[G::CT][4];
#pragma unroll
    for (int q = 0; q < G::CT; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) bf[q][u] = Kl[(16 * kb + 4 * g + u) * G::TW + 16 * (wc * G::CT + q) + c];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < G::RT; ++j) {
        const int rt = wr + G::WR * j;
        if (rt < MB && kb <= rt) {
#pragma unroll
          for (int q = 0; q < G::CT; ++q) acc[j][q] = mfma64(a[j][u], (double)bf[q][u], acc[j][q]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Forward: mean / variance of q(f) for every point (workgroups walk the chunk list).
// ---------------------------------------------------------------------------
template <int MB>
__global__ void __launch_bounds__(256)
gpk_var_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Z,
                   const double* __restrict__ Linv, const float* __restrict__ vmean,
                   const float* __restrict__ vstd, const float* __restrict__ hyp, int N, int M,
                   int D, int nchunks, float* __restrict__ mean_out, float* __restrict__ var_out,
                   int* __restrict__ flags, GpkOStr bs) {
  GPK_O_MODEL();
  GPK_O_ADD(Linv, M * M);
  GPK_O_ADD(mean_out, bs.bn);
  GPK_O_ADD(var_out, bs.bn);
  using G = VarGeo<MB>;
  constexpr int TW = G::TW, MP = G::MP;
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  const int Dq = dq_of(D), ds = Dq + 2;
  float* zs = vsm;                 // MP x ds
  float* xs = zs + MP * ds;        // TW x ds
  float* zn = xs + TW * ds;        // MP
  float* xn = zn + MP;             // TW
  float* vm = xn + TW;             // MP
  float* sm1 = vm + MP;            // MP
  float* cm = sm1 + MP;            // Dq
  float* Kl = cm + Dq;             // MP x TW
  float* redm = Kl + MP * TW;      // WR x TW
  float* redv = redm + G::WR * TW; // WR x TW
  const int tid = threadIdx.x;
  const int lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / G::WC, wc = wave - wr * G::WC;
  // hyp: [s2, noise, jitter, b0, w[D], ls[D]]
  const float s2 = hyp[0], jit = hyp[2], b0 = hyp[3];
  const float* w = hyp + 4;
  const float* ls = hyp + 4 + D;

  stage_inducing(Z, ls, vmean, vstd, M, D, MP, Dq, ds, zs, zn, cm, vm, sm1, Kl);
  const int nch = (N + TW - 1) / TW;
  int clamped = 0;
  // grid-stride over (window, chunk) pairs: the inducing-point staging is paid once
  for (int t = blockIdx.x; t < nchunks; t += gridDim.x) {
    const int b = t / nch, ch = t - b * nch;
    const int i0 = ch * TW;
    const int nvalid = N - i0 < TW ? N - i0 : TW;
    const float* Xw = X + ((size_t)b * N + i0) * D;
    lds_barrier();  // previous chunk done with xs / Kl / red; zs staged
    stage_points(Xw, ls, nvalid, D, TW, Dq, ds, cm, xs, xn);
    lds_barrier();
    build_kzx<MB, TW>(zs, xs, zn, xn, M, nvalid, Dq, ds, s2, Kl);
    lds_barrier();
    f64x4 acc[G::RT][G::CT];
    gemm_linv_k<MB>(Linv, Kl, M, acc);
    // epilogue: partial sum_m A m_m and sum_m A^2 (s_m^2 - 1) over the wave's rows
#pragma unroll
    for (int q = 0; q < G::CT; ++q) {
      float mp = 0.f, vp = 0.f;
#pragma unroll
      for (int j = 0; j < G::RT; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * (wr + G::WR * j) + g + 4 * r;
          const float a32 = (float)acc[j][q][r];  // A is cast to fp32 (reference)
          const int rr = row < MP ? row : 0;
          mp = __builtin_fmaf(a32, row < MP ? vm[rr] : 0.f, mp);
          vp = __builtin_fmaf(a32 * a32, row < MP ? sm1[rr] : 0.f, vp);
        }
      }
      mp += __shfl_xor(mp, 16, 64);
      mp += __shfl_xor(mp, 32, 64);
      vp += __shfl_xor(vp, 16, 64);
      vp += __shfl_xor(vp, 32, 64);
      if (g == 0) {
        redm[wr * TW + 16 * (wc * G::CT + q) + c] = mp;
        redv[wr * TW + 16 * (wc * G::CT + q) + c] = vp;
      }
    }
    lds_barrier();
    for (int col = tid; col < nvalid; col += blockDim.x) {
      float mm = 0.f, vv = 0.f;
#pragma unroll
      for (int q = 0; q < G::WR; ++q) {
        mm += redm[q * TW + col];
        vv += redv[q * TW + col];
      }
      const float* xr = Xw + (size_t)col * D;
      float lin = 0.f;
      for (int d = 0; d < D; ++d) lin = __builtin_fmaf(xr[d], w[d], lin);
      const float mean_i = mm + (lin + b0);
      float var_i = s2 + jit + vv;
      if (var_i < 1e-6f) { var_i = 1e-6f; clamped = 1; }  // MVN.variance clamp (fp32)
      mean_out[(size_t)b * N + i0 + col] = mean_i;
      var_out[(size_t)b * N + i0 + col] = var_i;
    }
  }
  if (flags != nullptr && clamped)
    (void)__hip_atomic_fetch_or(flags, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// Adjoint of the forward for the objective sum(gmean * mean) + sum(gvar * var).
// Per chunk (same tiling as the forward):
//   K_ZX (LDS), A = L^{-1} K_ZX (fp64 MFMA), var -> clamp mask on gvar,
//   dA = gmean_i m_m + 2 gvar_i (s_m^2 - 1) A_mi   (fp32: the reference's dA is the
//        gradient of an fp32 tensor), dA and K_ZX -> workspace for dL^{-1},
//   dK = L^{-T} dA (fp64 MFMA), Q = dK o K_ZX,
//   dX_i = (sum_p Q_pi zs_p - xs_i sum_p Q_pi) / l + gmean_i w     (written per point)
//   partials per workgroup: QX_p = sum_i Q_pi xs_i, q_p = sum_i Q_pi, sum_i gmean A,
//   sum_i gvar A^2, sum_i r_i xs_i^2, sum Q, sum gvar (reduced by gpk_var_red_kernel).
// ---------------------------------------------------------------------------
template <int MB, int DQ>
__global__ void __launch_bounds__(256, 1)
gpk_var_adj_kernel(const float* __restrict__ X, const float* __restrict__ Z,
                   const double* __restrict__ Linv, const float* __restrict__ vmean,
                   const float* __restrict__ vstd, const float* __restrict__ hyp,
                   const float* __restrict__ gmean, const float* __restrict__ gvar, int N, int M,
                   int D, int nchunks, long long BN, float* __restrict__ wsdA, float* __restrict__ wsK,
                   float* __restrict__ wspart, float* __restrict__ dX, GpkOStr bs) {
  GPK_O_MODEL();
  GPK_O_ADD(Linv, M * M);
  GPK_O_ADD(gmean, bs.bn);
  GPK_O_ADD(gvar, bs.bn);
  GPK_O_ADD(wsdA, bs.ws);
  GPK_O_ADD(wsK, bs.ws);
  GPK_O_ADD(wspart, bs.ws);
  GPK_O_ADD(dX, bs.bn * D);
  using G = VarGeo<MB>;
  constexpr int TW = G::TW, MP = G::MP, QST = G::QST;
  constexpr int Dq = DQ, ds = DQ + 2, NDT = DQ / 16;
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  float* zs = vsm;                    // MP x ds
  float* xs = zs + MP * ds;           // TW x ds
  float* zn = xs + TW * ds;           // MP
  float* xn = zn + MP;                // TW
  float* vm = xn + TW;                // MP
  float* sm1 = vm + MP;               // MP
  float* cm = sm1 + MP;               // Dq
  float* gmc = cm + Dq;               // TW
  float* gvc = gmc + TW;              // TW
  float* rcol = gvc + TW;             // TW   r_i = sum_p Q_pi
  float* qacc = rcol + TW;            // MP   sum_i Q_pi (this workgroup)
  float* dvma = qacc + MP;            // WC x MP
  float* dsma = dvma + G::WC * MP;    // WC x MP
  float* rx2 = dsma + G::WC * MP;     // 256  per-thread sum r_i xs_i^2 (thread -> one d)
  float* gxa = rx2 + 256;             // 256  per-thread sum gmean_i xs_i (thread -> one d)
  float* redw = gxa + 256;            // 2 x WR x TW
  float* Kl = redw + 2 * G::WR * TW;  // MP x TW     (later: Q^T zs partials, WR x TW x Dq)
  constexpr int KLN = MP * TW > G::WR * TW * DQ ? MP * TW : G::WR * TW * DQ;
  float* dAl = Kl + KLN;              // MP x TW dA  (later: Q^T, TW x QST)
  const int tid = threadIdx.x;
  const int lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / G::WC, wc = wave - wr * G::WC;
  const float s2 = hyp[0], jit = hyp[2];
  const float* w = hyp + 4;
  const float* ls = hyp + 4 + D;

  stage_inducing(Z, ls, vmean, vstd, M, D, MP, Dq, ds, zs, zn, cm, vm, sm1, Kl);
  for (int m = tid; m < MP; m += blockDim.x) {
    qacc[m] = 0.f;
    for (int q = 0; q < G::WC; ++q) { dvma[q * MP + m] = 0.f; dsma[q * MP + m] = 0.f; }
  }
  rx2[tid] = 0.f;
  gxa[tid] = 0.f;
  float sumQ = 0.f, sumgv = 0.f, sumgm = 0.f;
  // persistent f32 accumulators of QX = sum_i Q_pi xs_i: tiles (pt, dt) dealt over the waves
  constexpr int MAXQT = (MB * NDT + 3) / 4;  // QX tiles (MB x NDT) dealt over 4 waves
  f32x4 qx[MAXQT];
#pragma unroll
  for (int u = 0; u < MAXQT; ++u) qx[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nch = (N + TW - 1) / TW;
#pragma unroll 1
  for (int t = blockIdx.x; t < nchunks; t += gridDim.x) {
    const int b = t / nch, ch = t - b * nch;
    const int i0 = ch * TW;
    const int nvalid = N - i0 < TW ? N - i0 : TW;
    const size_t col0 = (size_t)b * N + i0;
    const float* Xw = X + col0 * D;
    lds_barrier();
    stage_points(Xw, ls, nvalid, D, TW, Dq, ds, cm, xs, xn);
    for (int j = tid; j < TW; j += blockDim.x) {
      gmc[j] = j < nvalid ? gmean[col0 + j] : 0.f;
      gvc[j] = j < nvalid ? gvar[col0 + j] : 0.f;
    }
    lds_barrier();
    build_kzx<MB, TW>(zs, xs, zn, xn, M, nvalid, Dq, ds, s2, Kl);
    lds_barrier();
    f64x4 acc[G::RT][G::CT];
    if (!(GPK_VAR_SKIP & 1)) gemm_linv_k<MB>(Linv, Kl, M, acc);
    else {
#pragma unroll
      for (int j = 0; j < G::RT; ++j)
#pragma unroll
        for (int q = 0; q < G::CT; ++q) acc[j][q] = f64x4{0.1, 0.1, 0.1, 0.1};
    }
    // variance -> clamp mask (no gradient below the clamp)
#pragma unroll
    for (int q = 0; q < G::CT; ++q) {
      float vp = 0.f;
#pragma unroll
      for (int j = 0; j < G::RT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * (wr + G::WR * j) + g + 4 * r;
          const float a32 = (float)acc[j][q][r];
          vp = __builtin_fmaf(a32 * a32, row < MP ? sm1[row] : 0.f, vp);
        }
      vp += __shfl_xor(vp, 16, 64);
      vp += __shfl_xor(vp, 32, 64);
      if (g == 0) redw[wr * TW + 16 * (wc * G::CT + q) + c] = vp;
    }
    lds_barrier();
    for (int col = tid; col < TW; col += blockDim.x) {
      float vv = 0.f;
      for (int q = 0; q < G::WR; ++q) vv += redw[q * TW + col];
      if (s2 + jit + vv < 1e-6f) gvc[col] = 0.f;  // clamp_min(1e-6): gradient masked
      sumgv += gvc[col];
      sumgm += gmc[col];
    }
    lds_barrier();
    // dA (fp32) -> LDS + workspace; partial sums for dvmean / dvstd
#pragma unroll
    for (int j = 0; j < G::RT; ++j) {
      const int rt = wr + G::WR * j;
      if (rt >= MB) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * rt + g + 4 * r;
        float pm = 0.f, ps = 0.f;
#pragma unroll
        for (int q = 0; q < G::CT; ++q) {
          const int col = 16 * (wc * G::CT + q) + c;
          const float a32 = (float)acc[j][q][r];
          const float gm = gmc[col], gv = gvc[col];
          const float da = gm * vm[row] + 2.f * gv * sm1[row] * a32;
          dAl[row * TW + col] = da;
          if (row < M && col < nvalid && !(GPK_VAR_SKIP & 4)) wsdA[(size_t)row * BN + col0 + col] = da;
          pm = __builtin_fmaf(gm, a32, pm);
          ps = __builtin_fmaf(gv, a32 * a32, ps);
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          pm += __shfl_xor(pm, off, 64);
          ps += __shfl_xor(ps, off, 64);
        }
        if (c == 0) {
          dvma[wc * MP + row] += pm;
          dsma[wc * MP + row] += ps;
        }
      }
    }
    // K_ZX -> workspace (row-major M x BN, coalesced along points)
    for (int e = tid; e < M * TW && !(GPK_VAR_SKIP & 4); e += blockDim.x) {
      const int p = e / TW, col = e - p * TW;
      if (col < nvalid) wsK[(size_t)p * BN + col0 + col] = Kl[p * TW + col];
    }
    lds_barrier();
    // dK = L^{-T} dA (fp64 MFMA): output rows p = the wave's row tiles, k = m >= p, in
    // k-blocks of 16 (k-order m = 16 kb + 4 g + u), next block's operands prefetched
    {
      int first = MB;
#pragma unroll
      for (int j = 0; j < G::RT; ++j) {
        const int rt = wr + G::WR * j;
        if (rt < MB) first = rt < first ? rt : first;
      }
#pragma unroll
      for (int j = 0; j < G::RT; ++j)
#pragma unroll
        for (int q = 0; q < G::CT; ++q) acc[j][q] = f64x4{0.0, 0.0, 0.0, 0.0};
      double an[G::RT][4];
      auto load_blk = [&](int kb, double (&dst)[G::RT][4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int m = 16 * kb + 4 * g + u;
          const double* row = Linv + (size_t)(m < M ? m : 0) * M;
#pragma unroll
          for (int j = 0; j < G::RT; ++j) {
            const int rt = wr + G::WR * j;
            const int p = 16 * rt + c;
            dst[j][u] = (rt < MB && kb >= rt && m < M && p < M) ? row[p] : 0.0;
          }
        }
      };
      load_blk(first, an);
      for (int kb = first; kb < MB && !(GPK_VAR_SKIP & 2); ++kb) {
        double a[G::RT][4];
#pragma unroll
        for (int j = 0; j < G::RT; ++j)
#pragma unroll
          for (int u = 0; u < 4; ++u) a[j][u] = an[j][u];
        if (kb + 1 < MB) load_blk(kb + 1, an);
        float bf[G::CT][4];
#pragma unroll
        for (int q = 0; q < G::CT; ++q)
#pragma unroll
          for (int u = 0; u < 4; ++u) bf[q][u] = dAl[(16 * kb + 4 * g + u) * TW + 16 * (wc * G::CT + q) + c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int j = 0; j < G::RT; ++j) {
            const int rt = wr + G::WR * j;
            if (rt < MB && kb >= rt) {
#pragma unroll
              for (int q = 0; q < G::CT; ++q) acc[j][q] = mfma64(a[j][u], (double)bf[q][u], acc[j][q]);
            }
          }
        }
      }
    }
    lds_barrier();  // every wave is done reading dAl
    // Q = dK o K_ZX: Q^T -> LDS (over dAl), sum Q, r_i partials, and Q^T zs on f32 MFMA
    f32x4 xz[G::CT][NDT];
#pragma unroll
    for (int q = 0; q < G::CT; ++q)
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) xz[q][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float rp[G::CT] = {};
#pragma unroll
    for (int j = 0; j < G::RT; ++j) {
      const int rt = wr + G::WR * j;
      if (rt >= MB || (GPK_VAR_SKIP & 8)) continue;
#pragma unroll
      for (int q = 0; q < G::CT; ++q) {
        const int col = 16 * (wc * G::CT + q) + c;
        float qv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rt + g + 4 * r;
          qv[r] = (float)acc[j][q][r] * Kl[row * TW + col];
          dAl[col * QST + row] = qv[r];
          sumQ += qv[r];
          rp[q] += qv[r];
        }
        // (Q^T zs)[col][d] += sum over this tile's rows (k-order g + 4r)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            xz[q][dt] = mfma32(qv[r], zs[(16 * rt + g + 4 * r) * ds + 16 * dt + c], xz[q][dt]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < G::CT; ++q) {
      float v = rp[q];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (g == 0) redw[wr * TW + 16 * (wc * G::CT + q) + c] = v;
    }
    lds_barrier();  // Q^T complete, K_ZX no longer needed, r partials in redw
    // Q^T zs partials -> LDS (over Kl): [wr][col][d]; xz[q][dt][r] = (Q^T zs)[16ct + 4g + r][16dt + c]
#pragma unroll
    for (int q = 0; q < G::CT; ++q)
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = 16 * (wc * G::CT + q) + 4 * g + r;
          Kl[(wr * TW + col) * Dq + 16 * dt + c] = xz[q][dt][r];
        }
      }
    for (int col = tid; col < TW; col += blockDim.x) {
      float v = 0.f;
      for (int q = 0; q < G::WR; ++q) v += redw[q * TW + col];
      rcol[col] = v;
    }
    // QX += sum_i Q_pi xs_i (f32 MFMA, A = Q from Q^T, B = xs); tiles dealt over the waves
#pragma unroll
    for (int u = 0; u < MAXQT; ++u) {
      const int tq = wave + 4 * u;
      if (tq < MB * NDT && !(GPK_VAR_SKIP & 8)) {
        const int pt = tq / NDT, dt = tq - pt * NDT;
        for (int k = 0; k < TW / 4; ++k)
          qx[u] = mfma32(dAl[(4 * k + g) * QST + 16 * pt + c], xs[(4 * k + g) * ds + 16 * dt + c], qx[u]);
      }
    }
    for (int p = tid; p < MP && !(GPK_VAR_SKIP & 16); p += blockDim.x) {
      float v = 0.f;
      for (int i = 0; i < TW; ++i) v += dAl[i * QST + p];
      qacc[p] += v;
    }
    lds_barrier();  // Q^T zs partials and r complete
    // dX per point; sum_i r_i xs_i^2 per d (thread tid always sees d = tid % Dq)
    for (int e = tid; e < TW * Dq && !(GPK_VAR_SKIP & 32); e += blockDim.x) {
      const int col = e / Dq, d = e - col * Dq;
      float v = 0.f;
      for (int q = 0; q < G::WR; ++q) v += Kl[(q * TW + col) * Dq + d];
      const float xv = xs[col * ds + d];
      const float r = rcol[col];
      if (col < nvalid && d < D) {
        dX[(col0 + col) * D + d] = (v - xv * r) / ls[d] + gmc[col] * w[d];
        rx2[tid] += r * xv * xv;
        gxa[tid] += gmc[col] * xv;   // LinearMean: dw = l (sum gmean xs + cm sum gmean)
      }
    }
  }
  lds_barrier();
  // per-workgroup partials:
  //   [QX (M x D) | q (M) | dvm (M) | dsm (M) | rx2 (D) | sumQ | sumgv | gx (D) | sumgm]
  const int P = M * D + 3 * M + 2 * D + 3;
  float* po = wspart + (size_t)blockIdx.x * P;
#pragma unroll
  for (int u = 0; u < MAXQT; ++u) {
    const int tq = wave + 4 * u;
    if (tq < MB * NDT) {
      const int pt = tq / NDT, dt = tq - pt * NDT;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 16 * pt + 4 * g + r, d = 16 * dt + c;
        if (p < M && d < D) po[p * D + d] = qx[u][r];
      }
    }
  }
  for (int m = tid; m < M; m += blockDim.x) {
    float a = 0.f, s = 0.f;
    for (int q = 0; q < G::WC; ++q) { a += dvma[q * MP + m]; s += dsma[q * MP + m]; }
    po[M * D + m] = qacc[m];
    po[M * D + M + m] = a;
    po[M * D + 2 * M + m] = s;
  }
  // sum r xs^2 and gmean xs over the threads that accumulated the same d (d = tid % Dq)
  for (int d = tid; d < D; d += blockDim.x) {
    float v = 0.f, u = 0.f;
    for (int t = d; t < 256; t += Dq) { v += rx2[t]; u += gxa[t]; }
    po[M * D + 3 * M + d] = v;
    po[M * D + 3 * M + D + 2 + d] = u;
  }
  sumQ = wave_sum(sumQ);
  if (lane == 0) redw[wave] = sumQ;
  lds_barrier();  // rx2 / gxa read, sumQ partials out
  rx2[tid] = sumgv;  // accumulated by the column threads
  gxa[tid] = sumgm;
  lds_barrier();
  if (tid == 0) {
    float v = 0.f, u = 0.f;
    for (int t = 0; t < 256; ++t) { v += rx2[t]; u += gxa[t]; }
    po[M * D + 3 * M + D] = (redw[0] + redw[1]) + (redw[2] + redw[3]);
    po[M * D + 3 * M + D + 1] = v;
    po[M * D + 3 * M + 2 * D + 2] = u;
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <int MB>
size_t var_fwd_lds(int D) {
  using G = VarGeo<MB>;
  const int Dq = dq_of(D), ds = Dq + 2;
  return (size_t)(G::MP * ds + G::TW * ds + G::MP + G::TW + 2 * G::MP + Dq + G::MP * G::TW +
                  2 * G::WR * G::TW) * sizeof(float);
}

template <int MB, int DQ>
size_t var_adj_lds() {
  using G = VarGeo<MB>;
  const int Dq = DQ, ds = Dq + 2;
  const size_t kl = (size_t)G::MP * G::TW > (size_t)G::WR * G::TW * Dq ? (size_t)G::MP * G::TW
                                                                       : (size_t)G::WR * G::TW * Dq;
  const size_t da = (size_t)G::MP * G::TW > (size_t)G::TW * G::QST ? (size_t)G::MP * G::TW
                                                                   : (size_t)G::TW * G::QST;
  return ((size_t)G::MP * ds + G::TW * ds + G::MP + G::TW + 2 * G::MP + Dq + 3 * G::TW + G::MP +
          2 * G::WC * G::MP + 2 * 256 + 2 * G::WR * G::TW + kl + da) * sizeof(float);
}

template <int MB>
int launch_var_fwd(const GpkVarArgs& a, int* flags, hipStream_t stream) {
  using G = VarGeo<MB>;
  const size_t lds = var_fwd_lds<MB>(a.D);
  if (lds > 160 * 1024) return -11;
  set_lds_once<gpk_var_fwd_kernel<MB>>();
  const long long nch = (long long)a.B * ((a.N + G::TW - 1) / G::TW);
  if (nch > 0x7fffffffLL) return -8;
  hipLaunchKernelGGL((gpk_var_fwd_kernel<MB>), dim3(chunk_grid(nch, 4), a.O), dim3(256), lds, stream,
                     a.X, a.Z, a.Linv, a.vmean, a.vstd, a.hyp, a.N, a.M, a.D, (int)nch, a.mean,
                     a.var, flags, fwd_strides(a));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return a.ell != nullptr ? gpk_launch_var_ell(a, stream) : 0;
}

template <int MB, int DQ>
int launch_var_adj(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream) {
  const GpkOStr bs = adj_strides(a, p.total);   // output o works in workspace slice o
  char* ws = (char*)a.ws;
  float* wsdA = (float*)(ws + p.off_dA);
  float* wsK = (float*)(ws + p.off_K);
  float* wspart = (float*)(ws + p.off_part);
  const size_t lds = var_adj_lds<MB, DQ>();
  if (lds > 160 * 1024) return -12;
  set_lds_once<gpk_var_adj_kernel<MB, DQ>>();
  hipLaunchKernelGGL((gpk_var_adj_kernel<MB, DQ>), dim3(p.nwg, a.O), dim3(256), lds, stream, a.X, a.Z,
                     a.Linv, a.vmean, a.vstd, a.hyp, a.gmean, a.gvar, a.N, a.M, a.D, p.nchunks,
                     p.BN, wsdA, wsK, wspart, a.dX, bs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return gpk_launch_var_adj_tail(a, p, stream);
}

}  // namespace

// Instantiations no shape reaches while a switch is on are left out: the L^{-1}-in-registers
// forward serves every M > 64, the register path every M <= 64 with D <= 32.
int gpk_launch_var_fwd_tiled(const GpkVarArgs& a, int* flags, hipStream_t stream) {
#define GPK_CALL_FWD(mb) \
  if constexpr (!(GPK_VAR_LREG && mb > 4)) return launch_var_fwd<mb>(a, flags, stream);
  GPK_MB_SWITCH((a.M + 15) / 16, GPK_CALL_FWD)
#undef GPK_CALL_FWD
  return -10;
}

int gpk_launch_var_adj_tiled(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream) {
#define GPK_CALL_ADJ(mb)                                                        \
  if (a.D > 32) return launch_var_adj<mb, 64>(a, p, stream);                    \
  if constexpr (!(GPK_VAR_REG && mb <= 4)) return launch_var_adj<mb, 32>(a, p, stream);
  GPK_MB_SWITCH((a.M + 15) / 16, GPK_CALL_ADJ)
#undef GPK_CALL_ADJ
  return -11;
}
