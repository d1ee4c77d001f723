// Variational hot path, saved-state adjoint of the L^{-1}-in-registers path:
// gpk_var_adjs_l_kernel and gpk_var_kgram_l_kernel. Shapes: M > 64 (GPK_VAR_LREG) with the
// training forward's saved A, where both LDS plans fit (var_saved_path; D <= 32 at M = 256).
#include "gpk_var_common.h"
#include "gpk_var_launch.h"

namespace {

// ---------------------------------------------------------------------------
// dL^{-1} of the saved-state adjoint (M > 64), from the forward's A instead of a dA / K_ZX
// workspace: with dA = gmean m + 2 gvar (s^2 - 1) A,
//   dL^{-1} = sum_i dA_i K_i^T = m u^T + 2 diag(s^2 - 1) G',   u = sum_i gmean_i K_i,
//   G' = sum_i gvar_i A_i K_i^T            (lower part only: dL^{-1} is lower triangular)
// (the same arithmetic as the reference's fp32 dA: A is the saved fp32 A, products exact on f32
// MFMA, no L^{-1} product -- a form through G = K diag(gvar) K^T would multiply G's rounding by
// L^{-1}'s conditioning). gpk_var_kgram_l_kernel: per workgroup over its chunks, wave w owns the
// G' tile rows I = w and MB-1-w (MB + 1 lower tiles for every wave, f32 MFMA accumulators). Per
// chunk: the saved A block -> LDS rows [p][point], K_ZX recomputed (f32 MFMA Gram, fp32 exp) ->
// LDS rows, gvar masked by the saved clamp mask; each tile product is 8 mfma_f32_16x16x4_f32
// with both operands read as two b128 per lane (the k index of step j on lane (c, g) is point
// 8 g + j). Partials gpart[wg] = G' tiles (acc layout) | u, summed in a fixed order afterwards
// (gpk_var_red_kernel), then var_gdl_elem (extra blocks of gpk_var_fin_kernel) forms dL^{-1}
// elementwise.
// ---------------------------------------------------------------------------
template <int MB, int DQ>
__global__ void __launch_bounds__(64 * GPK_KGRAM_SPL * ((MB + 1) / 2), GPK_KGRAM_SPL == 1 ? 2 : 4)
gpk_var_kgram_l_kernel(const float* __restrict__ X, const float* __restrict__ Z,
                       const float* __restrict__ vmean, const float* __restrict__ vstd,
                       const float* __restrict__ hyp, const float* __restrict__ gmean,
                       const float* __restrict__ gvar, const float* __restrict__ saved, int N, int M,
                       int D, int nchunks, float* __restrict__ gpart, GpkOStr bs) {
  GPK_O_MODEL();
  GPK_O_ADD(gmean, bs.bn);
  GPK_O_ADD(gvar, bs.bn);
  GPK_O_ADD(saved, bs.sv);
  GPK_O_ADD(gpart, bs.ws);
  using G = LGramGeo<MB, DQ>;
  using SV = LSaved<MB>;
  constexpr int NT = G::NT, DS = G::DS, NPASS = G::NPASS, DV = G::DV, KS = G::KS;
  constexpr int SPL = GPK_KGRAM_SPL, HS = G::HS;
  constexpr int NU = SV::tiles / 4;                 // f32x4 units of A per chunk
  static_assert(NU % NT == 0, "A block: whole passes");
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4, sub = tid & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the tile-row pair (IA, IB) of this wave and its share of the pair's slots
  // (slot s <= IA: tile (IA, s); slot IA + 1 + s': tile (IB, s')), [s0, s0 + HS)
  const int pr = wave / SPL, hf = wave - pr * SPL;
  const int IA = pr, IB = MB - 1 - pr;
  const bool two = IB != IA;
  const int nslot = two ? MB + 1 : IA + 1, s0 = hf * HS;
  const float s2 = hyp[0];
  const float* ls = hyp + 4 + D;
  const int nch = (N + LTW - 1) / LTW;
  float lsr[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) lsr[v] = ls[sub + 16 * v < D ? sub + 16 * v : 0];
  float xr[NPASS][DV];
  lload_points<NPASS, DV, NT>(X, blockIdx.x, nchunks, nch, N, D, xr);
  stage_inducing(Z, ls, vmean, vstd, M, D, G::MP, DQ, DS, vsm + G::oZs, vsm + G::oZn, vsm + G::oCm,
                 vsm + G::oVm, vsm + G::oSm1, vsm + G::oA);
  lds_barrier();
  float cmr[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) cmr[v] = vsm[G::oCm + sub + 16 * v];
  f32x4 gacc[HS];
#pragma unroll
  for (int s = 0; s < HS; ++s) gacc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 uacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  // the chunk's A units (4 rows of one point each): loaded one chunk ahead (registers)
  f32x4 au[NU / NT];
  auto load_a = [&](int t) {
    const float* sb = saved + (size_t)(t < nchunks ? t : 0) * SV::blk;
#pragma unroll
    for (int q = 0; q < NU / NT; ++q) au[q] = *(const f32x4*)(sb + 4 * (tid + q * NT));
  };
  load_a(blockIdx.x);

  for (int t = blockIdx.x; t < nchunks; t += gridDim.x) {
    const int b = t / nch, i0 = (t - b * nch) * LTW;
    const int nvalid = N - i0 < LTW ? N - i0 : LTW;
    const long long col0 = (long long)b * N + i0;
    float* sm = (float*)fresh_lds(vsm);
    float* Ar = sm + G::oA;
    float* Kr = sm + G::oK;
    const float* zs = sm + G::oZs;
    const float* zn = sm + G::oZn;
    float* xs = sm + G::oXs;
    float* xn = sm + G::oXn;
    float* gmc = sm + G::oGm;
    float* gvc = sm + G::oGv;
    const float* sb = saved + (size_t)t * SV::blk;
    lds_barrier();   // the previous chunk's reads are done
#pragma unroll
    for (int q = 0; q < NU / NT; ++q) {
      // unit e: tile (rt, ct) = e / 64, lane' = e % 64 -> rows 16 rt + g' + 4u, point 16 ct + c'
      const int e = tid + q * NT, tl = e >> 6, ln = e & 63, rt = tl >> 1, ct = tl & 1;
      const int col = 16 * ct + (ln & 15), r0 = 16 * rt + (ln >> 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) Ar[(r0 + 4 * u) * KS + col] = au[q][u];
    }
    lstage_points<NPASS, DV, NT, DS>(xr, lsr, cmr, D, nvalid, xs, xn);
    if (tid < LTW) {
      const bool ok = tid < nvalid;
      const float gm = gmean[ok ? col0 + tid : 0], gv = gvar[ok ? col0 + tid : 0];
      const float keep = sb[SV::tiles + tid];
      gmc[tid] = ok ? gm : 0.f;
      gvc[tid] = (ok && keep != 0.f) ? gv : 0.f;   // the variance clamp passes no gradient
    }
    if (t + (int)gridDim.x < nchunks) {
      lload_points<NPASS, DV, NT>(X, t + gridDim.x, nchunks, nch, N, D, xr);
      load_a(t + gridDim.x);   // (au was consumed by the LDS stores above)
    }
    lds_barrier();
    // K_ZX of the wave's rows -> Kr[row][point]; u partials (SPL = 2: half 0 row IA, half 1 IB)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !two) break;
      if (SPL == 2 && h != hf) continue;
      const int rt = h == 0 ? IA : IB;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float* za = zs + (16 * rt + c) * DS + g;
        const float* xb = xs + (16 * ct + c) * DS + g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < DQ / 4; ++k) acc = mfma32(za[4 * k], xb[4 * k], acc);
        const int col = 16 * ct + c;
        const float xnc = xn[col], gmv = gmc[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = 16 * rt + 4 * g + r;
          float dist = zn[p] + xnc - 2.f * acc[r];
          dist = dist < 0.f ? 0.f : dist;
          const float kv = (p < M && col < nvalid) ? s2 * __builtin_amdgcn_exp2f(kNHalfLog2e * dist) : 0.f;
          Kr[p * KS + col] = kv;
          uacc[h][r] = __builtin_fmaf(gmv, kv, uacc[h][r]);
        }
      }
    }
    lds_barrier();
    // G' tiles (I >= J): A[16 I + c][8 g + j] gvar_(8 g + j) and K[16 J + c][8 g + j]
    {
      const f32x4 gv0 = *(const f32x4*)(gvc + 8 * g), gv1 = *(const f32x4*)(gvc + 8 * g + 4);
      auto rowop = [&](const float* base, int rt, float (&o)[8]) {
        const f32x4 a0 = *(const f32x4*)(base + (16 * rt + c) * KS + 8 * g);
        const f32x4 a1 = *(const f32x4*)(base + (16 * rt + c) * KS + 8 * g + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { o[q] = a0[q]; o[4 + q] = a1[q]; }
      };
      float aA[8], aB[8];
      rowop(Ar, IA, aA);
      rowop(Ar, two ? IB : IA, aB);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        aA[q] *= gv0[q]; aA[4 + q] *= gv1[q];
        aB[q] *= gv0[q]; aB[4 + q] *= gv1[q];
      }
#pragma unroll
      for (int ls = 0; ls < HS; ++ls) {
        const int s = s0 + ls;
        if (s >= nslot) break;
        const bool isA = s <= IA;
        const int J = isA ? s : s - IA - 1;
        float bo[8];
        rowop(Kr, J, bo);
#pragma unroll
        for (int q = 0; q < 8; ++q) gacc[ls] = mfma32(isA ? aA[q] : aB[q], bo[q], gacc[ls]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // partials: tile (I, J) at (I (I + 1) / 2 + J) * 256 + lane * 4 + r (acc layout) | u
  float* po = gpart + (size_t)blockIdx.x * G::PG;
#pragma unroll
  for (int ls = 0; ls < HS; ++ls) {
    const int s = s0 + ls;
    if (s >= nslot) break;
    const bool isA = s <= IA;
    const int I = isA ? IA : IB, J = isA ? s : s - IA - 1;
    *(f32x4*)(po + (I * (I + 1) / 2 + J) * 256 + lane * 4) = gacc[ls];
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 1 && !two) break;
    if (SPL == 2 && h != hf) continue;
    const int rt = h == 0 ? IA : IB;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = row16_sum_f(uacc[h][r]);
      if (c == 0) po[G::NTILE * 256 + 16 * rt + 4 * g + r] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Adjoint for M > 64 from the training forward's saved state (gpk_variational_train_f32):
// ONE kernel in the adjk layout (wave w holds the L^{-1} COLUMN blocks of block rows
// pA = w, pB = MB-1-w). Per chunk: A (fp32, LSaved layout) straight into the LDS dA tiles by
// LDS-DMA (double-buffered), the clamp mask onto gvar; each wave turns ITS rows of A into
// dA = gmean m + 2 gvar (s^2 - 1) A in place (with the dvmean / dvstd row sums); then
// dK = L^{-T} dA on f32 MFMA from an fp32 copy of the wave's L^{-1} column blocks (round 6; the
// reference's dK is fp64: 68 instead of 136 VGPRs and twice the MFMA rate, 0.229 -> 0.180 ms at
// N = 192; the gradients stay within ~1e-6 of the fp64 oracle), K_ZX of the
// wave's rows recomputed (f32 MFMA, natural row order: every f32 MFMA output here is in the f32
// C layout, lane (g, c) reg r <-> row 4 g + r), Q = dK o K and the Q^T zs / QX contractions, dX
// per point and the fixed-order partials. dL^{-1} comes from gpk_var_kgram_l_kernel (G' = A
// diag(gvar) K_ZX^T from the same saved A, below). (Accumulating dL^{-1} = sum dA K^T in this
// pass as well -- the wave's tile columns are its K rows -- needs 68 more VGPRs than the 256 of
// two waves per SIMD: 98 VGPRs of spills, L^{-1} reloaded from scratch inside the GEMM, measured
// 0.232 ms; not kept.)
// ---------------------------------------------------------------------------
// dK of the wave with pA = RA from its fp32 column-block registers: slots 0..NA-1 are blocks
// (rt = RA + s, RA), the rest (rt = RB + s - NA, RB); B operands dA[rt] from LDS (the next slot's
// read while this slot's 8 MFMAs run).
template <int MB, int RA>
GPK_DEVICE void lcol_gemm32(const float (&Lc)[MB + 1][4], const float* dAl, int lane,
                            f32x4 (&dKa)[2], f32x4 (&dKb)[2]) {
  constexpr int RB = MB - 1 - RA;
  constexpr int NA = MB - RA;
  constexpr int NS = RB == RA ? NA : MB + 1;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  f32x4 k0 = *(const f32x4*)(dAl + ((RA * 2 + 0) * 64 + lane) * 4);
  f32x4 k1 = *(const f32x4*)(dAl + ((RA * 2 + 1) * 64 + lane) * 4);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s == NA) {
      dKa[0] = acc[0];
      dKa[1] = acc[1];
      acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 n0 = k0, n1 = k1;
    if (s + 1 < NS) {
      const int rtn = s + 1 < NA ? RA + s + 1 : RB + (s + 1 - NA);
      n0 = *(const f32x4*)(dAl + ((rtn * 2 + 0) * 64 + lane) * 4);
      n1 = *(const f32x4*)(dAl + ((rtn * 2 + 1) * 64 + lane) * 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[0] = mfma32(Lc[s][u], k0[u], acc[0]);
      acc[1] = mfma32(Lc[s][u], k1[u], acc[1]);
    }
    k0 = n0;
    k1 = n1;
    __builtin_amdgcn_sched_barrier(0);
  }
  if (RB == RA) {
    dKa[0] = acc[0];
    dKa[1] = acc[1];
    dKb[0] = dKb[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    dKb[0] = acc[0];
    dKb[1] = acc[1];
  }
}
template <int MB, int RA>
GPK_DEVICE void lcol_gemm32_for(int wave, const float (&Lc)[MB + 1][4], const float* dAl, int lane,
                                f32x4 (&dKa)[2], f32x4 (&dKb)[2]) {
  if constexpr (RA < (MB + 1) / 2) {
    if (wave == RA) lcol_gemm32<MB, RA>(Lc, dAl, lane, dKa, dKb);
    else lcol_gemm32_for<MB, RA + 1>(wave, Lc, dAl, lane, dKa, dKb);
  }
}

template <int MB, int DQ>
__global__ void __launch_bounds__(64 * ((MB + 1) / 2), 2)
gpk_var_adjs_l_kernel(const float* __restrict__ X, const float* __restrict__ Z,
                      const double* __restrict__ Linv, const float* __restrict__ vmean,
                      const float* __restrict__ vstd, const float* __restrict__ hyp,
                      const float* __restrict__ gmean, const float* __restrict__ gvar,
                      const float* __restrict__ saved, int N, int M, int D, int nchunks,
                      float* __restrict__ wspart, float* __restrict__ dX, float* __restrict__ cm_out,
                      GpkOStr bs) {
  GPK_O_MODEL();
  GPK_O_ADD(Linv, M * M);
  GPK_O_ADD(gmean, bs.bn);
  GPK_O_ADD(gvar, bs.bn);
  GPK_O_ADD(saved, bs.sv);
  GPK_O_ADD(wspart, bs.ws);
  GPK_O_ADD(dX, bs.bn * D);
  GPK_O_ADD(cm_out, bs.ws);
  using G = LAdjGeo<MB, DQ>;
  using SV = LSaved<MB>;
  constexpr int NWV = G::NWV, NT = G::NT, DS = G::DS, NPASS = G::NPASS, DV = G::DV, NDT = G::NDT;
  constexpr int NU = SV::tiles / 4;                 // f32x4 units of A per chunk
  static_assert(NU % NT == 0, "A block: whole passes");
  static_assert(MB % 2 == 0, "two distinct column blocks per wave");   // (MB in {6, 8, 12, 16})
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4, sub = tid & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pA = wave, pB = MB - 1 - wave;
  const float s2 = hyp[0];
  const float* w = hyp + 4;
  const float* ls = hyp + 4 + D;
  const int nch = (N + LTW - 1) / LTW;
  constexpr int oRows = G::kMisc, oXn = G::kMisc + 2 * G::MP, oGv = oXn + 2 * LTW;
  static_assert(2 * G::MP + 4 * LTW <= 2 * NT + NWV, "misc area");

  // L^{-1} column blocks (k-order g + 4u, as gpk_var_adjs_l_kernel), rounded to fp32
  float Lc[MB + 1][4];
  {
    const bool full = (M & 15) == 0;
    const int NA = MB - pA;
#pragma unroll
    for (int s = 0; s <= MB; ++s) {
      const bool isA = s < NA;
      const int P = isA ? pA : pB, rt = isA ? pA + s : pB + (s - NA);
      const bool ok = isA || rt < MB;
      const int col = 16 * P + c;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = 16 * rt + g + 4 * u;
        const bool in = ok && (full || (row < M && col < M));
        const double v = Linv[in ? (size_t)row * M + col : 0];
        Lc[s][u] = in ? (float)v : 0.f;
      }
      if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
  float lsr[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) lsr[v] = ls[sub + 16 * v < D ? sub + 16 * v : 0];
  float xr[NPASS][DV];
  lload_points<NPASS, DV, NT>(X, blockIdx.x, nchunks, nch, N, D, xr);
  stage_inducing(Z, ls, vmean, vstd, M, D, G::MP, DQ, DS, vsm + G::kZs, vsm + G::kZn, vsm + G::kCm,
                 vsm + G::kVm, vsm + G::kSm1, vsm + G::kKl);
  for (int e = tid; e < G::MP; e += NT) vsm[G::kQ + e] = 0.f;
  for (int e = tid; e < 2 * G::MP; e += NT) vsm[oRows + e] = 0.f;
  auto copy_a = [&](int t, float* buf) {
    const float* sb = saved + (size_t)t * SV::blk;
#pragma unroll
    for (int q = 0; q < NU / NT; ++q) {
      const int u0 = (q * NWV + wave) * 64;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sb + 4 * (u0 + lane)),
                                       (__attribute__((address_space(3))) void*)(buf + 4 * u0), 16, 0, 0);
    }
  };
  copy_a(blockIdx.x, vsm + G::kdA);
  lds_barrier();
  if (blockIdx.x == 0 && tid < D) cm_out[tid] = vsm[G::kCm + tid];
  float cmr[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) cmr[v] = vsm[G::kCm + sub + 16 * v];
  const int dd = tid % DQ;
  const float il_dd = dd < D ? 1.f / ls[dd < D ? dd : 0] : 0.f;
  const float w_dd = dd < D ? w[dd < D ? dd : 0] : 0.f;
  float rx2 = 0.f, gxa = 0.f, sumQ = 0.f, sumgm = 0.f, sumgv = 0.f;
  f32x4 qx[2][NDT];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) qx[h][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int par = 0;

  for (int t = blockIdx.x; t < nchunks; t += gridDim.x, par ^= 1) {
    const int b = t / nch, i0 = (t - b * nch) * LTW;
    const int nvalid = N - i0 < LTW ? N - i0 : LTW;
    const long long col0 = (long long)b * N + i0;
    float* sm = (float*)fresh_lds(vsm);
    float* dAl = sm + (par ? G::kKl : G::kdA);
    float* xzl = sm + G::kXz;
    float* red = sm + G::kRed;
    const float* zs = sm + G::kZs;
    const float* zn = sm + G::kZn;
    const float* vm = sm + G::kVm;
    const float* sm1 = sm + G::kSm1;
    float* qrow = sm + G::kQ;
    float* scr = sm + G::kScr + wave * 320;
    float* xs = sm + G::kXs + par * LTW * DS;
    float* xn = sm + oXn + par * LTW;
    float* gmc = sm + G::kGm + par * LTW;
    float* gvc = sm + oGv + par * LTW;
    float* rows = sm + oRows;
    {
      const float* sb = saved + (size_t)t * SV::blk;
      if (tid < LTW) {
        const bool ok = tid < nvalid;
        const float keep = sb[SV::tiles + tid];
        const float gm = gmean[ok ? col0 + tid : 0], gv = gvar[ok ? col0 + tid : 0];
        const float gvk = (ok && keep != 0.f) ? gv : 0.f;
        gmc[tid] = ok ? gm : 0.f;
        gvc[tid] = gvk;
        sumgm += ok ? gm : 0.f;
        sumgv += gvk;
      }
    }
    lstage_points<NPASS, DV, NT, DS>(xr, lsr, cmr, D, nvalid, xs, xn);
    if (t + (int)gridDim.x < nchunks) lload_points<NPASS, DV, NT>(X, t + gridDim.x, nchunks, nch, N, D, xr);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's A copy has landed
    lds_barrier();
    // ---- the wave's own rows: row sums of A, A -> dA in place
    {
      float gmq[2], gvq[2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        gmq[ct] = gmc[16 * ct + c];
        gvq[ct] = gvc[16 * ct + c];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rt = h == 0 ? pA : pB;
        float pm[4] = {0.f, 0.f, 0.f, 0.f}, ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          float* at = dAl + ((rt * 2 + ct) * 64 + lane) * 4;
          const f32x4 av = *(const f32x4*)at;
          f32x4 da;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int p = 16 * rt + g + 4 * r;
            pm[r] = __builtin_fmaf(gmq[ct], av[r], pm[r]);
            ps[r] = __builtin_fmaf(gvq[ct], av[r] * av[r], ps[r]);
            da[r] = gmq[ct] * vm[p] + 2.f * gvq[ct] * sm1[p] * av[r];
          }
          *(f32x4*)at = da;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a = row16_sum_f(pm[r]), q = row16_sum_f(ps[r]);
          if (c == 0) {
            const int p = 16 * rt + g + 4 * r;
            lds_acc(rows + p, a);
            lds_acc(rows + G::MP + p, q);
          }
        }
      }
    }
    lds_barrier();
    // ---- dK = L^{-T} dA (f32 MFMA) on the wave's block rows; K_ZX of those rows; Q = dK o K
    f32x4 Qt[2][2];
    {
      f32x4 dK[2][2];
      if (t + (int)gridDim.x < nchunks) copy_a(t + gridDim.x, sm + (par ? G::kdA : G::kKl));
      lcol_gemm32_for<MB, 0>(wave, Lc, dAl, lane, dK[0], dK[1]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rt = h == 0 ? pA : pB;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const float* za = zs + (16 * rt + c) * DS + g;
          const float* xb = xs + (16 * ct + c) * DS + g;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < DQ / 4; ++k) acc = mfma32(za[4 * k], xb[4 * k], acc);
          const int col = 16 * ct + c;
          const float xnc = xn[col];
          f32x4 kv;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int p = 16 * rt + 4 * g + r;
            float dist = zn[p] + xnc - 2.f * acc[r];
            dist = dist < 0.f ? 0.f : dist;
            kv[r] = (p < M && col < nvalid) ? s2 * __builtin_amdgcn_exp2f(kNHalfLog2e * dist) : 0.f;
            Qt[h][ct][r] = dK[h][ct][r] * kv[r];
          }
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int rt = h == 0 ? pA : pB;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = row16_sum_f(Qt[h][0][r] + Qt[h][1][r]);
        if (c == 0) lds_acc(qrow + 16 * rt + 4 * g + r, v);
      }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      float v = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) v += (Qt[h][ct][0] + Qt[h][ct][1]) + (Qt[h][ct][2] + Qt[h][ct][3]);
      sumQ += v;
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (g == 0) red[wave * LTW + 16 * ct + c] = v;
    }
    {
      f32x4 xz[2][NDT];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) xz[ct][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rt = h == 0 ? pA : pB;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const float zb = zs[(16 * rt + 4 * g + r) * DS + 16 * dt + c];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) xz[ct][dt] = mfma32(Qt[h][ct][r], zb, xz[ct][dt]);
          }
      }
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            xzl[(wave * LTW + 16 * ct + 4 * g + r) * DQ + 16 * dt + c] = xz[ct][dt][r];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
        for (int r = 0; r < 4; ++r) scr[lane * 5 + r] = Qt[h][ct][r];
        adj_lds_order();
        float aq[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) aq[s4] = scr[(16 * (c >> 2) + 4 * s4 + g) * 5 + (c & 3)];
        adj_lds_order();
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4)
            qx[h][dt] = mfma32(aq[s4], xs[(16 * ct + 4 * s4 + g) * DS + 16 * dt + c], qx[h][dt]);
      }
    }
    lds_barrier();
    for (int e = tid; e < LTW * DQ; e += NT) {
      const int col = e / DQ;
      float v = 0.f, r = 0.f;
#pragma unroll
      for (int q = 0; q < NWV; ++q) {
        v += xzl[(q * LTW + col) * DQ + dd];
        r += red[q * LTW + col];
      }
      const float xv = xs[col * DS + dd];
      if (col < nvalid && dd < D) {
        dX[(col0 + col) * D + dd] = (v - xv * r) * il_dd + gmc[col] * w_dd;
        rx2 = __builtin_fmaf(r * xv, xv, rx2);
        gxa = __builtin_fmaf(gmc[col], xv, gxa);
      }
    }
  }
  lds_barrier();
  // partial fields: QX (M x D) | q (M) | dvm (M) | dsm (M) | rx2 (D) | sumQ | sumgv | gx (D) | sumgm
  const int P = M * D + 3 * M + 2 * D + 3;
  float* po = wspart + (size_t)blockIdx.x * P;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int rt = h == 0 ? pA : pB;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 16 * rt + 4 * g + r, d = 16 * dt + c;
        if (p < M && d < D) po[p * D + d] = qx[h][dt][r];
      }
  }
  for (int m = tid; m < M; m += NT) {
    po[M * D + m] = vsm[G::kQ + m];
    po[M * D + M + m] = vsm[oRows + m];
    po[M * D + 2 * M + m] = vsm[oRows + G::MP + m];
  }
  lds_barrier();
  float* misc = vsm + G::kMisc;
  misc[tid] = rx2;
  misc[NT + tid] = gxa;
  sumQ = wave_sum(sumQ);
  if (lane == 0) misc[2 * NT + wave] = sumQ;
  lds_barrier();
  for (int d = tid; d < D; d += NT) {
    float v = 0.f, u = 0.f;
    for (int q = d; q < NT; q += DQ) { v += misc[q]; u += misc[NT + q]; }
    po[M * D + 3 * M + d] = v;
    po[M * D + 3 * M + D + 2 + d] = u;
  }
  if (tid == 0) {
    float v = 0.f;
    for (int q = 0; q < NWV; ++q) v += misc[2 * NT + q];
    po[M * D + 3 * M + D] = v;
  }
  if (wave == 0) {
    const float u = wave_sum(sumgm), v = wave_sum(sumgv);
    if (lane == 0) {
      po[M * D + 3 * M + 2 * D + 2] = u;
      po[M * D + 3 * M + D + 1] = v;
    }
  }
}

template <int MB, int DQ>
int launch_var_adj_saved(const GpkVarAdjArgs& a, const AdjSavedPlan& p, hipStream_t stream) {
  if constexpr (var_saved_fits<MB, DQ>()) {
    using LA = LAdjGeo<MB, DQ>;
    using LG = LGramGeo<MB, DQ>;
    const GpkOStr bs = adj_strides(a, p.total);   // output o works in workspace slice o
    char* ws = (char*)a.ws;
    float* gpart = (float*)(ws + p.off_gpart);
    float* wspart = (float*)(ws + p.off_part);
    double* tot = (double*)(ws + p.off_tot);
    double* gtot = (double*)(ws + p.off_gtot);
    set_lds_once<gpk_var_adjs_l_kernel<MB, DQ>>();
    hipLaunchKernelGGL((gpk_var_adjs_l_kernel<MB, DQ>), dim3(p.nwg, a.O), dim3(LA::NT), (size_t)LA::k_total * sizeof(float),
                       stream, a.X, a.Z, a.Linv, a.vmean, a.vstd, a.hyp, a.gmean, a.gvar, a.saved, a.N, a.M,
                       a.D, p.nchunks, wspart, a.dX, (float*)(ws + p.off_cm), bs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    set_lds_once<gpk_var_kgram_l_kernel<MB, DQ>>();
    hipLaunchKernelGGL((gpk_var_kgram_l_kernel<MB, DQ>), dim3(p.nwg_g, a.O), dim3(LG::NT), (size_t)LG::total * sizeof(float),
                       stream, a.X, a.Z, a.vmean, a.vstd, a.hyp, a.gmean, a.gvar, a.saved, a.N, a.M, a.D,
                       p.nchunks, gpart, bs);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    // one fixed-order reduction launch for both partial arrays (same workgroup count), then
    // the output launch with dL^{-1} in extra workgroups
    if (p.nwg == p.nwg_g) {
      if (int rc = gpk_launch_var_red(a, stream, wspart, p.nwg, p.P, tot, gpart, p.PG, gtot, bs)) return rc;
    } else {
      if (int rc = gpk_launch_var_red(a, stream, gpart, p.nwg_g, p.PG, gtot, nullptr, 0, nullptr, bs)) return rc;
      if (int rc = gpk_launch_var_red(a, stream, wspart, p.nwg, p.P, tot, nullptr, 0, nullptr, bs)) return rc;
    }
    return gpk_launch_var_fin(a, tot, bs, stream, (const float*)(ws + p.off_cm), gtot, MB);
  } else {
    return -13;
  }
}

}  // namespace

int gpk_launch_var_adjs_l(const GpkVarAdjArgs& a, const AdjSavedPlan& p, hipStream_t stream) {
#define GPK_CALL_ADJS(mb)                                             \
  if (a.D <= 32) return launch_var_adj_saved<mb, 32>(a, p, stream);   \
  return launch_var_adj_saved<mb, 64>(a, p, stream);
  GPK_MB_SWITCH((a.M + 15) / 16, GPK_CALL_ADJS)
#undef GPK_CALL_ADJS
  return -11;
}
