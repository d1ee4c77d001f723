// Variational (DeepGP) hot path: what more than one of its units uses. The units (one per
// kernel path; which shape reaches which is the map at the top of gpk_variational.hip):
//   gpk_var_reg.hip     register-resident path (M <= 64, D <= 32)
//   gpk_var_fwd_l.hip   L^{-1}-in-registers forward (M > 64)
//   gpk_var_adj_l.hip   its recompute adjoint
//   gpk_var_adjs_l.hip  its saved-state adjoint and K-Gram
//   gpk_var_tiled.hip   LDS-tiled fallback
//   gpk_var_tail.hip    ELL sum, dL^{-1} GEMM, fixed-order reductions, outputs
//   gpk_variational.hip the plans, the workspace sizes and the dispatch
// Everything here is unit-local (anonymous namespace): the device helpers and constants, the
// inducing-point staging, the geometry structs that size both a kernel's LDS and the host's
// plans, the build switches with their defaults, and the launchers' small host helpers.
// A change to a helper here re-canonicalises the device code of every kernel that calls it:
// prove such a change with scripts/isa_diff.py and scripts/var_ab.py.
#pragma once
#include "gpk_common.h"
#include "gpk_internal.h"

#include <mutex>

namespace {

constexpr float kLog2PiF = 1.8378770664093453f;
constexpr float kNHalfLog2e = -0.72134752044448170f;  // -0.5 * log2(e)

#define GPK_HOST_DEVICE_INLINE __host__ __device__ __forceinline__

// Batched (multi-output) launches: workgroup blockIdx.y = output o moves its base pointers to
// the output's slices before the single-output body runs (scalar adds, once per workgroup).
// GPK_O_MODEL: the inputs and the arrays M and D size; GPK_O_ADD: a pointer by an element
// stride; GPK_O_OPT: an optional one (a null pointer stays null).
#define GPK_O_MODEL()                                  \
  X += (size_t)blockIdx.y * bs.x;                      \
  Z += (size_t)blockIdx.y * (size_t)(M * D);           \
  vmean += (size_t)blockIdx.y * (size_t)M;             \
  vstd += (size_t)blockIdx.y * (size_t)M;              \
  hyp += (size_t)blockIdx.y * (size_t)(4 + 2 * D)
#define GPK_O_ADD(p, stride) (p) += (size_t)blockIdx.y * (size_t)(stride)
#define GPK_O_OPT(p, stride) \
  if ((p) != nullptr) (p) += (size_t)blockIdx.y * (size_t)(stride)

GPK_DEVICE f64x4 mfma64(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
GPK_DEVICE f32x4 mfma32(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// Sum over the 16 lanes of a row (lanes sharing g), DPP only.
GPK_DEVICE float row16_sum_f(float v) {
#define GPK_DPP_ADD(ctrl) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false));
  GPK_DPP_ADD(0xB1) GPK_DPP_ADD(0x4E) GPK_DPP_ADD(0x141) GPK_DPP_ADD(0x140)
#undef GPK_DPP_ADD
  return v;
}

// Add v into an LDS accumulator that only the calling wave updates, without a round trip: a
// no-return LDS add (no wait, where `*p += v` costs a read, a full LDS-latency wait and a
// write). One wave's LDS operations execute in issue order, so the adds land in program
// order: the sums stay deterministic.
GPK_DEVICE void lds_acc(float* p, float v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// Order of the per-wave scratch transposes: one wave's LDS operations execute in issue order,
// so a code-motion barrier is enough between a tile's writes, its reads and the next tile's
// writes (GPK_ADJ_LDS_WAIT=1: the waitcnt-draining wave_lds_sync instead, for A/B builds)
#ifndef GPK_ADJ_LDS_WAIT
#define GPK_ADJ_LDS_WAIT 0
#endif
GPK_DEVICE void adj_lds_order() {
#if GPK_ADJ_LDS_WAIT
  wave_lds_sync();
#else
  __builtin_amdgcn_wave_barrier();
#endif
}

// Per-chunk LDS base the compiler must treat as new on every iteration: the staged
// operands (L^{-1}, zs, norms) and their per-lane addresses would otherwise be hoisted out of the chunk loop as
// loop-invariant loads and pinned in (hundreds of) registers.
GPK_DEVICE const float* fresh_lds(const float* p) {
  int z = 0;
  asm volatile("" : "+s"(z));
  return p + z;
}
// The same for a global pointer whose per-lane addresses would be loop-invariant.
template <typename T>
GPK_DEVICE const T* fresh_ptr(const T* p) {
  asm volatile("" : "+s"(p));
  return p;
}

// ---------------------------------------------------------------------------
// Column-tile geometry shared by the forward and adjoint kernels.
//   MB  = 16-row blocks of the inducing dimension (M <= 16 MB <= 256)
//   4 waves = WR (along rows of A) x WC (along points); a wave owns row tiles
//   {wr + WR j} (interleaved: balances the triangular k-range) and CT = 2 column tiles.
//   TW  = points per chunk; a workgroup walks the chunks {part, part + S, ...} of window b.
// ---------------------------------------------------------------------------
template <int MB>
struct VarGeo {
  static constexpr int WR = MB <= 4 ? 1 : (MB <= 8 ? 2 : 4);
  static constexpr int WC = 4 / WR;
  static constexpr int RT = (MB + WR - 1) / WR;
  static constexpr int CT = 2;
  static constexpr int TW = 16 * CT * WC;
  static constexpr int MP = 16 * MB;
  static constexpr int QST = (MP % 32 == 0) ? MP + 16 : MP;  // Q^T row stride (bank spread)
};

// D padded to a power of two >= 16 (<= 64): MFMA k-steps and d-tiles, and 256 % Dq == 0.
GPK_HOST_DEVICE_INLINE int dq_of(int D) { return D <= 16 ? 16 : (D <= 32 ? 32 : 64); }

// Column means of zs (rows 0..M-1, columns 0..Dq-1, row stride ds) in ONE fixed order for
// every kernel that centres the inducing points (stage_inducing, gpk_var_fin_kernel): 8
// partial sums per column over the rows m = k (mod 8), ascending, then k = 0..7 (a serial
// sum over all M rows per column was ~20K cycles of dependent LDS reads at M = 256).
// scr: >= 8 Dq floats of free LDS. Ends with a barrier.
constexpr int kCmParts = 8;
GPK_DEVICE void col_means(const float* zs, int M, int D, int Dq, int ds, float* scr, float* cm) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int e = tid; e < kCmParts * Dq; e += T) {
    const int d = e % Dq, k = e / Dq;
    float a = 0.f;
    for (int m = k; m < M; m += kCmParts) a += zs[m * ds + d];
    scr[e] = a;
  }
  lds_barrier();
  for (int d = tid; d < Dq; d += T) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < kCmParts; ++k) a += scr[k * Dq + d];
    cm[d] = d < D ? a / (float)M : 0.f;   // GPyTorch _sq_dist centres by x1 = Z
  }
  lds_barrier();
}

// Stage the centred, scaled inducing points zs = Z/l - mean(Z/l) (rows >= M and
// columns >= D zero), their squared norms, the q(u) mean and s^2 - 1. scr: >= 8 Dq floats
// of LDS that is free during the staging.
GPK_DEVICE void stage_inducing(const float* __restrict__ Z, const float* __restrict__ ls,
                               const float* __restrict__ vmean, const float* __restrict__ vstd,
                               int M, int D, int MP, int Dq, int ds, float* zs, float* zn, float* cm,
                               float* vm, float* sm1, float* scr) {
  const int tid = threadIdx.x, T = blockDim.x;
  // 8 unconditional loads (clamped addresses) in flight per thread, then the stores:
  // a predicated load per loop iteration costs one full memory latency each
  for (int base = 0; base < MP * Dq; base += 8 * T) {
    float v[8], l[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * T + tid, m = e / Dq, d = e - m * Dq;
      const bool ok = e < MP * Dq && m < M && d < D;
      v[u] = Z[ok ? m * D + d : 0];
      l[u] = ls[ok ? d : 0];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * T + tid, m = e / Dq, d = e - m * Dq;
      if (e < MP * Dq) zs[m * ds + d] = (m < M && d < D) ? v[u] / l[u] : 0.f;
    }
  }
  for (int m = tid; m < MP; m += T) {
    vm[m] = (m < M) ? vmean[m] : 0.f;
    const float sd = (m < M) ? vstd[m] : 1.f;
    sm1[m] = sd * sd - 1.f;
  }
  lds_barrier();
  col_means(zs, M, D, Dq, ds, scr, cm);
  for (int e = tid; e < M * Dq; e += T) {
    const int m = e / Dq, d = e - m * Dq;
    zs[m * ds + d] -= cm[d];
  }
  lds_barrier();
  for (int m = tid; m < MP; m += T) {
    float s = 0.f;
    for (int d = 0; d < Dq; ++d) s = __builtin_fmaf(zs[m * ds + d], zs[m * ds + d], s);
    zn[m] = s;
  }
}

// ---------------------------------------------------------------------------
// L^{-1}-in-registers path (M > 64): chunk size, saved state, the row-block GEMM (forward and
// recompute adjoint), point staging, and the LDS plans of its kernels.
// ---------------------------------------------------------------------------
constexpr int LTW = 32;   // points per chunk (2 column tiles)

// Per-chunk block of the state the training forward keeps for the adjoint (M > 64):
// A = L^{-1} K_ZX of the chunk cast to fp32 (MB x 2 tiles, element u of lane (c, g) of tile
// (rt, ct) <-> row 16 rt + g + 4u, point 16 ct + c), then the clamp mask of its LTW points
// (1: var_i >= 1e-6, 0: clamped or padding).
template <int MB>
struct LSaved {
  static constexpr int tiles = MB * 2 * 256;
  static constexpr int blk = tiles + LTW;
};

// A[rA] / A[rB] of one chunk for the wave with rA = RA: slots 0..RA are blocks (RA, s),
// slots RA+1..MB blocks (MB-1-RA, s-RA-1). The next slot's K_ZX operands (one b128 per
// column tile) are read while this slot's 8 MFMAs run; a scheduling fence per slot keeps
// the reads from all being hoisted.
template <int MB, int RA>
GPK_DEVICE void lreg_gemm(const double (&Lr)[MB + 1][4], const float* Kl, int lane,
                          f64x4 (&aA)[2], f64x4 (&aB)[2]) {
  constexpr int RB = MB - 1 - RA;
  constexpr int NS = RB == RA ? RA + 1 : MB + 1;
  f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
  f32x4 k0 = *(const f32x4*)(Kl + (0 * 64 + lane) * 4);
  f32x4 k1 = *(const f32x4*)(Kl + (1 * 64 + lane) * 4);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s == RA + 1) {
      aA[0] = acc[0];
      aA[1] = acc[1];
      acc[0] = acc[1] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    f32x4 n0 = k0, n1 = k1;
    if (s + 1 < NS) {
      const int kbn = s + 1 <= RA ? s + 1 : s - RA;
      n0 = *(const f32x4*)(Kl + ((kbn * 2 + 0) * 64 + lane) * 4);
      n1 = *(const f32x4*)(Kl + ((kbn * 2 + 1) * 64 + lane) * 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[0] = mfma64(Lr[s][u], (double)k0[u], acc[0]);
      acc[1] = mfma64(Lr[s][u], (double)k1[u], acc[1]);
    }
    k0 = n0;
    k1 = n1;
    __builtin_amdgcn_sched_barrier(0);
  }
  if (RB == RA) {
    aA[0] = acc[0];
    aA[1] = acc[1];
    aB[0] = aB[1] = f64x4{0.0, 0.0, 0.0, 0.0};
  } else {
    aB[0] = acc[0];
    aB[1] = acc[1];
  }
}
template <int MB, int RA>
GPK_DEVICE void lreg_gemm_for(int wave, const double (&Lr)[MB + 1][4], const float* Kl, int lane,
                              f64x4 (&aA)[2], f64x4 (&aB)[2]) {
  if constexpr (RA < (MB + 1) / 2) {
    if (wave == RA) lreg_gemm<MB, RA>(Lr, Kl, lane, aA, aB);
    else lreg_gemm_for<MB, RA + 1>(wave, Lr, Kl, lane, aA, aB);
  }
}

template <int MB, int DQ>
struct LGeo {
  static constexpr int NWV = (MB + 1) / 2;              // waves
  static constexpr int NT = 64 * NWV;
  static constexpr int MP = 16 * MB;
  static constexpr int DS = DQ + 2;                     // zs / xs row stride (floats)
  static constexpr int NPASS = (LTW * 16 + NT - 1) / NT; // point-staging passes (16 thr / point)
  static constexpr int DV = DQ / 16;                    // dims per staging thread
  // LDS (floats): Kl first (b128 aligned)
  static constexpr int oKl = 0;                          // MB x 2 tiles x 64 lanes x 4
  static constexpr int oRed = oKl + MP * LTW;            // NWV x 2 x LTW
  static constexpr int oZs = oRed + NWV * 2 * LTW;       // MP x DS
  static constexpr int oZn = oZs + MP * DS;
  static constexpr int oVm = oZn + MP;
  static constexpr int oSm1 = oVm + MP;
  static constexpr int oCm = oSm1 + MP;                  // DQ
  static constexpr int oXs = oCm + DQ;                   // LTW x DS
  static constexpr int oXn = oXs + LTW * DS;             // LTW
  static constexpr int oLin = oXn + LTW;                 // 2 x LTW (chunk parity)
  static constexpr int total = oLin + 2 * LTW;
};

// pi(c): the zs row order that lands an f32 Gram accumulator in the f64 C layout (m = g + 4u)
GPK_DEVICE int pi16(int c) { return (c >> 2) + 4 * (c & 3); }

template <int MB, int DQ>
struct LAdjGeo {
  static constexpr int NWV = (MB + 1) / 2, NT = 64 * NWV, MP = 16 * MB, DS = DQ + 2;
  static constexpr int NPASS = (LTW * 16 + NT - 1) / NT, DV = DQ / 16, NDT = DQ / 16;
  // gpk_var_adja_l_kernel
  static constexpr int aKl = 0;                          // MP x LTW
  static constexpr int aRed = aKl + MP * LTW;            // NWV x LTW
  static constexpr int aZs = aRed + NWV * LTW;           // MP x DS
  static constexpr int aZn = aZs + MP * DS;
  static constexpr int aVm = aZn + MP;
  static constexpr int aSm1 = aVm + MP;
  static constexpr int aCm = aSm1 + MP;                  // DQ
  static constexpr int aRows = aCm + DQ;                 // 2 x MP: dvm | dsm
  static constexpr int aXs = aRows + 2 * MP;             // LTW x DS
  static constexpr int aXn = aXs + LTW * DS;             // LTW
  static constexpr int aGm = aXn + LTW;                  // 2 x LTW (chunk parity)
  static constexpr int aGv = aGm + 2 * LTW;              // 2 x LTW
  static constexpr int a_total = aGv + 2 * LTW;
  // gpk_var_adjk_l_kernel
  static constexpr int kKl = 0;                          // MP x LTW
  static constexpr int kdA = kKl + MP * LTW;             // MP x LTW
  static constexpr int kXz = kdA + MP * LTW;             // NWV x LTW x DQ  Q^T zs partials
  static constexpr int kRed = kXz + NWV * LTW * DQ;      // NWV x LTW       r partials
  static constexpr int kZs = kRed + NWV * LTW;           // MP x DS
  static constexpr int kZn = kZs + MP * DS;
  static constexpr int kVm = kZn + MP;
  static constexpr int kSm1 = kVm + MP;
  static constexpr int kCm = kSm1 + MP;                  // DQ
  static constexpr int kQ = kCm + DQ;                    // MP  q_p
  static constexpr int kScr = kQ + MP;                   // NWV x 320 transpose scratch
  static constexpr int kXs = kScr + NWV * 320;           // 2 x LTW x DS (chunk parity)
  static constexpr int kGm = kXs + 2 * LTW * DS;         // 2 x LTW
  static constexpr int kMisc = kGm + 2 * LTW;            // 2 NT + NWV
  static constexpr int k_total = kMisc + 2 * NT + NWV;
  static constexpr bool fits = (size_t)a_total * 4 <= 160 * 1024 && (size_t)k_total * 4 <= 160 * 1024;
};

// The chunk's points (16 threads per point, dims sub + 16 v) -> xs (and |xs|^2 -> xn if given).
template <int NPASS, int DV, int NT, int DS>
GPK_DEVICE void lstage_points(const float (&xr)[NPASS][DV], const float (&lsr)[DV], const float (&cmr)[DV],
                              int D, int nvalid, float* xs, float* xn) {
  const int tid = threadIdx.x, sub = tid & 15;
#pragma unroll
  for (int q = 0; q < NPASS; ++q) {
    const int j = (tid >> 4) + q * (NT / 16);
    float nrm = 0.f;
    const bool okj = j < nvalid;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const int d = sub + 16 * v;
      const float xv = (okj && d < D) ? xr[q][v] / lsr[v] - cmr[v] : 0.f;
      nrm = __builtin_fmaf(xv, xv, nrm);
      if (j < LTW) xs[j * DS + d] = xv;
    }
    if (xn != nullptr) {
      nrm = row16_sum_f(nrm);
      if (sub == 0 && j < LTW) xn[j] = nrm;
    }
  }
}
template <int NPASS, int DV, int NT>
GPK_DEVICE void lload_points(const float* X, int t, int nchunks, int nch, int N, int D, float (&xr)[NPASS][DV]) {
  const int tid = threadIdx.x, sub = tid & 15;
  const int b = t / nch, i0 = (t - b * nch) * LTW;
#pragma unroll
  for (int q = 0; q < NPASS; ++q) {
    const int j = (tid >> 4) + q * (NT / 16), i = i0 + j;
    const bool ok = t < nchunks && j < LTW && i < N;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const int d = sub + 16 * v;
      const bool okd = ok && d < D;
      const float x = X[okd ? ((size_t)b * N + i) * D + d : 0];
      xr[q][v] = okd ? x : 0.f;
    }
  }
}

#ifndef GPK_KGRAM_SPL
#define GPK_KGRAM_SPL 2   // waves per G' tile-row pair (1: 8 waves x 17 tiles, 209 VGPRs, 2 waves/SIMD)
#endif
template <int MB, int DQ, int SPL = GPK_KGRAM_SPL>
struct LGramGeo {
  static constexpr int NWV = SPL * ((MB + 1) / 2), NT = 64 * NWV, MP = 16 * MB, DS = DQ + 2;
  static constexpr int HS = (MB + 1 + SPL - 1) / SPL;      // G' slots per wave (of the pair's MB + 1)
  static constexpr int NPASS = (LTW * 16 + NT - 1) / NT, DV = DQ / 16;
  static constexpr int KS = LTW + 4;                       // row stride of the A / K blocks (floats)
  static constexpr int NTILE = MB * (MB + 1) / 2;
  static constexpr int PG = NTILE * 256 + MP;              // partial row: tiles | u
  static constexpr int oA = 0;                             // MP x KS  A[p][point]
  static constexpr int oK = oA + MP * KS;                  // MP x KS  K[p][point]
  static constexpr int oZs = oK + MP * KS;                 // MP x DS
  static constexpr int oZn = oZs + MP * DS;
  static constexpr int oVm = oZn + MP;
  static constexpr int oSm1 = oVm + MP;
  static constexpr int oCm = oSm1 + MP;                    // DQ
  static constexpr int oXs = oCm + DQ;                     // LTW x DS
  static constexpr int oXn = oXs + LTW * DS;               // LTW
  static constexpr int oGm = oXn + LTW;                    // LTW
  static constexpr int oGv = oGm + LTW;                    // LTW
  static constexpr int total = oGv + LTW;
};

constexpr int DLKC = 32;   // gpk_dlinv_kernel: columns staged per step (the split-K plan rounds to it)

// ---------------------------------------------------------------------------
// Register-resident path (M <= 64, D <= 32): constants and the LDS plan.
// ---------------------------------------------------------------------------
#ifndef GPK_FWD_OCC
#define GPK_FWD_OCC 3   // waves per SIMD gpk_var_fwd_r_kernel's register budget is sized for (3: 161
                         // VGPRs, cfg 5 forward 55.7 vs 56.6 us unbounded; a next-chunk point
                         // prefetch measured slower at 3 (spills) and at 2 waves/SIMD)
#endif
constexpr int RLS = 66;        // L^{-1} row stride (doubles)
constexpr int kGTiles = 10;                  // lower 16 x 16 tiles of a 64 x 64 G
constexpr int kGPart = kGTiles * 256 + 64;   // floats per workgroup K-Gram partial

// NW waves per workgroup; FG: the adjoint also accumulates the K-Gram G / u per wave
// (gpk_var_adj_r_kernel with the K-Gram folded in, 8 waves: 154 KB at DQ = 32)
template <int DQ, int NW = 4, bool FG = false>
struct RegLds {
  static constexpr int ZS = DQ + 1;
  static constexpr int zs = 0;                      // 64 x ZS
  static constexpr int zn = zs + 64 * ZS;           // 64
  static constexpr int vm = zn + 64;                // 64
  static constexpr int sm1 = vm + 64;               // 64
  static constexpr int cm = sm1 + 64;               // DQ
  static constexpr int li = ((cm + DQ + 3) / 4) * 4;          // 64 x RLS doubles (16-B aligned)
  static constexpr int fwd_total = li + 2 * 64 * RLS;
  // adjoint only: per-wave transpose scratch, per-wave row accumulators, reductions
  static constexpr int scr = fwd_total;             // NW x 320
  static constexpr int rows = scr + NW * 320;       // NW waves x 4 x 64 (dvm, dsm, q, u)
  static constexpr int qxr = rows + NW * 4 * 64;    // 64 x DQ  (workgroup QX)
  static constexpr int misc = qxr + 64 * DQ;        // NW x (2 DQ + 3)
  static constexpr int gacc = ((misc + NW * (2 * DQ + 3) + 3) / 4) * 4;   // NW x 10 G tiles
  static constexpr int adj_total = gacc + (FG ? NW * kGTiles * 256 : 0);
};

// ---------------------------------------------------------------------------
// Host side: one-time kernel attributes, grids, per-output strides, and which path serves a shape.
// ---------------------------------------------------------------------------
// hipFuncSetAttribute once per kernel instantiation (thread-safe; the C ABI has no
// mutable global state beyond this idempotent one-time setup).
template <auto Kernel, int Bytes = 160 * 1024>
void set_lds_once() {
  static std::once_flag once;  // one flag per kernel instantiation
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Bytes);
    (void)hipGetLastError();   // never leave a sticky error for the launch check to pick up
  });
}

// Workgroups for a chunk list: every chunk once, at most ~4 per CU so the inducing-point
// staging of a workgroup is amortised over several chunks.
inline int chunk_grid(long long nchunks, int per_cu) {
  const long long cap = 256LL * per_cu;
  return (int)(nchunks < cap ? nchunks : cap);
}

// Per-output strides of a launch (GpkOStr): the forward's, and the adjoint's over workspace
// slices of ws_bytes (a plan's total, a multiple of 256) each.
inline GpkOStr fwd_strides(const GpkVarArgs& a) {
  return {a.x_stride, (long long)a.B * a.N, (long long)(gpk_var_saved_bytes(a.B, a.N, a.M, a.D) / sizeof(float)), 0};
}
inline GpkOStr adj_strides(const GpkVarAdjArgs& a, size_t ws_bytes) {
  return {a.x_stride, (long long)a.B * a.N, (long long)(gpk_var_saved_bytes(a.B, a.N, a.M, a.D) / sizeof(float)),
          (long long)(ws_bytes / sizeof(float))};
}

// The saved-state adjoint (gpk_var_adjs_l_kernel + K-Gram) serves M > 64 when its LDS plan fits
// (D <= 32 at M = 256); the training forward then keeps A for it.
// 0: A/B builds with the LDS-tiled forward for M > 64 (that forward keeps no state, so the
// saved-state training pair is off too: var_saved_path is false and saved_bytes 0)
#ifndef GPK_VAR_LREG
#define GPK_VAR_LREG 1
#endif
template <int MB, int DQ>
constexpr bool var_saved_fits() {
  if constexpr (MB >= 5) return LAdjGeo<MB, DQ>::fits && (size_t)LGramGeo<MB, DQ>::total * 4 <= 160 * 1024;
  return false;
}
template <int MB, int DQ>
bool var_saved_path(int M) { return GPK_VAR_LREG && var_saved_fits<MB, DQ>() && M > 64; }

// register-resident path (M <= 64, D <= 32): 32-point chunks, one per wave, 4 waves per
// workgroup, 2 workgroups per CU
#ifndef GPK_VAR_REG
#define GPK_VAR_REG 1   // 0: A/B builds without the register-resident path
#endif
GPK_HOST_DEVICE_INLINE bool var_reg_path(int M, int D) { return GPK_VAR_REG && M <= 64 && D <= 32; }
constexpr int kAdjRWaves = 8;   // waves per register-path adjoint workgroup (K-Gram folded in)

template <int MB, int DQ>
constexpr bool var_adj_lreg_fits() {
  if constexpr (MB >= 5) return LAdjGeo<MB, DQ>::fits;
  return false;
}
GPK_HOST_DEVICE_INLINE int adj_dq(int D) { return D <= 32 ? 32 : 64; }

// Instantiated row-block counts; M is padded up to the next one (zero rows).
#define GPK_MB_SWITCH(MBV, CALL)                                                   \
  {                                                                                \
    const int mbv_ = (MBV);                                                        \
    if (mbv_ <= 1) { CALL(1) } else if (mbv_ <= 2) { CALL(2) }                     \
    else if (mbv_ <= 3) { CALL(3) } else if (mbv_ <= 4) { CALL(4) }                \
    else if (mbv_ <= 6) { CALL(6) } else if (mbv_ <= 8) { CALL(8) }                \
    else if (mbv_ <= 12) { CALL(12) } else if (mbv_ <= 16) { CALL(16) }            \
  }

}  // namespace
