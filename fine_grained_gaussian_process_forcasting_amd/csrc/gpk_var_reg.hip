// Variational hot path, register-resident unit: gpk_var_fwd_r_kernel and gpk_var_adj_r_kernel
// (K-Gram folded in), RegLds. Shapes: M <= 64 and D <= 32 (var_reg_path, GPK_VAR_REG), the first
// match of the dispatch in gpk_variational.hip. The GPK_ADJR_* dev hooks live here too.
#include "gpk_var_common.h"
#include "gpk_var_launch.h"

namespace {

// ---------------------------------------------------------------------------
// Register-resident variants for M <= 64, D <= 32 (BASELINE cfg 5: M = 64, D = 32).
// With at most 4 row tiles every wave owns ALL rows of its points, so the waves of a
// workgroup never exchange data: each wave walks its own 32-point chunks (2 column
// tiles) and keeps K_ZX, A = L^{-1} K_ZX, dA, dK and Q in MFMA registers. The f32 Gram
// feeds the zs rows in the order pi(x) = (x >> 2) + 4 (x & 3), so its accumulator holds
// row g + 4r in register r -- the f64 MFMA layout -- and K_ZX tiles are directly the B
// operands of the f64 products. L^{-1} (fp64, row stride 66: conflict-free reads) and zs
// live in LDS, shared by the 4 waves; only the adjoint's Q^T needs a per-wave LDS
// transpose (one tile at a time).
// ---------------------------------------------------------------------------
// stage zs, norms, q(u) moments (stage_inducing) and L^{-1} (zero padded to 64 x 64)
template <int DQ>
GPK_DEVICE void stage_reg(const float* Z, const float* ls, const float* vmean, const float* vstd,
                          const double* Linv, int M, int D, float* sm) {
  using L = RegLds<DQ>;
  stage_inducing(Z, ls, vmean, vstd, M, D, 64, DQ, L::ZS, sm + L::zs, sm + L::zn, sm + L::cm,
                 sm + L::vm, sm + L::sm1, sm + L::li);   // (L^{-1} is staged afterwards)
  double* li = (double*)(sm + L::li);
  for (int base = 0; base < 64 * 64; base += 8 * (int)blockDim.x) {   // 8 loads in flight
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * blockDim.x + threadIdx.x, r = e >> 6, c = e & 63;
      v[u] = Linv[(e < 64 * 64 && r < M && c < M) ? (size_t)r * M + c : 0];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * blockDim.x + threadIdx.x, r = e >> 6, c = e & 63;
      if (e < 64 * 64) li[r * RLS + c] = (r < M && c < M) ? v[u] : 0.0;
    }
  }
  lds_barrier();
}

GPK_DEVICE int pi_row(int x) { return (x >> 2) + 4 * (x & 3); }


// Points i0 + 16q + c of window b: Gram B operands xb[q][s] = xs[i][4s + g], squared
// norms (full, every lane), and optionally x . w (full).
template <int DQ>
struct RegPoints {
  float xb[2][DQ / 4];
  float xn[2];
  float lin[2];
};

template <int DQ, bool LIN>
GPK_DEVICE void load_points(const float* X, int N, int D, int b, int i0, const float (&il)[DQ / 4],
                            const float (&cmv)[DQ / 4], const float (&wv)[DQ / 4], RegPoints<DQ>& P) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int i = i0 + 16 * q + c;
    const bool ok = i < N;
    const float* xr = X + ((size_t)b * N + (ok ? i : 0)) * D;
    float nn = 0.f, lw = 0.f;
#pragma unroll
    for (int s = 0; s < DQ / 4; ++s) {
      const int d = 4 * s + g;
      const float raw = (ok && d < D) ? xr[d] : 0.f;
      const float v = (d < D) ? raw * il[s] - cmv[s] : 0.f;
      P.xb[q][s] = ok ? v : 0.f;
      nn = __builtin_fmaf(P.xb[q][s], P.xb[q][s], nn);
      if (LIN) lw = __builtin_fmaf(raw, wv[s], lw);
    }
    nn += __shfl_xor(nn, 16, 64);
    nn += __shfl_xor(nn, 32, 64);
    P.xn[q] = nn;
    if (LIN) {
      lw += __shfl_xor(lw, 16, 64);
      lw += __shfl_xor(lw, 32, 64);
      P.lin[q] = lw;
    }
  }
}

// K_ZX tiles (register r <-> row 16 rt + g + 4r, column 16q + c), zero outside M x N
template <int DQ>
GPK_DEVICE void build_k_reg(const float* sm, const RegPoints<DQ>& P, int M, int N, int i0, float s2,
                            f32x4 (&K)[4][2]) {
  using L = RegLds<DQ>;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const float* zs = sm + L::zs;
  const float* zn = sm + L::zn;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    float za[DQ / 4];
#pragma unroll
    for (int s = 0; s < DQ / 4; ++s) za[s] = zs[(16 * rt + pi_row(c)) * L::ZS + 4 * s + g];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < DQ / 4; ++s) acc = mfma32(za[s], P.xb[q][s], acc);
      const bool ok = i0 + 16 * q + c < N;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 16 * rt + g + 4 * r;
        const float d2 = __builtin_fmaxf(zn[p] + P.xn[q] - 2.f * acc[r], 0.f);
        K[rt][q][r] = (ok && p < M) ? s2 * __builtin_amdgcn_exp2f(kNHalfLog2e * d2) : 0.f;
      }
    }
  }
}

// A = L^{-1} K (fp64 MFMA, k-order m = 16 kb + g + 4u; L^{-1} lower: kb <= rt), one row
// tile at a time, cast to fp32 as the reference does (A.float()): the f64 accumulators of
// only one row tile are live at a time.
template <int DQ>
GPK_DEVICE void linv_times_k(const float* sm, const f32x4 (&K)[4][2], f32x4 (&A)[4][2]) {
  using L = RegLds<DQ>;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const double* li = (const double*)(sm + L::li);
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int kb = 0; kb <= rt; ++kb)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double la = li[(16 * rt + c) * RLS + 16 * kb + g + 4 * u];
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[q] = mfma64(la, (double)K[kb][q][u], acc[q]);
      }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) A[rt][q][r] = (float)acc[q][r];
  }
}

// per-lane constants of the dims this lane touches as a Gram operand: 4s + g
template <int DQ>
GPK_DEVICE void dim_consts(const float* sm, const float* ls, const float* w, int D, float (&il)[DQ / 4],
                           float (&cmv)[DQ / 4], float (&wv)[DQ / 4]) {
  using L = RegLds<DQ>;
  const int g = (threadIdx.x & 63) >> 4;
  // every load issued first (clamped in-bounds addresses), then masked
  float lv[DQ / 4], wl[DQ / 4];
#pragma unroll
  for (int s = 0; s < DQ / 4; ++s) {
    const int d = 4 * s + g, dc = d < D ? d : 0;
    lv[s] = ls[dc];
    wl[s] = w != nullptr ? w[dc] : 0.f;
  }
#pragma unroll
  for (int s = 0; s < DQ / 4; ++s) {
    const int d = 4 * s + g;
    il[s] = d < D ? 1.f / lv[s] : 0.f;
    cmv[s] = sm[L::cm + d];
    wv[s] = d < D ? wl[s] : 0.f;
  }
}

template <int DQ>
__global__ void __launch_bounds__(256, GPK_FWD_OCC)
gpk_var_fwd_r_kernel(const float* __restrict__ X, const float* __restrict__ Z,
                     const double* __restrict__ Linv, const float* __restrict__ vmean,
                     const float* __restrict__ vstd, const float* __restrict__ hyp, int B, int N,
                     int M, int D, float* __restrict__ mean_out, float* __restrict__ var_out,
                     int* __restrict__ flags, GpkOStr bs) {
  GPK_O_MODEL();
  GPK_O_ADD(Linv, M * M);
  GPK_O_ADD(mean_out, bs.bn);
  GPK_O_ADD(var_out, bs.bn);
  using L = RegLds<DQ>;
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  const float s2 = hyp[0], jit = hyp[2], b0 = hyp[3];
  const float* w = hyp + 4;
  const float* ls = hyp + 4 + D;
  stage_reg<DQ>(Z, ls, vmean, vstd, Linv, M, D, vsm);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = threadIdx.x >> 6;
  float il[DQ / 4], cmv[DQ / 4], wv[DQ / 4];
  dim_consts<DQ>(vsm, ls, w, D, il, cmv, wv);
  const int nch = (N + 31) / 32;
  const long long total = (long long)B * nch;
  int clamped = 0;
  for (long long t = (long long)blockIdx.x * 4 + wave; t < total; t += (long long)gridDim.x * 4) {
    const int b = (int)(t / nch), i0 = (int)(t - (long long)b * nch) * 32;
    const float* sm = fresh_lds(vsm);
    const float* vm = sm + L::vm;
    const float* sm1 = sm + L::sm1;
    RegPoints<DQ> P;
    load_points<DQ, true>(X, N, D, b, i0, il, cmv, wv, P);
    f32x4 K[4][2];
    build_k_reg<DQ>(sm, P, M, N, i0, s2, K);
    f32x4 A[4][2];
    linv_times_k<DQ>(sm, K, A);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float mp = 0.f, vp = 0.f;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = 16 * rt + g + 4 * r;
          const float a32 = A[rt][q][r];   // A is cast to fp32 (reference)
          mp = __builtin_fmaf(a32, vm[p], mp);
          vp = __builtin_fmaf(a32 * a32, sm1[p], vp);
        }
      mp += __shfl_xor(mp, 16, 64);
      mp += __shfl_xor(mp, 32, 64);
      vp += __shfl_xor(vp, 16, 64);
      vp += __shfl_xor(vp, 32, 64);
      const int i = i0 + 16 * q + c;
      if (g == q && i < N) {
        float var_i = s2 + jit + vp;
        if (var_i < 1e-6f) { var_i = 1e-6f; clamped = 1; }   // MVN.variance clamp (fp32)
        mean_out[(size_t)b * N + i] = mp + (P.lin[q] + b0);
        var_out[(size_t)b * N + i] = var_i;
      }
    }
  }
  if (flags != nullptr && clamped)
    (void)__hip_atomic_fetch_or(flags, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// FG (the K-Gram folded in, NW = 8): the same pass also accumulates the K-Gram partials of
// gpk_var_kgram_r_kernel -- G = K_ZX diag(gvar) K_ZX^T (10 lower tiles, per-wave fp32 in LDS)
// and u = sum gmean K_ZX -- from the K_ZX tiles it already holds, so X is read once per
// adjoint instead of twice and the clamp-masked gvar never goes to HBM. The K-Gram partial
// follows the adjoint partial in the workgroup's row (one reduction launch for both), and
// block 0 writes the centre cm for gpk_var_fin_kernel.

#ifndef GPK_ADJR_STAMPS
#define GPK_ADJR_STAMPS 0   // dev builds: per-phase s_memtime cycle totals per wave (gpk_dev_adjr_stamps)
#endif
#if GPK_ADJR_STAMPS
__device__ unsigned g_adjr_st[4096 * 16];
extern "C" int gpk_dev_adjr_stamps(unsigned* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_adjr_st), (size_t)n * sizeof(unsigned), 0,
                                  hipMemcpyDeviceToHost);
}
#endif
#ifndef GPK_ADJR_SKIP
#define GPK_ADJR_SKIP 0   // timing-only ablations (wrong results): 1 G, 2 dK, 4 Q^T zs, 8 QX, 16 dX, 64 A
#endif
#ifndef GPK_ADJR_DK32
#define GPK_ADJR_DK32 1   // dK = L^{-T} dA on f32 MFMA (0: fp64, the round-5 form)
#endif
template <int DQ, int NW, bool FG>
__global__ void __launch_bounds__(64 * NW, 8 / NW)
gpk_var_adj_r_kernel(const float* __restrict__ X, const float* __restrict__ Z,
                     const double* __restrict__ Linv, const float* __restrict__ vmean,
                     const float* __restrict__ vstd, const float* __restrict__ hyp,
                     const float* __restrict__ gmean, const float* __restrict__ gvar, int B, int N,
                     int M, int D, long long BN, float* __restrict__ wsgv,
                     float* __restrict__ wspart, float* __restrict__ cm_out, float* __restrict__ dX,
                     GpkOStr bs) {
  GPK_O_MODEL();
  GPK_O_ADD(Linv, M * M);
  GPK_O_ADD(gmean, bs.bn);
  GPK_O_ADD(gvar, bs.bn);
  GPK_O_ADD(wsgv, bs.ws);
  GPK_O_ADD(wspart, bs.ws);
  GPK_O_ADD(cm_out, bs.ws);
  GPK_O_ADD(dX, bs.bn * D);
  using L = RegLds<DQ, NW, FG>;
  constexpr int NDT = DQ / 16;
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  const float s2 = hyp[0], jit = hyp[2];
  const float* w = hyp + 4;
  const float* ls = hyp + 4 + D;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = tid >> 6;
  stage_reg<DQ>(Z, ls, vmean, vstd, Linv, M, D, vsm);
  float* rows = vsm + L::rows + wave * 4 * 64;    // this wave's dvm | dsm | q | u accumulators
  for (int e = lane; e < 4 * 64; e += 64) rows[e] = 0.f;
  float* scr = vsm + L::scr + wave * 320;
  float* ga = vsm + L::gacc + wave * (kGTiles * 256);   // FG: this wave's G tiles (acc order)
  if constexpr (FG)
    for (int e = lane; e < kGTiles * 64; e += 64) *(f32x4*)(ga + 4 * e) = f32x4{0.f, 0.f, 0.f, 0.f};
  float il[DQ / 4], cmv[DQ / 4], wv[DQ / 4];
  dim_consts<DQ>(vsm, ls, nullptr, D, il, cmv, wv);
  // constants of the dims 16 dt + c (QX / dX operands)
  float ilc[NDT], cmc[NDT], wc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    const int d = 16 * dt + c;
    const float lsv = ls[d < D ? d : 0], wv_ = w[d < D ? d : 0];   // unconditional loads
    ilc[dt] = d < D ? 1.f / lsv : 0.f;
    cmc[dt] = vsm[L::cm + d];
    wc[dt] = d < D ? wv_ : 0.f;
  }
  f32x4 qx[4][NDT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) qx[rt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float rx2[NDT] = {}, gx[NDT] = {};
  float sumQ = 0.f, sumgv = 0.f, sumgm = 0.f;

  const int nch = (N + 31) / 32;
  const long long total = (long long)B * nch;
#if GPK_ADJR_STAMPS
  unsigned long long st_acc[10] = {}, st_last = __builtin_amdgcn_s_memtime();
#define GPK_ADJR_ST(k)                                          \
  {                                                             \
    __builtin_amdgcn_sched_barrier(0);                          \
    const unsigned long long _n = __builtin_amdgcn_s_memtime(); \
    st_acc[k] += _n - st_last;                                  \
    st_last = _n;                                               \
    __builtin_amdgcn_sched_barrier(0);                          \
  }
#else
#define GPK_ADJR_ST(k)
#endif
  for (long long t = (long long)blockIdx.x * NW + wave; t < total; t += (long long)gridDim.x * NW) {
    GPK_ADJR_ST(0)
    const int b = (int)(t / nch), i0 = (int)(t - (long long)b * nch) * 32;
    const size_t col0 = (size_t)b * N;
    const float* sm = fresh_lds(vsm);
    const float* zs = sm + L::zs;
    const float* vm = sm + L::vm;
    const float* sm1 = sm + L::sm1;
    const double* li = (const double*)(sm + L::li);
    RegPoints<DQ> P;
    load_points<DQ, false>(X, N, D, b, i0, il, cmv, wv, P);
    f32x4 K[4][2];
    build_k_reg<DQ>(sm, P, M, N, i0, s2, K);
    GPK_ADJR_ST(1)
    f32x4 A[4][2];
    if (GPK_ADJR_SKIP & 64) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int q = 0; q < 2; ++q) A[rt][q] = K[rt][q];
    } else {
      linv_times_k<DQ>(sm, K, A);
    }
    GPK_ADJR_ST(2)
    // variance -> clamp mask; point gradients
    float gmq[2], gvq[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float vp = 0.f;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a32 = A[rt][q][r];
          vp = __builtin_fmaf(a32 * a32, sm1[16 * rt + g + 4 * r], vp);
        }
      vp += __shfl_xor(vp, 16, 64);
      vp += __shfl_xor(vp, 32, 64);
      const int i = i0 + 16 * q + c;
      const bool ok = i < N;
      const float gml = gmean[col0 + (ok ? i : 0)], gvl = gvar[col0 + (ok ? i : 0)];   // clamped
      gmq[q] = ok ? gml : 0.f;
      gvq[q] = ok ? gvl : 0.f;
      if (s2 + jit + vp < 1e-6f) gvq[q] = 0.f;   // clamp_min(1e-6): gradient masked
      if (g == 0) {
        sumgv += gvq[q];
        sumgm += gmq[q];
      }
    }
    // dA (fp32, in A's registers) and the dvmean / dvstd row partials
    f32x4 (&dA)[4][2] = A;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 16 * rt + g + 4 * r;
        const float vmp = vm[p], smp = sm1[p];
        float pm = 0.f, ps = 0.f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float a32 = A[rt][q][r];
          dA[rt][q][r] = gmq[q] * vmp + 2.f * gvq[q] * smp * a32;
          pm = __builtin_fmaf(gmq[q], a32, pm);
          ps = __builtin_fmaf(gvq[q], a32 * a32, ps);
        }
        pm = row16_sum_f(pm);
        ps = row16_sum_f(ps);
        float pu = 0.f;
        if constexpr (FG) pu = row16_sum_f(__builtin_fmaf(gmq[1], K[rt][1][r], gmq[0] * K[rt][0][r]));
        if (c == 0) {
          lds_acc(rows + p, pm);
          lds_acc(rows + 64 + p, ps);
          if constexpr (FG) lds_acc(rows + 192 + p, pu);
        }
      }
    GPK_ADJR_ST(3)
    // dL^{-1} = vm u^T + 2 (s^2 - 1) o L^{-1} G with u = sum gmean K_ZX and
    // G = K_ZX diag(gvar) K_ZX^T, so neither dA nor K_ZX makes an HBM round trip
    if constexpr (FG && !(GPK_ADJR_SKIP & 1)) {
      // G(rt, rp) += sum_points K_rt diag(gv) K_rp^T: each K tile transposed through the
      // wave's scratch (points -> k), then sum_s mfma(K^T.reg[s], (gv K)^T.reg[s]) as in
      // gpk_var_kgram_r_kernel (same acc layout); the tiles live in LDS between chunks
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float aK[4][4], aW[4][4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) scr[lane * 5 + r] = K[rt][q][r];
          adj_lds_order();
#pragma unroll
          for (int s = 0; s < 4; ++s) aK[rt][s] = scr[((c & 3) * 16 + 4 * s + g) * 5 + (c >> 2)];
          adj_lds_order();
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float gvp = __shfl(gvq[q], 4 * s + g, 64);   // gvar of point 16 q + 4 s + g
#pragma unroll
          for (int rt = 0; rt < 4; ++rt) aW[rt][s] = aK[rt][s] * gvp;
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int rp = 0; rp <= rt; ++rp) {
            f32x4* gp = (f32x4*)(ga + 4 * ((rt * (rt + 1) / 2 + rp) * 64 + lane));
            f32x4 acc = *gp;
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma32(aK[rt][s], aW[rp][s], acc);
            *gp = acc;
          }
      }
    } else if constexpr (!FG) {
      // the clamp-masked gvar -> workspace for gpk_var_kgram_r_kernel
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int i = i0 + 16 * q + c;
        if (i < N && g == 0) wsgv[col0 + i] = gvq[q];
      }
    }
    GPK_ADJR_ST(4)
    // dK = L^{-T} dA (L^{-T} upper: kb >= rt), then Q = dK o K_ZX (in K's registers). Round 6:
    // on f32 MFMA (GPK_ADJR_DK32; the reference's dK is fp64, the gradients stay ~1e-6 from the
    // fp64 oracle) with the L^{-1} columns fed in pi order, so the f32 C layout of the result
    // (row 4 g + r) holds dK row g + 4 r -- K's layout -- in register r.
#pragma unroll
    for (int rt = 0; rt < 4 && !(GPK_ADJR_SKIP & 2); ++rt) {
      if constexpr (GPK_ADJR_DK32) {
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        const int cp = pi16(c);
#pragma unroll
        for (int kb = rt; kb < 4; ++kb)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float la = (float)li[(16 * kb + g + 4 * u) * RLS + 16 * rt + cp];
#pragma unroll
            for (int q = 0; q < 2; ++q) acc[q] = mfma32(la, dA[kb][q][u], acc[q]);
          }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) K[rt][q][r] = acc[q][r] * K[rt][q][r];
      } else {
        f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
        for (int kb = rt; kb < 4; ++kb)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const double la = li[(16 * kb + g + 4 * u) * RLS + 16 * rt + c];
#pragma unroll
            for (int q = 0; q < 2; ++q) acc[q] = mfma64(la, (double)dA[kb][q][u], acc[q]);
          }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) K[rt][q][r] = (float)acc[q][r] * K[rt][q][r];
      }
    }
    GPK_ADJR_ST(5)
    // r_i = sum_p Q_pi (every lane c of a column), q_p row partials, sum Q
    float rq[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float v = 0.f;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) v += (K[rt][q][0] + K[rt][q][1]) + (K[rt][q][2] + K[rt][q][3]);
      sumQ += v;
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      rq[q] = v;
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = row16_sum_f(K[rt][0][r] + K[rt][1][r]);
        if (c == 0) lds_acc(rows + 128 + 16 * rt + g + 4 * r, v);
      }
    GPK_ADJR_ST(6)
    // (Q^T zs)_i: f32 MFMA with k = p (rows g + 4r of each row tile)
    f32x4 xz[2][NDT];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) xz[q][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const float zb = zs[(16 * rt + g + 4 * r) * L::ZS + 16 * dt + c];
#pragma unroll
          for (int q = 0; q < 2; ++q)
            if (!(GPK_ADJR_SKIP & 4)) xz[q][dt] = mfma32(K[rt][q][r], zb, xz[q][dt]);
        }
    GPK_ADJR_ST(7)
    // QX_p += sum_i Q_pi xs_i: Q tiles transposed through LDS (k = point 4s + g)
#pragma unroll
    for (int q = 0; q < 2 && !(GPK_ADJR_SKIP & 8); ++q) {
      float xb2[4][NDT];
#pragma unroll
      for (int s = 0; s < 4; ++s)     // unconditional (clamped) loads: all in flight together
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const int i = i0 + 16 * q + 4 * s + g, d = 16 * dt + c;
          xb2[s][dt] = X[(i < N && d < D) ? (col0 + i) * D + d : 0];
        }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const int i = i0 + 16 * q + 4 * s + g, d = 16 * dt + c;
          xb2[s][dt] = (i < N && d < D) ? xb2[s][dt] * ilc[dt] - cmc[dt] : 0.f;
        }
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) scr[lane * 5 + r] = K[rt][q][r];
        adj_lds_order();
        float aq[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) aq[s] = scr[((c & 3) * 16 + 4 * s + g) * 5 + (c >> 2)];
        adj_lds_order();   // the next tile overwrites scr
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int s = 0; s < 4; ++s) qx[rt][dt] = mfma32(aq[s], xb2[s][dt], qx[rt][dt]);
      }
    }
    GPK_ADJR_ST(8)
    // dX_i = ((Q^T zs)_i - xs_i r_i) / l + gmean_i w; sum_i r_i xs_i^2, sum_i gmean_i xs_i
    // (the point values are requested up front, unconditionally: clamped addresses)
    float xo[2][4][NDT];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const int i = i0 + 16 * q + 4 * g + r, d = 16 * dt + c;
          xo[q][r][dt] = X[(i < N && d < D) ? (col0 + i) * D + d : 0];
        }
    // (branch-free but for the stores: a load whose only use sits under the point / dim
    // guard is sunk into it by the compiler and waited for one point at a time)
#pragma unroll
    for (int q = 0; q < 2 && !(GPK_ADJR_SKIP & 16); ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pc = 4 * g + r;                  // point (within the tile) of register r
        const float rr = __shfl(rq[q], pc, 64);
        const float gm = __shfl(gmq[q], pc, 64);
        const int i = i0 + 16 * q + pc;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const int d = 16 * dt + c;
          const bool ok = i < N && d < D;
          const float xv = ok ? xo[q][r][dt] * ilc[dt] - cmc[dt] : 0.f;
          const float dxv = (xz[q][dt][r] - xv * rr) * ilc[dt] + gm * wc[dt];
          if (ok) dX[(col0 + i) * D + d] = dxv;
          rx2[dt] = __builtin_fmaf(rr * xv, xv, rx2[dt]);
          gx[dt] = __builtin_fmaf(gm, xv, gx[dt]);
        }
      }
    GPK_ADJR_ST(9)
  }
#if GPK_ADJR_STAMPS
  if (lane == 0) {
#pragma unroll
    for (int k2 = 0; k2 < 10; ++k2) g_adjr_st[(blockIdx.x * NW + wave) * 16 + k2] = (unsigned)st_acc[k2];
  }
#endif
#undef GPK_ADJR_ST


  // ---- workgroup partials, summed over the waves in a fixed order:
  //   [QX (M x D) | q (M) | dvm (M) | dsm (M) | rx2 (D) | sumQ | sumgv | gx (D) | sumgm]
  float* qxr = vsm + L::qxr;
  float* misc = vsm + L::misc + wave * (2 * DQ + 3);
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    float v = rx2[dt], u = gx[dt];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    u += __shfl_xor(u, 16, 64);
    u += __shfl_xor(u, 32, 64);
    if (g == 0) {
      misc[16 * dt + c] = v;
      misc[DQ + 16 * dt + c] = u;
    }
  }
  sumQ = wave_sum(sumQ);
  sumgv = wave_sum(sumgv);
  sumgm = wave_sum(sumgm);
  if (lane == 0) {
    misc[2 * DQ] = sumQ;
    misc[2 * DQ + 1] = sumgv;
    misc[2 * DQ + 2] = sumgm;
  }
  for (int wv2 = 0; wv2 < NW; ++wv2) {
    lds_barrier();
    if (wave == wv2) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int e = (16 * rt + 4 * g + r) * DQ + 16 * dt + c;
            qxr[e] = (wv2 == 0 ? 0.f : qxr[e]) + qx[rt][dt][r];
          }
    }
  }
  lds_barrier();
  const int P = M * D + 3 * M + 2 * D + 3;
  float* po = wspart + (size_t)blockIdx.x * (P + (FG ? kGPart : 0));
  if (FG && blockIdx.x == 0 && tid < D) cm_out[tid] = vsm[L::cm + tid];
  for (int e = tid; e < M * D; e += blockDim.x) {
    const int p = e / D, d = e - p * D;
    po[e] = qxr[p * DQ + d];
  }
  const float* rw = vsm + L::rows;
  for (int m = tid; m < M; m += blockDim.x) {
    float a = 0.f, s = 0.f, qq = 0.f;
    for (int u = 0; u < NW; ++u) {
      a += rw[u * 256 + m];
      s += rw[u * 256 + 64 + m];
      qq += rw[u * 256 + 128 + m];
    }
    po[M * D + m] = qq;
    po[M * D + M + m] = a;
    po[M * D + 2 * M + m] = s;
  }
  const float* ms = vsm + L::misc;
  for (int d = tid; d < D; d += blockDim.x) {
    float v = 0.f, u = 0.f;
    for (int k = 0; k < NW; ++k) {
      v += ms[k * (2 * DQ + 3) + d];
      u += ms[k * (2 * DQ + 3) + DQ + d];
    }
    po[M * D + 3 * M + d] = v;
    po[M * D + 3 * M + D + 2 + d] = u;
  }
  if (tid == 0) {
    float a = 0.f, v = 0.f, u = 0.f;
    for (int k = 0; k < NW; ++k) {
      a += ms[k * (2 * DQ + 3) + 2 * DQ];
      v += ms[k * (2 * DQ + 3) + 2 * DQ + 1];
      u += ms[k * (2 * DQ + 3) + 2 * DQ + 2];
    }
    po[M * D + 3 * M + D] = a;
    po[M * D + 3 * M + D + 1] = v;
    po[M * D + 3 * M + 2 * D + 2] = u;
  }
  if constexpr (FG) {
    // K-Gram partial [G lower tiles (10 x 256, acc order) | u (64)], waves in a fixed order
    const float* gw = vsm + L::gacc;
    float* pg = po + P;
    for (int e = tid; e < kGTiles * 256; e += blockDim.x) {
      const int t2 = e >> 8, r = (e >> 6) & 3, ln = e & 63;
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < NW; ++k) v += gw[k * (kGTiles * 256) + 4 * (t2 * 64 + ln) + r];
      pg[e] = v;
    }
    for (int m = tid; m < 64; m += blockDim.x) {
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < NW; ++k) v += rw[k * 256 + 192 + m];
      pg[kGTiles * 256 + m] = v;
    }
  }
}

template <int DQ>
int launch_var_fwd_r(const GpkVarArgs& a, int* flags, hipStream_t stream) {
  const size_t lds = (size_t)RegLds<DQ>::fwd_total * sizeof(float);
  set_lds_once<gpk_var_fwd_r_kernel<DQ>>();
  const long long nch = (long long)a.B * ((a.N + 31) / 32);
  const long long nwg = (nch + 3) / 4 < 768 ? (nch + 3) / 4 : 768;
  hipLaunchKernelGGL((gpk_var_fwd_r_kernel<DQ>), dim3((unsigned)nwg, a.O), dim3(256), lds, stream, a.X, a.Z,
                     a.Linv, a.vmean, a.vstd, a.hyp, a.B, a.N, a.M, a.D, a.mean, a.var, flags, fwd_strides(a));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return a.ell != nullptr ? gpk_launch_var_ell(a, stream) : 0;
}

}  // namespace

int gpk_launch_var_fwd_r(const GpkVarArgs& a, int* flags, hipStream_t stream) {
  return a.D <= 16 ? launch_var_fwd_r<16>(a, flags, stream) : launch_var_fwd_r<32>(a, flags, stream);
}

int gpk_launch_var_adj_r(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream) {
  const GpkOStr bs = adj_strides(a, p.total);   // output o works in workspace slice o
  char* ws = (char*)a.ws;
  float* wsdA = (float*)(ws + p.off_dA);
  float* wspart = (float*)(ws + p.off_part);
  constexpr int RQ = 32;   // the adjoint's DQ (adj_dq) of every D this path serves
  float* wsgv = wsdA;   // FG: the centre cm (D floats)
  double* tot = (double*)(ws + p.off_tot);
  constexpr int NW = kAdjRWaves;
  constexpr bool FG = true;   // the K-Gram folded into the adjoint (round 5)
  double* gtot = tot + p.P;   // the K-Gram totals after the adjoint totals
  static_assert(RegLds<RQ, NW, FG>::adj_total * sizeof(float) <= 160 * 1024, "LDS per workgroup");
  const size_t lds = (size_t)RegLds<RQ, NW, FG>::adj_total * sizeof(float);
  set_lds_once<gpk_var_adj_r_kernel<RQ, NW, FG>>();
  hipLaunchKernelGGL((gpk_var_adj_r_kernel<RQ, NW, FG>), dim3(p.nwg, a.O), dim3(64 * NW), lds, stream, a.X,
                     a.Z, a.Linv, a.vmean, a.vstd, a.hyp, a.gmean, a.gvar, a.B, a.N, a.M, a.D, p.BN,
                     wsgv, wspart, wsgv, a.dX, bs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  // one fixed-order reduction of the [adjoint | K-Gram] rows; dL^{-1} in the output launch
  const int PR = p.P + kGPart;
  if (int rc = gpk_launch_var_red(a, stream, wspart, p.nwg, PR, tot, nullptr, 0, nullptr, bs)) return rc;
  return gpk_launch_var_fin(a, tot, bs, stream, wsgv, gtot, 0);
}
