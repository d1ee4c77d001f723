// Variational (DeepGP) hot path for gfx950.
//
// Reference (oracle/gp_oracle.py::variational_forward):
//   ToyDeepGPHiddenLayer / DeepGPp (denoising_model/DeepGP.py:15-99) driven through
//   upstream variational/variational_strategy.py (whitened):
//     K_ZZ + jitter (fp32) -> fp64 -> L = psd_safe_cholesky (fp64 ladder 1e-8 x10^i)
//     A    = L^{-1} K_ZX        (fp64, cast to fp32)
//     mean = A^T m + x w + b0   (LinearMean, DeepGP.py:42-45)
//     var  = s2 + jitter + sum_m A_mi^2 (s_m^2 - 1), clamped >= 1e-6 (MVN.variance)
//     ELL  = sum_i -0.5 [((y_i - mean_i)^2 + var_i)/noise + log noise + log 2pi]
//
// (the shared K_ZZ factor and its adjoint: gpk_kzz.hip, gpk_kzz_grad.hip)
//
// Three kernel families and a shared tail, one unit each; which shape goes where (M inducing
// points, D input dims; gpk_launch_var / launch_var_adj below, the first match):
//   M <= 64, D <= 32 (GPK_VAR_REG)   register-resident path: gpk_var_fwd_r_kernel,
//                                    gpk_var_adj_r_kernel (K-Gram folded in), RegLds
//   M > 64 (GPK_VAR_LREG)            L^{-1}-in-registers path: gpk_var_fwd_l_kernel (training keeps
//                                    A where the saved-state adjoint serves, LSaved); adjoint with
//                                    that state: gpk_var_adjs_l_kernel + gpk_var_kgram_l_kernel;
//                                    without: gpk_var_adja_l_kernel + gpk_var_adjk_l_kernel, if their
//                                    LDS plan fits and the dA / K_ZX workspace stays under 2 GB
//   everything else                  LDS-tiled path (today only the fallback): M <= 64 with D in
//                                    (32, 64], and the M > 64 adjoints left over by the line above
//   every path                       gpk_var_ell_kernel after a forward; gpk_dlinv_kernel (paths
//                                    with a dA / K_ZX workspace), gpk_var_red_kernel and
//                                    gpk_var_fin_kernel after an adjoint
// This unit: the plans (adj_plan, adj_plan_common, adj_saved_plan), the workspace / saved-state
// sizes and the dispatch. The per-unit launchers (gpk_var_launch.h) pick (MB, DQ) themselves.
#include "gpk_var_common.h"
#include "gpk_var_launch.h"

namespace {

AdjPlan adj_plan_common(AdjPlan p, int B, int N, int M, int D);

template <int MB>
AdjPlan adj_plan(int B, int N, int M, int D) {
  using G = VarGeo<MB>;
  AdjPlan p{};
  if constexpr (MB >= 5) {
    const bool fits = adj_dq(D) == 32 ? var_adj_lreg_fits<MB, 32>() : var_adj_lreg_fits<MB, 64>();
    const bool small_ws = (long long)M * B * N * 4 < (1LL << 31);   // 32-bit buffer offsets
    if (GPK_VAR_LREG && M > 64 && fits && small_ws) {   // persistent, <= 2 waves / SIMD
      const long long nch = (long long)B * ((N + LTW - 1) / LTW);
      p.nchunks = (int)nch;
      p.nwg = chunk_grid(nch, LAdjGeo<MB, 32>::NWV <= 4 ? 2 : 1);
      return adj_plan_common(p, B, N, M, D);
    }
  }
  if (var_reg_path(M, D)) {
    // workspace (the K-Gram folded into the adjoint): the centre (64) | rows of
    // [adjoint | K-Gram] partials | their fp64 totals (the K-Gram totals at + P)
    const long long nch = (long long)B * ((N + 31) / 32);
    p.nchunks = (int)nch;
    // one workgroup per CU (8 waves, K-Gram folded in)
    const long long nwg_max = 2048 / kAdjRWaves;
    p.nwg = (int)((nch + kAdjRWaves - 1) / kAdjRWaves < nwg_max ? (nch + kAdjRWaves - 1) / kAdjRWaves : nwg_max);
    p = adj_plan_common(p, B, N, M, D);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    p.off_dA = o; o = al(o + 64 * sizeof(float));
    p.off_K = o;
    p.off_part = o; o = al(o + (size_t)p.nwg * (p.P + kGPart) * sizeof(float));
    p.off_tot = o; o = al(o + (size_t)(p.P + kGPart) * sizeof(double));
    p.off_dl = o;
    p.total = o;
    return p;
  }
  p.nchunks = B * ((N + G::TW - 1) / G::TW);
  p.nwg = chunk_grid(p.nchunks, 2);
  return adj_plan_common(p, B, N, M, D);
}

AdjPlan adj_plan_common(AdjPlan p, int B, int N, int M, int D) {
  p.P = M * D + 3 * M + 2 * D + 3;
  p.fin_lds = (size_t)M * D * sizeof(float);
  p.BN = (long long)B * N;
  const int MT = (M + 63) / 64;
  p.ntiles = MT * (MT + 1) / 2;
  long long want = 512 / p.ntiles;
  if (want < 1) want = 1;
  long long cps = (p.BN + want - 1) / want;
  cps = ((cps + DLKC - 1) / DLKC) * DLKC;
  if (cps < DLKC) cps = DLKC;
  p.cols_per_split = cps;
  p.nsplit = (int)((p.BN + cps - 1) / cps);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t o = 0;
  p.off_dA = o; o = al(o + (size_t)M * p.BN * sizeof(float));
  p.off_K = o; o = al(o + (size_t)M * p.BN * sizeof(float));
  p.off_part = o; o = al(o + (size_t)p.nwg * p.P * sizeof(float));
  p.off_tot = o; o = al(o + (size_t)p.P * sizeof(double));
  p.off_dl = o; o = al(o + (size_t)p.nsplit * p.ntiles * 4096 * sizeof(double));
  p.total = o;
  return p;
}

template <int MB, int DQ>
AdjSavedPlan adj_saved_plan(int B, int N, int M, int D) {
  using LG = LGramGeo<MB, DQ>;
  AdjSavedPlan p{};
  const long long nch = (long long)B * ((N + LTW - 1) / LTW);
  p.nchunks = (int)nch;
  p.nwg = chunk_grid(nch, 1);      // 256 VGPRs: one 8-wave workgroup per CU
  p.nwg_g = chunk_grid(nch, 1);
  p.P = M * D + 3 * M + 2 * D + 3;
  p.PG = LG::PG;
  p.BN = (long long)B * N;
  p.fin_lds = (size_t)M * D * sizeof(float);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t o = 0;
  p.off_gpart = o; o = al(o + (size_t)p.nwg_g * p.PG * sizeof(float));
  p.off_part = o; o = al(o + (size_t)p.nwg * p.P * sizeof(float));
  p.off_tot = o; o = al(o + (size_t)p.P * sizeof(double));
  p.off_gtot = o; o = al(o + (size_t)p.PG * sizeof(double));
  p.off_cm = o; o = al(o + 64 * sizeof(float));
  p.total = o;
  return p;
}

template <int MB, int DQ>
int launch_var_adj(const GpkVarAdjArgs& a, hipStream_t stream) {
  if (a.saved != nullptr) {
    if (!var_saved_path<MB, DQ>(a.M)) return -13;
    return gpk_launch_var_adjs_l(a, adj_saved_plan<MB, DQ>(a.B, a.N, a.M, a.D), stream);
  }
  const AdjPlan p = adj_plan<MB>(a.B, a.N, a.M, a.D);
  if (var_reg_path(a.M, a.D)) return gpk_launch_var_adj_r(a, p, stream);
  if constexpr (var_adj_lreg_fits<MB, DQ>()) {
    if (GPK_VAR_LREG && a.M > 64 && (long long)a.M * p.BN * 4 < (1LL << 31))
      return gpk_launch_var_adj_l(a, p, stream);
  }
  return gpk_launch_var_adj_tiled(a, p, stream);
}

}  // namespace

int gpk_launch_var(const GpkVarArgs& a, int* flags, hipStream_t stream) {
  if (flags != nullptr) {
    const hipError_t e = hipMemsetAsync(flags, 0, sizeof(int), stream);
    if (e != hipSuccess) return (int)e;
  }
  if (var_reg_path(a.M, a.D)) return gpk_launch_var_fwd_r(a, flags, stream);
  if (GPK_VAR_LREG && a.M > 64) return gpk_launch_var_fwd_l(a, flags, stream);
  return gpk_launch_var_fwd_tiled(a, flags, stream);
}

size_t gpk_var_adjoint_ws_bytes(int B, int N, int M, int D) {
#define GPK_CALL_WS(mb) return adj_plan<mb>(B, N, M, D).total;
  GPK_MB_SWITCH((M + 15) / 16, GPK_CALL_WS)
#undef GPK_CALL_WS
  return 0;
}

// the saved-state path (training forward keeps A; M > 64, its LDS plan fits): bytes of the saved
// state and of the adjoint's workspace, 0 when the path does not serve the shape
size_t gpk_var_saved_bytes(int B, int N, int M, int D) {
#define GPK_CALL_SV(mb)                                                                        \
  if (adj_dq(D) == 32) return var_saved_path<mb, 32>(M) ? (size_t)B * ((N + LTW - 1) / LTW) *  \
                                  LSaved<mb>::blk * sizeof(float) : 0;                        \
  return var_saved_path<mb, 64>(M) ? (size_t)B * ((N + LTW - 1) / LTW) * LSaved<mb>::blk * sizeof(float) : 0;
  GPK_MB_SWITCH((M + 15) / 16, GPK_CALL_SV)
#undef GPK_CALL_SV
  return 0;
}
size_t gpk_var_adjoint_saved_ws_bytes(int B, int N, int M, int D) {
  if (gpk_var_saved_bytes(B, N, M, D) == 0) return 0;
#define GPK_CALL_SW(mb)                                                        \
  if (adj_dq(D) == 32) return adj_saved_plan<mb, 32>(B, N, M, D).total;        \
  return adj_saved_plan<mb, 64>(B, N, M, D).total;
  GPK_MB_SWITCH((M + 15) / 16, GPK_CALL_SW)
#undef GPK_CALL_SW
  return 0;
}

int gpk_launch_var_adjoint(const GpkVarAdjArgs& a, hipStream_t stream) {
#define GPK_CALL_ADJ(mb)                                         \
  if (a.D <= 32) return launch_var_adj<mb, 32>(a, stream);       \
  return launch_var_adj<mb, 64>(a, stream);
  GPK_MB_SWITCH((a.M + 15) / 16, GPK_CALL_ADJ)
#undef GPK_CALL_ADJ
  return -11;
}
