// Variational hot path: the plans the dispatcher (gpk_variational.hip) hands the per-unit
// launchers, and those launchers. Each launcher picks the (MB, DQ) instantiation for a.M / a.D
// inside its own unit, so every kernel template is instantiated in exactly one unit.
#pragma once
#include "gpk_internal.h"

// recompute adjoint (every path): chunk grid, split-K plan of the dL^{-1} GEMM, workspace layout
struct AdjPlan {
  int nchunks, nwg, P, ntiles, nsplit;
  long long BN, cols_per_split;
  size_t off_dA, off_K, off_part, off_tot, off_dl, total;  // byte offsets
  size_t fin_lds;
};

// ---- the saved-state adjoint (M > 64): workspace G' partials | adjoint partials | their fp64 totals
// | the finalisation partials
struct AdjSavedPlan {
  int nchunks, nwg, nwg_g, P, PG;
  long long BN;
  size_t off_gpart, off_part, off_tot, off_gtot, off_cm, total, fin_lds;
};

// gpk_var_reg.hip (var_reg_path: M <= 64, D <= 32)
int gpk_launch_var_fwd_r(const GpkVarArgs& a, int* flags, hipStream_t stream);
int gpk_launch_var_adj_r(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream);
// gpk_var_fwd_l.hip, gpk_var_adj_l.hip, gpk_var_adjs_l.hip (GPK_VAR_LREG, M > 64)
int gpk_launch_var_fwd_l(const GpkVarArgs& a, int* flags, hipStream_t stream);
int gpk_launch_var_adj_l(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream);
int gpk_launch_var_adjs_l(const GpkVarAdjArgs& a, const AdjSavedPlan& p, hipStream_t stream);
// gpk_var_tiled.hip (everything else)
int gpk_launch_var_fwd_tiled(const GpkVarArgs& a, int* flags, hipStream_t stream);
int gpk_launch_var_adj_tiled(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream);
// gpk_var_tail.hip: the ELL sum after a forward; after an adjoint, one fixed-order reduction
// launch of nwg partial rows of P floats -> tot (and of a second array, P2 floats -> tot2, when
// wspart2 is given), the output launch (gtot: dL^{-1} from K-Gram totals in extra workgroups,
// gdl_mb = 0 register path, MB saved-state path), and dL^{-1} GEMM + reductions + outputs
int gpk_launch_var_ell(const GpkVarArgs& a, hipStream_t stream);
int gpk_launch_var_red(const GpkVarAdjArgs& a, hipStream_t stream, const float* wspart, int nwg, int P,
                       double* tot, const float* wspart2, int P2, double* tot2, GpkOStr bs);
int gpk_launch_var_fin(const GpkVarAdjArgs& a, const double* tot, GpkOStr bs, hipStream_t stream,
                       const float* cm_in = nullptr, const double* gtot = nullptr, int gdl_mb = 0);
int gpk_launch_var_adj_tail(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream);
