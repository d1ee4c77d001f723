// Exact-GP hot path for gfx950: per-window RBF Gram + jittered Cholesky +
// forward solve + marginal log likelihood, fused into ONE kernel launch.
//
// Replaces, per window b (reference semantics: oracle/gp_oracle.py::exact_mll):
//   K_hat = s2 * exp(-0.5 * ||(x_i - x_j)/l||^2) + sigma2 * I   (GPModel.py:7-13,
//           upstream kernels/rbf_kernel.py + likelihoods/gaussian_likelihood.py)
//   L     = psd_safe_cholesky(K_hat)                          (upstream linear_operator
//           utils/cholesky.py: jitter ladder 1e-6,1e-5,1e-4 applied per window)
//   mll   = -0.5 * (||L^{-1}(y-c)||^2 + 2 sum log L_ii + N log 2pi) / N
//           (upstream mlls/exact_marginal_log_likelihood.py, MVN.log_prob)
//
// Design: one workgroup of W waves per window, two workgroups
// per CU. The padded K_hat (NB x NB tiles of 16x16, upper triangle) lives in
// REGISTERS as MFMA accumulators (acc layout, see gpk_common.h) of the W-1
// worker waves; the right-hand side y - c is a block column in LDS. Tiles are
// dealt to workers in row-descending order (plan_tile), so at step k the tiles
// a wave still has to update are a PREFIX of its slots. The blocked
// right-looking Cholesky works on R = L^T (accumulators hold -T, so every
// update is a plain MFMA accumulate).
// The last wave is the DIAGONAL wave and owns the critical path alone:
//   factor (k,k) -> publish R_kk^{-T} -> R_{k,k+1} = R_kk^{-T} T'_{k,k+1} ->
//   T''_{k+1,k+1} = T'_{k+1,k+1} - R_{k,k+1}^T R_{k,k+1} -> factor (k+1,k+1)
// (look-ahead), fed by the workers with (k,k+1) and (k+1,k+1) updated through
// panel k-1. It never joins a barrier: the workers synchronise among
// themselves (LDS counter) and every hand-off is an LDS flag holding a
// monotone epoch. The workers per step: trailing update from panel k-1 (the
// two hand-over tiles first), upper-L zeroing, right-hand side, the deferred
// RBF of block row k+2 (the Gram is additive, so it may land after earlier
// updates), then the TRSM of block row k into panel k once R_kk^{-T} is out.
// Diagonal tiles are factored by one wave in one sweep: lanes 0-15 hold columns
// of R, lanes 16-31 columns of R^{-T}, and both are produced by the SAME
// DPP-broadcast instruction stream.
// Flag waits read LDS only (ds_read + lgkmcnt): the L stores stream out behind
// the factorisation instead of being drained at each step.
// In the column-ownership plan (N in 241..256 at two windows per CU, worker_step_col)
// the right-hand side is not a tile at all: each of its block rows is 16 floats in
// LDS, updated by the wave that owns that block column with a VALU matvec straight
// from the TRSM's result registers, and z_k travels as 16 unrounded fp32 words.
#include "gpk_exact_launch.h"

// N -> NB -> the unit that holds NB's instantiations.
int gpk_launch_exact(const GpkExactArgs& a, hipStream_t stream) {
  const int NB = (a.N + 15) / 16;
  if (NB <= 8) return gpk_launch_exact_nb1_8(a, NB, stream);
  if (NB == 9 || NB == 16) return gpk_launch_exact_nb9_nb16(a, NB, stream);
  if (NB <= 11) return gpk_launch_exact_nb10_11(a, NB, stream);
  if (NB <= 13) return gpk_launch_exact_nb12_13(a, NB, stream);
  if (NB <= 15) return gpk_launch_exact_nb14_15(a, NB, stream);
  return -6;
}
