// Launch descriptor of the adjoint of the dense covariance of q(f) (gpk_variational_cov_grad_f32,
// gpk_variational_cov_grad.hip), shared by the kernels' unit and the C-ABI shim.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct GpkVarCovGradArgs {
  const float* X;        // (B, N, D), or (O, B, N, D) with x_stride = B N D
  const float* Z;        // (O, M, D)
  const double* Linv;    // (O, M, M)
  const float* vstd;     // (O, M)
  const float* hyp;      // (O, 4 + 2 D), as GpkVarCovArgs
  const float* state;    // the forward's workspace: per output A (B, M, as), then the means (B, 64)
  const float* gcov;     // (O, B, N, N) dObjective / dcov, any matrix
  int B, N, M, D, O;
  long long x_stride;    // elements between two outputs' inputs (0: shared)
  void* ws;              // O slices of gpk_var_cov_grad_ws_bytes
  float* dX;             // (O, B, N, D) out
  double* dLinv;         // (O, M, M) out, lower, upper zero
  float* dZ;             // (O, M, D) out
  float* dpar;           // (O, M + 1 + D) out: dvstd, ds2, dlengthscale
};

// 0 for a shape the kernels do not take.
size_t gpk_var_cov_grad_ws_bytes(int B, int N, int M, int D);
int gpk_launch_var_cov_grad(const GpkVarCovGradArgs& a, hipStream_t stream);

// The part of the pipeline that runs from a dA the caller has materialised in the workspace
// (row-major (B, M, as) floats at *off_dA bytes into it): q, dlinv, reduce, finish -- no t, no
// kxx, for an objective that has no K_XX term (the Cholesky q(u) adjoint, gpk_var_chol.hip).
// Same kernels, same workspace plan (the query returns the plan's size, 0 for a refused shape);
// state and gcov are not read, the dw and kxx partials are zero-filled so that dpar[0..M) comes
// out 0 and ds2 / dlengthscale carry the K_ZX part alone; vstd only needs to be readable.
// O >= 1 outputs on grid y, as gpk_launch_var_cov_grad. The caller's workspace slices and dpar
// rows may be longer than the plan's: output o's slice starts ws_stride bytes (a multiple of
// 16, >= the plan's size) after output o - 1's, its dpar row dpar_stride floats (>= M + 1 + D)
// after; the pipeline writes the head of each.
size_t gpk_var_cov_grad_tail_plan(int B, int N, int M, int D, size_t* off_dA, int* as);

// What the pipeline's plan and the plans stacked on it (gpk_var_chol.hip, gpk_var_chol_cov.hip)
// share: the split of an fp64 lower-block Gram over the windows (vd_lower_gram, gpk_var_dense.h)
// -- WS windows per split (one window each up to B = 32, at most 32 splits), nsplit splits,
// npairs 64 x 64 blocks in the lower triangle of an M x M matrix -- and the rounding of a byte
// offset up to 16. Each plan keeps its own offsets.
struct GpkVarGramSplit {
  int WS, nsplit, npairs;
};
inline GpkVarGramSplit gpk_var_gram_split(int B, int M) {
  GpkVarGramSplit s;
  s.WS = B > 32 ? (B + 31) / 32 : 1;
  s.nsplit = B > 0 ? (B + s.WS - 1) / s.WS : 0;
  const int nb = (M + 63) / 64;
  s.npairs = nb * (nb + 1) / 2;
  return s;
}
inline size_t gpk_up16(size_t v) { return (v + 15) & ~(size_t)15; }
int gpk_launch_var_cov_grad_from_dA(const GpkVarCovGradArgs& a, size_t ws_stride, int dpar_stride,
                                    hipStream_t stream);

// The same from a caller-supplied dA for an objective that does have a K_XX term (the dense
// covariance of a Cholesky q(u), gpk_var_chol_cov.hip): q, dlinv, kxx, reduce, finish -- the
// sequence of gpk_launch_var_cov_grad without t. kxx reads gcov and the windows' own means of
// x / l: a.state is the caller's saved state, state_stride the floats between two outputs' states
// and mu_offset the floats from an output's state to its means (B, 64) -- passed, not derived,
// because a state that holds more than one panel puts them elsewhere (mu_offset >= B * M * as).
// Only dw is zero-filled (dpar[0..M) comes out 0); ds2 / dlengthscale carry both parts.
int gpk_launch_var_cov_grad_from_dA_kxx(const GpkVarCovGradArgs& a, size_t ws_stride, int dpar_stride,
                                        long long state_stride, long long mu_offset, hipStream_t stream);
