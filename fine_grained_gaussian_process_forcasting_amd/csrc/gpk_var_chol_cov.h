// Launch descriptors of the dense covariance of q(f) for a Cholesky q(u) and of its adjoint
// (gpk_variational_chol_cov_f32 / _grad_f32, gpk_var_chol_cov.hip), shared by the kernels' unit
// and the C-ABI shim.
//
// Forward workspace = the adjoint's saved state, per output (floats): the stacked panel
// S (B, 2 M, as) with as = N rounded up to 64 -- for window b the rows 0 .. M - 1 hold
// W = L_q^T A and the rows M .. 2 M - 1 hold A = L^{-1} K_ZX (columns >= N hold zeros) -- then
// the window's own mean of x / l (B, 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct GpkVarCholCovArgs {
  const float* X;        // (B, N, D), or (O, B, N, D) with x_stride = B N D
  const float* Z;        // (O, M, D)
  const double* Linv;    // (O, M, M)
  const float* vchol;    // (O, M, M): L_q = tril(C), the strict upper triangle is never read
  const float* hyp;      // (O, 4 + 2 D), as GpkVarCovArgs
  int B, N, M, D, O;
  long long x_stride;    // elements between two outputs' inputs (0: shared)
  float* state;          // O slices of gpk_var_chol_cov_state_bytes, out
  float* cov;            // (O, B, N, N) out
};

struct GpkVarCholCovGradArgs {
  const float* X;
  const float* Z;
  const double* Linv;
  const float* vchol;
  const float* hyp;
  const float* state;    // the forward's workspace
  const float* gcov;     // (O, B, N, N) dObjective / dcov, any matrix
  int B, N, M, D, O;
  long long x_stride;
  void* ws;              // O slices of gpk_var_chol_cov_grad_ws_bytes
  float* dX;             // (O, B, N, D) out
  double* dLinv;         // (O, M, M) out, lower, upper zero
  float* dZ;             // (O, M, D) out
  float* dpar;           // (O, 1 + D) out: ds2, dlengthscale
  float* dchol;          // (O, M, M) out, lower, upper zero
};

// 0 for a shape the kernels do not take.
size_t gpk_var_chol_cov_state_bytes(int B, int N, int M);
size_t gpk_var_chol_cov_grad_ws_bytes(int B, int N, int M, int D);
int gpk_launch_var_chol_cov(const GpkVarCholCovArgs& a, hipStream_t stream);
int gpk_launch_var_chol_cov_grad(const GpkVarCholCovGradArgs& a, hipStream_t stream);
