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
