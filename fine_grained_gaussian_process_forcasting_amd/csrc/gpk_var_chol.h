// Launch descriptors of the Cholesky (full-covariance) q(u) path of the variational GP
// (gpk_variational_chol_f32 / gpk_variational_chol_adjoint_f32 / gpk_cholesky_kl_f32,
// gpk_var_chol.hip), shared by the kernels' unit and the C-ABI shim.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct GpkVarCholArgs {
  const float* X;        // (B, N, D)
  const float* Z;        // (M, D)
  const double* Linv;    // (M, M)
  const float* vmean;    // (M,)
  const float* vchol;    // (M, M), the lower triangle is read
  const float* hyp;      // (4 + 2 D), as gpk_variational_f32
  int B, N, M, D;
  float* mean;           // (B, N) out
  float* var;            // (B, N) out
  int* flags;            // (1,) or NULL
  float* saved;          // gpk_var_chol_saved_bytes, or NULL (inference)
};

struct GpkVarCholAdjArgs {
  const float* X;
  const float* Z;
  const double* Linv;
  const float* vmean;
  const float* vchol;
  const float* hyp;
  const float* gmean;    // (B, N)
  const float* gvar;     // (B, N)
  const float* saved;    // the forward's state
  int B, N, M, D;
  void* ws;              // gpk_var_chol_adjoint_ws_bytes
  float* dX;             // (B, N, D) out
  double* dLinv;         // (M, M) out, lower, upper zero
  float* dZ;             // (M, D) out
  float* dpar;           // (M + 2 D + 2) out: dvmean, ds2, dlengthscale, dweights, dbias
  float* dchol;          // (M, M) out, lower, upper zero
};

// 0 for a shape the kernels do not take.
size_t gpk_var_chol_saved_bytes(int B, int N, int M, int D);
size_t gpk_var_chol_adjoint_ws_bytes(int B, int N, int M, int D);
int gpk_launch_var_chol(const GpkVarCholArgs& a, hipStream_t stream);
int gpk_launch_var_chol_adjoint(const GpkVarCholAdjArgs& a, hipStream_t stream);
int gpk_launch_chol_kl(const float* m, const float* chol, int M, float* kl, const float* gkl, float* dm,
                       float* dchol, hipStream_t stream);
