// Launch descriptors of the Cholesky (full-covariance) q(u) path of the variational GP
// (gpk_variational_chol_f32 / gpk_variational_chol_adjoint_f32 / gpk_cholesky_kl_f32,
// gpk_var_chol.hip), shared by the kernels' unit and the C-ABI shim.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// O outputs run with the output index on grid y: every array but X and flags carries a dense
// leading O (O = 1: the single-output call).
struct GpkVarCholArgs {
  const float* X;        // (B, N, D), or (O, B, N, D) with x_stride = B N D
  const float* Z;        // (O, M, D)
  const double* Linv;    // (O, M, M)
  const float* vmean;    // (O, M)
  const float* vchol;    // (O, M, M), the lower triangle is read
  const float* hyp;      // (O, 4 + 2 D), as gpk_variational_f32
  int B, N, M, D;
  float* mean;           // (O, B, N) out
  float* var;            // (O, B, N) out
  int* flags;            // (1,) or NULL, every output ORs into it
  float* saved;          // O slices of gpk_var_chol_saved_bytes, or NULL (inference)
  int O;
  long long x_stride;    // elements between two outputs' inputs (0: shared)
};

struct GpkVarCholAdjArgs {
  const float* X;
  const float* Z;
  const double* Linv;
  const float* vmean;
  const float* vchol;
  const float* hyp;
  const float* gmean;    // (O, B, N)
  const float* gvar;     // (O, B, N)
  const float* saved;    // the forward's state
  int B, N, M, D;
  void* ws;              // O slices of gpk_var_chol_adjoint_ws_bytes
  float* dX;             // (O, B, N, D) out
  double* dLinv;         // (O, M, M) out, lower, upper zero
  float* dZ;             // (O, M, D) out
  float* dpar;           // (O, M + 2 D + 2) out: dvmean, ds2, dlengthscale, dweights, dbias
  float* dchol;          // (O, M, M) out, lower, upper zero
  int O;
  long long x_stride;
};

// 0 for a shape the kernels do not take.
size_t gpk_var_chol_saved_bytes(int B, int N, int M, int D);
size_t gpk_var_chol_adjoint_ws_bytes(int B, int N, int M, int D);
int gpk_launch_var_chol(const GpkVarCholArgs& a, hipStream_t stream);
int gpk_launch_var_chol_adjoint(const GpkVarCholAdjArgs& a, hipStream_t stream);
// m (O, M), chol (O, M, M), kl / gkl (O,), dm (O, M), dchol (O, M, M).
int gpk_launch_chol_kl(const float* m, const float* chol, int O, int M, float* kl, const float* gkl,
                       float* dm, float* dchol, hipStream_t stream);
