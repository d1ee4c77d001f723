// Launch descriptors of the joint posterior covariance (gpk_exact_posterior_cov_f32), shared
// by the posterior kernels (phase 1: gpk_posterior.hip, gpk_exact_large.hip), the covariance
// kernel (phase 2: gpk_posterior_cov.hip) and the C-ABI shim.
//
// Workspace layout (floats): V = L^{-1} K*, row-major (B, N, vs) with the row stride
// vs = gpk_post_cov_vstride(Ns) (Ns rounded up to 64; columns >= Ns hold zeros or are left
// unwritten, rows >= N do not exist), then mu (B, 64): the training mean of x / l that centred
// phase 1's Gram (entries >= D are not read).
#pragma once
#include <type_traits>

#include "gpk_internal.h"

// Phase 1: the plain posterior kernels keep GpkPostArgs as their only argument; their STOREV
// instantiations take this extension of it.
struct GpkPostVArgs : GpkPostArgs {
  float* V;    // (B, N, vs) out
  float* mu;   // (B, 64) out
  int vs;
};

template <bool STOREV>
using GpkPostArgsOf = std::conditional_t<STOREV, GpkPostVArgs, GpkPostArgs>;

int gpk_post_cov_vstride(int Ns);
size_t gpk_post_cov_ws_floats(int B, int N, int Ns);
int gpk_launch_exact_posterior_storev(const GpkPostVArgs& a, hipStream_t stream);
int gpk_launch_exact_large_posterior_storev(const GpkPostVArgs& a, hipStream_t stream);

// Phase 2: cov = K(xs, xs) - V^T V, diagonal = var.
struct GpkPostCovArgs {
  const float* hyp;    // as GpkExactArgs
  int n_ls;
  const float* Xs;     // (B, Ns, D) test inputs
  const float* V;      // (B, N, vs) phase 1's V
  const float* mu;     // (B, 64) phase 1's training mean of x / l
  const float* var;    // (B, Ns) phase 1's variance: the diagonal of cov
  int B, N, Ns, D, vs;
  float* cov;          // (B, Ns, Ns) out
  long long hyp_stride = 0;  // as GpkExactArgs
};
int gpk_launch_exact_posterior_cov(const GpkPostCovArgs& a, hipStream_t stream);

// The same kernel's variational mode (gpk_variational_cov_f32): cov = K(x, x) + jitter I +
// A^T diag(vstd^2 - 1) A, phase 1 in gpk_variational_cov.hip. Workspace per output (floats):
// A = L^{-1} K_ZX row-major (B, M, as) with as = gpk_post_cov_vstride(N), then the window's
// own mean of x / l (B, 64); ws_stride floats between two outputs' slices.
struct GpkVarCovArgs {
  const float* hyp;     // as GpkVarArgs (s2, jitter and the lengthscales are read)
  const float* X;       // (B, N, D) inputs
  const float* A;       // the workspace
  const float* vstd;    // (M,)
  int B, M, N, D, as;
  float* cov;           // (B, N, N) out
  long long x_stride;   // elements between two outputs' inputs (0: shared)
  long long ws_stride;  // floats between two outputs' workspace slices
};
template <bool VAR>
using GpkCovArgsOf = std::conditional_t<VAR, GpkVarCovArgs, GpkPostCovArgs>;
size_t gpk_var_cov_ws_floats(int B, int N, int M);
// Whether the SYRK-shaped phase 2 of a dense covariance of q(f) (mean-field or Cholesky q(u),
// gpk_var_chol_cov.hip) takes the shape: one workgroup per 64 x 64 tile with tile row <= tile
// column and window fits grid x.
inline bool gpk_var_cov_tile_grid_ok(int B, int N, int M) {
  if (B < 0 || N < 1 || M < 1 || M > 256) return false;
  const long long T = ((long long)N + 63) / 64;
  return (long long)B * (T * (T + 1) / 2) <= 0x7fffffffLL;
}
int gpk_launch_variational_cov_phase1(const GpkVarCovArgs& a, float* ws, const float* Z, const double* Linv,
                                      int O, hipStream_t stream);
int gpk_launch_variational_cov_phase2(const GpkVarCovArgs& a, int O, hipStream_t stream);

// Batched Cholesky root of dense covariances fused with sampling (gpk_mvn_root.hip).
constexpr int kGpkMvnRootMaxN = 256;
int gpk_launch_mvn_root(const float* cov, const float* mean, const float* eps, int B, int n, int S,
                        float jitter, float* R, float* samples, int* info, hipStream_t stream);

// One-right-hand-side solve against such a root (gpk_tri_solve.hip): R w = d or R^T w = d.
int gpk_launch_tri_solve(const float* R, const float* d, int B, int n, int trans, float* w, hipStream_t stream);

// Adjoint of the root and of the draws (gpk_mvn_root_grad.hip). Workspace: one packed 16 x 16
// tile triangle per matrix, B * T (T + 1) / 2 * 256 floats with T = ceil(n / 16).
size_t gpk_mvn_root_grad_ws_floats(int B, int n);
int gpk_launch_mvn_root_grad(const float* R, const float* gR, const float* gsamples, const float* eps, int B,
                             int n, int S, float* ws, float* dcov, float* dmean, hipStream_t stream);
