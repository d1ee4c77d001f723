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
};
int gpk_launch_exact_posterior_cov(const GpkPostCovArgs& a, hipStream_t stream);
