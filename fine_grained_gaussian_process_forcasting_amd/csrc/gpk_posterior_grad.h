// Launch descriptor of the adjoint of the exact-GP posterior (gpk_exact_posterior_grad_f32,
// gpk_posterior_grad.hip), shared by the kernels' unit and the C-ABI shim.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct GpkPostGradArgs {
  const float* X;        // (B, N, D) training inputs
  const float* L;        // (B, N, N) training factor, lower
  const float* z;        // (B, N) L^{-1}(y - c)
  const float* hyp;      // as GpkExactArgs: [outputscale, noise, mean_constant, lengthscale[n_ls]]
  int n_ls;
  const float* Xs;       // (B, Ns, D) test inputs
  const float* state;    // the forward's workspace (gpk_posterior_cov.h): V (B, N, vs), then mu (B, 64)
  const float* gmean;    // (B, Ns) or nullptr
  const float* gvar;     // (B, Ns) or nullptr
  const float* gcov;     // (B, Ns, Ns) or nullptr, any matrix
  int B, N, Ns, D;
  void* ws;              // gpk_post_grad_ws_bytes(B, N, Ns, D) bytes
  float* dX;             // (B, N, D) out or nullptr
  float* dy;             // (B, N) out or nullptr
  float* dXs;            // (B, Ns, D) out or nullptr
  float* dhyp;           // (B, 3 + n_ls) out: per-window d/d{s2, noise, c, lengthscale...}
  long long hyp_stride = 0;  // floats between two windows' hyper vectors; 0 = one vector shared by all
};

// 0 for a shape the kernels do not take (1 <= N, Ns <= 256, 1 <= D <= 64).
size_t gpk_post_grad_ws_bytes(int B, int N, int Ns, int D);
int gpk_launch_exact_posterior_grad(const GpkPostGradArgs& a, hipStream_t stream);
