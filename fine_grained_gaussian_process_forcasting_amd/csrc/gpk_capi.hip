// C-ABI shim: argument validation + dispatch to the gfx950 kernels.
// Declarations and the reference interfaces each entry point replaces: include/gpk.h.
#include "../../include/gpk.h"
#include "gpk_internal.h"
#include "gpk_elbo.h"
#include "gpk_kzz.h"
#include "gpk_posterior_cov.h"
#include "gpk_posterior_grad.h"
#include "gpk_variational_cov_grad.h"
#include "gpk_var_chol.h"
#include "gpk_var_chol_cov.h"

size_t gpk_mvn_root_refine_ws_floats(int B, int n);
int gpk_launch_mvn_root_refine(const float* cov, const float* R, int B, int n, float jitter, float* ws,
                               float* Rout, hipStream_t stream);
size_t gpk_exact_append_ws_floats(int B, int N, int m);
int gpk_launch_exact_append(const float* X, const float* L, const float* z, const float* hyp, int n_ls,
                            long long hyp_stride, const float* Xn, const float* yn, int B, int N, int m, int D,
                            float jitter, float* ws, float* Lout, float* zout, int* info, hipStream_t stream);

extern "C" {

int gpk_version(void) { return 400; }

const char* gpk_strerror(int code) {
  if (code == 0) return "success";
  if (code < 0) {
    switch (code) {
      case -6: return "gpk: N exceeds the supported maximum (gpk_exact_max_n; gpk_mvn_root_grad_f32: n outside "
                      "1 .. gpk_mvn_root_max_n)";
      case -7: return "gpk: D too large for the LDS staging layout (gpk_mvn_root_grad_f32: S < 0)";
      case -8: return "gpk: invalid argument 8 (gpk_mvn_root_grad_f32: workspace missing or not 16-byte aligned)";
      case -9: return "gpk: invalid argument 9 (gpk_mvn_root_grad_f32: dcov is NULL)";
      default: return "gpk: invalid argument (negative code = argument index)";
    }
  }
  return hipGetErrorString((hipError_t)code);
}

int gpk_exact_max_n(void) { return kGpkExactMaxN; }

// hyp_stride of the *_perwin_f32 entry points: 0 (one hyper vector for every window) or at least
// the vector's length.
static bool hyp_stride_ok(long long hyp_stride, int n_lengthscale) {
  return hyp_stride == 0 || hyp_stride >= 3 + (long long)n_lengthscale;
}

int gpk_exact_mll_perwin_f32(const float* X, const float* y, const float* hyp, int n_lengthscale,
                             long long hyp_stride, int B, int N, int D, double jitter, int max_tries,
                             float* L, float* z, float* mll, int* info, void* stream) {
  if (X == nullptr) return -1;
  if (y == nullptr) return -2;
  if (hyp == nullptr) return -3;
  if (n_lengthscale != 1 && n_lengthscale != D) return -4;
  if (!hyp_stride_ok(hyp_stride, n_lengthscale)) return -5;
  if (B < 0) return -5;
  if (N < 1) return -6;
  if (D < 1) return -7;
  if (!(jitter >= 0.0)) return -8;
  if (max_tries < 0 || max_tries > 12) return -9;
  if (mll == nullptr) return -12;
  if (info == nullptr) return -13;
  if (N > gpk_exact_max_n()) return -6;
  if (N > kGpkExactRegMaxN && L == nullptr) return -10;   // the blocked path factors in L
  if (N > kGpkExactRegMaxN && D > 64) return -7;
  if (B == 0) return 0;
  GpkExactArgs a{X, y, hyp, n_lengthscale, B, N, D, jitter, max_tries, L, z, mll, info, hyp_stride};
  if (N > kGpkExactRegMaxN) return gpk_launch_exact_large(a, (hipStream_t)stream);
  return gpk_launch_exact(a, (hipStream_t)stream);
}

int gpk_exact_mll_f32(const float* X, const float* y, const float* hyp, int n_lengthscale,
                      int B, int N, int D, double jitter, int max_tries, float* L, float* z,
                      float* mll, int* info, void* stream) {
  return gpk_exact_mll_perwin_f32(X, y, hyp, n_lengthscale, 0, B, N, D, jitter, max_tries, L, z, mll, info,
                                  stream);
}

size_t gpk_exact_grad_workspace_bytes(int B, int N) {
  if (B < 0 || N < 1 || N > gpk_exact_max_n()) return 0;
  if (N > kGpkExactRegMaxN) return gpk_exact_large_grad_ws_floats(B, N) * sizeof(float);
  return gpk_exact_grad_ws_floats(B, N) * sizeof(float);
}

int gpk_exact_mll_grad_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                  int n_lengthscale, long long hyp_stride, int B, int N, int D,
                                  const float* gout, void* workspace, float* dX, float* dy, float* dhyp,
                                  void* stream) {
  if (X == nullptr) return -1;
  if (L == nullptr) return -2;
  if (z == nullptr) return -3;
  if (hyp == nullptr) return -4;
  if (n_lengthscale != 1 && n_lengthscale != D) return -5;
  if (!hyp_stride_ok(hyp_stride, n_lengthscale)) return -6;
  if (B < 0) return -6;
  if (N < 1 || N > gpk_exact_max_n()) return -7;
  if (D < 1 || D > 64) return -8;
  if (gout == nullptr) return -9;
  if (workspace == nullptr && B > 0 && gpk_exact_grad_workspace_bytes(B, N) > 0) return -10;
  if (dhyp == nullptr) return -13;
  if (B == 0) return 0;
  GpkExactGradArgs a{X, L, z, hyp, n_lengthscale, B, N, D, gout, (float*)workspace, dX, dy, dhyp, hyp_stride};
  if (N > kGpkExactRegMaxN) return gpk_launch_exact_large_grad(a, (hipStream_t)stream);
  return gpk_launch_exact_grad(a, (hipStream_t)stream);
}

int gpk_exact_mll_grad_f32(const float* X, const float* L, const float* z, const float* hyp,
                           int n_lengthscale, int B, int N, int D, const float* gout, void* workspace,
                           float* dX, float* dy, float* dhyp, void* stream) {
  return gpk_exact_mll_grad_perwin_f32(X, L, z, hyp, n_lengthscale, 0, B, N, D, gout, workspace, dX, dy, dhyp,
                                       stream);
}

int gpk_exact_posterior_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                   int n_lengthscale, long long hyp_stride, const float* Xs, int B, int N,
                                   int Ns, int D, float* mean, float* var, void* stream) {
  if (X == nullptr) return -1;
  if (L == nullptr) return -2;
  if (z == nullptr) return -3;
  if (hyp == nullptr) return -4;
  if (n_lengthscale != 1 && n_lengthscale != D) return -5;
  if (!hyp_stride_ok(hyp_stride, n_lengthscale)) return -6;
  if (Xs == nullptr) return -6;
  if (B < 0) return -7;
  if (N < 1 || N > gpk_exact_max_n()) return -8;
  if (Ns < 0) return -9;
  if (D < 1 || D > 64) return -10;
  if (mean == nullptr) return -11;
  if (var == nullptr) return -12;
  if (B == 0 || Ns == 0) return 0;
  GpkPostArgs a{X, L, z, hyp, n_lengthscale, Xs, B, N, Ns, D, mean, var, hyp_stride};
  if (N > kGpkExactRegMaxN) return gpk_launch_exact_large_posterior(a, (hipStream_t)stream);
  return gpk_launch_exact_posterior(a, (hipStream_t)stream);
}

int gpk_exact_posterior_f32(const float* X, const float* L, const float* z, const float* hyp,
                            int n_lengthscale, const float* Xs, int B, int N, int Ns, int D,
                            float* mean, float* var, void* stream) {
  return gpk_exact_posterior_perwin_f32(X, L, z, hyp, n_lengthscale, 0, Xs, B, N, Ns, D, mean, var, stream);
}

size_t gpk_exact_posterior_cov_workspace_bytes(int B, int N, int Ns) {
  if (B < 0 || N < 1 || N > gpk_exact_max_n() || Ns < 0) return 0;
  if (N > kGpkExactRegMaxN && B > 65535) return 0;
  return gpk_post_cov_ws_floats(B, N, Ns) * sizeof(float);
}

int gpk_exact_posterior_cov_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                       int n_lengthscale, long long hyp_stride, const float* Xs, int B, int N,
                                       int Ns, int D, void* workspace, float* mean, float* var, float* cov,
                                       void* stream) {
  if (X == nullptr) return -1;
  if (L == nullptr) return -2;
  if (z == nullptr) return -3;
  if (hyp == nullptr) return -4;
  if (n_lengthscale != 1 && n_lengthscale != D) return -5;
  if (!hyp_stride_ok(hyp_stride, n_lengthscale)) return -6;
  if (Xs == nullptr) return -6;
  if (B < 0) return -7;
  if (N < 1 || N > gpk_exact_max_n()) return -8;
  if (Ns < 0) return -9;
  if (D < 1 || D > 64) return -10;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -11;   // V rows are read 16 B at a time
  if (mean == nullptr) return -12;
  if (var == nullptr) return -13;
  if (cov == nullptr) return -14;
  if (B == 0 || Ns == 0) return 0;
  if (N > kGpkExactRegMaxN && B > 65535) return -7;   // the blocked kernel keeps B on gridDim.y
  const int vs = gpk_post_cov_vstride(Ns);
  float* V = (float*)workspace;
  float* mu = V + (size_t)B * N * vs;   // after V: the workspace layout of gpk_posterior_cov.h
  GpkPostVArgs a{};
  static_cast<GpkPostArgs&>(a) = GpkPostArgs{X, L, z, hyp, n_lengthscale, Xs, B, N, Ns, D, mean, var, hyp_stride};
  a.V = V;
  a.mu = mu;
  a.vs = vs;
  const int rc = N > kGpkExactRegMaxN ? gpk_launch_exact_large_posterior_storev(a, (hipStream_t)stream)
                                      : gpk_launch_exact_posterior_storev(a, (hipStream_t)stream);
  if (rc != 0) return rc;
  GpkPostCovArgs c{hyp, n_lengthscale, Xs, V, mu, var, B, N, Ns, D, vs, cov, hyp_stride};
  return gpk_launch_exact_posterior_cov(c, (hipStream_t)stream);
}

int gpk_exact_posterior_cov_f32(const float* X, const float* L, const float* z, const float* hyp,
                                int n_lengthscale, const float* Xs, int B, int N, int Ns, int D,
                                void* workspace, float* mean, float* var, float* cov, void* stream) {
  return gpk_exact_posterior_cov_perwin_f32(X, L, z, hyp, n_lengthscale, 0, Xs, B, N, Ns, D, workspace, mean, var,
                                            cov, stream);
}

// ---- appending observations to a cached factor (gpk_exact_append.hip)
size_t gpk_exact_append_workspace_bytes(int B, int N, int m) {
  if (B < 0 || N < 1 || m < 1 || m > kGpkMvnRootMaxN || N + m > gpk_exact_max_n()) return 0;
  if (N > kGpkExactRegMaxN && B > 65535) return 0;
  return gpk_exact_append_ws_floats(B, N, m) * sizeof(float);
}

int gpk_exact_append_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                int n_lengthscale, long long hyp_stride, const float* Xn, const float* yn,
                                int B, int N, int m, int D, float jitter, void* workspace, float* Lout,
                                float* zout, int* info, void* stream) {
  if (X == nullptr) return -1;
  if (L == nullptr) return -2;
  if (z == nullptr) return -3;
  if (hyp == nullptr) return -4;
  if (n_lengthscale != 1 && n_lengthscale != D) return -5;
  if (!hyp_stride_ok(hyp_stride, n_lengthscale)) return -6;
  if (Xn == nullptr) return -6;
  if (yn == nullptr) return -7;
  if (B < 0) return -8;
  if (N < 1 || N > gpk_exact_max_n()) return -9;
  if (m < 1 || m > kGpkMvnRootMaxN || N + m > gpk_exact_max_n()) return -10;
  if (D < 1 || D > 64) return -11;
  if (!(jitter >= 0.f)) return -12;
  if (B > 0 && (workspace == nullptr || ((size_t)workspace & 15) != 0)) return -13;   // V rows are read 16 B at a time
  if (Lout == nullptr) return -14;
  if (zout == nullptr) return -15;
  if (info == nullptr) return -16;
  if (B == 0) return 0;
  if (N > kGpkExactRegMaxN && B > 65535) return -8;   // the blocked phase 1 keeps B on gridDim.y
  return gpk_launch_exact_append(X, L, z, hyp, n_lengthscale, hyp_stride, Xn, yn, B, N, m, D, jitter,
                                 (float*)workspace, Lout, zout, info, (hipStream_t)stream);
}

int gpk_exact_append_f32(const float* X, const float* L, const float* z, const float* hyp, int n_lengthscale,
                         const float* Xn, const float* yn, int B, int N, int m, int D, float jitter,
                         void* workspace, float* Lout, float* zout, int* info, void* stream) {
  return gpk_exact_append_perwin_f32(X, L, z, hyp, n_lengthscale, 0, Xn, yn, B, N, m, D, jitter, workspace, Lout,
                                     zout, info, stream);
}

// ---- adjoint of the exact posterior (gpk_posterior_grad.hip)
size_t gpk_exact_posterior_grad_workspace_bytes(int B, int N, int Ns, int D) {
  return gpk_post_grad_ws_bytes(B, N, Ns, D);
}

int gpk_exact_posterior_grad_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                        int n_lengthscale, long long hyp_stride, const float* Xs,
                                        const float* state, const float* gmean, const float* gvar,
                                        const float* gcov, int B, int N, int Ns, int D, void* workspace,
                                        float* dX, float* dy, float* dXs, float* dhyp, void* stream) {
  if (X == nullptr) return -1;
  if (L == nullptr) return -2;
  if (z == nullptr) return -3;
  if (hyp == nullptr) return -4;
  if (n_lengthscale != 1 && n_lengthscale != D) return -5;
  if (!hyp_stride_ok(hyp_stride, n_lengthscale)) return -6;
  if (Xs == nullptr) return -6;
  if (state == nullptr || ((size_t)state & 15) != 0) return -7;   // V rows are read 16 B at a time
  if (gmean == nullptr && gvar == nullptr && gcov == nullptr) return -8;
  if (B < 0) return -11;
  if (N < 1 || N > kGpkExactRegMaxN) return -12;
  if (Ns < 1 || Ns > kGpkMvnRootMaxN) return -13;
  if (D < 1 || D > 64) return -14;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -15;
  if (dhyp == nullptr) return -19;
  if (B > 0 && gpk_post_grad_ws_bytes(B, N, Ns, D) == 0) return -11;
  if (B == 0) return 0;
  GpkPostGradArgs a{X, L, z, hyp, n_lengthscale, Xs, state, gmean, gvar, gcov, B, N, Ns, D, workspace,
                    dX, dy, dXs, dhyp, hyp_stride};
  return gpk_launch_exact_posterior_grad(a, (hipStream_t)stream);
}

int gpk_exact_posterior_grad_f32(const float* X, const float* L, const float* z, const float* hyp,
                                 int n_lengthscale, const float* Xs, const float* state,
                                 const float* gmean, const float* gvar, const float* gcov,
                                 int B, int N, int Ns, int D, void* workspace,
                                 float* dX, float* dy, float* dXs, float* dhyp, void* stream) {
  return gpk_exact_posterior_grad_perwin_f32(X, L, z, hyp, n_lengthscale, 0, Xs, state, gmean, gvar, gcov, B, N,
                                             Ns, D, workspace, dX, dy, dXs, dhyp, stream);
}

int gpk_kzz_chol_f64(const float* Z, const float* hyp, int M, int D, float jitter,
                     double chol_jitter, int max_tries, double* L, double* Linv, int* info,
                     void* stream) {
  if (Z == nullptr) return -1;
  if (hyp == nullptr) return -2;
  if (M < 1 || M > 256) return -3;
  if (D < 1 || D > 64) return -4;
  if (max_tries < 0 || max_tries > 12) return -7;
  if (L == nullptr) return -8;
  if (Linv == nullptr) return -9;
  if (info == nullptr) return -10;
  GpkKzzArgs a{Z, hyp, M, D, jitter, chol_jitter, max_tries, L, Linv, info};
  return gpk_launch_kzz16(a, (hipStream_t)stream);
}

size_t gpk_kzz_backward_workspace_bytes(int M, int D) {
  if (M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_kzz_grad_ws_bytes(M, D);
}

int gpk_kzz_backward_f64(const double* dLinv, const double* L, const double* Linv, const float* Z,
                         const float* hyp, int M, int D, void* workspace, float* dZ, float* dhyp,
                         void* stream) {
  if (dLinv == nullptr) return -1;
  if (L == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (Z == nullptr) return -4;
  if (hyp == nullptr) return -5;
  if (M < 1 || M > 256) return -6;
  if (D < 1 || D > 64) return -7;
  if (workspace == nullptr) return -8;
  if (dZ == nullptr) return -9;
  if (dhyp == nullptr) return -10;
  GpkKzzGradArgs a{dLinv, L, Linv, Z, hyp, M, D, workspace, dZ, dhyp};
  return gpk_launch_kzz_grad(a, (hipStream_t)stream);
}

int gpk_gauss_ell_f32(const float* y, const float* mean, const float* var, const float* noise, int R,
                      int N, float* ell, void* stream) {
  if (y == nullptr) return -1;
  if (mean == nullptr) return -2;
  if (var == nullptr) return -3;
  if (noise == nullptr) return -4;
  if (R < 0) return -5;
  if (N < 1) return -6;
  if (ell == nullptr) return -7;
  if (R == 0) return 0;
  return gpk_launch_ell(y, mean, var, noise, R, N, ell, (hipStream_t)stream);
}

int gpk_gauss_ell_grad_f32(const float* y, const float* mean, const float* var, const float* noise,
                           const float* gell, int R, int N, float* dy, float* dmean, float* dvar,
                           float* dnoise_part, void* stream) {
  if (y == nullptr) return -1;
  if (mean == nullptr) return -2;
  if (var == nullptr) return -3;
  if (noise == nullptr) return -4;
  if (gell == nullptr) return -5;
  if (R < 0) return -6;
  if (N < 1) return -7;
  if (R == 0) return 0;
  return gpk_launch_ell_grad(y, mean, var, noise, gell, R, N, dy, dmean, dvar, dnoise_part,
                             (hipStream_t)stream);
}

int gpk_meanfield_kl_f32(const float* m, const float* s, int M, float* kl, const float* gkl,
                         float* dm, float* ds, void* stream) {
  if (m == nullptr) return -1;
  if (s == nullptr) return -2;
  if (M < 1) return -3;
  if (gkl == nullptr && kl == nullptr) return -4;
  if (gkl != nullptr && (dm == nullptr || ds == nullptr)) return -6;
  return gpk_launch_kl(m, s, M, kl, gkl, dm, ds, (hipStream_t)stream);
}

int gpk_variational_elbo_f32(const float* y, long long ldy, const float* mean, long long ldm,
                             const float* var, long long ldv, const float* noise, const float* m,
                             const float* s, int M, int R, int N, float kl_scale, float min_var,
                             float* elbo, int* clamp_flag, void* stream) {
  if (y == nullptr) return -1;
  if (ldy < N) return -2;
  if (mean == nullptr) return -3;
  if (ldm < N) return -4;
  if (var == nullptr) return -5;
  if (ldv < N) return -6;
  if (noise == nullptr) return -7;
  if (m == nullptr) return -8;
  if (s == nullptr) return -9;
  if (M < 1) return -10;
  if (R < 0) return -11;
  if (N < 1) return -12;
  if (elbo == nullptr) return -15;
  if (R == 0) return 0;
  return gpk_launch_elbo(y, ldy, mean, ldm, var, ldv, noise, m, s, M, R, N, kl_scale, min_var, elbo,
                         clamp_flag, (hipStream_t)stream);
}

int gpk_variational_elbo_grad_f32(const float* y, long long ldy, const float* mean, long long ldm,
                                  const float* var, long long ldv, const float* noise, const float* m,
                                  const float* s, int M, int R, int N, float kl_scale, const float* gelbo,
                                  float* dmean, float* dvar, float* dnoise_part, float* dm, float* ds,
                                  void* stream) {
  if (y == nullptr) return -1;
  if (ldy < N) return -2;
  if (mean == nullptr) return -3;
  if (ldm < N) return -4;
  if (var == nullptr) return -5;
  if (ldv < N) return -6;
  if (noise == nullptr) return -7;
  if (m == nullptr) return -8;
  if (s == nullptr) return -9;
  if (M < 1) return -10;
  if (R < 0) return -11;
  if (N < 1) return -12;
  if (R > 0 && gelbo == nullptr) return -14;
  if (dm == nullptr || ds == nullptr || (R > 0 && (dmean == nullptr || dvar == nullptr || dnoise_part == nullptr)))
    return -15;
  if (R == 0) {
    // an empty batch (the forward's no-op): no rows, and the KL enters scaled by sum g = 0
    hipError_t e = hipMemsetAsync(dm, 0, sizeof(float) * (size_t)M, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(ds, 0, sizeof(float) * (size_t)M, (hipStream_t)stream);
    return e == hipSuccess ? 0 : (int)e;
  }
  return gpk_launch_elbo_grad(y, ldy, mean, ldm, var, ldv, noise, m, s, M, R, N, kl_scale, gelbo, dmean,
                              dvar, dnoise_part, dm, ds, (hipStream_t)stream);
}

int gpk_record_check(const int* info, int n, const float* in0, long long n0, const float* in1,
                     long long n1, int kind, int* ring, long long* counter, int slots, int item,
                     int items, int* sticky, void* stream) {
  if (kind < 0 || kind > 2) return -7;
  if (kind != 2 && info == nullptr) return -1;
  if (kind == 0 && (n < 1 || (n0 > 0 && in0 == nullptr) || (n1 > 0 && in1 == nullptr))) return -2;
  if (ring == nullptr && kind != 2) return -8;
  if (counter == nullptr) return -9;
  if (slots < 1) return -10;
  if (kind != 2 && (item < 0 || item >= items)) return -11;
  if (kind == 0 && sticky == nullptr) return -13;
  return gpk_launch_verdict(info, n, in0, n0, in1, n1, kind, ring, counter, slots, item, items, sticky,
                            kind == 2, (hipStream_t)stream);
}

int gpk_variational_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                        const float* vstd, const float* hyp, const float* y, int B, int N, int M,
                        int D, float* mean, float* var, float* ell, int* flags, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vmean == nullptr) return -4;
  if (vstd == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (B < 0) return -8;
  if (N < 1) return -9;
  if (M < 1 || M > 256) return -10;
  if (D < 1 || D > 64) return -11;
  if (mean == nullptr) return -12;
  if (var == nullptr) return -13;
  if (ell != nullptr && y == nullptr) return -7;
  if (B == 0) return 0;
  GpkVarArgs a{X, Z, Linv, vmean, vstd, hyp, y, B, N, M, D, mean, var, ell};
  return gpk_launch_var(a, flags, (hipStream_t)stream);
}

size_t gpk_variational_saved_bytes(int B, int N, int M, int D) {
  if (B < 1 || N < 1 || M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_var_saved_bytes(B, N, M, D);
}
int gpk_variational_train_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                              const float* vstd, const float* hyp, const float* y, int B, int N, int M,
                              int D, float* mean, float* var, float* ell, int* flags, void* saved,
                              void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vmean == nullptr) return -4;
  if (vstd == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (B < 0) return -8;
  if (N < 1) return -9;
  if (M < 1 || M > 256) return -10;
  if (D < 1 || D > 64) return -11;
  if (mean == nullptr) return -12;
  if (var == nullptr) return -13;
  if (ell != nullptr && y == nullptr) return -7;
  if (saved == nullptr && gpk_var_saved_bytes(B, N, M, D) > 0) return -16;
  if (B == 0) return 0;
  GpkVarArgs a{X, Z, Linv, vmean, vstd, hyp, y, B, N, M, D, mean, var, ell, (float*)saved};
  return gpk_launch_var(a, flags, (hipStream_t)stream);
}
size_t gpk_variational_adjoint_saved_workspace_bytes(int B, int N, int M, int D) {
  if (B < 1 || N < 1 || M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_var_adjoint_saved_ws_bytes(B, N, M, D);
}
int gpk_variational_adjoint_saved_f32(const float* X, const float* Z, const double* Linv,
                                      const float* vmean, const float* vstd, const float* hyp,
                                      const float* gmean, const float* gvar, const void* saved, int B,
                                      int N, int M, int D, void* workspace, float* dX, double* dLinv,
                                      float* dZ, float* dpar, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vmean == nullptr) return -4;
  if (vstd == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (gmean == nullptr) return -7;
  if (gvar == nullptr) return -8;
  if (saved == nullptr) return -9;
  if (B < 1) return -10;
  if (N < 1) return -11;
  if (M < 1 || M > 256) return -12;
  if (D < 1 || D > 64) return -13;
  if (gpk_var_saved_bytes(B, N, M, D) == 0) return -12;
  if (workspace == nullptr) return -14;
  if (dX == nullptr) return -15;
  if (dLinv == nullptr) return -16;
  if (dZ == nullptr) return -17;
  if (dpar == nullptr) return -18;
  GpkVarAdjArgs a{X, Z, Linv, vmean, vstd, hyp, gmean, gvar, B, N, M, D, workspace, dX, dLinv, dZ, dpar,
                  (const float*)saved};
  return gpk_launch_var_adjoint(a, (hipStream_t)stream);
}
size_t gpk_variational_adjoint_workspace_bytes(int B, int N, int M, int D) {
  if (B < 1 || N < 1 || M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_var_adjoint_ws_bytes(B, N, M, D);
}

int gpk_variational_adjoint_f32(const float* X, const float* Z, const double* Linv,
                                const float* vmean, const float* vstd, const float* hyp,
                                const float* gmean, const float* gvar, int B, int N, int M, int D,
                                void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vmean == nullptr) return -4;
  if (vstd == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (gmean == nullptr) return -7;
  if (gvar == nullptr) return -8;
  if (B < 1) return -9;
  if (N < 1) return -10;
  if (M < 1 || M > 256) return -11;
  if (D < 1 || D > 64) return -12;
  if (workspace == nullptr) return -13;
  if (dX == nullptr) return -14;
  if (dLinv == nullptr) return -15;
  if (dZ == nullptr) return -16;
  if (dpar == nullptr) return -17;
  GpkVarAdjArgs a{X, Z, Linv, vmean, vstd, hyp, gmean, gvar, B, N, M, D, workspace, dX, dLinv, dZ, dpar};
  return gpk_launch_var_adjoint(a, (hipStream_t)stream);
}

// ---- multi-output (batched) variational chain: output o on grid dimension y of every launch
constexpr int kGpkMaxOutputs = 65535;   // gridDim.y

int gpk_kzz_chol_f64_batched(const float* Z, const float* hyp, int O, int M, int D, float jitter,
                             double chol_jitter, int max_tries, double* L, double* Linv, int* info,
                             void* stream) {
  if (Z == nullptr) return -1;
  if (hyp == nullptr) return -2;
  if (O < 1 || O > kGpkMaxOutputs) return -3;
  if (M < 1 || M > 256) return -4;
  if (D < 1 || D > 64) return -5;
  if (max_tries < 0 || max_tries > 12) return -8;
  if (L == nullptr) return -9;
  if (Linv == nullptr) return -10;
  if (info == nullptr) return -11;
  GpkKzzArgs a{Z, hyp, M, D, jitter, chol_jitter, max_tries, L, Linv, info, O};
  return gpk_launch_kzz16(a, (hipStream_t)stream);
}

size_t gpk_kzz_backward_batched_workspace_bytes(int O, int M, int D) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * gpk_kzz_backward_workspace_bytes(M, D);
}

int gpk_kzz_backward_f64_batched(const double* dLinv, const double* L, const double* Linv,
                                 const float* Z, const float* hyp, int O, int M, int D, void* workspace,
                                 float* dZ, float* dhyp, void* stream) {
  if (dLinv == nullptr) return -1;
  if (L == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (Z == nullptr) return -4;
  if (hyp == nullptr) return -5;
  if (O < 1 || O > kGpkMaxOutputs) return -6;
  if (M < 1 || M > 256) return -7;
  if (D < 1 || D > 64) return -8;
  if (workspace == nullptr) return -9;
  if (dZ == nullptr) return -10;
  if (dhyp == nullptr) return -11;
  GpkKzzGradArgs a{dLinv, L, Linv, Z, hyp, M, D, workspace, dZ, dhyp, O};
  return gpk_launch_kzz_grad(a, (hipStream_t)stream);
}

int gpk_variational_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                const float* vmean, const float* vstd, const float* hyp, int O, int B,
                                int N, int M, int D, float* mean, float* var, int* flags, void* saved,
                                void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vmean == nullptr) return -5;
  if (vstd == nullptr) return -6;
  if (hyp == nullptr) return -7;
  if (O < 1 || O > kGpkMaxOutputs) return -8;
  if (B < 0) return -9;
  if (N < 1) return -10;
  if (M < 1 || M > 256) return -11;
  if (D < 1 || D > 64) return -12;
  if (mean == nullptr) return -13;
  if (var == nullptr) return -14;
  if (saved != nullptr && (B < 1 || gpk_var_saved_bytes(B, N, M, D) == 0)) return -16;
  if (B == 0) return 0;
  GpkVarArgs a{X, Z, Linv, vmean, vstd, hyp, nullptr, B, N, M, D, mean, var, nullptr, (float*)saved, O,
               shared_x ? 0LL : (long long)B * N * D};
  return gpk_launch_var(a, flags, (hipStream_t)stream);
}

size_t gpk_variational_adjoint_batched_workspace_bytes(int O, int B, int N, int M, int D, int has_saved) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * (has_saved ? gpk_variational_adjoint_saved_workspace_bytes(B, N, M, D)
                                : gpk_variational_adjoint_workspace_bytes(B, N, M, D));
}

int gpk_variational_adjoint_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                        const float* vmean, const float* vstd, const float* hyp,
                                        const float* gmean, const float* gvar, const void* saved, int O,
                                        int B, int N, int M, int D, void* workspace, float* dX,
                                        double* dLinv, float* dZ, float* dpar, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vmean == nullptr) return -5;
  if (vstd == nullptr) return -6;
  if (hyp == nullptr) return -7;
  if (gmean == nullptr) return -8;
  if (gvar == nullptr) return -9;
  if (O < 1 || O > kGpkMaxOutputs) return -11;
  if (B < 1) return -12;
  if (N < 1) return -13;
  if (M < 1 || M > 256) return -14;
  if (D < 1 || D > 64) return -15;
  if (saved != nullptr && gpk_var_saved_bytes(B, N, M, D) == 0) return -10;
  if (workspace == nullptr) return -16;
  if (dX == nullptr) return -17;
  if (dLinv == nullptr) return -18;
  if (dZ == nullptr) return -19;
  if (dpar == nullptr) return -20;
  GpkVarAdjArgs a{X, Z, Linv, vmean, vstd, hyp, gmean, gvar, B, N, M, D, workspace, dX, dLinv, dZ, dpar,
                  (const float*)saved, O, shared_x ? 0LL : (long long)B * N * D};
  return gpk_launch_var_adjoint(a, (hipStream_t)stream);
}

// ---- dense covariance of q(f): phase 1 (A = Linv K_ZX, gpk_variational_cov.hip), then the
//      variational mode of the covariance kernel (gpk_posterior_cov.hip)
size_t gpk_variational_cov_workspace_bytes(int B, int N, int M) {
  if (!gpk_var_cov_tile_grid_ok(B, N, M)) return 0;
  return gpk_var_cov_ws_floats(B, N, M) * sizeof(float);
}

size_t gpk_variational_cov_batched_workspace_bytes(int O, int B, int N, int M) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * gpk_variational_cov_workspace_bytes(B, N, M);
}

static int var_cov_run(const float* X, long long x_stride, const float* Z, const double* Linv,
                       const float* vstd, const float* hyp, int O, int B, int N, int M, int D,
                       void* workspace, float* cov, hipStream_t stream) {
  GpkVarCovArgs a{hyp, X, (const float*)workspace, vstd, B, M, N, D, gpk_post_cov_vstride(N), cov, x_stride,
                  (long long)gpk_var_cov_ws_floats(B, N, M)};
  const int rc = gpk_launch_variational_cov_phase1(a, (float*)workspace, Z, Linv, O, stream);
  if (rc != 0) return rc;
  return gpk_launch_variational_cov_phase2(a, O, stream);
}

int gpk_variational_cov_f32(const float* X, const float* Z, const double* Linv, const float* vstd,
                            const float* hyp, int B, int N, int M, int D, void* workspace,
                            float* cov, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vstd == nullptr) return -4;
  if (hyp == nullptr) return -5;
  if (B < 0) return -6;
  if (N < 1) return -7;
  if (M < 1 || M > 256) return -8;
  if (D < 1 || D > 64) return -9;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -10;   // A rows are read 16 B at a time
  if (cov == nullptr) return -11;
  if (!gpk_var_cov_tile_grid_ok(B, N, M)) return -7;
  if (B == 0) return 0;
  return var_cov_run(X, 0, Z, Linv, vstd, hyp, 1, B, N, M, D, workspace, cov, (hipStream_t)stream);
}

int gpk_variational_cov_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                    const float* vstd, const float* hyp, int O, int B, int N, int M,
                                    int D, void* workspace, float* cov, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vstd == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (O < 1 || O > kGpkMaxOutputs) return -7;
  if (B < 0) return -8;
  if (N < 1) return -9;
  if (M < 1 || M > 256) return -10;
  if (D < 1 || D > 64) return -11;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -12;
  if (cov == nullptr) return -13;
  if (!gpk_var_cov_tile_grid_ok(B, N, M)) return -9;
  if (B == 0) return 0;
  return var_cov_run(X, shared_x ? 0LL : (long long)B * N * D, Z, Linv, vstd, hyp, O, B, N, M, D, workspace,
                     cov, (hipStream_t)stream);
}

// ---- adjoint of the dense covariance of q(f) (gpk_variational_cov_grad.hip)
size_t gpk_variational_cov_grad_workspace_bytes(int B, int N, int M, int D) {
  return gpk_var_cov_grad_ws_bytes(B, N, M, D);
}

size_t gpk_variational_cov_grad_batched_workspace_bytes(int O, int B, int N, int M, int D) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * gpk_var_cov_grad_ws_bytes(B, N, M, D);
}

int gpk_variational_cov_grad_f32(const float* X, const float* Z, const double* Linv, const float* vstd,
                                 const float* hyp, const void* state, const float* gcov, int B, int N,
                                 int M, int D, void* workspace, float* dX, double* dLinv, float* dZ,
                                 float* dpar, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vstd == nullptr) return -4;
  if (hyp == nullptr) return -5;
  if (state == nullptr || ((size_t)state & 15) != 0) return -6;
  if (gcov == nullptr) return -7;
  if (B < 0) return -8;
  if (N < 1 || N > kGpkMvnRootMaxN) return -9;
  if (M < 1 || M > 256) return -10;
  if (D < 1 || D > 64) return -11;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -12;
  if (dX == nullptr) return -13;
  if (dLinv == nullptr) return -14;
  if (dZ == nullptr) return -15;
  if (dpar == nullptr) return -16;
  if (B > 0 && gpk_var_cov_grad_ws_bytes(B, N, M, D) == 0) return -8;
  if (B == 0) return 0;
  GpkVarCovGradArgs a{X, Z, Linv, vstd, hyp, (const float*)state, gcov, B, N, M, D, 1, 0LL, workspace,
                      dX, dLinv, dZ, dpar};
  return gpk_launch_var_cov_grad(a, (hipStream_t)stream);
}

int gpk_variational_cov_grad_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                         const float* vstd, const float* hyp, const void* state,
                                         const float* gcov, int O, int B, int N, int M, int D,
                                         void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                         void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vstd == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (state == nullptr || ((size_t)state & 15) != 0) return -7;
  if (gcov == nullptr) return -8;
  if (O < 1 || O > kGpkMaxOutputs) return -9;
  if (B < 0) return -10;
  if (N < 1 || N > kGpkMvnRootMaxN) return -11;
  if (M < 1 || M > 256) return -12;
  if (D < 1 || D > 64) return -13;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -14;
  if (dX == nullptr) return -15;
  if (dLinv == nullptr) return -16;
  if (dZ == nullptr) return -17;
  if (dpar == nullptr) return -18;
  if (B > 0 && gpk_var_cov_grad_ws_bytes(B, N, M, D) == 0) return -10;
  if (B == 0) return 0;
  GpkVarCovGradArgs a{X, Z, Linv, vstd, hyp, (const float*)state, gcov, B, N, M, D, O,
                      shared_x ? 0LL : (long long)B * N * D, workspace, dX, dLinv, dZ, dpar};
  return gpk_launch_var_cov_grad(a, (hipStream_t)stream);
}

size_t gpk_variational_chol_saved_bytes(int B, int N, int M, int D) {
  return gpk_var_chol_saved_bytes(B, N, M, D);
}

int gpk_variational_chol_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                             const float* vchol, const float* hyp, int B, int N, int M, int D, float* mean,
                             float* var, int* flags, void* saved, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vmean == nullptr) return -4;
  if (vchol == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (B < 0) return -7;
  if (N < 1) return -8;
  if (M < 1 || M > 256) return -9;
  if (D < 1 || D > 64) return -10;
  if (mean == nullptr) return -11;
  if (var == nullptr) return -12;
  if (saved != nullptr && ((size_t)saved & 15) != 0) return -14;
  if (B == 0) return 0;
  GpkVarCholArgs a{X, Z, Linv, vmean, vchol, hyp, B, N, M, D, mean, var, flags, (float*)saved, 1, 0LL};
  return gpk_launch_var_chol(a, (hipStream_t)stream);
}

size_t gpk_variational_chol_batched_saved_bytes(int O, int B, int N, int M, int D) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * gpk_var_chol_saved_bytes(B, N, M, D);
}

int gpk_variational_chol_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                     const float* vmean, const float* vchol, const float* hyp, int O, int B,
                                     int N, int M, int D, float* mean, float* var, int* flags, void* saved,
                                     void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vmean == nullptr) return -5;
  if (vchol == nullptr) return -6;
  if (hyp == nullptr) return -7;
  if (O < 1 || O > kGpkMaxOutputs) return -8;
  if (B < 0) return -9;
  if (N < 1) return -10;
  if (M < 1 || M > 256) return -11;
  if (D < 1 || D > 64) return -12;
  if (mean == nullptr) return -13;
  if (var == nullptr) return -14;
  if (saved != nullptr && (((size_t)saved & 15) != 0 || B < 1 || gpk_var_chol_saved_bytes(B, N, M, D) == 0))
    return -16;
  if (B == 0) return 0;
  GpkVarCholArgs a{X, Z, Linv, vmean, vchol, hyp, B, N, M, D, mean, var, flags, (float*)saved, O,
                   shared_x ? 0LL : (long long)B * N * D};
  return gpk_launch_var_chol(a, (hipStream_t)stream);
}

size_t gpk_variational_chol_adjoint_workspace_bytes(int B, int N, int M, int D) {
  return gpk_var_chol_adjoint_ws_bytes(B, N, M, D);
}

int gpk_variational_chol_adjoint_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                                     const float* vchol, const float* hyp, const float* gmean,
                                     const float* gvar, const void* saved, int B, int N, int M, int D,
                                     void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                     float* dchol, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vmean == nullptr) return -4;
  if (vchol == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (gmean == nullptr) return -7;
  if (gvar == nullptr) return -8;
  if (saved == nullptr || ((size_t)saved & 15) != 0) return -9;
  if (B < 0) return -10;
  if (N < 1 || N > 256) return -11;
  if (M < 1 || M > 256) return -12;
  if (D < 1 || D > 64) return -13;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -14;
  if (dX == nullptr) return -15;
  if (dLinv == nullptr) return -16;
  if (dZ == nullptr) return -17;
  if (dpar == nullptr) return -18;
  if (dchol == nullptr) return -19;
  if (B > 0 && gpk_var_chol_adjoint_ws_bytes(B, N, M, D) == 0) return -10;
  if (B == 0) return 0;
  GpkVarCholAdjArgs a{X, Z, Linv, vmean, vchol, hyp, gmean, gvar, (const float*)saved, B, N, M, D, workspace,
                      dX, dLinv, dZ, dpar, dchol, 1, 0LL};
  return gpk_launch_var_chol_adjoint(a, (hipStream_t)stream);
}

size_t gpk_variational_chol_adjoint_batched_workspace_bytes(int O, int B, int N, int M, int D) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * gpk_var_chol_adjoint_ws_bytes(B, N, M, D);
}

int gpk_variational_chol_adjoint_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                             const float* vmean, const float* vchol, const float* hyp,
                                             const float* gmean, const float* gvar, const void* saved, int O,
                                             int B, int N, int M, int D, void* workspace, float* dX,
                                             double* dLinv, float* dZ, float* dpar, float* dchol,
                                             void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vmean == nullptr) return -5;
  if (vchol == nullptr) return -6;
  if (hyp == nullptr) return -7;
  if (gmean == nullptr) return -8;
  if (gvar == nullptr) return -9;
  if (saved == nullptr || ((size_t)saved & 15) != 0) return -10;
  if (O < 1 || O > kGpkMaxOutputs) return -11;
  if (B < 0) return -12;
  if (N < 1 || N > 256) return -13;
  if (M < 1 || M > 256) return -14;
  if (D < 1 || D > 64) return -15;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -16;
  if (dX == nullptr) return -17;
  if (dLinv == nullptr) return -18;
  if (dZ == nullptr) return -19;
  if (dpar == nullptr) return -20;
  if (dchol == nullptr) return -21;
  if (B > 0 && gpk_var_chol_adjoint_ws_bytes(B, N, M, D) == 0) return -12;
  if (B == 0) return 0;
  GpkVarCholAdjArgs a{X, Z, Linv, vmean, vchol, hyp, gmean, gvar, (const float*)saved, B, N, M, D, workspace,
                      dX, dLinv, dZ, dpar, dchol, O, shared_x ? 0LL : (long long)B * N * D};
  return gpk_launch_var_chol_adjoint(a, (hipStream_t)stream);
}

// ---- dense covariance of q(f) for a Cholesky q(u) and its adjoint (gpk_var_chol_cov.hip)
size_t gpk_variational_chol_cov_workspace_bytes(int B, int N, int M) {
  return gpk_var_chol_cov_state_bytes(B, N, M);
}

size_t gpk_variational_chol_cov_batched_workspace_bytes(int O, int B, int N, int M) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * gpk_var_chol_cov_state_bytes(B, N, M);
}

int gpk_variational_chol_cov_f32(const float* X, const float* Z, const double* Linv, const float* vchol,
                                 const float* hyp, int B, int N, int M, int D, void* workspace, float* cov,
                                 void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vchol == nullptr) return -4;
  if (hyp == nullptr) return -5;
  if (B < 0) return -6;
  if (N < 1) return -7;
  if (M < 1 || M > 256) return -8;
  if (D < 1 || D > 64) return -9;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -10;   // panel rows are read 16 B at a time
  if (cov == nullptr) return -11;
  if (gpk_var_chol_cov_state_bytes(B, N, M) == 0 && B > 0) return -7;
  if (B == 0) return 0;
  GpkVarCholCovArgs a{X, Z, Linv, vchol, hyp, B, N, M, D, 1, 0LL, (float*)workspace, cov};
  return gpk_launch_var_chol_cov(a, (hipStream_t)stream);
}

int gpk_variational_chol_cov_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                         const float* vchol, const float* hyp, int O, int B, int N, int M,
                                         int D, void* workspace, float* cov, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vchol == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (O < 1 || O > kGpkMaxOutputs) return -7;
  if (B < 0) return -8;
  if (N < 1) return -9;
  if (M < 1 || M > 256) return -10;
  if (D < 1 || D > 64) return -11;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -12;
  if (cov == nullptr) return -13;
  if (gpk_var_chol_cov_state_bytes(B, N, M) == 0 && B > 0) return -9;
  if (B == 0) return 0;
  GpkVarCholCovArgs a{X, Z, Linv, vchol, hyp, B, N, M, D, O, shared_x ? 0LL : (long long)B * N * D,
                      (float*)workspace, cov};
  return gpk_launch_var_chol_cov(a, (hipStream_t)stream);
}

size_t gpk_variational_chol_cov_grad_workspace_bytes(int B, int N, int M, int D) {
  return gpk_var_chol_cov_grad_ws_bytes(B, N, M, D);
}

size_t gpk_variational_chol_cov_grad_batched_workspace_bytes(int O, int B, int N, int M, int D) {
  if (O < 1 || O > kGpkMaxOutputs) return 0;
  return (size_t)O * gpk_var_chol_cov_grad_ws_bytes(B, N, M, D);
}

int gpk_variational_chol_cov_grad_f32(const float* X, const float* Z, const double* Linv, const float* vchol,
                                      const float* hyp, const void* state, const float* gcov, int B, int N,
                                      int M, int D, void* workspace, float* dX, double* dLinv, float* dZ,
                                      float* dpar, float* dchol, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -2;
  if (Linv == nullptr) return -3;
  if (vchol == nullptr) return -4;
  if (hyp == nullptr) return -5;
  if (state == nullptr || ((size_t)state & 15) != 0) return -6;
  if (gcov == nullptr) return -7;
  if (B < 0) return -8;
  if (N < 1 || N > kGpkMvnRootMaxN) return -9;
  if (M < 1 || M > 256) return -10;
  if (D < 1 || D > 64) return -11;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -12;
  if (dX == nullptr) return -13;
  if (dLinv == nullptr) return -14;
  if (dZ == nullptr) return -15;
  if (dpar == nullptr) return -16;
  if (dchol == nullptr) return -17;
  if (B > 0 && gpk_var_chol_cov_grad_ws_bytes(B, N, M, D) == 0) return -8;
  if (B == 0) return 0;
  GpkVarCholCovGradArgs a{X, Z, Linv, vchol, hyp, (const float*)state, gcov, B, N, M, D, 1, 0LL, workspace,
                          dX, dLinv, dZ, dpar, dchol};
  return gpk_launch_var_chol_cov_grad(a, (hipStream_t)stream);
}

int gpk_variational_chol_cov_grad_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                              const float* vchol, const float* hyp, const void* state,
                                              const float* gcov, int O, int B, int N, int M, int D,
                                              void* workspace, float* dX, double* dLinv, float* dZ,
                                              float* dpar, float* dchol, void* stream) {
  if (X == nullptr) return -1;
  if (Z == nullptr) return -3;
  if (Linv == nullptr) return -4;
  if (vchol == nullptr) return -5;
  if (hyp == nullptr) return -6;
  if (state == nullptr || ((size_t)state & 15) != 0) return -7;
  if (gcov == nullptr) return -8;
  if (O < 1 || O > kGpkMaxOutputs) return -9;
  if (B < 0) return -10;
  if (N < 1 || N > kGpkMvnRootMaxN) return -11;
  if (M < 1 || M > 256) return -12;
  if (D < 1 || D > 64) return -13;
  if (workspace == nullptr || ((size_t)workspace & 15) != 0) return -14;
  if (dX == nullptr) return -15;
  if (dLinv == nullptr) return -16;
  if (dZ == nullptr) return -17;
  if (dpar == nullptr) return -18;
  if (dchol == nullptr) return -19;
  if (B > 0 && gpk_var_chol_cov_grad_ws_bytes(B, N, M, D) == 0) return -10;
  if (B == 0) return 0;
  GpkVarCholCovGradArgs a{X, Z, Linv, vchol, hyp, (const float*)state, gcov, B, N, M, D, O,
                          shared_x ? 0LL : (long long)B * N * D, workspace, dX, dLinv, dZ, dpar, dchol};
  return gpk_launch_var_chol_cov_grad(a, (hipStream_t)stream);
}

int gpk_cholesky_kl_f32(const float* m, const float* chol, int M, float* kl, const float* gkl, float* dm,
                        float* dchol, void* stream) {
  if (m == nullptr) return -1;
  if (chol == nullptr) return -2;
  if (M < 1 || M > 16384) return -3;
  if (gkl == nullptr && kl == nullptr) return -4;
  if (gkl != nullptr && dm == nullptr) return -6;
  if (gkl != nullptr && dchol == nullptr) return -7;
  return gpk_launch_chol_kl(m, chol, 1, M, kl, gkl, dm, dchol, (hipStream_t)stream);
}

int gpk_cholesky_kl_batched_f32(const float* m, const float* chol, int O, int M, float* kl, const float* gkl,
                                float* dm, float* dchol, void* stream) {
  if (m == nullptr) return -1;
  if (chol == nullptr) return -2;
  if (O < 1 || O > kGpkMaxOutputs) return -3;
  if (M < 1 || M > 16384) return -4;
  if (gkl == nullptr && kl == nullptr) return -5;
  if (gkl != nullptr && dm == nullptr) return -7;
  if (gkl != nullptr && dchol == nullptr) return -8;
  return gpk_launch_chol_kl(m, chol, O, M, kl, gkl, dm, dchol, (hipStream_t)stream);
}

int gpk_mvn_root_max_n(void) { return kGpkMvnRootMaxN; }

int gpk_mvn_root_f32(const float* cov, const float* mean, const float* eps, int B, int n, int S,
                     float jitter, float* R, float* samples, int* info, void* stream) {
  if (cov == nullptr) return -1;
  if (S > 0 && mean == nullptr) return -2;
  if (S > 0 && eps == nullptr) return -3;
  if (B < 0) return -4;
  if (n < 1 || n > kGpkMvnRootMaxN) return -5;
  if (S < 0) return -6;
  if (!(jitter >= 0.f)) return -7;
  if (S > 0 && samples == nullptr) return -9;
  if (info == nullptr) return -10;
  if (B == 0) return 0;
  return gpk_launch_mvn_root(cov, mean, eps, B, n, S, jitter, R, samples, info, (hipStream_t)stream);
}

int gpk_tri_solve_f32(const float* R, const float* d, int B, int n, int trans, float* w, void* stream) {
  if (R == nullptr) return -1;
  if (d == nullptr) return -2;
  if (B < 0) return -3;
  if (n < 1 || n > kGpkMvnRootMaxN) return -4;
  if (trans != 0 && trans != 1) return -5;
  if (w == nullptr) return -6;
  if (B == 0) return 0;
  return gpk_launch_tri_solve(R, d, B, n, trans, w, (hipStream_t)stream);
}

size_t gpk_mvn_root_grad_workspace_bytes(int B, int n) {
  if (B < 0 || n < 1 || n > kGpkMvnRootMaxN) return 0;
  return gpk_mvn_root_grad_ws_floats(B, n) * sizeof(float);
}

int gpk_mvn_root_grad_f32(const float* R, const float* gR, const float* gsamples, const float* eps,
                          int B, int n, int S, void* workspace, float* dcov, float* dmean, void* stream) {
  if (R == nullptr) return -1;
  if (S > 0 && gsamples == nullptr) return -3;
  if (S > 0 && eps == nullptr) return -4;
  if (B < 0) return -5;
  if (n < 1 || n > kGpkMvnRootMaxN) return -6;
  if (S < 0) return -7;
  if (gpk_mvn_root_grad_workspace_bytes(B, n) > 0 && (workspace == nullptr || ((size_t)workspace & 15) != 0))
    return -8;   // tiles are read 16 B at a time
  if (dcov == nullptr) return -9;
  if (B == 0) return 0;
  return gpk_launch_mvn_root_grad(R, gR, gsamples, eps, B, n, S, (float*)workspace, dcov, dmean,
                                  (hipStream_t)stream);
}

size_t gpk_mvn_root_refine_workspace_bytes(int B, int n) {
  if (B < 0 || n < 1 || n > kGpkMvnRootMaxN) return 0;
  return gpk_mvn_root_refine_ws_floats(B, n) * sizeof(float);
}

int gpk_mvn_root_refine_f32(const float* cov, const float* R, int B, int n, float jitter, void* workspace,
                            float* Rout, void* stream) {
  if (cov == nullptr) return -1;
  if (R == nullptr) return -2;
  if (B < 0) return -3;
  if (n < 1 || n > kGpkMvnRootMaxN) return -4;
  if (!(jitter >= 0.f)) return -5;
  if (gpk_mvn_root_refine_workspace_bytes(B, n) > 0 && (workspace == nullptr || ((size_t)workspace & 15) != 0))
    return -6;
  if (Rout == nullptr || Rout == R) return -7;
  if (B == 0) return 0;
  return gpk_launch_mvn_root_refine(cov, R, B, n, jitter, (float*)workspace, Rout, (hipStream_t)stream);
}

int gpk_window_gather_f32(const float* table, long long n_rows, int F, const long long* rows, int B,
                          int T, int n_enc, int pred_len, int target_col, float* enc, float* dec,
                          float* y, void* stream) {
  if (table == nullptr) return -1;
  if (n_rows < 0) return -2;
  if (F < 1) return -3;
  if (rows == nullptr && B > 0) return -4;
  if (B < 0) return -5;
  if (T < 1) return -6;
  if (n_enc < 0 || n_enc > T) return -7;
  if (pred_len < 0 || n_enc + pred_len > T) return -8;
  if (target_col < 0 || target_col >= F) return -9;
  if (enc == nullptr && B > 0 && n_enc > 0) return -10;
  if (dec == nullptr && B > 0 && T - n_enc - pred_len > 0) return -11;
  if (y == nullptr && B > 0 && pred_len > 0) return -12;
  if (B == 0) return 0;
  return gpk_launch_window_gather(table, F, rows, B, n_enc, T - n_enc - pred_len, pred_len,
                                  target_col, enc, dec, y, (hipStream_t)stream);
}

// Diagnostic (not part of the product ABI): same as gpk_exact_mll_f32 for N in
// (240, 256], plus per-workgroup phase clocks and a per-step timeline (32 + 1024 x u64 per window) in `stamps`.
int gpk_debug_exact_stamps(const float* X, const float* y, const float* hyp, int n_lengthscale,
                           int B, int N, int D, double jitter, int max_tries, float* L, float* z,
                           float* mll, int* info, unsigned long long* stamps, void* stream) {
  GpkExactArgs a{X, y, hyp, n_lengthscale, B, N, D, jitter, max_tries, L, z, mll, info};
  return gpk_launch_exact_stamps(a, stamps, (hipStream_t)stream);
}

}  // extern "C"
