// C-ABI shim: argument validation + dispatch to the gfx950 kernels.
// Declarations and the reference interfaces each entry point replaces: include/gpk.h.
#include <initializer_list>

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

// ---- families of sibling symbols ("One body per family"): the validation ladder and
//      the launch of an operation are written once, in a static body; the exported symbols forward.
namespace {

constexpr int kGpkMaxOutputs = 65535;   // gridDim.y

// The code of a refused argument is its position in the caller's own list. A body numbers the
// arguments by its family's *_batched list; a single-output list is that list without shared_x
// (position 2, in the families that have it) and without O.
struct ArgPos {
  bool batched;           // entered through the *_batched symbol
  int pos_O;              // position of O in the *_batched list
  bool shared_x = true;   // that list has shared_x at position 2
  int operator()(int p) const { return batched ? -p : -(p - (shared_x && p > 2) - (p > pos_O)); }
};

// Elements between two outputs' inputs: 0 when every output reads the same X (a single-output call).
static long long x_stride_of(int shared_x, int B, int N, int D) { return shared_x ? 0LL : (long long)B * N * D; }

// Every *_batched_workspace_bytes / *_batched_saved_bytes query: O slices of the single-output size.
static size_t per_output(int O, size_t single_bytes) {
  return O < 1 || O > kGpkMaxOutputs ? 0 : (size_t)O * single_bytes;
}

// Position of the first NULL among the arguments at consecutive positions from `first`, 0 if none.
static int first_null(int first, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) {
    if (p == nullptr) return first;
    ++first;
  }
  return 0;
}

// 1-based index of the first of B, N, M, D outside its range, 0 if none: min_B <= B, 1 <= N <= max_N
// (0: no upper limit), 1 <= M <= 256, 1 <= D <= 64.
static int first_bad_size(int B, int N, int M, int D, int min_B, int max_N) {
  if (B < min_B) return 1;
  if (N < 1 || (max_N > 0 && N > max_N)) return 2;
  if (M < 1 || M > 256) return 3;
  if (D < 1 || D > 64) return 4;
  return 0;
}

static bool bad_outputs(int O) { return O < 1 || O > kGpkMaxOutputs; }
static bool misaligned(const void* p) { return ((size_t)p & 15) != 0; }   // rows are read 16 B at a time

static int kzz_chol(bool batched, const GpkKzzArgs& a, hipStream_t stream) {
  const ArgPos at{batched, 3, false};
  if (int p = first_null(1, {a.Z, a.hyp})) return at(p);
  if (bad_outputs(a.O)) return at(3);
  if (a.M < 1 || a.M > 256) return at(4);
  if (a.D < 1 || a.D > 64) return at(5);
  if (a.max_tries < 0 || a.max_tries > 12) return at(8);
  if (int p = first_null(9, {a.L, a.Linv, a.info})) return at(p);
  return gpk_launch_kzz16(a, stream);
}

static int kzz_backward(bool batched, const GpkKzzGradArgs& a, hipStream_t stream) {
  const ArgPos at{batched, 6, false};
  if (int p = first_null(1, {a.dLinv, a.L, a.Linv, a.Z, a.hyp})) return at(p);
  if (bad_outputs(a.O)) return at(6);
  if (a.M < 1 || a.M > 256) return at(7);
  if (a.D < 1 || a.D > 64) return at(8);
  if (int p = first_null(9, {a.ws, a.dZ, a.dhyp})) return at(p);
  return gpk_launch_kzz_grad(a, stream);
}

// Mean-field forward. Its three lists differ by more than shared_x and O (y and ell on the single
// lists only, saved on two of them), so each symbol names its positions: Z .. hyp, B .. D and
// mean, var are consecutive from Z, B and mean; 0 = not in the list.
struct VarFwdPos { int Z, y, O, B, mean, saved; };
constexpr VarFwdPos kVarFwdSingle{2, 7, 0, 8, 12, 16};    // gpk_variational_f32 (no saved) and _train_f32
constexpr VarFwdPos kVarFwdBatched{3, 0, 8, 9, 13, 16};   // gpk_variational_batched_f32

// `train`: gpk_variational_train_f32 wants its saved state wherever the shape has a saved-state path
// (and takes NULL elsewhere); the other two refuse a non-NULL one with B < 1 or without such a path.
static int var_forward(const VarFwdPos& p, bool train, GpkVarArgs a, int shared_x, int* flags, hipStream_t stream) {
  if (a.X == nullptr) return -1;
  if (int q = first_null(p.Z, {a.Z, a.Linv, a.vmean, a.vstd, a.hyp})) return -q;
  if (bad_outputs(a.O)) return -p.O;
  if (int k = first_bad_size(a.B, a.N, a.M, a.D, 0, 0)) return -(p.B + k - 1);
  if (int q = first_null(p.mean, {a.mean, a.var})) return -q;
  if (a.ell != nullptr && a.y == nullptr) return -p.y;
  if (train ? a.saved == nullptr && gpk_var_saved_bytes(a.B, a.N, a.M, a.D) > 0
            : a.saved != nullptr && (a.B < 1 || gpk_var_saved_bytes(a.B, a.N, a.M, a.D) == 0))
    return -p.saved;
  if (a.B == 0) return 0;
  a.x_stride = x_stride_of(shared_x, a.B, a.N, a.D);
  return gpk_launch_var(a, flags, stream);
}

// Mean-field adjoint: gpk_variational_adjoint_f32 has no saved argument, _saved_f32 requires it,
// _batched_f32 takes it or NULL. Z .. gvar, B .. D and workspace .. dpar are consecutive.
// `no_path` is where a saved state for a shape without a saved-state path is reported: under M by
// _saved_f32, under saved by _batched_f32.
struct VarAdjPos { int Z, saved, O, B, no_path, workspace; };
constexpr VarAdjPos kVarAdjSingle{2, 0, 0, 9, 0, 13};         // gpk_variational_adjoint_f32
constexpr VarAdjPos kVarAdjSaved{2, 9, 0, 10, 12, 14};        // gpk_variational_adjoint_saved_f32
constexpr VarAdjPos kVarAdjBatched{3, 10, 11, 12, 10, 16};    // gpk_variational_adjoint_batched_f32

static int var_adjoint(const VarAdjPos& p, bool need_saved, GpkVarAdjArgs a, int shared_x, hipStream_t stream) {
  if (a.X == nullptr) return -1;
  if (int q = first_null(p.Z, {a.Z, a.Linv, a.vmean, a.vstd, a.hyp, a.gmean, a.gvar})) return -q;
  if (need_saved && a.saved == nullptr) return -p.saved;
  if (bad_outputs(a.O)) return -p.O;
  if (int k = first_bad_size(a.B, a.N, a.M, a.D, 1, 0)) return -(p.B + k - 1);
  if (a.saved != nullptr && gpk_var_saved_bytes(a.B, a.N, a.M, a.D) == 0) return -p.no_path;
  if (int q = first_null(p.workspace, {a.ws, a.dX, a.dLinv, a.dZ, a.dpar})) return -q;
  a.x_stride = x_stride_of(shared_x, a.B, a.N, a.D);
  return gpk_launch_var_adjoint(a, stream);
}

// Dense covariance of q(f): phase 1 (A = Linv K_ZX, gpk_variational_cov.hip), then the variational
// mode of the covariance kernel (gpk_posterior_cov.hip).
static int var_cov(bool batched, const float* X, int shared_x, const float* Z, const double* Linv,
                   const float* vstd, const float* hyp, int O, int B, int N, int M, int D, void* workspace,
                   float* cov, hipStream_t stream) {
  const ArgPos at{batched, 7};
  if (X == nullptr) return at(1);
  if (int p = first_null(3, {Z, Linv, vstd, hyp})) return at(p);
  if (bad_outputs(O)) return at(7);
  if (int k = first_bad_size(B, N, M, D, 0, 0)) return at(7 + k);
  if (workspace == nullptr || misaligned(workspace)) return at(12);
  if (cov == nullptr) return at(13);
  if (!gpk_var_cov_tile_grid_ok(B, N, M)) return at(9);
  if (B == 0) return 0;
  GpkVarCovArgs a{hyp, X, (const float*)workspace, vstd, B, M, N, D, gpk_post_cov_vstride(N), cov,
                  x_stride_of(shared_x, B, N, D), (long long)gpk_var_cov_ws_floats(B, N, M)};
  const int rc = gpk_launch_variational_cov_phase1(a, (float*)workspace, Z, Linv, O, stream);
  if (rc != 0) return rc;
  return gpk_launch_variational_cov_phase2(a, O, stream);
}

// Adjoint of the dense covariance of q(f) (gpk_variational_cov_grad.hip).
static int var_cov_grad(bool batched, GpkVarCovGradArgs a, int shared_x, hipStream_t stream) {
  const ArgPos at{batched, 9};
  if (a.X == nullptr) return at(1);
  if (int p = first_null(3, {a.Z, a.Linv, a.vstd, a.hyp})) return at(p);
  if (a.state == nullptr || misaligned(a.state)) return at(7);
  if (a.gcov == nullptr) return at(8);
  if (bad_outputs(a.O)) return at(9);
  if (int k = first_bad_size(a.B, a.N, a.M, a.D, 0, kGpkMvnRootMaxN)) return at(9 + k);
  if (a.ws == nullptr || misaligned(a.ws)) return at(14);
  if (int p = first_null(15, {a.dX, a.dLinv, a.dZ, a.dpar})) return at(p);
  if (a.B > 0 && gpk_var_cov_grad_ws_bytes(a.B, a.N, a.M, a.D) == 0) return at(10);
  if (a.B == 0) return 0;
  a.x_stride = x_stride_of(shared_x, a.B, a.N, a.D);
  return gpk_launch_var_cov_grad(a, stream);
}

// Cholesky q(u): forward, adjoint, KL (gpk_var_chol.hip).
static int var_chol(bool batched, GpkVarCholArgs a, int shared_x, hipStream_t stream) {
  const ArgPos at{batched, 8};
  if (a.X == nullptr) return at(1);
  if (int p = first_null(3, {a.Z, a.Linv, a.vmean, a.vchol, a.hyp})) return at(p);
  if (bad_outputs(a.O)) return at(8);
  if (int k = first_bad_size(a.B, a.N, a.M, a.D, 0, 0)) return at(8 + k);
  if (int p = first_null(13, {a.mean, a.var})) return at(p);
  // both siblings refuse a misaligned saved; only _batched_f32 also refuses one with B < 1 or for a
  // shape without a saved state
  if (a.saved != nullptr &&
      (misaligned(a.saved) || (batched && (a.B < 1 || gpk_var_chol_saved_bytes(a.B, a.N, a.M, a.D) == 0))))
    return at(16);
  if (a.B == 0) return 0;
  a.x_stride = x_stride_of(shared_x, a.B, a.N, a.D);
  return gpk_launch_var_chol(a, stream);
}

static int var_chol_adjoint(bool batched, GpkVarCholAdjArgs a, int shared_x, hipStream_t stream) {
  const ArgPos at{batched, 11};
  if (a.X == nullptr) return at(1);
  if (int p = first_null(3, {a.Z, a.Linv, a.vmean, a.vchol, a.hyp, a.gmean, a.gvar})) return at(p);
  if (a.saved == nullptr || misaligned(a.saved)) return at(10);
  if (bad_outputs(a.O)) return at(11);
  if (int k = first_bad_size(a.B, a.N, a.M, a.D, 0, 256)) return at(11 + k);
  if (a.ws == nullptr || misaligned(a.ws)) return at(16);
  if (int p = first_null(17, {a.dX, a.dLinv, a.dZ, a.dpar, a.dchol})) return at(p);
  if (a.B > 0 && gpk_var_chol_adjoint_ws_bytes(a.B, a.N, a.M, a.D) == 0) return at(12);
  if (a.B == 0) return 0;
  a.x_stride = x_stride_of(shared_x, a.B, a.N, a.D);
  return gpk_launch_var_chol_adjoint(a, stream);
}

static int cholesky_kl(bool batched, const float* m, const float* chol, int O, int M, float* kl, const float* gkl,
                       float* dm, float* dchol, hipStream_t stream) {
  const ArgPos at{batched, 3, false};
  if (int p = first_null(1, {m, chol})) return at(p);
  if (bad_outputs(O)) return at(3);
  if (M < 1 || M > 16384) return at(4);
  if (gkl == nullptr && kl == nullptr) return at(5);
  if (gkl != nullptr && dm == nullptr) return at(7);
  if (gkl != nullptr && dchol == nullptr) return at(8);
  return gpk_launch_chol_kl(m, chol, O, M, kl, gkl, dm, dchol, stream);
}

// Dense covariance of q(f) for a Cholesky q(u) and its adjoint (gpk_var_chol_cov.hip).
static int var_chol_cov(bool batched, GpkVarCholCovArgs a, int shared_x, hipStream_t stream) {
  const ArgPos at{batched, 7};
  if (a.X == nullptr) return at(1);
  if (int p = first_null(3, {a.Z, a.Linv, a.vchol, a.hyp})) return at(p);
  if (bad_outputs(a.O)) return at(7);
  if (int k = first_bad_size(a.B, a.N, a.M, a.D, 0, 0)) return at(7 + k);
  if (a.state == nullptr || misaligned(a.state)) return at(12);
  if (a.cov == nullptr) return at(13);
  if (gpk_var_chol_cov_state_bytes(a.B, a.N, a.M) == 0 && a.B > 0) return at(9);
  if (a.B == 0) return 0;
  a.x_stride = x_stride_of(shared_x, a.B, a.N, a.D);
  return gpk_launch_var_chol_cov(a, stream);
}

static int var_chol_cov_grad(bool batched, GpkVarCholCovGradArgs a, int shared_x, hipStream_t stream) {
  const ArgPos at{batched, 9};
  if (a.X == nullptr) return at(1);
  if (int p = first_null(3, {a.Z, a.Linv, a.vchol, a.hyp})) return at(p);
  if (a.state == nullptr || misaligned(a.state)) return at(7);
  if (a.gcov == nullptr) return at(8);
  if (bad_outputs(a.O)) return at(9);
  if (int k = first_bad_size(a.B, a.N, a.M, a.D, 0, kGpkMvnRootMaxN)) return at(9 + k);
  if (a.ws == nullptr || misaligned(a.ws)) return at(14);
  if (int p = first_null(15, {a.dX, a.dLinv, a.dZ, a.dpar, a.dchol})) return at(p);
  if (a.B > 0 && gpk_var_chol_cov_grad_ws_bytes(a.B, a.N, a.M, a.D) == 0) return at(10);
  if (a.B == 0) return 0;
  a.x_stride = x_stride_of(shared_x, a.B, a.N, a.D);
  return gpk_launch_var_chol_cov_grad(a, stream);
}

}  // namespace

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

// ---- K_ZZ factor and its backward: single-output and multi-output (output o on grid dimension y)
int gpk_kzz_chol_f64(const float* Z, const float* hyp, int M, int D, float jitter,
                     double chol_jitter, int max_tries, double* L, double* Linv, int* info,
                     void* stream) {
  return kzz_chol(false, GpkKzzArgs{Z, hyp, M, D, jitter, chol_jitter, max_tries, L, Linv, info, 1},
                  (hipStream_t)stream);
}

int gpk_kzz_chol_f64_batched(const float* Z, const float* hyp, int O, int M, int D, float jitter,
                             double chol_jitter, int max_tries, double* L, double* Linv, int* info,
                             void* stream) {
  return kzz_chol(true, GpkKzzArgs{Z, hyp, M, D, jitter, chol_jitter, max_tries, L, Linv, info, O},
                  (hipStream_t)stream);
}

size_t gpk_kzz_backward_workspace_bytes(int M, int D) {
  if (M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_kzz_grad_ws_bytes(M, D);
}

size_t gpk_kzz_backward_batched_workspace_bytes(int O, int M, int D) {
  return per_output(O, gpk_kzz_backward_workspace_bytes(M, D));
}

int gpk_kzz_backward_f64(const double* dLinv, const double* L, const double* Linv, const float* Z,
                         const float* hyp, int M, int D, void* workspace, float* dZ, float* dhyp,
                         void* stream) {
  return kzz_backward(false, GpkKzzGradArgs{dLinv, L, Linv, Z, hyp, M, D, workspace, dZ, dhyp, 1},
                      (hipStream_t)stream);
}

int gpk_kzz_backward_f64_batched(const double* dLinv, const double* L, const double* Linv,
                                 const float* Z, const float* hyp, int O, int M, int D, void* workspace,
                                 float* dZ, float* dhyp, void* stream) {
  return kzz_backward(true, GpkKzzGradArgs{dLinv, L, Linv, Z, hyp, M, D, workspace, dZ, dhyp, O},
                      (hipStream_t)stream);
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

// ---- mean-field variational forward and adjoint
int gpk_variational_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                        const float* vstd, const float* hyp, const float* y, int B, int N, int M,
                        int D, float* mean, float* var, float* ell, int* flags, void* stream) {
  GpkVarArgs a{X, Z, Linv, vmean, vstd, hyp, y, B, N, M, D, mean, var, ell};
  return var_forward(kVarFwdSingle, false, a, 1, flags, (hipStream_t)stream);
}

size_t gpk_variational_saved_bytes(int B, int N, int M, int D) {
  if (B < 1 || N < 1 || M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_var_saved_bytes(B, N, M, D);
}

int gpk_variational_train_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                              const float* vstd, const float* hyp, const float* y, int B, int N, int M,
                              int D, float* mean, float* var, float* ell, int* flags, void* saved,
                              void* stream) {
  GpkVarArgs a{X, Z, Linv, vmean, vstd, hyp, y, B, N, M, D, mean, var, ell, (float*)saved};
  return var_forward(kVarFwdSingle, true, a, 1, flags, (hipStream_t)stream);
}

int gpk_variational_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                const float* vmean, const float* vstd, const float* hyp, int O, int B,
                                int N, int M, int D, float* mean, float* var, int* flags, void* saved,
                                void* stream) {
  GpkVarArgs a{X, Z, Linv, vmean, vstd, hyp, nullptr, B, N, M, D, mean, var, nullptr, (float*)saved, O};
  return var_forward(kVarFwdBatched, false, a, shared_x, flags, (hipStream_t)stream);
}

size_t gpk_variational_adjoint_workspace_bytes(int B, int N, int M, int D) {
  if (B < 1 || N < 1 || M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_var_adjoint_ws_bytes(B, N, M, D);
}

size_t gpk_variational_adjoint_saved_workspace_bytes(int B, int N, int M, int D) {
  if (B < 1 || N < 1 || M < 1 || M > 256 || D < 1 || D > 64) return 0;
  return gpk_var_adjoint_saved_ws_bytes(B, N, M, D);
}

size_t gpk_variational_adjoint_batched_workspace_bytes(int O, int B, int N, int M, int D, int has_saved) {
  return per_output(O, has_saved ? gpk_variational_adjoint_saved_workspace_bytes(B, N, M, D)
                                 : gpk_variational_adjoint_workspace_bytes(B, N, M, D));
}

int gpk_variational_adjoint_f32(const float* X, const float* Z, const double* Linv,
                                const float* vmean, const float* vstd, const float* hyp,
                                const float* gmean, const float* gvar, int B, int N, int M, int D,
                                void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                void* stream) {
  GpkVarAdjArgs a{X, Z, Linv, vmean, vstd, hyp, gmean, gvar, B, N, M, D, workspace, dX, dLinv, dZ, dpar};
  return var_adjoint(kVarAdjSingle, false, a, 1, (hipStream_t)stream);
}

int gpk_variational_adjoint_saved_f32(const float* X, const float* Z, const double* Linv,
                                      const float* vmean, const float* vstd, const float* hyp,
                                      const float* gmean, const float* gvar, const void* saved, int B,
                                      int N, int M, int D, void* workspace, float* dX, double* dLinv,
                                      float* dZ, float* dpar, void* stream) {
  GpkVarAdjArgs a{X, Z, Linv, vmean, vstd, hyp, gmean, gvar, B, N, M, D, workspace, dX, dLinv, dZ, dpar,
                  (const float*)saved};
  return var_adjoint(kVarAdjSaved, true, a, 1, (hipStream_t)stream);
}

int gpk_variational_adjoint_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                        const float* vmean, const float* vstd, const float* hyp,
                                        const float* gmean, const float* gvar, const void* saved, int O,
                                        int B, int N, int M, int D, void* workspace, float* dX,
                                        double* dLinv, float* dZ, float* dpar, void* stream) {
  GpkVarAdjArgs a{X, Z, Linv, vmean, vstd, hyp, gmean, gvar, B, N, M, D, workspace, dX, dLinv, dZ, dpar,
                  (const float*)saved, O};
  return var_adjoint(kVarAdjBatched, false, a, shared_x, (hipStream_t)stream);
}

// ---- dense covariance of q(f) and its adjoint
size_t gpk_variational_cov_workspace_bytes(int B, int N, int M) {
  if (!gpk_var_cov_tile_grid_ok(B, N, M)) return 0;
  return gpk_var_cov_ws_floats(B, N, M) * sizeof(float);
}

size_t gpk_variational_cov_batched_workspace_bytes(int O, int B, int N, int M) {
  return per_output(O, gpk_variational_cov_workspace_bytes(B, N, M));
}

int gpk_variational_cov_f32(const float* X, const float* Z, const double* Linv, const float* vstd,
                            const float* hyp, int B, int N, int M, int D, void* workspace,
                            float* cov, void* stream) {
  return var_cov(false, X, 1, Z, Linv, vstd, hyp, 1, B, N, M, D, workspace, cov, (hipStream_t)stream);
}

int gpk_variational_cov_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                    const float* vstd, const float* hyp, int O, int B, int N, int M,
                                    int D, void* workspace, float* cov, void* stream) {
  return var_cov(true, X, shared_x, Z, Linv, vstd, hyp, O, B, N, M, D, workspace, cov, (hipStream_t)stream);
}

size_t gpk_variational_cov_grad_workspace_bytes(int B, int N, int M, int D) {
  return gpk_var_cov_grad_ws_bytes(B, N, M, D);
}

size_t gpk_variational_cov_grad_batched_workspace_bytes(int O, int B, int N, int M, int D) {
  return per_output(O, gpk_var_cov_grad_ws_bytes(B, N, M, D));
}

int gpk_variational_cov_grad_f32(const float* X, const float* Z, const double* Linv, const float* vstd,
                                 const float* hyp, const void* state, const float* gcov, int B, int N,
                                 int M, int D, void* workspace, float* dX, double* dLinv, float* dZ,
                                 float* dpar, void* stream) {
  GpkVarCovGradArgs a{X, Z, Linv, vstd, hyp, (const float*)state, gcov, B, N, M, D, 1, 0LL, workspace,
                      dX, dLinv, dZ, dpar};
  return var_cov_grad(false, a, 1, (hipStream_t)stream);
}

int gpk_variational_cov_grad_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                         const float* vstd, const float* hyp, const void* state,
                                         const float* gcov, int O, int B, int N, int M, int D,
                                         void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                         void* stream) {
  GpkVarCovGradArgs a{X, Z, Linv, vstd, hyp, (const float*)state, gcov, B, N, M, D, O, 0LL, workspace,
                      dX, dLinv, dZ, dpar};
  return var_cov_grad(true, a, shared_x, (hipStream_t)stream);
}

// ---- Cholesky q(u)
size_t gpk_variational_chol_saved_bytes(int B, int N, int M, int D) {
  return gpk_var_chol_saved_bytes(B, N, M, D);
}

size_t gpk_variational_chol_batched_saved_bytes(int O, int B, int N, int M, int D) {
  return per_output(O, gpk_var_chol_saved_bytes(B, N, M, D));
}

int gpk_variational_chol_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                             const float* vchol, const float* hyp, int B, int N, int M, int D, float* mean,
                             float* var, int* flags, void* saved, void* stream) {
  GpkVarCholArgs a{X, Z, Linv, vmean, vchol, hyp, B, N, M, D, mean, var, flags, (float*)saved, 1, 0LL};
  return var_chol(false, a, 1, (hipStream_t)stream);
}

int gpk_variational_chol_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                     const float* vmean, const float* vchol, const float* hyp, int O, int B,
                                     int N, int M, int D, float* mean, float* var, int* flags, void* saved,
                                     void* stream) {
  GpkVarCholArgs a{X, Z, Linv, vmean, vchol, hyp, B, N, M, D, mean, var, flags, (float*)saved, O, 0LL};
  return var_chol(true, a, shared_x, (hipStream_t)stream);
}

size_t gpk_variational_chol_adjoint_workspace_bytes(int B, int N, int M, int D) {
  return gpk_var_chol_adjoint_ws_bytes(B, N, M, D);
}

size_t gpk_variational_chol_adjoint_batched_workspace_bytes(int O, int B, int N, int M, int D) {
  return per_output(O, gpk_var_chol_adjoint_ws_bytes(B, N, M, D));
}

int gpk_variational_chol_adjoint_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                                     const float* vchol, const float* hyp, const float* gmean,
                                     const float* gvar, const void* saved, int B, int N, int M, int D,
                                     void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                     float* dchol, void* stream) {
  GpkVarCholAdjArgs a{X, Z, Linv, vmean, vchol, hyp, gmean, gvar, (const float*)saved, B, N, M, D, workspace,
                      dX, dLinv, dZ, dpar, dchol, 1, 0LL};
  return var_chol_adjoint(false, a, 1, (hipStream_t)stream);
}

int gpk_variational_chol_adjoint_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                             const float* vmean, const float* vchol, const float* hyp,
                                             const float* gmean, const float* gvar, const void* saved, int O,
                                             int B, int N, int M, int D, void* workspace, float* dX,
                                             double* dLinv, float* dZ, float* dpar, float* dchol,
                                             void* stream) {
  GpkVarCholAdjArgs a{X, Z, Linv, vmean, vchol, hyp, gmean, gvar, (const float*)saved, B, N, M, D, workspace,
                      dX, dLinv, dZ, dpar, dchol, O, 0LL};
  return var_chol_adjoint(true, a, shared_x, (hipStream_t)stream);
}

int gpk_cholesky_kl_f32(const float* m, const float* chol, int M, float* kl, const float* gkl, float* dm,
                        float* dchol, void* stream) {
  return cholesky_kl(false, m, chol, 1, M, kl, gkl, dm, dchol, (hipStream_t)stream);
}

int gpk_cholesky_kl_batched_f32(const float* m, const float* chol, int O, int M, float* kl, const float* gkl,
                                float* dm, float* dchol, void* stream) {
  return cholesky_kl(true, m, chol, O, M, kl, gkl, dm, dchol, (hipStream_t)stream);
}

// ---- dense covariance of q(f) for a Cholesky q(u) and its adjoint
size_t gpk_variational_chol_cov_workspace_bytes(int B, int N, int M) {
  return gpk_var_chol_cov_state_bytes(B, N, M);
}

size_t gpk_variational_chol_cov_batched_workspace_bytes(int O, int B, int N, int M) {
  return per_output(O, gpk_var_chol_cov_state_bytes(B, N, M));
}

int gpk_variational_chol_cov_f32(const float* X, const float* Z, const double* Linv, const float* vchol,
                                 const float* hyp, int B, int N, int M, int D, void* workspace, float* cov,
                                 void* stream) {
  GpkVarCholCovArgs a{X, Z, Linv, vchol, hyp, B, N, M, D, 1, 0LL, (float*)workspace, cov};
  return var_chol_cov(false, a, 1, (hipStream_t)stream);
}

int gpk_variational_chol_cov_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                         const float* vchol, const float* hyp, int O, int B, int N, int M,
                                         int D, void* workspace, float* cov, void* stream) {
  GpkVarCholCovArgs a{X, Z, Linv, vchol, hyp, B, N, M, D, O, 0LL, (float*)workspace, cov};
  return var_chol_cov(true, a, shared_x, (hipStream_t)stream);
}

size_t gpk_variational_chol_cov_grad_workspace_bytes(int B, int N, int M, int D) {
  return gpk_var_chol_cov_grad_ws_bytes(B, N, M, D);
}

size_t gpk_variational_chol_cov_grad_batched_workspace_bytes(int O, int B, int N, int M, int D) {
  return per_output(O, gpk_var_chol_cov_grad_ws_bytes(B, N, M, D));
}

int gpk_variational_chol_cov_grad_f32(const float* X, const float* Z, const double* Linv, const float* vchol,
                                      const float* hyp, const void* state, const float* gcov, int B, int N,
                                      int M, int D, void* workspace, float* dX, double* dLinv, float* dZ,
                                      float* dpar, float* dchol, void* stream) {
  GpkVarCholCovGradArgs a{X, Z, Linv, vchol, hyp, (const float*)state, gcov, B, N, M, D, 1, 0LL, workspace,
                          dX, dLinv, dZ, dpar, dchol};
  return var_chol_cov_grad(false, a, 1, (hipStream_t)stream);
}

int gpk_variational_chol_cov_grad_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                              const float* vchol, const float* hyp, const void* state,
                                              const float* gcov, int O, int B, int N, int M, int D,
                                              void* workspace, float* dX, double* dLinv, float* dZ,
                                              float* dpar, float* dchol, void* stream) {
  GpkVarCholCovGradArgs a{X, Z, Linv, vchol, hyp, (const float*)state, gcov, B, N, M, D, O, 0LL, workspace,
                          dX, dLinv, dZ, dpar, dchol};
  return var_chol_cov_grad(true, a, shared_x, (hipStream_t)stream);
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
