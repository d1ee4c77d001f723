/*
 * gpk.h — C ABI of the MI355X-native GP blur/denoise kernels (libgpk.so).
 *
 * Plain pointers and sizes only; every buffer is DEVICE memory owned by the
 * caller (contiguous, row-major). `stream` is a hipStream_t passed as void*
 * (0 = legacy default stream); all work is enqueued on it, nothing
 * synchronises, nothing is allocated. The library keeps no pointer after a
 * call returns and holds no mutable global state (safe for concurrent callers,
 * e.g. Optuna's n_jobs=4 threads in reference train.py:86).
 *
 * Return codes: 0 = success; <0 = invalid argument (-k: k-th argument, LAPACK
 * style); >0 = a hipError_t from the launch. Per-window numerical status goes
 * to info[b] (see each function).
 */
#ifndef GPK_H_
#define GPK_H_
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library version (major*10000 + minor*100 + patch). */
int gpk_version(void);

/* Human-readable text for a return code of any gpk_* function. */
const char* gpk_strerror(int code);

/* Largest N the exact entry points accept: 800, GPyTorch's settings.max_cholesky_size (the
 * exact MLL leaves Cholesky for CG / Lanczos above it). N <= 256 runs the fused register /
 * LDS-resident kernels; 256 < N <= 800 the blocked kernels of gpk_exact_large.hip, which
 * factor in place in L (so L is required there) and need D <= 64. */
int gpk_exact_max_n(void);

/*
 * Exact GP marginal log likelihood, fused per window b in [0, B):
 *   K_hat = s2 * exp(-0.5*||(x_i - x_j)/l||^2) + noise * I
 *   L     = psd_safe_cholesky(K_hat) with the fp32 jitter ladder
 *           jitter * 10^t (t < max_tries), applied to failing windows only
 *   z     = L^{-1} (y - c)
 *   mll   = -0.5 * (|z|^2 + 2 sum_i log L_ii + N log 2pi) / N
 *
 * Replaces (reference): ExactGPModel.forward (denoising_model/GPModel.py:10-13)
 * + ExactMarginalLogLikelihood(likelihood, model)(output, y) — the canonical
 * GPyTorch partner of GPModel.py (upstream mlls/exact_marginal_log_likelihood.py,
 * linear_operator utils/cholesky.py::psd_safe_cholesky); SURVEY.md §8a rows a1-a7.
 *
 * X    : (B, N, D) float     y : (B, N) float
 * hyp  : device float[3 + n_lengthscale] =
 *        {outputscale s2, noise, mean_constant c, lengthscale[n_lengthscale]}
 *        (constrained values: softplus already applied by the caller)
 * n_lengthscale : 1 (GPModel.py:8) or D (ARD)
 * jitter, max_tries : ladder (GPyTorch defaults 1e-6 and 3 for fp32)
 * L    : (B, N, N) float out, lower factor with zeroed upper triangle; may be NULL for
 *        N <= 256 (required above: the blocked path's working storage, -10 if NULL)
 * z    : (B, N) float out; may be NULL
 * mll  : (B,) float out
 * info : (B,) int out: 0 = factored without jitter; -t = factored after t
 *        ladder steps (caller emits GPyTorch's NumericalWarning); k > 0 = still
 *        not positive definite at column k after max_tries (caller raises
 *        NotPSDError, or NanError if the inputs hold NaN).
 */
int gpk_exact_mll_f32(const float* X, const float* y, const float* hyp,
                      int n_lengthscale, int B, int N, int D, double jitter,
                      int max_tries, float* L, float* z, float* mll, int* info,
                      void* stream);

/*
 * Analytic backward of gpk_exact_mll_f32 (per window b, objective sum_b gout[b] mll[b]):
 *   G = gout (alpha alpha^T - K_hat^{-1}) / (2N),  alpha = K_hat^{-1} (y - c) = L^{-T} z
 *   dhyp[b] = {sum G o E, tr G, gout sum(alpha)/N, dl...}  (E = K / s2, l: 1 or D entries)
 *   dX = dK/dX contracted with G,  dy = -gout alpha / N
 * from the forward's L and z (nothing is refactored).
 *
 * Replaces (reference): the autograd backward that train.py:166 (loss.backward())
 * runs through GPyTorch's ExactMarginalLogLikelihood for ExactGPModel
 * (denoising_model/GPModel.py:5-13; upstream linear_operator inv_quad_logdet /
 * psd_safe_cholesky backward, kernels/rbf_kernel.py backward); SURVEY.md §8f row 1.
 *
 * L : (B, N, N) float, z : (B, N) float (gpk_exact_mll_f32 outputs)   gout : (B,) float
 * workspace : gpk_exact_grad_workspace_bytes(B, N) bytes of device memory (the lower block
 *             tiles of K_hat^{-1} per window, ~145 KB at N = 256, plus small vectors; for
 *             N > 256, L^{-1} and K_hat^{-1} as Np x Np each, Np = N rounded up to 32)
 * dX : (B, N, D) float out or NULL (D <= 64)   dy : (B, N) float out or NULL
 * dhyp : (B, 3 + n_lengthscale) float out (per window; the caller sums over b)
 */
size_t gpk_exact_grad_workspace_bytes(int B, int N);
int gpk_exact_mll_grad_f32(const float* X, const float* L, const float* z, const float* hyp,
                           int n_lengthscale, int B, int N, int D, const float* gout, void* workspace,
                           float* dX, float* dy, float* dhyp, void* stream);

/*
 * Exact-GP posterior at new inputs (eval mode), per window b, from the training
 * factor of gpk_exact_mll_f32 (nothing is refactored):
 *   K*   = s2 * exp(-0.5 ||(x_n - xs_t)/l||^2)       (N x Ns, training x test)
 *   V    = L^{-1} K*
 *   mean = c + V^T z          = c + K*^T K_hat^{-1} (y - c)
 *   var  = s2 - colsum(V o V) = diag(K** - K*^T K_hat^{-1} K*)   (latent f, unclamped)
 *
 * Replaces (reference): ExactGPModel in eval mode (denoising_model/GPModel.py:10-13;
 * SURVEY.md §3.3) -> upstream models/exact_gp.py __call__ ->
 * exact_prediction_strategies.py exact_predictive_mean / exact_predictive_covar (diag).
 *
 * X : (B, N, D) float training inputs   L : (B, N, N) float   z : (B, N) float
 * hyp : as gpk_exact_mll_f32   Xs : (B, Ns, D) float test inputs (D <= 64, N <= 800)
 * mean, var : (B, Ns) float out
 */
int gpk_exact_posterior_f32(const float* X, const float* L, const float* z, const float* hyp,
                            int n_lengthscale, const float* Xs, int B, int N, int Ns, int D,
                            float* mean, float* var, void* stream);

/*
 * Joint exact-GP posterior at new inputs (eval mode), per window b: gpk_exact_posterior_f32
 * plus the dense predictive covariance of the latent f, from the same training factor
 * (nothing is refactored):
 *   V    = L^{-1} K*                                  (K* as above; kept in the workspace)
 *   mean = c + V^T z,   var = s2 - colsum(V o V)      (bitwise those of gpk_exact_posterior_f32)
 *   cov  = K(xs, xs) - V^T V = K** - K*^T K_hat^{-1} K*,   K** = s2 * exp(-0.5 ||(xs_i - xs_j)/l||^2)
 * cov is symmetric bit for bit and its diagonal is var bit for bit. Two phases on `stream`: the
 * posterior kernel storing V, then one workgroup per 64 x 64 tile of the upper block triangle
 * (K** by a centred fp32-MFMA Gram, V^T V on fp32 MFMA in a fixed order; every product exact
 * fp32, no atomics: run-to-run deterministic).
 *
 * Replaces (reference): upstream exact_prediction_strategies.exact_predictive_covar (the full
 * matrix, not only its diagonal), reached from ExactGPModel in eval mode
 * (denoising_model/GPModel.py:10-13) through models/exact_gp.py __call__.
 *
 * Memory per call: the workspace, gpk_exact_posterior_cov_workspace_bytes(B, N, Ns) bytes
 * (B * N * Ns floats of V, Ns rounded up to 64, and 64 B floats: the training mean of x / l
 * that centres both Grams), plus the B * Ns^2 floats of cov.
 * The query returns 0 for a shape the call does not accept.
 *
 * X, L, z, hyp, n_lengthscale, Xs, mean, var : as gpk_exact_posterior_f32 (N <= 800, D <= 64)
 * workspace : device memory of the size above, 16-byte aligned
 * cov : (B, Ns, Ns) float out, dense
 * For N > 256 the blocked kernel keeps B on the grid's y dimension: B <= 65535 there (-7).
 */
size_t gpk_exact_posterior_cov_workspace_bytes(int B, int N, int Ns);
int gpk_exact_posterior_cov_f32(const float* X, const float* L, const float* z, const float* hyp,
                                int n_lengthscale, const float* Xs, int B, int N, int Ns, int D,
                                void* workspace, float* mean, float* var, float* cov, void* stream);

/*
 * Adjoint of gpk_exact_posterior_cov_f32, per window b: from the gradients of the objective with
 * respect to mean (gmean), var (gvar) and cov (gcov, ANY Ns x Ns matrix, not assumed symmetric),
 * each optional, the gradients with respect to the training inputs and targets, the test inputs
 * and the hyper-parameters. With G = gcov + diag(gvar), H = G + G^T, W = L^{-T} V = K_hat^{-1} K*,
 * alpha = L^{-T} z and u = W gmean:
 *   dK*  = -W H + alpha gmean^T       dK_hat = 1/2 W H W^T - 1/2 (u alpha^T + alpha u^T)
 *   dK** = 1/2 H       dy = u       dc = sum gmean - sum u       dnoise = tr dK_hat
 * and every block K = s2 E(a, b), a = x / l, gives with Q = dK o K (the diagonal of the two
 * square blocks apart)
 *   da_i = (Q b)_i - rowsum(Q)_i a_i      db_j = (Q^T a)_j - colsum(Q)_j b_j
 *   dl_d = -sum (a o da + b o db)_d / l_d       ds2 = sum Q / s2 + tr dK_hat + 1/2 tr H.
 * No Cholesky adjoint is involved; the jitter the ladder added is a constant. All three Grams are
 * centred by the forward's training mean of x / l (read from `state`), so no difference sees the
 * offset of the inputs. Every tile product runs on the fp32 MFMA with exact fp32 products; no
 * atomics, fixed summation orders: a second launch gives the same bits, and the outputs of a
 * window come from that window alone.
 *
 * Replaces (reference): torch autograd through upstream exact_prediction_strategies
 * (exact_predictive_mean / exact_predictive_covar), i.e. the backward of
 * model(x).mean / .variance / .covariance_matrix, rsample and log_prob of ExactGPModel in eval
 * mode (denoising_model/GPModel.py:10-13) when a gradient flows.
 *
 * Memory per call: the workspace, gpk_exact_posterior_grad_workspace_bytes(B, N, Ns, D) bytes
 * (W and T = W H, B * N * Ns floats each with Ns rounded up to 64; the per-column-block partials
 * of the training side, ceil(Ns / 64) * B * N * D' floats with D' = D rounded up to 16 / 32 / 64;
 * the gradients in scaled coordinates, B * (N + Ns) * D' floats). The query returns 0 for a shape
 * the call does not accept: 1 <= N <= 256, 1 <= Ns <= 256 (gpk_mvn_root_max_n), 1 <= D <= 64.
 *
 * X, L, z, hyp, n_lengthscale, Xs : as gpk_exact_posterior_cov_f32
 * state : the workspace of the gpk_exact_posterior_cov_f32 call on the same arguments, unchanged
 * gmean, gvar : (B, Ns) float or NULL   gcov : (B, Ns, Ns) float or NULL; at least one is given
 * workspace : device memory of the size above, 16-byte aligned
 * dX : (B, N, D), dy : (B, N), dXs : (B, Ns, D) float out, each may be NULL
 * dhyp : (B, 3 + n_lengthscale) float out, per window d/d{s2, noise, c, lengthscale...} in the
 *        layout of gpk_exact_mll_grad_f32 (the caller sums over b)
 * Returns -(argument index) for an invalid argument (-8 when gmean, gvar and gcov are all NULL);
 * B == 0 returns 0 and launches nothing.
 */
size_t gpk_exact_posterior_grad_workspace_bytes(int B, int N, int Ns, int D);
int gpk_exact_posterior_grad_f32(const float* X, const float* L, const float* z, const float* hyp,
                                 int n_lengthscale, const float* Xs, const float* state,
                                 const float* gmean, const float* gvar, const float* gcov,
                                 int B, int N, int Ns, int D, void* workspace,
                                 float* dX, float* dy, float* dXs, float* dhyp, void* stream);

/*
 * Per-window hyper-parameters: the five exact entry points above with one hyper vector PER
 * WINDOW, GPyTorch's batch-independent exact GP (batch_shape = [B] on the mean, the kernel and
 * the likelihood). Each takes its sibling's arguments plus `hyp_stride` directly after
 * n_lengthscale, the number of floats between two consecutive windows' hyper vectors:
 *   hyp_stride == 0 : hyp is one float[3 + n_lengthscale] shared by every window; the call IS the
 *                     sibling (the siblings are this call with hyp_stride 0), bit for bit
 *   hyp_stride >= 3 + n_lengthscale : hyp is (B, hyp_stride) row-major and window b reads row b,
 *                     hyp + b * hyp_stride = {s2, noise, c, lengthscale[n_lengthscale]}; floats of
 *                     a row past the vector are not read
 * Window b's kernel matrix, factor, jitter ladder, mll, posterior and gradients then depend on row
 * b alone. dhyp keeps its dense (B, 3 + n_lengthscale) layout: row b is the gradient with respect
 * to hyp row b, the same quantity the siblings write, only not meant to be summed over b (a
 * caller that shares some entries between windows sums those columns itself).
 * Workspace sizes and every other argument are those of the sibling, and so are the return codes
 * (argument indices count as in the sibling's list); any other hyp_stride returns minus its own
 * argument index, -5 from gpk_exact_mll_perwin_f32 and -6 from the other four, before anything is
 * launched.
 */
int gpk_exact_mll_perwin_f32(const float* X, const float* y, const float* hyp, int n_lengthscale,
                             long long hyp_stride, int B, int N, int D, double jitter, int max_tries,
                             float* L, float* z, float* mll, int* info, void* stream);
int gpk_exact_mll_grad_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                  int n_lengthscale, long long hyp_stride, int B, int N, int D,
                                  const float* gout, void* workspace, float* dX, float* dy, float* dhyp,
                                  void* stream);
int gpk_exact_posterior_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                   int n_lengthscale, long long hyp_stride, const float* Xs, int B, int N,
                                   int Ns, int D, float* mean, float* var, void* stream);
int gpk_exact_posterior_cov_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                       int n_lengthscale, long long hyp_stride, const float* Xs, int B, int N,
                                       int Ns, int D, void* workspace, float* mean, float* var, float* cov,
                                       void* stream);
int gpk_exact_posterior_grad_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                        int n_lengthscale, long long hyp_stride, const float* Xs,
                                        const float* state, const float* gmean, const float* gvar,
                                        const float* gcov, int B, int N, int Ns, int D, void* workspace,
                                        float* dX, float* dy, float* dXs, float* dhyp, void* stream);

/*
 * Appending observations to a cached exact-GP factor, per window b: from the training factor L
 * and z = L^{-1}(y - c) of gpk_exact_mll_f32 and m new points (Xn, yn), the factor and whitened
 * targets of the N' = N + m concatenated points, in O(N^2 m) (nothing is refactored):
 *   V  = L^{-1} K(X, Xn)                                   (N x m)
 *   S  = K(Xn, Xn) + (noise + jitter) I - V^T V            (m x m, the Schur complement)
 *   R  = chol(S)        zn = R^{-1} (yn - c - V^T z)
 *   L' = [[L, 0], [V^T, R]]        z' = [z ; zn]
 * By the uniqueness of the Cholesky factor these are what gpk_exact_mll_f32 returns for
 * ([X ; Xn], [y ; yn]) up to rounding, so every consumer of (L, z) takes them unchanged
 * (gpk_exact_posterior_f32, gpk_exact_posterior_cov_f32, a further gpk_exact_append_f32).
 * L'[:N, :N] and z'[:N] are bit-exact copies of the inputs. One launch chain on `stream`: the
 * joint posterior's two phases at Xn (V, S), the noise of the window's own hyper vector onto
 * S's diagonal, gpk_mvn_root_f32's factorisation, gpk_tri_solve_f32, and one memory-bound
 * finish that assembles L' (16-byte stores; V^T through an LDS transpose). One rung of
 * psd_safe_cholesky's ladder: there is no retry inside, the caller relaunches the whole batch
 * with jitter * 10^t as for gpk_mvn_root_f32. Fixed order, no atomics: deterministic.
 *
 * Replaces (reference): upstream models/exact_gp.py ExactGP.get_fantasy_model ->
 * exact_prediction_strategies.py get_fantasy_strategy (the low-rank update of the cached
 * training factor and mean cache), for ExactGPModel (denoising_model/GPModel.py:4-13).
 *
 * Memory per call: the workspace, gpk_exact_append_workspace_bytes(B, N, m) bytes (that of
 * gpk_exact_posterior_cov_f32 at Ns = m, plus B (2 m^2 + 4 m) floats: S, R, the posterior mean
 * and variance at Xn, the residual and zn), plus the outputs. The query returns 0 for a shape
 * the call does not accept: 1 <= N, 1 <= m <= gpk_mvn_root_max_n() = 256,
 * N + m <= gpk_exact_max_n() = 800, B <= 65535 when N > 256 (the blocked phase 1).
 *
 * X, L, z, hyp, n_lengthscale : as gpk_exact_posterior_cov_f32 (1 <= D <= 64)
 * Xn : (B, m, D) float   yn : (B, m) float   jitter : >= 0, added to S's diagonal beside the noise
 * workspace : device memory of the size above, 16-byte aligned
 * Lout : (B, N + m, N + m) float out, the full square, upper triangle exactly zero
 * zout : (B, N + m) float out
 * info : (B,) int out. 0 = factored; k > 0 = pivot k (1-based) of the Schur complement was not
 *        positive or was NaN: the new rows of Lout[b] and zout[b] then hold NaN
 * Returns -(argument index) for an invalid argument (a rejected m or N + m: -10); B == 0 returns 0
 * and launches nothing. gpk_exact_append_perwin_f32 takes hyp_stride after n_lengthscale as the
 * other *_perwin_f32 entry points (-6 for a bad stride); stride 0 is gpk_exact_append_f32, bit
 * for bit.
 */
size_t gpk_exact_append_workspace_bytes(int B, int N, int m);
int gpk_exact_append_f32(const float* X, const float* L, const float* z, const float* hyp, int n_lengthscale,
                         const float* Xn, const float* yn, int B, int N, int m, int D, float jitter,
                         void* workspace, float* Lout, float* zout, int* info, void* stream);
int gpk_exact_append_perwin_f32(const float* X, const float* L, const float* z, const float* hyp,
                                int n_lengthscale, long long hyp_stride, const float* Xn, const float* yn,
                                int B, int N, int m, int D, float jitter, void* workspace, float* Lout,
                                float* zout, int* info, void* stream);

/*
 * Dropping the m oldest observations from a cached exact-GP factor, per window b: from the training
 * factor L and z = L^{-1}(y - c) of gpk_exact_mll_f32 / gpk_exact_append_f32, the factor and
 * whitened targets of the last n = N - m points, in O(n^2 m) (nothing is refactored). With
 *   L = [[L11, 0], [L21, L22]]     z = [z1 ; z2]     U = L21 (n x m)
 * the kept points' matrix is L22 L22^T + U U^T (whatever jitter the ladder put on the diagonal
 * included), so L' = chol(L22 L22^T + U U^T), a positive rank-m update, run as rotations: for
 * column j and t = 0 .. m-1, with rho_t^2 = L_jj^2 + sum_{s<=t} U_js^2,
 *   cos_t = rho_{t-1} / rho_t    sin_t = U_jt / rho_t
 *   (L_ij, U_it) <- (cos_t L_ij + sin_t U_it, cos_t U_it - sin_t L_ij)    for every row i > j
 * and L'_jj = rho_{m-1}; the same rotations on the pairs (z2_j, z1_t) leave z' = L'^{-1}(y[m:] - c)
 * in z2's place. By the uniqueness of the Cholesky factor these are what gpk_exact_mll_f32 returns
 * for (X[:, m:], y[:, m:]) at the same total jitter, up to rounding, so every consumer of (L, z)
 * takes them unchanged, gpk_exact_append_f32 included: drop m, append m keeps N constant and a
 * look-back window slides over a stream with no factorisation launch. It replaces a refit of the
 * kept points (gpk_exact_mll_f32, O(n^3)).
 *
 * Replaces (reference): nothing upstream. GPyTorch has no counterpart: this is the inverse of
 * exact_prediction_strategies.py get_fantasy_strategy's low-rank update, for ExactGPModel
 * (denoising_model/GPModel.py:4-13) on a streaming look-back.
 *
 * Neither X, y nor the hyper-parameters enter: there is no hyp argument, no workspace and no
 * _perwin twin. A positive update has no failing pivot: there is no info; a NaN in window b's
 * inputs gives NaN in window b's outputs only. One workgroup per window (B on gridDim.x), one
 * thread per row, workgroup barriers only; m > 32 runs as two exact updates of rank 32 and m - 32,
 * the second in place on Lout. Memory per call: the outputs only. Fixed order, no atomics, a
 * window's outputs depend on that window alone: deterministic, and independent of B.
 *
 * L : (B, N, N) float, lower factor, upper triangle not read     z : (B, N) float
 * Limits: 1 <= m <= gpk_exact_drop_max_m() = 64, m < N <= gpk_exact_max_n() = 800
 * Lout : (B, N - m, N - m) float out, the full square, upper triangle exactly zero
 * zout : (B, N - m) float out; neither output may overlap L or z (-6 / -7)
 * Returns -(argument index) for an invalid argument (a rejected m: -5); B == 0 returns 0 and
 * launches nothing.
 */
int gpk_exact_drop_max_m(void);
int gpk_exact_drop_f32(const float* L, const float* z, int B, int N, int m, float* Lout, float* zout,
                       void* stream);

/*
 * Shared inducing-point factorisation of the whitened VariationalStrategy:
 *   A    = K_ZZ + jitter (fp32 add, as K_ZZ.add_jitter), then upcast to fp64
 *   L    = psd_safe_cholesky(A) with the fp64 ladder chol_jitter * 10^t
 *   Linv = L^{-1}
 * K_ZZ = s2 * exp(-0.5 ||(z_i - z_j)/l||^2) with ARD lengthscales (GPyTorch's centred
 * GEMM-form squared distance, diagonal not zeroed: Z requires grad in the reference).
 * Factor: ONE workgroup (16 waves: 15 hold the upper triangle as fp64-MFMA register tiles,
 * a diagonal wave factors each 16 x 16 diagonal block one step ahead; 16-column right-looking
 * steps; the fp64 ladder restarted in-kernel); inverse: one workgroup per 16-column block
 * column (block forward substitution on fp64 MFMA), the block columns on different CUs.
 *
 * Replaces (reference): the per-window (b-fold redundant) fp64 Cholesky that
 * VariationalStrategy._cholesky_factor runs for ToyDeepGPHiddenLayer
 * (denoising_model/DeepGP.py:33-38, inducing points expanded to the batch by
 * upstream _expand_inputs); SURVEY.md §8a rows a7/a9.
 *
 * Z   : (M, D) float (M <= 256, D <= 64)     hyp : device float[1 + D] = {s2, lengthscale[D]}
 * L, Linv : (M, M) double out (lower, zero upper)   info : (1,) int out, codes as above
 */
int gpk_kzz_chol_f64(const float* Z, const float* hyp, int M, int D, float jitter,
                     double chol_jitter, int max_tries, double* L, double* Linv, int* info,
                     void* stream);

/*
 * Adjoint of gpk_kzz_chol_f64, once per optimizer step for all GP calls that shared the
 * factor (fp64 throughout):
 *   Lbar = -tril(Linv^T G Linv^T),  S = Linv^T Phi(L^T Lbar) Linv,  Kbar = (S + S^T)/2
 *   (Phi = lower triangle with the diagonal halved), then the RBF adjoint over K_ZZ
 *   (without its jitter): W = Kbar o K, dZ = 2 (W zs - zs o W1)/l, dl, ds2 = sum W / s2.
 * Five fp64-MFMA tile GEMM launches + a W-tile kernel + one fixed-order reduction
 * (run-to-run deterministic).
 *
 * Replaces (reference): the autograd backward of psd_safe_cholesky + the triangular solve
 * inside upstream VariationalStrategy (denoising_model/DeepGP.py:33-38) that train.py:166
 * runs -- b times per GP call in the reference (Z expanded over the batch), once per step
 * here; SURVEY.md §8f rows 1 and 3.
 *
 * dLinv : (M, M) double, lower (G = dObjective/dLinv)   L, Linv : gpk_kzz_chol_f64 outputs
 * Z : (M, D) float   hyp : device float[1 + D] = {s2, lengthscale[D]} (as gpk_kzz_chol_f64)
 * workspace : gpk_kzz_backward_workspace_bytes(M, D) bytes of device memory
 * dZ : (M, D) float out    dhyp : (1 + D) float out = {ds2, dlengthscale[D]}
 */
size_t gpk_kzz_backward_workspace_bytes(int M, int D);
int gpk_kzz_backward_f64(const double* dLinv, const double* L, const double* Linv, const float* Z,
                         const float* hyp, int M, int D, void* workspace, float* dZ, float* dhyp,
                         void* stream);

/*
 * ELBO terms of the variational path, one launch each way (fixed-order sums):
 *   ell_r = sum_i -0.5 [((y_ri - mean_ri)^2 + var_ri) / noise + log noise + log 2 pi]
 *   kl    = 0.5 [sum s^2 + sum m^2 - M - sum log s^2]         (whitened mean-field q(u))
 * gpk_gauss_ell_grad_f32: for the objective sum_r gell_r ell_r -> dy, dmean, dvar (each
 * (R, N) or NULL) and dnoise_part (R,) per-row partials of d/dnoise (or NULL).
 * gpk_meanfield_kl_f32: gkl == NULL -> kl (1,) out; else the backward dm = gkl m,
 * ds = gkl (s - 1/s).
 *
 * Replaces (reference): upstream GaussianLikelihood.expected_log_prob (summed over the
 * points by VariationalELBO._log_likelihood_term) and
 * MeanFieldVariationalDistribution.kl_divergence, as the ELBO at forecast_denoising.py:86-89
 * evaluates them, and their autograd backward (train.py:166); SURVEY.md §8a row a14.
 *
 * y, mean, var : (R, N) float;  noise : device float[1];  ell, gell : (R,) float
 * m, s : (M,) float (variational mean / stddev);  kl, gkl : (1,) float
 */
int gpk_gauss_ell_f32(const float* y, const float* mean, const float* var, const float* noise, int R,
                      int N, float* ell, void* stream);
int gpk_gauss_ell_grad_f32(const float* y, const float* mean, const float* var, const float* noise,
                           const float* gell, int R, int N, float* dy, float* dmean, float* dvar,
                           float* dnoise_part, void* stream);
int gpk_meanfield_kl_f32(const float* m, const float* s, int M, float* kl, const float* gkl,
                         float* dm, float* ds, void* stream);

/*
 * The per-row ELBO of VariationalELBO (combine_terms, one whitened mean-field layer) in one
 * launch each way:
 *   elbo_r = ell_r / N - kl_scale * KL(N(m, diag s^2) || N(0, I)),  kl_scale = beta / num_data
 *   ell_r  = sum_i -0.5 [((y_ri - mean_ri)^2 + var_ri) / noise + log noise + log 2 pi]
 * Rows r of y / mean / var start at r * ld (ld >= N: a point slice of a joint output needs no
 * copy). clamp_flag (or NULL): set to 1 if any var_ri <= min_var (the kernel-clamped entries:
 * MultivariateNormal.variance's NumericalWarning). The backward (objective sum_r g_r elbo_r)
 * writes dmean, dvar (R, N contiguous), per-row d/dnoise partials and dm, ds (M). R = 0 is
 * accepted by both (the forward writes nothing; the backward zero-fills dm and ds).
 *
 * Replaces (reference): DeepApproximateMLL(VariationalELBO(likelihood, model, num_data=d))
 * at forecast_denoising.py:86-89 (upstream mlls/variational_elbo.py +
 * _approximate_mll.py: expected_log_prob(...).sum(-1).div(N) - kl.div(num_data / beta))
 * and its autograd backward (train.py:166); SURVEY.md §8a row a14.
 */
int gpk_variational_elbo_f32(const float* y, long long ldy, const float* mean, long long ldm,
                             const float* var, long long ldv, const float* noise, const float* m,
                             const float* s, int M, int R, int N, float kl_scale, float min_var,
                             float* elbo, int* clamp_flag, void* stream);
int gpk_variational_elbo_grad_f32(const float* y, long long ldy, const float* mean, long long ldm,
                                  const float* var, long long ldv, const float* noise, const float* m,
                                  const float* s, int M, int R, int N, float kl_scale, const float* gelbo,
                                  float* dmean, float* dvar, float* dnoise_part, float* dm, float* ds,
                                  void* stream);

/*
 * Condensed verdict of one host-side numerical check inside a captured HIP graph
 * (graphs.GraphedStep): kind 0 = a psd_safe_cholesky info vector (n entries; in0 / in1 =
 * the factorised inputs, scanned for NaN only when a factorisation failed), kind 1 = the
 * variance-clamp flag word, kind 2 = end of the step (advance the replay counter).
 *   ring[(counter % slots) * items + item] = {max info, max(-info, 0), NaN in the inputs}
 *   sticky |= (max info > 0)
 * so the host reads the verdicts of a block of replays with one copy and warns / raises
 * per replay exactly as GPyTorch's eager psd_safe_cholesky / MultivariateNormal.variance
 * checks (linear_operator utils/cholesky.py).
 * ring : (slots, items, 3) int device;  counter : (1,) int64 device;  sticky : (1,) int device
 */
int gpk_record_check(const int* info, int n, const float* in0, long long n0, const float* in1,
                     long long n1, int kind, int* ring, long long* counter, int slots, int item,
                     int items, int* sticky, void* stream);

/*
 * Batched variational predictive distribution and expected log likelihood:
 *   K_ZX = s2 * exp(-0.5 ||(z_m - x_i)/l||^2)       (fp32, GPyTorch's centred GEMM form)
 *   A    = Linv @ K_ZX                              (fp64, then cast to fp32)
 *   mean = A^T m + x @ w + b0                       (LinearMean)
 *   var  = max(s2 + jitter + sum_m A_mi^2 (s_m^2 - 1), 1e-6)
 *   ell  = sum_i -0.5 [((y_i - mean_i)^2 + var_i)/noise + log noise + log 2pi]
 *
 * Replaces (reference): DeepGPp.predict / ToyDeepGPHiddenLayer.__call__
 * (denoising_model/DeepGP.py:51-99) via upstream VariationalStrategy.forward,
 * DeepGPLayer.__call__, GaussianLikelihood.expected_log_prob as used by
 * denoise_model_2.add_gp_noise (denoise_model_2.py:32-40) and the ELBO at
 * forecast_denoising.py:86-89; SURVEY.md §8a rows a9-a14.
 *
 * X : (B, N, D) float (D <= 64)  Z : (M, D)  Linv : (M, M) double (gpk_kzz_chol_f64)
 * vmean, vstd : (M,) float (MeanFieldVariationalDistribution mean / stddev)
 * hyp : device float[4 + 2D] = {s2, noise, jitter, bias, weights[D], lengthscale[D]}
 * y : (B, N) float or NULL;  mean, var : (B, N) float out;  ell : (B,) float out or NULL
 * (needs y)   flags : (1,) int out or NULL: bit 0 set when the variance clamp fired
 * (the caller emits GPyTorch's NumericalWarning from MultivariateNormal.variance).
 */
int gpk_variational_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                        const float* vstd, const float* hyp, const float* y, int B, int N, int M,
                        int D, float* mean, float* var, float* ell, int* flags, void* stream);

/*
 * Adjoint of gpk_variational_f32 for the objective sum(gmean * mean) + sum(gvar * var)
 * (var's clamp at 1e-6 passes no gradient), everything but the K_ZZ factor:
 *   dA    = gmean_i m_m + 2 gvar_i (s_m^2 - 1) A_mi         (fp32, as the reference's dA)
 *   dK    = Linv^T dA,  Q = dK o K_ZX
 *   dX    (B, N, D) float out: RBF adjoint + gmean_i w
 *   dLinv (M, M) double out: sum over all points of dA K_ZX^T (lower, upper zero) -- the
 *         caller back-propagates it through the shared K_ZZ factor once per step
 *   dZ    (M, D) float out: the K_ZX part of dZ
 *   dpar  (2M + 2D + 2) float out: {dvmean (M), dvstd (M), ds2 (K_ZX and variance parts),
 *         dl (D, K_ZX part), dweights (D), dbias}  (LinearMean: dweights = X^T gmean)
 * workspace : gpk_variational_adjoint_workspace_bytes(B, N, M, D) bytes of device memory.
 * All sums are in a fixed order (run-to-run deterministic).
 *
 * Replaces (reference): the autograd backward that train.py:166 runs through
 * VariationalStrategy / DeepGPLayer for DeepGPp (denoising_model/DeepGP.py:51-99,
 * forecast_denoising.py:86-104); SURVEY.md §8f row 1.
 */
size_t gpk_variational_adjoint_workspace_bytes(int B, int N, int M, int D);
int gpk_variational_adjoint_f32(const float* X, const float* Z, const double* Linv,
                                const float* vmean, const float* vstd, const float* hyp,
                                const float* gmean, const float* gvar, int B, int N, int M, int D,
                                void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                void* stream);

/*
 * Training pair of the variational path for M > 64 (the reference's DeepGP default M = 256,
 * denoising_model/DeepGP.py:15): the forward keeps state the adjoint consumes, so the adjoint
 * neither repeats the forward's A = Linv K_ZX GEMM nor round-trips dA / K_ZX through HBM.
 *   gpk_variational_saved_bytes(B, N, M, D): bytes of that state; 0 when the shape is served
 *     by the recompute adjoint only (M <= 64, or the saved path's LDS plan does not fit).
 *   gpk_variational_train_f32: gpk_variational_f32 + `saved` (device, saved_bytes bytes; may be
 *     NULL only when saved_bytes is 0, else -16): A (fp32, as the reference casts it) and the
 *     variance clamp mask of every point.
 *   gpk_variational_adjoint_saved_f32: gpk_variational_adjoint_f32 from that state (same
 *     outputs, same argument meaning; saved = argument 9, -12 when saved_bytes is 0 for the
 *     shape), workspace of gpk_variational_adjoint_saved_workspace_bytes(B, N, M, D) bytes.
 *     dLinv = sum_i dA_i K_i^T is formed as m u^T + 2 diag(s^2 - 1) G' with u = K_ZX gmean and
 *     G' = A diag(gvar) K_ZX^T on the saved fp32 A (products exact on f32 MFMA), i.e. the
 *     reference's own fp32 dA, without a dA / K_ZX workspace.
 * Replaces (reference): the same forward / autograd backward as the two functions above.
 */
size_t gpk_variational_saved_bytes(int B, int N, int M, int D);
int gpk_variational_train_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                              const float* vstd, const float* hyp, const float* y, int B, int N, int M,
                              int D, float* mean, float* var, float* ell, int* flags, void* saved,
                              void* stream);
size_t gpk_variational_adjoint_saved_workspace_bytes(int B, int N, int M, int D);
int gpk_variational_adjoint_saved_f32(const float* X, const float* Z, const double* Linv,
                                      const float* vmean, const float* vstd, const float* hyp,
                                      const float* gmean, const float* gvar, const void* saved, int B,
                                      int N, int M, int D, void* workspace, float* dX, double* dLinv,
                                      float* dZ, float* dpar, void* stream);

/*
 * Multi-output (batched) variational chain: O independent GPs of one DeepGP layer
 * (output_dims = O: inducing points (O, M, D), q(u) batch (O,), kernel hyper-parameters per
 * output) in ONE launch of every kernel -- the output index on grid dimension y, each
 * output's workgroups exactly those of the single-output function at the same (B, N, M, D),
 * so every result is bit-identical to O single-output calls. Every array of the
 * single-output functions gains a dense leading O; 1 <= O <= 65535 (gridDim.y), B, N, M, D
 * limited as there.
 *
 * Replaces (reference): ToyDeepGPHiddenLayer with output_dims = O
 * (denoising_model/DeepGP.py:24-31: inducing points (O, M, D), batch_shape [O] on the
 * variational distribution, mean and kernel) through upstream VariationalStrategy with a
 * batch of GPs, and its autograd backward (train.py:166); SURVEY.md §8a rows a7-a11.
 *
 *   gpk_kzz_chol_f64_batched: gpk_kzz_chol_f64 per output -- O factor workgroups in one
 *     launch (one CU each), T x O inverse workgroups in a second; the fp64 jitter ladder
 *     restarts per output and reports in info[o].
 *     Z : (O, M, D)   hyp : (O, 1 + D)   L, Linv : (O, M, M) double out   info : (O,) int out
 *   gpk_kzz_backward_f64_batched: gpk_kzz_backward_f64 per output, each of its launches once.
 *     dLinv, L, Linv : (O, M, M)   Z : (O, M, D)   hyp : (O, 1 + D)
 *     workspace : gpk_kzz_backward_batched_workspace_bytes(O, M, D) bytes (O slices; 0 for an
 *     unsupported shape)   dZ : (O, M, D) out   dhyp : (O, 1 + D) out
 */
int gpk_kzz_chol_f64_batched(const float* Z, const float* hyp, int O, int M, int D, float jitter,
                             double chol_jitter, int max_tries, double* L, double* Linv, int* info,
                             void* stream);
size_t gpk_kzz_backward_batched_workspace_bytes(int O, int M, int D);
int gpk_kzz_backward_f64_batched(const double* dLinv, const double* L, const double* Linv,
                                 const float* Z, const float* hyp, int O, int M, int D, void* workspace,
                                 float* dZ, float* dhyp, void* stream);

/*
 * gpk_variational_f32 / gpk_variational_train_f32 and their adjoints for O outputs at once
 * (no y / ell: the ELBO terms of a multi-output layer are formed by the caller).
 *   X : (B, N, D) read by every output when shared_x != 0 (the layer's own case: DeepGPLayer
 *       expands its input over O with stride 0, so no (O, B, N, D) copy is made), else
 *       (O, B, N, D)
 *   Z : (O, M, D)   Linv : (O, M, M) double   vmean, vstd : (O, M)   hyp : (O, 4 + 2D)
 *   mean, var : (O, B, N) float out   flags : (1,) int out or NULL, every output ORs into it
 *   saved : NULL (inference forward / recompute adjoint) or O x
 *       gpk_variational_saved_bytes(B, N, M, D) bytes (training forward; the adjoint then runs
 *       from that state); non-NULL at a shape whose saved size is 0 is an argument error
 *       (forward -16, adjoint -10)
 *   gmean, gvar : (O, B, N)
 *   workspace : gpk_variational_adjoint_batched_workspace_bytes(O, B, N, M, D, has_saved)
 *       bytes, O slices of the single-output query (the saved-state one when has_saved != 0);
 *       0 for an unsupported shape
 *   dX : (O, B, N, D) float out, per output also with shared inputs (the caller sums over O)
 *   dLinv : (O, M, M) double out   dZ : (O, M, D) out   dpar : (O, 2M + 2D + 2) out
 * All sums keep the single-output order (run-to-run deterministic).
 *
 * Replaces (reference): DeepGPLayer.__call__ / VariationalStrategy.forward for
 * ToyDeepGPHiddenLayer(output_dims = O) (denoising_model/DeepGP.py:24-31, 42-49) and the
 * autograd backward train.py:166 runs through it; SURVEY.md §8a rows a9-a11, §8f row 1.
 */
int gpk_variational_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                const float* vmean, const float* vstd, const float* hyp, int O, int B,
                                int N, int M, int D, float* mean, float* var, int* flags, void* saved,
                                void* stream);
size_t gpk_variational_adjoint_batched_workspace_bytes(int O, int B, int N, int M, int D, int has_saved);
int gpk_variational_adjoint_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                        const float* vmean, const float* vstd, const float* hyp,
                                        const float* gmean, const float* gvar, const void* saved, int O,
                                        int B, int N, int M, int D, void* workspace, float* dX,
                                        double* dLinv, float* dZ, float* dpar, void* stream);

/*
 * Dense predictive covariance of the variational q(f) (eval mode), per window b, from the
 * shared K_ZZ factor of gpk_kzz_chol_f64:
 *   K_ZX = s2 * exp(-0.5 ||(z_m - x_i)/l||^2)        (fp32, the arithmetic of gpk_variational_f32)
 *   A    = Linv K_ZX                                  (fp64 MFMA, cast to fp32; kept in the workspace)
 *   cov  = K_XX + jitter I + A^T diag(vstd^2 - 1) A   (N x N)
 *   K_XX = s2 * exp(-0.5 d2) with upstream _sq_dist semantics for x1 == x2: inputs / l centred
 *          by the window's mean, d2 clamped at 0, diagonal exactly 0 (K_ii = s2)
 * The diagonal is the unclamped variance s2 + jitter + sum_m A_mi^2 (vstd_m^2 - 1). cov is
 * symmetric bit for bit. Two phases on `stream`: one workgroup per (window, 64-point column
 * block) storing A and the window's mean of x / l, then one workgroup per 64 x 64 tile of the
 * upper block triangle (the variational mode of the exact posterior's covariance kernel: the
 * weight vstd_m^2 - 1 folded into one operand, fp32 MFMA in a fixed order, no atomics:
 * run-to-run deterministic).
 *
 * Replaces (reference): upstream variational/variational_strategy.py forward's
 * predictive_covar (SumLinearOperator(data_data_covar.add_jitter, MatmulLinearOperator(...)))
 * evaluated densely, as MultivariateNormal.rsample / covariance_matrix of a DeepGP layer
 * output do (denoising_model/DeepGP.py:62-64 ``x.rsample()`` of a layer fed with a skip input).
 *
 * Memory per call: the workspace, gpk_variational_cov_workspace_bytes(B, N, M) bytes (B * M * N
 * floats of A, N rounded up to 64, and 64 B floats of means), plus the B * N^2 floats of cov.
 * The query returns 0 for a shape the call does not accept.
 *
 * X : (B, N, D) float   Z : (M, D) float   Linv : (M, M) double   vstd : (M,) float
 * hyp : as gpk_variational_f32 {s2, noise, jitter, bias, weights[D], lengthscale[D]}; noise,
 *       bias and weights are not read
 * M <= 256, D <= 64, N >= 1, B >= 0   workspace : device memory of the size above, 16-byte aligned
 * cov : (B, N, N) float out, dense
 *
 * The batched call runs O outputs (independent GPs of a multi-output layer) with o on a grid
 * dimension: leading dense O on Z, Linv, vstd, hyp and cov; X (B, N, D) read by every output
 * (shared_x != 0) or (O, B, N, D); the workspace is O slices of the single-output query.
 * Output o is bit-identical to a single-output call on output o's arrays.
 */
size_t gpk_variational_cov_workspace_bytes(int B, int N, int M);
int gpk_variational_cov_f32(const float* X, const float* Z, const double* Linv, const float* vstd,
                            const float* hyp, int B, int N, int M, int D, void* workspace,
                            float* cov, void* stream);
size_t gpk_variational_cov_batched_workspace_bytes(int O, int B, int N, int M);
int gpk_variational_cov_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                    const float* vstd, const float* hyp, int O, int B, int N, int M,
                                    int D, void* workspace, float* cov, void* stream);

/*
 * Adjoint of gpk_variational_cov_f32: from g = dObjective / dcov (B, N, N; any matrix, H = g + g^T
 * is formed inside) and the forward's workspace (A = Linv K_ZX in fp32 and the windows' means of
 * x / l, which the caller keeps as the saved state instead of a second fp64 product), with
 * w_m = vstd_m^2 - 1:
 *   T = A H     dvstd_m = vstd_m sum_b sum_i T_mi A_mi     dA = diag(w) T
 *   dLinv = tril(sum_b dA K_ZX^T)                           (fp64, lower, upper triangle zero:
 *                                                            gpk_variational_adjoint_f32's convention)
 *   Q = (Linv^T dA) o K_ZX   and the RBF tail of K_ZX:  dZ, dX, dlengthscale, ds2
 *   P = H o K_XX (K_ii = s2 exactly, no dX from the diagonal):  dX, dlengthscale, ds2
 * Every difference z - x, x_i - x_j is formed from the values the forward centred (Z / l by its
 * column means, x / l by the window's mean). The jitter has no gradient, nor has the clamp of the
 * squared distance at 0. Linv^T dA runs on the fp32 MFMA (Linv cast on load), dLinv is accumulated
 * on the fp64 MFMA; all partial sums are reduced in fp64 in a fixed order, no atomics: run-to-run
 * deterministic; a window's dX depends on that window alone. Six launches on `stream`, no host
 * synchronisation; allocates nothing and keeps no pointers.
 *
 * Replaces (reference): the autograd backward of upstream variational/variational_strategy.py
 * forward's predictive_covar evaluated densely, which train.py:166 ``loss.backward()`` runs
 * through the skip-input draw of denoising_model/DeepGP.py:62-64 ``x.rsample()``.
 *
 * Memory per call: the workspace, gpk_variational_cov_grad_workspace_bytes(B, N, M, D) bytes
 * (2 B M N floats for dA and K_ZX, N rounded up to 64, min(B, 32) M^2 doubles of dLinv partials
 * and a few KiB per workgroup of the other partials); 0 for a shape the call does not accept.
 * The saved state is the forward's workspace: B * M * as * 4 + 256 B bytes, as = N rounded up to 64.
 *
 * X, Z, Linv, vstd, hyp : as gpk_variational_cov_f32   state : the workspace that call filled for
 * the same arguments, 16-byte aligned   gcov : (B, N, N) float
 * workspace : device memory of the size above, 16-byte aligned
 * dX : (B, N, D) float out   dLinv : (M, M) double out   dZ : (M, D) float out (the K_ZX part)
 * dpar : (M + 1 + D) float out = {dvstd[M], ds2, dlengthscale[D]}
 * M <= 256, D <= 64, 1 <= N <= 256 (the bound of gpk_mvn_root_f32), B >= 0 (B = 0 launches nothing).
 *
 * The batched call runs O outputs with o on grid dimension y of every launch: leading dense O on
 * Z, Linv, vstd, hyp, state (the batched forward's workspace), gcov, dLinv, dZ, dpar and dX
 * ((O, B, N, D) also with shared inputs: the caller sums over O); the workspace is O slices of
 * the single-output query. Output o is bit-identical to a single-output call on o's arrays.
 */
size_t gpk_variational_cov_grad_workspace_bytes(int B, int N, int M, int D);
int gpk_variational_cov_grad_f32(const float* X, const float* Z, const double* Linv, const float* vstd,
                                 const float* hyp, const void* state, const float* gcov, int B, int N,
                                 int M, int D, void* workspace, float* dX, double* dLinv, float* dZ,
                                 float* dpar, void* stream);
size_t gpk_variational_cov_grad_batched_workspace_bytes(int O, int B, int N, int M, int D);
int gpk_variational_cov_grad_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                         const float* vstd, const float* hyp, const void* state,
                                         const float* gcov, int O, int B, int N, int M, int D,
                                         void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                         void* stream);

/*
 * Variational predictive distribution with a Cholesky (full-covariance) q(u) = N(m, L_q L_q^T),
 * whitened (prior N(0, I)), L_q = tril(C) of the parameter C = chol_variational_covar: the strict
 * upper triangle of C is never read, its diagonal may be negative. Per window b:
 *   K_ZX, A = Linv K_ZX                              exactly as gpk_variational_f32 (fp64, cast to fp32)
 *   W    = L_q^T A                                   (M, N), fp32 MFMA
 *   mean = A^T m + x @ w + b0
 *   var  = max(s2 + jitter - sum_m A_mi^2 + sum_m W_mi^2, 1e-6)      flags bit 0: the clamp fired
 * and the adjoint for the objective sum(gmean * mean) + sum(gvar * var), gvar zeroed where the
 * clamp fired, everything but the K_ZZ factor:
 *   dA = gmean_i m + 2 gvar_i (L_q w_i - a_i)        dvmean = sum_{b,i} gmean_i a_i
 *   dchol = 2 tril(sum_{b,i} gvar_i a_i w_i^T)       (M, M) float, lower, upper triangle zero
 *   dLinv = tril(sum dA K_ZX^T) (fp64, lower, upper zero), Q = (Linv^T dA) o K_ZX and the RBF tail
 *   dX (RBF adjoint + gmean_i w), dZ (the K_ZX part), dl, ds2 (K_ZX part + sum of the unclamped
 *   gvar), dweights = X^T gmean, dbias = sum gmean
 *   dpar : (M + 2 D + 2) float = {dvmean[M], ds2, dlengthscale[D], dweights[D], dbias}
 * The forward runs one workgroup per (window, 64-point block): fp64 MFMA for A, fp32 MFMA for W
 * with L_q staged through LDS in 16-row panels, its zero tiles skipped. With `saved` (training)
 * it keeps A as (B, M, as) floats, as = N rounded up to 64, and the clamp mask (B, as); the
 * adjoint reads A from there, recomputes W, and from dA on runs the q / dlinv / reduce / finish
 * kernels of gpk_variational_cov_grad_f32 on a dA it materialises in their workspace. Seven
 * launches and two memsets on `stream`, no host synchronisation, no atomics in any sum, fixed
 * summation orders: two calls give the same bits; a window's mean / var / dX depend on that
 * window alone.
 *
 * gpk_cholesky_kl_f32: KL(q || N(0, I)) = 1/2 [|L_q|_F^2 + |m|^2 - M - sum_k log(L_q,kk^2)], one
 * launch each way (gkl == NULL: kl (1,) out; else dm = gkl m, dchol = gkl (tril(C) - diag(1 / C_kk)),
 * upper triangle zero), the M^2 sum in fp64 in a fixed order.
 *
 * Replaces (reference): upstream variational/cholesky_variational_distribution.py (forward:
 * CholLinearOperator of the masked chol_variational_covar) inside
 * variational/variational_strategy.py forward, and _variational_strategy.py::kl_divergence
 * (torch.distributions.kl of the two MVNs), reached from denoising_model/DeepGP.py:28-38 when the
 * distribution class is swapped for CholeskyVariationalDistribution; and their autograd backward.
 *
 * Memory per call: saved = gpk_variational_chol_saved_bytes(B, N, M, D) = (B M as + B as) * 4 bytes;
 * the adjoint's workspace = gpk_variational_chol_adjoint_workspace_bytes(B, N, M, D): the
 * gpk_variational_cov_grad_f32 workspace (dA and K_ZX, 2 B M as floats, and its partials) + B M as
 * floats of W diag(gvar) + min(B, 32) M^2 doubles of dchol partials + B ceil(N / 64) (M + 66)
 * floats of row partials. Both queries return 0 for a shape that is not served.
 *
 * X : (B, N, D) float   Z : (M, D) float   Linv : (M, M) double   vmean : (M,) float
 * vchol : (M, M) float, row-major, lower read only   hyp : gpk_variational_f32's vector
 * mean, var : (B, N) float out   flags : (1,) int or NULL   saved : NULL (inference) or device
 * memory of the size above, 16-byte aligned   gmean, gvar : (B, N) float
 * Forward: M <= 256, D <= 64, N >= 1, B >= 0. Adjoint: additionally N <= 256 (the shared pipeline).
 * B = 0 launches nothing.
 */
size_t gpk_variational_chol_saved_bytes(int B, int N, int M, int D);
int gpk_variational_chol_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                             const float* vchol, const float* hyp, int B, int N, int M, int D, float* mean,
                             float* var, int* flags, void* saved, void* stream);
size_t gpk_variational_chol_adjoint_workspace_bytes(int B, int N, int M, int D);
int gpk_variational_chol_adjoint_f32(const float* X, const float* Z, const double* Linv, const float* vmean,
                                     const float* vchol, const float* hyp, const float* gmean,
                                     const float* gvar, const void* saved, int B, int N, int M, int D,
                                     void* workspace, float* dX, double* dLinv, float* dZ, float* dpar,
                                     float* dchol, void* stream);
int gpk_cholesky_kl_f32(const float* m, const float* chol, int M, float* kl, const float* gkl, float* dm,
                        float* dchol, void* stream);

/*
 * gpk_variational_chol_f32, its adjoint and gpk_cholesky_kl_f32 for O outputs at once (a
 * multi-output layer with a Cholesky q(u): batch_shape [O] on the distribution, mean and kernel).
 * The output index is grid dimension y of every launch; a workgroup offsets its base pointers by
 * it and is otherwise the single-output workgroup at the same (B, N, M, D), so output o is
 * bit-identical to a single-output call on output o's arrays. The single-output entry points are
 * the O = 1 case of the same launchers. The chain stays seven launches and two memsets each way
 * whatever O is (the zero-fill of the shared pipeline's dw / K_XX partials is one strided memset
 * over the O slices each).
 *   X : (B, N, D) read by every output when shared_x != 0 (DeepGPLayer's stride-0 expansion: no
 *       (O, B, N, D) copy is made), else (O, B, N, D)
 *   Z : (O, M, D)   Linv : (O, M, M) double   vmean : (O, M)   vchol : (O, M, M), lower read
 *   hyp : (O, 4 + 2D)   mean, var : (O, B, N) float out
 *   flags : (1,) int out or NULL: one word, every output ORs into it (the only atomic)
 *   saved : NULL (inference) or gpk_variational_chol_batched_saved_bytes(O, B, N, M, D) bytes,
 *       16-byte aligned: O slices of the single-output state; non-NULL at a shape whose saved size
 *       is 0 is an argument error (-16)
 *   gmean, gvar : (O, B, N)
 *   workspace : gpk_variational_chol_adjoint_batched_workspace_bytes(O, B, N, M, D) bytes,
 *       16-byte aligned: O slices of the single-output query. Each slice opens with the
 *       gpk_variational_cov_grad_f32 plan; W diag(gvar) and the row partials follow it.
 *   dX : (O, B, N, D) float out, per output also with shared inputs (the caller sums over O)
 *   dLinv : (O, M, M) double out   dZ : (O, M, D) out   dpar : (O, M + 2D + 2) out
 *   dchol : (O, M, M) out, lower, upper triangle zero
 *   gpk_cholesky_kl_batched_f32: m (O, M), chol (O, M, M), kl and gkl (O,), dm (O, M),
 *       dchol (O, M, M); one launch each way, output o on grid y.
 * Both queries return O x the single-output value, 0 for a shape the single-output query refuses
 * or O outside 1 .. 65535 (gridDim.y). Shape bounds are the single-output ones: M <= 256,
 * D <= 64, and N <= 256 for the adjoint; B = 0 launches nothing. Every argument is validated
 * before the first HIP call; an argument error is -(argument index).
 *
 * Replaces (reference): ToyDeepGPHiddenLayer(output_dims = O) (denoising_model/DeepGP.py:24-38)
 * with upstream variational/cholesky_variational_distribution.py of batch_shape [O] through
 * variational/variational_strategy.py forward and _variational_strategy.py::kl_divergence, and the
 * autograd backward train.py:166 runs through them.
 *
 * Memory at O = 4: saved and workspace are 4 x the single-output figures above.
 */
size_t gpk_variational_chol_batched_saved_bytes(int O, int B, int N, int M, int D);
int gpk_variational_chol_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                     const float* vmean, const float* vchol, const float* hyp, int O, int B,
                                     int N, int M, int D, float* mean, float* var, int* flags, void* saved,
                                     void* stream);
size_t gpk_variational_chol_adjoint_batched_workspace_bytes(int O, int B, int N, int M, int D);
int gpk_variational_chol_adjoint_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                             const float* vmean, const float* vchol, const float* hyp,
                                             const float* gmean, const float* gvar, const void* saved, int O,
                                             int B, int N, int M, int D, void* workspace, float* dX,
                                             double* dLinv, float* dZ, float* dpar, float* dchol,
                                             void* stream);
int gpk_cholesky_kl_batched_f32(const float* m, const float* chol, int O, int M, float* kl, const float* gkl,
                                float* dm, float* dchol, void* stream);

/*
 * Dense covariance of q(f) for a Cholesky q(u) (gpk_variational_chol_f32's distribution) and its
 * adjoint. Per window b, with A = Linv K_ZX exactly as gpk_variational_cov_f32 forms it (fp32 Gram,
 * fp64 MFMA solve, cast to fp32) and L_q = tril(C) (the strict upper triangle of C is never read,
 * a diagonal entry may be negative):
 *   W   = L_q^T A                                    (M, N), fp32 MFMA
 *   cov = K_XX + jitter I + W^T W - A^T A            diag: s2 + jitter + sum_m W_mi^2 - sum_m A_mi^2
 * (unclamped: the 1e-6 floor of gpk_variational_chol_f32 belongs to .variance). Two launches on
 * `stream`: phase 1, one workgroup per (window, 64-point block), writes the stacked panel
 * S = [W; A] as (B, 2 M, as) floats, as = N rounded up to 64, and then the window's own mean of
 * x / l (B, 64) into the workspace; phase 2 is the SYRK S^T diag(+1, -1) S of
 * gpk_variational_cov_f32's phase 2 over the 2 M rows: cov[i][j] == cov[j][i] bitwise, the
 * diagonal from the same accumulators. The workspace is the adjoint's saved state.
 *
 * The adjoint, for g = dObjective / dcov (any (N, N) matrix per window), H = g + g^T:
 *   T = S H = [T_W; T_A]     dA = L_q T_W - T_A     dchol = tril(sum_b A T_W^T)   (lower, upper zero)
 * and from dA on exactly gpk_variational_cov_grad_f32 (dLinv, Q and the RBF tail of K_ZX, P = H o
 * K_XX): its q / dlinv / kxx / reduce / finish kernels run on the dA materialised in their
 * workspace. Eight launches and one memset on `stream`, no host synchronisation, no atomics in any
 * sum, fixed summation orders in fp64: two calls give the same bits; a window's cov and dX depend
 * on that window alone. The jitter has no gradient.
 *
 * Replaces (reference): upstream variational/variational_strategy.py forward's predictive_covar
 * with variational/cholesky_variational_distribution.py's q(u), evaluated densely by
 * MultivariateNormal.covariance_matrix / rsample (denoising_model/DeepGP.py:62-64 ``x.rsample()``),
 * and the autograd backward train.py:166 runs through it.
 *
 * Memory per call: workspace / saved state = gpk_variational_chol_cov_workspace_bytes(B, N, M) =
 * (2 B M as + 64 B) * 4 bytes; the adjoint's workspace =
 * gpk_variational_chol_cov_grad_workspace_bytes(B, N, M, D): the gpk_variational_cov_grad_f32
 * workspace + 2 B M as floats of T + min(B, 32) M^2 doubles of dchol partials. Both queries return
 * 0 for a shape that is not served.
 *
 * X : (B, N, D) float   Z : (M, D) float   Linv : (M, M) double   vchol : (M, M) float, row-major,
 * lower read only   hyp : gpk_variational_f32's vector (s2, jitter and the lengthscales are read)
 * workspace : device memory of the queried size, 16-byte aligned   cov : (B, N, N) float out
 * state : the workspace the forward filled for the same arguments, 16-byte aligned
 * gcov : (B, N, N) float   dX : (B, N, D) float out   dLinv : (M, M) double out, lower, upper zero
 * dZ : (M, D) float out (the K_ZX part)   dpar : (1 + D) float out = {ds2, dlengthscale[D]}
 * dchol : (M, M) float out, lower, upper zero
 * Forward: M <= 256, D <= 64, N >= 1, B >= 0. Adjoint: additionally N <= 256 (the shared
 * pipeline). B = 0 launches nothing.
 *
 * The batched calls run O outputs with o on grid dimension y of every launch: X (B, N, D) read by
 * every output when shared_x != 0, else (O, B, N, D); a leading dense O on Z, Linv, vchol, hyp,
 * the workspace / state (O slices of the single-output query), cov, gcov, dLinv, dZ, dpar, dchol
 * and dX ((O, B, N, D) also with shared inputs: the caller sums over O). Output o is bit-identical
 * to a single-output call on o's arrays; the single-output entry points are the O = 1 case of the
 * same launchers. The batched queries return O x the single-output value, 0 for a refused shape
 * or O outside 1 .. 65535. Every argument is validated before the first HIP call; an argument
 * error is -(argument index).
 */
size_t gpk_variational_chol_cov_workspace_bytes(int B, int N, int M);
int gpk_variational_chol_cov_f32(const float* X, const float* Z, const double* Linv, const float* vchol,
                                 const float* hyp, int B, int N, int M, int D, void* workspace, float* cov,
                                 void* stream);
size_t gpk_variational_chol_cov_batched_workspace_bytes(int O, int B, int N, int M);
int gpk_variational_chol_cov_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                         const float* vchol, const float* hyp, int O, int B, int N, int M,
                                         int D, void* workspace, float* cov, void* stream);
size_t gpk_variational_chol_cov_grad_workspace_bytes(int B, int N, int M, int D);
int gpk_variational_chol_cov_grad_f32(const float* X, const float* Z, const double* Linv, const float* vchol,
                                      const float* hyp, const void* state, const float* gcov, int B, int N,
                                      int M, int D, void* workspace, float* dX, double* dLinv, float* dZ,
                                      float* dpar, float* dchol, void* stream);
size_t gpk_variational_chol_cov_grad_batched_workspace_bytes(int O, int B, int N, int M, int D);
int gpk_variational_chol_cov_grad_batched_f32(const float* X, int shared_x, const float* Z, const double* Linv,
                                              const float* vchol, const float* hyp, const void* state,
                                              const float* gcov, int O, int B, int N, int M, int D,
                                              void* workspace, float* dX, double* dLinv, float* dZ,
                                              float* dpar, float* dchol, void* stream);

/*
 * Batched Cholesky root of dense covariances, fused with sampling: per matrix b
 *   R R^T = cov[b] + jitter I        (lower factor, fp32, one workgroup, the matrix in LDS)
 *   samples[s, b, i] = mean[b, i] + sum_{j <= i} R[b, i, j] eps[s, b, j]   (ascending j)
 * One rung of psd_safe_cholesky's ladder: there is no retry inside the kernel, the caller
 * relaunches the whole batch with jitter * 10^t, as upstream adds the jitter to every matrix
 * of a batch when one fails.
 *
 * Replaces (reference): upstream linear_operator utils/cholesky.py psd_safe_cholesky's
 * torch.linalg.cholesky_ex and distributions/multivariate_normal.py rsample's root matmul
 * (denoising_model/DeepGP.py:62-64 ``x.rsample()``; DeepGPp.predict(x)[1].rsample() in eval).
 *
 * cov : (B, n, n) float, dense; only the lower triangle is read   jitter : added to the
 *       diagonal in fp32 on load
 * R : (B, n, n) float out or NULL; lower factor, upper triangle zero
 * mean : (B, n)   eps : (S, B, n)   samples : (S, B, n) out. S = 0 with NULL eps / mean /
 *       samples gives the factor only; S > 0 needs all three
 * info : (B,) int out. 0 = factored; k > 0 = the pivot of column k (1-based) was not positive
 *       or was NaN: R[b] and the samples of b are then unspecified and must not be read
 * 1 <= n <= gpk_mvn_root_max_n() = 256, B >= 0. Deterministic (fixed order, no atomics).
 */
int gpk_mvn_root_max_n(void);
int gpk_mvn_root_f32(const float* cov, const float* mean, const float* eps, int B, int n, int S,
                     float jitter, float* R, float* samples, int* info, void* stream);

/*
 * Adjoint of gpk_mvn_root_f32: per matrix b, from the forward's factor R (R R^T = cov + jitter I)
 * and the upstream gradients of R and of the draws,
 *   Rbar  = tril(gR) + tril(sum_s gsamples[s, b, :] (x) eps[s, b, :])      (n x n, lower)
 *   P     = Phi(R^T Rbar)        Phi: lower triangle, diagonal halved
 *   Sbar  = R^{-T} P R^{-1}
 *   dcov  = (Sbar + Sbar^T) / 2                                            (dense)
 *   dmean = sum_s gsamples[s, b, :]                                        (ascending s)
 * The forward reads cov as a symmetric matrix through its lower triangle; dcov is the symmetric
 * gradient torch.linalg.cholesky's backward returns, symmetric bit for bit. The jitter has no
 * gradient. One workgroup per matrix: R, then R^{-1} (inverted in place, block row by block
 * row), as packed 16 x 16 tiles in LDS; P and P R^{-1} stream through the workspace; every
 * product on the fp32 MFMA in a fixed order, no atomics: run-to-run deterministic. Allocates
 * nothing and keeps no pointers.
 *
 * Replaces (reference): the autograd backward of upstream linear_operator utils/cholesky.py
 * psd_safe_cholesky (torch.linalg.cholesky's backward) and of distributions/
 * multivariate_normal.py rsample's root matmul, which train.py:166 ``loss.backward()`` runs
 * through the skip-input draw of denoising_model/DeepGP.py:62-64 ``x.rsample()``.
 *
 * Memory per call: the workspace, gpk_mvn_root_grad_workspace_bytes(B, n) bytes
 * (B * T (T + 1) / 2 KiB with T = ceil(n / 16): 136 KiB per matrix at n = 256), plus the
 * B * n^2 floats of dcov. The query returns 0 for a shape the call does not accept.
 *
 * R : (B, n, n) float, the forward's output; the upper triangle is ignored
 * gR : (B, n, n) float or NULL; only the lower triangle is read
 * gsamples, eps : (S, B, n) float; both required when S > 0, ignored when S = 0
 * workspace : device memory of the size above, 16-byte aligned
 * dcov : (B, n, n) float out   dmean : (B, n) float out or NULL
 * gR NULL with S = 0 zero-fills dcov. 1 <= n <= gpk_mvn_root_max_n() = 256, B >= 0 (B = 0
 * launches nothing).
 */
size_t gpk_mvn_root_grad_workspace_bytes(int B, int n);
int gpk_mvn_root_grad_f32(const float* R, const float* gR, const float* gsamples, const float* eps,
                          int B, int n, int S, void* workspace, float* dcov, float* dmean, void* stream);

/*
 * One-right-hand-side solve against a batch of lower-triangular roots, per matrix b:
 *   trans = 0:  R w = d        trans = 1:  R^T w = d
 * One workgroup per matrix, sixteen columns at a time: the diagonal block is solved by 16 lanes,
 * the other rows subtract their 16 products in ascending k. fp32 FMA in a fixed order, no atomics:
 * run-to-run deterministic. The strict upper triangle of R is not read. Allocates nothing.
 *
 * Replaces (reference): torch.linalg.solve_triangular in upstream distributions/
 * multivariate_normal.py log_prob (the whitening R^{-1}(value - mean) against the root that
 * gpk_mvn_root_f32 produced), and with trans = 1 the solve of its autograd backward
 * (dd = R^{-T} gw, dR = -tril(dd w^T)).
 *
 * R : (B, n, n) float   d : (B, n) float   w : (B, n) float out (may not alias d)
 * 1 <= n <= gpk_mvn_root_max_n() = 256, B >= 0 (B = 0 launches nothing).
 */
int gpk_tri_solve_f32(const float* R, const float* d, int B, int n, int trans, float* w, void* stream);

/*
 * One refinement step of the fp32 root of gpk_mvn_root_f32, per matrix b:
 *   E = cov + jitter I - R R^T   (accumulated in fp64)      Y = R^{-1} E R^{-T}
 *   Rout = R + R Phi(Y)          Phi: lower triangle, diagonal halved
 * For a near-singular cov (one that needed the jitter ladder) the fp32 factor is
 * cond * 2^-24 from the true one and its gradient amplifies that once more; Rout is as close
 * to the factor of cov + jitter I as fp32 storage allows. The autograd formula of gpk::mvn_root
 * feeds it to gpk_mvn_root_grad_f32 when the rung that succeeded had jitter > 0. One workgroup
 * per matrix, tiles, inversion and MFMA as gpk_mvn_root_grad_f32; fixed order, no atomics.
 *
 * Replaces (reference): nothing upstream computes this; it stands in for the accuracy the
 * backward of psd_safe_cholesky would have on an fp64 factor (train.py:166 through
 * denoising_model/DeepGP.py:62-64 when the ladder engages).
 *
 * Memory per call: the workspace, gpk_mvn_root_refine_workspace_bytes(B, n) bytes
 * (B * T (T + 1) KiB, T = ceil(n / 16)); 0 for a shape the call does not accept.
 *
 * cov : (B, n, n) float, lower triangle read   R : (B, n, n) float, lower triangle read
 * workspace : 16-byte aligned   Rout : (B, n, n) float out, upper triangle zero; not R itself
 * 1 <= n <= gpk_mvn_root_max_n(), B >= 0, jitter >= 0.
 */
size_t gpk_mvn_root_refine_workspace_bytes(int B, int n);
int gpk_mvn_root_refine_f32(const float* cov, const float* R, int B, int n, float jitter, void* workspace,
                            float* Rout, void* stream);

/*
 * GPU-resident training-window gather:
 *   for window b with first row r = rows[b] of the (id, time)-sorted table:
 *     enc[b] = table[r      : r + n_enc]                  (n_enc, F)
 *     dec[b] = table[r + n_enc : r + T - pred_len]        (T - n_enc - pred_len, F)
 *     y[b]   = table[r + T - pred_len : r + T, target_col] (pred_len,)
 *   r = -1 gives an all-zero window (the reference's zero-filled tail when max_samples
 *   exceeds the valid sampling locations). Bit-exact copies (float32 table).
 *
 * Replaces (reference): the host NumPy windowing of Utils/base_train.py:29-97
 * (sample_train_val_test; windows chosen as in batch_sampled_data :100-153) and the
 * per-step host->device copies of train.py:160-161; the window CHOICE stays on the host
 * (the reference's np.random sequence, reproduced by the caller).
 *
 * table : (n_rows, F) float, device    rows : (B,) int64, device (each r + T <= n_rows, or -1)
 * enc : (B, n_enc, F) float out   dec : (B, T - n_enc - pred_len, F) float out   y : (B, pred_len) float out
 */
int gpk_window_gather_f32(const float* table, long long n_rows, int F, const long long* rows, int B,
                          int T, int n_enc, int pred_len, int target_col, float* enc, float* dec,
                          float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPK_H_ */
