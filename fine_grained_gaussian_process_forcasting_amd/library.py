"""torch.library registration of the gfx950 GP kernels (namespace ``gpk``).

SURVEY.md §8b ("Who calls it"): the model classes reach the kernels through
``torch.library`` custom ops with registered autograd formulas, so the ops are visible
to the dispatcher (FakeTensor shape propagation, ``torch.library.opcheck``, tracing)
instead of being opaque Python. Each op is one C-ABI call of include/gpk.h on
``torch.cuda.current_stream()`` (ops.py); nothing here computes on the CPU.

  (every exact op: hyper is (3 + n_ls,) shared by the B windows, or (B, 3 + n_ls), one row per window)
  gpk::exact_mll(X, y, hyper, jitter, max_tries) -> (mll, L, z, info)         [autograd]
  gpk::exact_mll_grad(X, L, z, hyper, gout) -> (dX, dy, dhyp)
  gpk::exact_posterior(X, L, z, hyper, Xs) -> (mean, var)                     [eval only]
  gpk::exact_posterior_cov(X, L, z, hyper, Xs) -> (mean, var, cov)            [eval only]
  gpk::exact_append(X, L, z, hyper, Xn, yn, jitter) -> (L2, z2, info)         [eval only]
  gpk::exact_drop(L, z, m) -> (L2, z2)                                        [eval only]
  gpk::exact_posterior_train(X, y, hyper, Xs, jitter, max_tries)
      -> (mean, var, cov, L, z, state, info)                                  [autograd]
  gpk::exact_posterior_grad(X, L, z, hyper, Xs, state, gmean, gvar, gcov) -> (dX, dy, dXs, dhyp)
  gpk::kzz_factor(Z, s2, ls, jitter, chol_jitter, max_tries) -> (Linv, L, info) [autograd]
  gpk::variational_fwd(x, Linv, Z, vmean, vstd, s2, ls, w, b0, jitter) -> (mean, var, flags, hyper)
                                                                               [autograd]
  gpk::variational_adj(x, Linv, Z, vmean, vstd, hyper, gmean, gvar) -> (dX, dLinv, dZ, dpar)
      (the three above also for the O output GPs of a multi-output layer, Z (O, M, D): a leading O
      on every array, the inputs shared or per output, one launch chain for all outputs)
  gpk::variational_chol_fwd(x, Linv, Z, vmean, vchol, s2, ls, w, b0, jitter, save)
      -> (mean, var, flags, hyper, saved): q(u) = N(vmean, tril(vchol) tril(vchol)^T)    [autograd]
  gpk::variational_chol_adj(x, Linv, Z, vmean, vchol, hyper, gmean, gvar, saved)
      -> (dX, dLinv, dZ, dpar, dchol)
  gpk::cholesky_kl(m, chol) -> kl (1,)                                        [autograd]
  gpk::cholesky_kl_grad(m, chol, gkl) -> (dm, dchol)
      (the four above also for the O outputs of a multi-output layer, one launch chain each way:
      Z (O, M, D); m (O, M), chol (O, M, M) -> kl (O,))
  gpk::gauss_ell(y, mean, var, noise) -> ell (R,)                             [autograd]
  gpk::meanfield_kl(m, s) -> kl (1,)                                          [autograd]
  gpk::variational_elbo(y, mean, var, noise, m, s, kl_scale, min_var) -> (elbo (R,), flag)
                                                                               [autograd]
  gpk::variational_cov(x, Linv, Z, vstd, hyper) -> cov                        [eval only]
  gpk::variational_cov_train(x, Linv, Z, vstd, s2, ls, jitter) -> (cov, hyper, state)
                                                                               [autograd]
  gpk::variational_cov_grad(x, Linv, Z, vstd, hyper, state, gcov) -> (dX, dLinv, dZ, dpar)
      (both also for the O outputs of a multi-output layer: Z (O, M, D))
  gpk::variational_chol_cov(x, Linv, Z, vchol, hyper) -> cov                  [eval only]
  gpk::variational_chol_cov_train(x, Linv, Z, vchol, s2, ls, jitter) -> (cov, hyper, state)
                                                                               [autograd]
  gpk::variational_chol_cov_grad(x, Linv, Z, vchol, hyper, state, gcov)
      -> (dX, dLinv, dZ, dpar, dchol)
      (the three above for a Cholesky q(u); Z (M, D) or (O, M, D))
  gpk::mvn_root(cov, jitter, mean, eps, want_R) -> (R, samples, info)         [autograd]
  gpk::mvn_root_grad(R, gR, gsamples, eps) -> (dcov, dmean)
  gpk::mvn_root_refine(cov, jitter, R) -> R refined (the backward's factor when jitter > 0)
  gpk::tri_solve(R, d, trans) -> w with R w = d or R^T w = d (log_prob's whitening) [autograd]

Reference call sites they serve: GPModel.py:10-13 + ExactMarginalLogLikelihood
(exact_mll), ExactGPModel in eval mode (exact_posterior), DeepGP.py:33-73 VariationalStrategy (kzz_factor, variational_fwd),
the ELBO at forecast_denoising.py:86-89 (gauss_ell, meanfield_kl), and the backward of
train.py:166 (the *_grad / *_adj ops).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native, ops

# ---------------------------------------------------------------------------
# exact GP marginal log likelihood (gpk_exact_mll_f32 / gpk_exact_mll_grad_f32)
# ---------------------------------------------------------------------------


@torch.library.custom_op("gpk::exact_mll", mutates_args=(), device_types="cuda")
def exact_mll(X: Tensor, y: Tensor, hyper: Tensor, jitter: float, max_tries: int,
              want_factor: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """want_factor=False (no gradient needed) skips writing L and z (empty outputs)."""
    out = ops.exact_mll(X, y, None, None, None, None, jitter=jitter, max_tries=max_tries,
                        want_L=want_factor, want_z=want_factor, hyper=hyper)
    if not want_factor:
        return out.mll, X.new_empty(0), X.new_empty(0), out.info
    return out.mll, out.L, out.z, out.info


@exact_mll.register_fake
def _(X, y, hyper, jitter, max_tries, want_factor):
    B, N, _ = X.shape
    if not want_factor:
        return X.new_empty(B), X.new_empty(0), X.new_empty(0), X.new_empty(B, dtype=torch.int32)
    return (X.new_empty(B), X.new_empty(B, N, N), X.new_empty(B, N),
            X.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("gpk::exact_mll_grad", mutates_args=(), device_types="cuda")
def exact_mll_grad(X: Tensor, L: Tensor, z: Tensor, hyper: Tensor,
                   gout: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    g = ops.exact_mll_grad(X, L, z, hyper, gout)
    return g.dX, g.dy, g.dhyp


@exact_mll_grad.register_fake
def _(X, L, z, hyper, gout):
    B, N, D = X.shape
    return X.new_empty(B, N, D), X.new_empty(B, N), X.new_empty(B, hyper.shape[-1])


@torch.library.custom_op("gpk::exact_posterior", mutates_args=(), device_types="cuda")
def exact_posterior(X: Tensor, L: Tensor, z: Tensor, hyper: Tensor, Xs: Tensor) -> Tuple[Tensor, Tensor]:
    p = ops.exact_posterior(X, L, z, hyper, Xs)
    return p.mean, p.var


@exact_posterior.register_fake
def _(X, L, z, hyper, Xs):
    B, Ns, _ = Xs.shape
    return Xs.new_empty(B, Ns), Xs.new_empty(B, Ns)


@torch.library.custom_op("gpk::exact_posterior_cov", mutates_args=(), device_types="cuda")
def exact_posterior_cov(X: Tensor, L: Tensor, z: Tensor, hyper: Tensor,
                        Xs: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    p = ops.exact_posterior_cov(X, L, z, hyper, Xs)
    return p.mean, p.var, p.cov


@exact_posterior_cov.register_fake
def _(X, L, z, hyper, Xs):
    B, Ns, _ = Xs.shape
    return Xs.new_empty(B, Ns), Xs.new_empty(B, Ns), Xs.new_empty(B, Ns, Ns)


@torch.library.custom_op("gpk::exact_append", mutates_args=(), device_types="cuda")
def exact_append(X: Tensor, L: Tensor, z: Tensor, hyper: Tensor, Xn: Tensor, yn: Tensor,
                 jitter: float) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (L2 (B, N + m, N + m), z2 (B, N + m), info): the cached factor with m observations
    appended (gpk_exact_append_f32); one rung of the jitter ladder, run by the caller."""
    return ops.exact_append(X, L, z, hyper, Xn, yn, jitter)


@exact_append.register_fake
def _(X, L, z, hyper, Xn, yn, jitter):
    B, N, _ = X.shape
    n2 = N + Xn.shape[1]
    return X.new_empty(B, n2, n2), X.new_empty(B, n2), X.new_empty(B, dtype=torch.int32)


@torch.library.custom_op("gpk::exact_drop", mutates_args=(), device_types="cuda")
def exact_drop(L: Tensor, z: Tensor, m: int) -> Tuple[Tensor, Tensor]:
    """-> (L2 (B, N - m, N - m), z2 (B, N - m)): the cached factor without its m oldest observations
    (gpk_exact_drop_f32), a rank-m update of the trailing block; no hyper-parameters enter."""
    return ops.exact_drop(L, z, m)


@exact_drop.register_fake
def _(L, z, m):
    B, N, _ = L.shape
    return L.new_empty(B, N - m, N - m), L.new_empty(B, N - m)


# The differentiable posterior (gpk_exact_mll_f32 for the factor, gpk_exact_posterior_cov_f32 keeping
# its workspace as the saved state, gpk_exact_posterior_grad_f32 from it): what ExactGPModel calls
# in eval mode when a gradient can flow.


@torch.library.custom_op("gpk::exact_posterior_train", mutates_args=(), device_types="cuda")
def exact_posterior_train(X: Tensor, y: Tensor, hyper: Tensor, Xs: Tensor, jitter: float,
                          max_tries: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (mean (B, Ns), var (B, Ns), cov (B, Ns, Ns), L, z, state, info): the training factor
    from the live parameters, then the joint posterior; state is the posterior's workspace
    (V = L^{-1} K* in fp32 and the centring mean), which the backward reads."""
    f = ops.exact_mll(X, y, None, None, None, None, jitter=jitter, max_tries=max_tries, want_L=True,
                      want_z=True, hyper=hyper)
    p, state = ops.exact_posterior_cov(X, f.L, f.z, hyper, Xs, return_state=True)
    return p.mean, p.var, p.cov, f.L, f.z, state, f.info


def _post_state_numel(X, Xs):
    B, N, Ns = X.shape[0], X.shape[1], Xs.shape[1]
    return max(1, _native.lib().gpk_exact_posterior_cov_workspace_bytes(B, N, Ns) // 4)


@exact_posterior_train.register_fake
def _(X, y, hyper, Xs, jitter, max_tries):
    B, N, _ = X.shape
    Ns = Xs.shape[1]
    return (Xs.new_empty(B, Ns), Xs.new_empty(B, Ns), Xs.new_empty(B, Ns, Ns), X.new_empty(B, N, N),
            X.new_empty(B, N), X.new_empty(_post_state_numel(X, Xs)), X.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("gpk::exact_posterior_grad", mutates_args=(), device_types="cuda")
def exact_posterior_grad(X: Tensor, L: Tensor, z: Tensor, hyper: Tensor, Xs: Tensor, state: Tensor,
                         gmean: Optional[Tensor] = None, gvar: Optional[Tensor] = None,
                         gcov: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (dX (B, N, D), dy (B, N), dXs (B, Ns, D), dhyp (B, 3 + n_ls) per window)."""
    g = ops.exact_posterior_grad(X, L, z, hyper, Xs, state, gmean, gvar, gcov)
    return g.dX, g.dy, g.dXs, g.dhyp


@exact_posterior_grad.register_fake
def _(X, L, z, hyper, Xs, state, gmean=None, gvar=None, gcov=None):
    B, N, D = X.shape
    return X.new_empty(B, N, D), X.new_empty(B, N), torch.empty_like(Xs), X.new_empty(B, hyper.shape[-1])


def _dhyper(dhyp, hyper):
    """The kernels' per-window dhyp (B, 3 + n_ls) as the gradient of ``hyper``: its rows when hyper
    is (B, 3 + n_ls), one row per window; their sum when every window shares one vector."""
    return dhyp if hyper.dim() == 2 else dhyp.sum(0)


def _post_train_setup(ctx, inputs, output):
    X, y, hyper, Xs, jitter, max_tries = inputs
    mean, var, cov, L, z, state, info = output
    ctx.save_for_backward(X, L, z, hyper, Xs, state)
    ctx.mark_non_differentiable(L, z, state, info)
    ctx.set_materialize_grads(False)   # an unused mean, var or cov reaches the C entry as NULL


@torch.autograd.function.once_differentiable
def _post_train_backward(ctx, gmean, gvar, gcov, _gL, _gz, _gstate, _ginfo):
    X, L, z, hyper, Xs, state = ctx.saved_tensors
    if gmean is None and gvar is None and gcov is None:
        return None, None, None, None, None, None
    gmean, gvar, gcov = (g.contiguous() if g is not None else None for g in (gmean, gvar, gcov))
    dX, dy, dXs, dhyp = torch.ops.gpk.exact_posterior_grad(X, L, z, hyper, Xs, state, gmean, gvar, gcov)
    return dX, dy, _dhyper(dhyp, hyper), dXs, None, None


exact_posterior_train.register_autograd(_post_train_backward, setup_context=_post_train_setup)


def _exact_setup(ctx, inputs, output):
    X, y, hyper, jitter, max_tries, want_factor = inputs
    mll, L, z, info = output
    ctx.save_for_backward(X, L, z, hyper)
    ctx.mark_non_differentiable(L, z, info)


def _exact_backward(ctx, gmll, _gL, _gz, _ginfo):
    X, L, z, hyper = ctx.saved_tensors
    if L.numel() == 0:
        raise RuntimeError("gpk::exact_mll was called with want_factor=False; no backward")
    dX, dy, dhyp = torch.ops.gpk.exact_mll_grad(X, L, z, hyper, gmll.contiguous())
    return dX, dy, _dhyper(dhyp, hyper), None, None, None


exact_mll.register_autograd(_exact_backward, setup_context=_exact_setup)

# ---------------------------------------------------------------------------
# The variational ops below take both forms of a layer: Z (M, D) is one GP; Z (O, M, D) the O output
# GPs of a multi-output layer (output_dims = O) on ONE launch chain, every per-output array with a
# leading O (``lead`` = Z.shape[:-2]) and the inputs x (B, N, D) shared by the outputs or
# (O, B, N, D). The op bodies dispatch on Z.dim() to the single or the ``_batched`` name of ops.py;
# the kernels return per-dimension, per-output gradients, which the helpers below fold.
# ---------------------------------------------------------------------------


def _fold_x(dX, x, Z):
    """dX (O, B, N, D) per output -> the gradient of inputs (B, N, D) shared by the outputs."""
    return dX.sum(0) if Z.dim() == 3 and x.dim() == 3 else dX


def _fold_ls(dls, ls, Z):
    """dls (..., D) per dimension -> the gradient of ``ls``: summed over D for a lengthscale shared
    by the dimensions (one value; one per output for Z (O, M, D))."""
    if Z.dim() == 3:
        return dls.sum(-1).reshape(ls.shape) if ls.numel() == Z.shape[0] else dls.reshape(ls.shape)
    return dls.sum().reshape(ls.shape) if ls.numel() == 1 else dls.reshape(ls.shape)


def _fold_mean(dw, db0, w, b0, Z):
    """dw (..., D), db0 (...) -> the gradients of the mean's w and b0: summed over O for a mean
    shared by the outputs (w (D,), b0 one value)."""
    if Z.dim() == 3:
        dw = dw.sum(0) if w.numel() == Z.shape[-1] else dw
        db0 = db0.sum() if b0.numel() == 1 else db0
    return dw.reshape(w.shape), db0.reshape(b0.shape)


# ---------------------------------------------------------------------------
# shared K_ZZ factor (gpk_kzz_chol_f64) + its M x M adjoint (ops.kzz_backward)
# ---------------------------------------------------------------------------


def _kzz_hyper_batched(Z, s2, ls):
    O, _, D = Z.shape
    return torch.cat([s2.detach().reshape(O, 1).float(), ls.detach().reshape(O, -1).expand(O, D).float()], dim=1)


@torch.library.custom_op("gpk::kzz_factor", mutates_args=(), device_types="cuda")
def kzz_factor(Z: Tensor, s2: Tensor, ls: Tensor, jitter: float, chol_jitter: float,
               max_tries: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Z (M, D), s2 (), ls (D,) or (1,) -> (Linv, L (M, M) float64, info (1,)); Z (O, M, D), s2 (O,),
    ls (O, D) or (O, 1) -> (Linv, L (O, M, M), info (O,))."""
    if Z.dim() == 3:
        kz = ops.kzz_cholesky_batched(Z.detach(), _kzz_hyper_batched(Z, s2, ls), jitter=jitter,
                                      chol_jitter=chol_jitter, max_tries=max_tries)
    else:
        lsv = ls.detach().reshape(-1).expand(Z.shape[-1]).contiguous().float()
        kz = ops.kzz_cholesky(Z.detach(), None, None, jitter=jitter, chol_jitter=chol_jitter,
                              max_tries=max_tries, hyper=torch.cat([s2.detach().reshape(1).float(), lsv]))
    return kz.Linv, kz.L, kz.info


@kzz_factor.register_fake
def _(Z, s2, ls, jitter, chol_jitter, max_tries):
    lead, M = Z.shape[:-2], Z.shape[-2]
    return (Z.new_empty(*lead, M, M, dtype=torch.float64), Z.new_empty(*lead, M, M, dtype=torch.float64),
            Z.new_empty(tuple(lead) or (1,), dtype=torch.int32))


def _kzz_setup(ctx, inputs, output):
    Z, s2, ls = inputs[:3]
    Linv, L, info = output
    ctx.save_for_backward(Z, s2, ls, L, Linv)
    ctx.mark_non_differentiable(L, info)


def _kzz_backward(ctx, dLinv, _dL, _dinfo):
    """The dLinv of every call that shared the factor(s) -> one K_ZZ adjoint."""
    Z, s2, ls, L, Linv = ctx.saved_tensors
    if dLinv is None:
        return None, None, None, None, None, None
    if Z.dim() == 3:
        dZ, dhyp = ops.kzz_backward_batched(dLinv, L, Linv, Z, _kzz_hyper_batched(Z, s2, ls))
        ds2, dls = dhyp[:, 0], dhyp[:, 1:]
    else:
        dZ, ds2, dls = ops.kzz_backward(dLinv, L, Linv, Z, s2, ls)
    return (dZ.to(Z.dtype), ds2.reshape(s2.shape).to(s2.dtype), _fold_ls(dls, ls, Z).to(ls.dtype),
            None, None, None)


kzz_factor.register_autograd(_kzz_backward, setup_context=_kzz_setup)

# ---------------------------------------------------------------------------
# variational predictive distribution (gpk_variational_f32 / gpk_variational_adjoint_f32 and
# gpk_variational_batched_f32 / gpk_variational_adjoint_batched_f32)
# ---------------------------------------------------------------------------


def _var_hyper(x, s2, ls, w, b0, jitter):
    D = x.shape[-1]
    lsv = ls.detach().reshape(-1).expand(D).contiguous().float()
    return ops.pack_variational_hyper(s2.detach(), 1.0, jitter, b0.detach(), w.detach(), lsv, D, x.device)


def _var_hyper_batched(x, O, s2, ls, w, b0, jitter):
    """(O, 4 + 2D) rows {s2, noise = 1, jitter, b0, w[D], ls[D]}; a mean shared by all outputs
    (w (D,), b0 one value) is repeated."""
    D = x.shape[-1]
    one = x.new_ones(O, 1)
    return torch.cat([s2.detach().reshape(O, 1).float(), one, one * float(jitter),
                      b0.detach().reshape(-1, 1).expand(O, 1).float(), w.detach().reshape(-1, D).expand(O, D).float(),
                      ls.detach().reshape(O, -1).expand(O, D).float()], dim=1)


def _pack_hyper(x, Z, s2, ls, w, b0, jitter):
    """The packed hyper vector of the variational kernels: (4 + 2D,), or (O, 4 + 2D) for Z (O, M, D).
    Two packers: one output goes through ops.pack_variational_hyper and its cached constants (one
    cat kernel per call)."""
    if Z.dim() == 3:
        return _var_hyper_batched(x, Z.shape[0], s2, ls, w, b0, jitter)
    return _var_hyper(x, s2, ls, w, b0, jitter)


def _saved_numel(x, Z, save):
    if not save:
        return 0
    B, N, D = x.shape[-3:]
    O = Z.shape[0] if Z.dim() == 3 else 1
    return O * (_native.lib().gpk_variational_saved_bytes(B, N, Z.shape[-2], D) // 4)


@torch.library.custom_op("gpk::variational_fwd", mutates_args=(), device_types="cuda")
def variational_fwd(x: Tensor, Linv: Tensor, Z: Tensor, vmean: Tensor, vstd: Tensor, s2: Tensor,
                    ls: Tensor, w: Tensor, b0: Tensor, jitter: float,
                    save: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (mean, var, clamp flags, packed hyper vector, saved state). The hyper vector is
    returned so the backward reuses it (one pack per GP call, not one per direction).
    ``save`` (a gradient will be needed): the forward keeps A = Linv K_ZX and the clamp mask
    for the saved-state adjoint where it serves the shape (M > 64; gpk_variational_train_f32),
    else the state is empty and the adjoint recomputes.
    Z (O, M, D): Linv (O, M, M), vmean / vstd (O, M), s2 (O,), ls (O, D) or (O, 1); the mean per
    output (w (O, D), b0 (O,)) or shared (w (D,), b0 one value) -> mean, var (O, B, N), clamp flags
    (1,), packed hyper (O, 4 + 2D)."""
    hyper = _pack_hyper(x, Z, s2, ls, w, b0, jitter)
    if Z.dim() == 3:
        out = ops.variational_forward_batched(x, Z, Linv, vmean, vstd, hyper, save=save)
    else:
        out = ops.variational_forward(x, Z, Linv, vmean, vstd, hyper=hyper, save=save)
    saved = out.saved if out.saved is not None else x.new_empty(0)
    return out.mean, out.var, out.flags, hyper, saved


@variational_fwd.register_fake
def _(x, Linv, Z, vmean, vstd, s2, ls, w, b0, jitter, save=False):
    B, N, D = x.shape[-3:]
    lead = Z.shape[:-2]
    return (x.new_empty(*lead, B, N), x.new_empty(*lead, B, N), x.new_empty(1, dtype=torch.int32),
            x.new_empty(*lead, 4 + 2 * D), x.new_empty(_saved_numel(x, Z, save)))


@torch.library.custom_op("gpk::variational_adj", mutates_args=(), device_types="cuda")
def variational_adj(x: Tensor, Linv: Tensor, Z: Tensor, vmean: Tensor, vstd: Tensor, hyper: Tensor,
                    gmean: Tensor, gvar: Tensor, saved: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (dX, dLinv, dZ (K_ZX part), dpar = [dvmean (M), dvstd (M), ds2, dls (D), dw (D), db0]).
    ``saved``: the forward's state (empty: recompute the forward inside the adjoint).
    Z (O, M, D): dX (O, B, N, D) per output, dLinv (O, M, M), dZ (O, M, D), dpar (O, 2M + 2D + 2)."""
    adjoint = ops.variational_adjoint_batched if Z.dim() == 3 else ops.variational_adjoint
    adj = adjoint(x, Z, Linv, vmean, vstd, hyper, gmean, gvar, saved=saved if saved.numel() > 0 else None)
    return adj.dX, adj.dLinv, adj.dZ, adj.dpar


@variational_adj.register_fake
def _(x, Linv, Z, vmean, vstd, hyper, gmean, gvar, saved):
    M, D = Z.shape[-2:]
    lead = Z.shape[:-2]
    return (x.new_empty(*lead, *x.shape[-3:]), torch.empty_like(Linv), torch.empty_like(Z),
            x.new_empty(*lead, 2 * M + 2 * D + 2))


def _var_setup(ctx, inputs, output):
    x, Linv, Z, vmean, vstd, s2, ls, w, b0, jitter = inputs[:10]
    ctx.save_for_backward(x, Linv, Z, vmean, vstd, s2, ls, w, b0, output[3], output[4])
    ctx.mark_non_differentiable(output[2], output[3], output[4])


def _var_backward(ctx, gmean, gvar, _gflags, _ghyper, _gsaved):
    x, Linv, Z, vmean, vstd, s2, ls, w, b0, hyper, saved = ctx.saved_tensors
    M, D = Z.shape[-2:]
    shape = Z.shape[:-2] + x.shape[-3:-1]
    if gmean is None:
        gmean = x.new_zeros(shape)
    if gvar is None:
        gvar = x.new_zeros(shape)
    dX, dLinv, dZ, dpar = torch.ops.gpk.variational_adj(x, Linv, Z, vmean, vstd, hyper,
                                                        gmean.contiguous(), gvar.contiguous(), saved)
    dX = _fold_x(dX, x, Z)
    dls = _fold_ls(dpar[..., 2 * M + 1:2 * M + 1 + D], ls, Z)
    dw, db0 = _fold_mean(dpar[..., 2 * M + 1 + D:2 * M + 1 + 2 * D], dpar[..., 2 * M + 1 + 2 * D], w, b0, Z)
    return (dX, dLinv, dZ, dpar[..., :M].reshape(vmean.shape), dpar[..., M:2 * M].reshape(vstd.shape),
            dpar[..., 2 * M].reshape(s2.shape), dls, dw, db0, None, None)


variational_fwd.register_autograd(_var_backward, setup_context=_var_setup)


# ---------------------------------------------------------------------------
# ELBO terms (gpk_gauss_ell_f32 / gpk_meanfield_kl_f32)
# ---------------------------------------------------------------------------


@torch.library.custom_op("gpk::gauss_ell",mutates_args=(), device_types="cuda")
def gauss_ell(y: Tensor, mean: Tensor, var: Tensor, noise: Tensor) -> Tensor:
    """(R,) sums over N of GaussianLikelihood.expected_log_prob for (R, N) rows."""
    return ops.gauss_ell(y.contiguous().float(), mean.contiguous().float(), var.contiguous().float(),
                         noise.reshape(1).contiguous().float())


@gauss_ell.register_fake
def _(y, mean, var, noise):
    return mean.new_empty(mean.shape[0])


@torch.library.custom_op("gpk::gauss_ell_grad", mutates_args=(), device_types="cuda")
def gauss_ell_grad(y: Tensor, mean: Tensor, var: Tensor, noise: Tensor,
                   gell: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return ops.gauss_ell_grad(y.contiguous().float(), mean.contiguous().float(), var.contiguous().float(),
                              noise.reshape(1).contiguous().float(), gell.contiguous().float())


@gauss_ell_grad.register_fake
def _(y, mean, var, noise, gell):
    return (torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean), mean.new_empty(1))


def _ell_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _ell_backward(ctx, gell):
    y, mean, var, noise = ctx.saved_tensors
    dy, dmean, dvar, dnoise = torch.ops.gpk.gauss_ell_grad(y, mean, var, noise, gell.contiguous())
    return dy, dmean, dvar, dnoise.reshape(noise.shape)


gauss_ell.register_autograd(_ell_backward, setup_context=_ell_setup)


@torch.library.custom_op("gpk::meanfield_kl", mutates_args=(), device_types="cuda")
def meanfield_kl(m: Tensor, s: Tensor) -> Tensor:
    """(1,) KL(N(m, diag s^2) || N(0, I)) of the whitened mean-field q(u)."""
    return ops.meanfield_kl(m.contiguous().float(), s.contiguous().float())


@meanfield_kl.register_fake
def _(m, s):
    return m.new_empty(1)


@torch.library.custom_op("gpk::meanfield_kl_grad", mutates_args=(), device_types="cuda")
def meanfield_kl_grad(m: Tensor, s: Tensor, gkl: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.meanfield_kl_grad(m.contiguous().float(), s.contiguous().float(), gkl.reshape(1).contiguous().float())


@meanfield_kl_grad.register_fake
def _(m, s, gkl):
    return torch.empty_like(m), torch.empty_like(s)


def _kl_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _kl_backward(ctx, gkl):
    m, s = ctx.saved_tensors
    dm, ds = torch.ops.gpk.meanfield_kl_grad(m, s, gkl)
    return dm, ds


meanfield_kl.register_autograd(_kl_backward, setup_context=_kl_setup)


@torch.library.custom_op("gpk::variational_elbo", mutates_args=(), device_types="cuda")
def variational_elbo(y: Tensor, mean: Tensor, var: Tensor, noise: Tensor, vmean: Tensor, vstd: Tensor,
                     kl_scale: float, min_var: float) -> Tuple[Tensor, Tensor]:
    """(R,) per-row ELBO ell_r / N - kl_scale KL(q(u)) and the variance-clamp flag (1,)."""
    return ops.variational_elbo(y, mean, var, noise.reshape(1).contiguous().float(), vmean, vstd, kl_scale,
                                min_var)


@variational_elbo.register_fake
def _(y, mean, var, noise, vmean, vstd, kl_scale, min_var):
    return mean.new_empty(mean.shape[0]), mean.new_empty(1, dtype=torch.int32)


@torch.library.custom_op("gpk::variational_elbo_grad", mutates_args=(), device_types="cuda")
def variational_elbo_grad(y: Tensor, mean: Tensor, var: Tensor, noise: Tensor, vmean: Tensor, vstd: Tensor,
                          kl_scale: float, gelbo: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return ops.variational_elbo_grad(y, mean, var, noise.reshape(1).contiguous().float(), vmean, vstd,
                                     kl_scale, gelbo)


@variational_elbo_grad.register_fake
def _(y, mean, var, noise, vmean, vstd, kl_scale, gelbo):
    R, N = mean.shape
    return (mean.new_empty(R, N), mean.new_empty(R, N), mean.new_empty(1), torch.empty_like(vmean),
            torch.empty_like(vstd))


def _elbo_setup(ctx, inputs, output):
    y, mean, var, noise, vmean, vstd, kl_scale, min_var = inputs
    ctx.kl_scale = kl_scale
    ctx.save_for_backward(y, mean, var, noise, vmean, vstd)
    ctx.mark_non_differentiable(output[1])


def _elbo_backward(ctx, gelbo, _gflag):
    y, mean, var, noise, vmean, vstd = ctx.saved_tensors
    dmean, dvar, dnoise, dm, ds = torch.ops.gpk.variational_elbo_grad(y, mean, var, noise, vmean, vstd,
                                                                      ctx.kl_scale, gelbo.contiguous())
    return (None, dmean, dvar, dnoise.reshape(noise.shape), dm.reshape(vmean.shape), ds.reshape(vstd.shape),
            None, None)


variational_elbo.register_autograd(_elbo_backward, setup_context=_elbo_setup)

# ---------------------------------------------------------------------------
# draws: dense covariance of q(f) (gpk_variational_cov_f32; no autograd formula: gp.py calls it
# only when no gradient can flow, and gpk::variational_cov_train below when one can) and the batched
# Cholesky root fused with sampling (gpk_mvn_root_f32) with its adjoint (gpk_mvn_root_grad_f32).
# ---------------------------------------------------------------------------


@torch.library.custom_op("gpk::variational_cov", mutates_args=(), device_types="cuda")
def variational_cov(x: Tensor, Linv: Tensor, Z: Tensor, vstd: Tensor, hyper: Tensor) -> Tensor:
    """Z (M, D): x (B, N, D) -> cov (B, N, N). Z (O, M, D), the outputs of a multi-output
    layer on one launch chain: x (B, N, D) shared or (O, B, N, D) -> cov (O, B, N, N)."""
    if Z.dim() == 3:
        return ops.variational_cov_batched(x, Z, Linv, vstd, hyper)
    return ops.variational_cov(x, Z, Linv, vstd, hyper)


@variational_cov.register_fake
def _(x, Linv, Z, vstd, hyper):
    B, N = x.shape[-3], x.shape[-2]
    return x.new_empty(*Z.shape[:-2], B, N, N)


# The differentiable covariance (gpk_variational_cov_f32 keeping its workspace as the saved state,
# gpk_variational_cov_grad_f32 from it): what gp.py calls when a gradient can flow.


def _cov_hyper(x, Z, s2, ls, jitter):
    """The packed hyper vector gpk_variational_cov_f32 reads (s2, jitter and the lengthscales; the
    mean's entries are not read and stay 0): (4 + 2D,), or (O, 4 + 2D) for Z (O, M, D)."""
    return _pack_hyper(x, Z, s2, ls, x.new_zeros(x.shape[-1]), x.new_zeros(1), jitter)


@torch.library.custom_op("gpk::variational_cov_train", mutates_args=(), device_types="cuda")
def variational_cov_train(x: Tensor, Linv: Tensor, Z: Tensor, vstd: Tensor, s2: Tensor, ls: Tensor,
                          jitter: float) -> Tuple[Tensor, Tensor, Tensor]:
    """gpk::variational_cov from the parameters, for a gradient: -> (cov, packed hyper, state).
    The state is the forward's workspace (A = Linv K_ZX in fp32 and the windows' means), which
    the backward reads instead of a second fp64 product. Z (O, M, D): the batched form, with s2
    (O,), ls (O, D) or (O, 1), vstd (O, M) and x (B, N, D) shared or (O, B, N, D)."""
    hyper = _cov_hyper(x, Z, s2, ls, jitter)
    if Z.dim() == 3:
        cov, state = ops.variational_cov_batched(x, Z, Linv, vstd, hyper, return_state=True)
    else:
        cov, state = ops.variational_cov(x, Z, Linv, vstd, hyper, return_state=True)
    return cov, hyper, state


def _cov_state_numel(x, Z):
    B, N = x.shape[-3], x.shape[-2]
    if B == 0:
        return 0
    O = Z.shape[0] if Z.dim() == 3 else 1
    return max(1, O * (_native.lib().gpk_variational_cov_workspace_bytes(B, N, Z.shape[-2]) // 4))


@variational_cov_train.register_fake
def _(x, Linv, Z, vstd, s2, ls, jitter):
    B, N, D = x.shape[-3:]
    lead = Z.shape[:-2]
    return x.new_empty(*lead, B, N, N), x.new_empty(*lead, 4 + 2 * D), x.new_empty(_cov_state_numel(x, Z))


@torch.library.custom_op("gpk::variational_cov_grad", mutates_args=(), device_types="cuda")
def variational_cov_grad(x: Tensor, Linv: Tensor, Z: Tensor, vstd: Tensor, hyper: Tensor, state: Tensor,
                         gcov: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (dX, dLinv, dZ (the K_ZX part), dpar = [dvstd (M), ds2, dls (D)]); Z (O, M, D): every
    array with a leading O, dX (O, B, N, D) per output also for shared inputs."""
    if Z.dim() == 3:
        return ops.variational_cov_grad_batched(x, Z, Linv, vstd, hyper, state, gcov)
    return ops.variational_cov_grad(x, Z, Linv, vstd, hyper, state, gcov)


@variational_cov_grad.register_fake
def _(x, Linv, Z, vstd, hyper, state, gcov):
    M, D = Z.shape[-2:]
    lead = Z.shape[:-2]
    return (x.new_empty(*lead, *x.shape[-3:]), torch.empty_like(Linv), torch.empty_like(Z),
            x.new_empty(*lead, M + 1 + D))


def _covt_setup(ctx, inputs, output):
    x, Linv, Z, vstd, s2, ls, jitter = inputs
    ctx.save_for_backward(x, Linv, Z, vstd, s2, ls, output[1], output[2])
    ctx.mark_non_differentiable(output[1], output[2])


@torch.autograd.function.once_differentiable
def _covt_backward(ctx, gcov, _ghyper, _gstate):
    x, Linv, Z, vstd, s2, ls, hyper, state = ctx.saved_tensors
    M, D = Z.shape[-2:]
    dX, dLinv, dZ, dpar = torch.ops.gpk.variational_cov_grad(x, Linv, Z, vstd, hyper, state,
                                                             gcov.contiguous())
    return (_fold_x(dX, x, Z), dLinv, dZ, dpar[..., :M].reshape(vstd.shape), dpar[..., M].reshape(s2.shape),
            _fold_ls(dpar[..., M + 1:], ls, Z), None)


variational_cov_train.register_autograd(_covt_backward, setup_context=_covt_setup)


# The same three ops for a Cholesky q(u) (gpk_variational_chol_cov_f32 and its adjoint
# gpk_variational_chol_cov_grad_f32): vchol = chol_variational_covar, (M, M) or (O, M, M).


@torch.library.custom_op("gpk::variational_chol_cov", mutates_args=(), device_types="cuda")
def variational_chol_cov(x: Tensor, Linv: Tensor, Z: Tensor, vchol: Tensor, hyper: Tensor) -> Tensor:
    """Z (M, D): x (B, N, D) -> cov (B, N, N). Z (O, M, D), the outputs of a multi-output layer on
    one launch chain: x (B, N, D) shared or (O, B, N, D) -> cov (O, B, N, N)."""
    return ops.variational_chol_cov(x, Z, Linv, vchol, hyper)


@variational_chol_cov.register_fake
def _(x, Linv, Z, vchol, hyper):
    B, N = x.shape[-3], x.shape[-2]
    return x.new_empty(*Z.shape[:-2], B, N, N)


@torch.library.custom_op("gpk::variational_chol_cov_train", mutates_args=(), device_types="cuda")
def variational_chol_cov_train(x: Tensor, Linv: Tensor, Z: Tensor, vchol: Tensor, s2: Tensor, ls: Tensor,
                               jitter: float) -> Tuple[Tensor, Tensor, Tensor]:
    """gpk::variational_chol_cov from the parameters, for a gradient: -> (cov, packed hyper, state).
    The state is the forward's workspace (the stacked [W; A] panels in fp32 and the windows' means).
    Z (O, M, D): the batched form, with s2 (O,), ls (O, D) or (O, 1), vchol (O, M, M) and x
    (B, N, D) shared or (O, B, N, D)."""
    hyper = _cov_hyper(x, Z, s2, ls, jitter)
    cov, state = ops.variational_chol_cov(x, Z, Linv, vchol, hyper, return_state=True)
    return cov, hyper, state


def _chol_cov_state_numel(x, Z):
    B, N = x.shape[-3], x.shape[-2]
    if B == 0:
        return 0
    O = Z.shape[0] if Z.dim() == 3 else 1
    return max(1, O * (_native.lib().gpk_variational_chol_cov_workspace_bytes(B, N, Z.shape[-2]) // 4))


@variational_chol_cov_train.register_fake
def _(x, Linv, Z, vchol, s2, ls, jitter):
    B, N, D = x.shape[-3:]
    lead = Z.shape[:-2]
    return (x.new_empty(*lead, B, N, N), x.new_empty(*lead, 4 + 2 * D),
            x.new_empty(_chol_cov_state_numel(x, Z)))


@torch.library.custom_op("gpk::variational_chol_cov_grad", mutates_args=(), device_types="cuda")
def variational_chol_cov_grad(x: Tensor, Linv: Tensor, Z: Tensor, vchol: Tensor, hyper: Tensor, state: Tensor,
                              gcov: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (dX, dLinv, dZ (the K_ZX part), dpar = [ds2, dls (D)], dchol); Z (O, M, D): every array
    with a leading O, dX (O, B, N, D) per output also for shared inputs."""
    return ops.variational_chol_cov_grad(x, Z, Linv, vchol, hyper, state, gcov)


@variational_chol_cov_grad.register_fake
def _(x, Linv, Z, vchol, hyper, state, gcov):
    lead = Z.shape[:-2]
    return (x.new_empty(*lead, *x.shape[-3:]), torch.empty_like(Linv), torch.empty_like(Z),
            x.new_empty(*lead, 1 + Z.shape[-1]), torch.empty_like(vchol))


def _ccovt_setup(ctx, inputs, output):
    x, Linv, Z, vchol, s2, ls, jitter = inputs
    ctx.save_for_backward(x, Linv, Z, vchol, s2, ls, output[1], output[2])
    ctx.mark_non_differentiable(output[1], output[2])


@torch.autograd.function.once_differentiable
def _ccovt_backward(ctx, gcov, _ghyper, _gstate):
    x, Linv, Z, vchol, s2, ls, hyper, state = ctx.saved_tensors
    dX, dLinv, dZ, dpar, dchol = torch.ops.gpk.variational_chol_cov_grad(x, Linv, Z, vchol, hyper, state,
                                                                         gcov.contiguous())
    return (_fold_x(dX, x, Z), dLinv, dZ, dchol.reshape(vchol.shape), dpar[..., 0].reshape(s2.shape),
            _fold_ls(dpar[..., 1:], ls, Z), None)


variational_chol_cov_train.register_autograd(_ccovt_backward, setup_context=_ccovt_setup)


@torch.library.custom_op("gpk::mvn_root", mutates_args=(), device_types="cuda")
def mvn_root(cov: Tensor, jitter: float, mean: Optional[Tensor] = None, eps: Optional[Tensor] = None,
             want_R: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (R (B, n, n) or empty, samples (S, B, n) or empty, info (B,) int32)."""
    R, samples, info = ops.mvn_root(cov, jitter, mean, eps, want_R)
    return (R if R is not None else cov.new_empty(0), samples if samples is not None else cov.new_empty(0),
            info)


@mvn_root.register_fake
def _(cov, jitter, mean=None, eps=None, want_R=True):
    B, n, _ = cov.shape
    return (cov.new_empty(B, n, n) if want_R else cov.new_empty(0),
            cov.new_empty(eps.shape[0], B, n) if eps is not None else cov.new_empty(0),
            cov.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("gpk::mvn_root_grad", mutates_args=(), device_types="cuda")
def mvn_root_grad(R: Tensor, gR: Optional[Tensor] = None, gsamples: Optional[Tensor] = None,
                  eps: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (dcov (B, n, n) symmetric, dmean (B, n)): the adjoint of gpk::mvn_root."""
    dcov, dmean = ops.mvn_root_grad(R, gR, gsamples, eps)
    return dcov, dmean


@mvn_root_grad.register_fake
def _(R, gR=None, gsamples=None, eps=None):
    B, n, _ = R.shape
    return R.new_empty(B, n, n), R.new_empty(B, n)


@torch.library.custom_op("gpk::mvn_root_refine", mutates_args=(), device_types="cuda")
def mvn_root_refine(cov: Tensor, jitter: float, R: Tensor) -> Tensor:
    """One refinement step of the fp32 root with an fp64 residual (gpk_mvn_root_refine_f32)."""
    return ops.mvn_root_refine(cov, jitter, R)


@mvn_root_refine.register_fake
def _(cov, jitter, R):
    return torch.empty_like(R)


@torch.library.custom_op("gpk::tri_solve", mutates_args=(), device_types="cuda")
def tri_solve(R: Tensor, d: Tensor, trans: bool) -> Tensor:
    """w (B, n) with R w = d, or R^T w = d when trans, for lower-triangular R (B, n, n)
    (gpk_tri_solve_f32): the whitening of MultivariateNormal.log_prob against the HIP root."""
    return ops.tri_solve(R, d, trans)


@tri_solve.register_fake
def _(R, d, trans):
    return torch.empty_like(d)


def _tri_solve_setup(ctx, inputs, output):
    R, d, trans = inputs
    ctx.trans = trans
    ctx.save_for_backward(R, output)


def _tri_solve_backward(ctx, gw):
    # w = op(R)^{-1} d: dd = op(R)^{-T} gw (the same kernel, transposed), d op(R) = -dd w^T, lower part
    R, w = ctx.saved_tensors
    gd = torch.ops.gpk.tri_solve(R, gw.contiguous(), not ctx.trans)
    outer = gd.unsqueeze(-1) * w.unsqueeze(-2)
    gR = -torch.tril(outer.transpose(-1, -2) if ctx.trans else outer)
    return gR, gd, None


tri_solve.register_autograd(_tri_solve_backward, setup_context=_tri_solve_setup)


def _mvn_root_setup(ctx, inputs, output):
    cov, jitter, mean, eps, want_R = inputs
    R, samples, info = output
    ctx.has_eps = eps is not None
    ctx.want_R = want_R
    ctx.mean_shape = mean.shape if mean is not None else None
    ctx.jitter = jitter
    # a rung with jitter: the matrix is near-singular, the backward refines the fp32 factor
    ctx.save_for_backward(R, eps, cov if jitter > 0.0 and want_R else None)
    ctx.mark_non_differentiable(info)
    ctx.set_materialize_grads(False)


@torch.autograd.function.once_differentiable
def _mvn_root_backward(ctx, gR, gsamples, _ginfo):
    R, eps, cov = ctx.saved_tensors
    if not ctx.want_R:
        raise RuntimeError("gpk::mvn_root was called with want_R=False; its backward needs the factor: "
                           "call it with want_R=True when a gradient can flow")
    if not ctx.has_eps or gsamples is None:
        gsamples = eps_k = None
    else:
        gsamples, eps_k = gsamples.contiguous(), eps
    if gR is not None:
        gR = gR.contiguous()
    if cov is not None:
        # the ladder engaged: the fp32 factor is cond * 2^-24 off, which the adjoint amplifies
        R = torch.ops.gpk.mvn_root_refine(cov, ctx.jitter, R)
    dcov, dmean = torch.ops.gpk.mvn_root_grad(R, gR, gsamples, eps_k)
    deps = None
    if ctx.has_eps and ctx.needs_input_grad[3] and gsamples is not None:
        deps = torch.einsum("bji,sbj->sbi", R, gsamples)   # R^T g per draw
    if ctx.mean_shape is None or not ctx.needs_input_grad[2]:
        dmean = None
    return dcov, None, dmean, deps, None


mvn_root.register_autograd(_mvn_root_backward, setup_context=_mvn_root_setup)

# ---------------------------------------------------------------------------
# Cholesky (full-covariance) q(u): gpk_variational_chol_f32 / gpk_variational_chol_adjoint_f32 /
# gpk_cholesky_kl_f32 and their batched forms (upstream CholeskyVariationalDistribution inside
# VariationalStrategy); Z (M, D) or (O, M, D) as above, m (M,) or (O, M) for the KL
# ---------------------------------------------------------------------------


def _chol_saved_numel(x, Z, save):
    B, N, D = x.shape[-3:]
    if not save or B < 1:
        return 0
    lib = _native.lib()
    if Z.dim() == 3:
        return lib.gpk_variational_chol_batched_saved_bytes(Z.shape[0], B, N, Z.shape[1], D) // 4
    return lib.gpk_variational_chol_saved_bytes(B, N, Z.shape[0], D) // 4


@torch.library.custom_op("gpk::variational_chol_fwd", mutates_args=(), device_types="cuda")
def variational_chol_fwd(x: Tensor, Linv: Tensor, Z: Tensor, vmean: Tensor, vchol: Tensor, s2: Tensor,
                         ls: Tensor, w: Tensor, b0: Tensor, jitter: float,
                         save: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (mean, var, clamp flags, packed hyper vector, saved state): gpk::variational_fwd with
    q(u) = N(vmean, tril(vchol) tril(vchol)^T). ``save`` (a gradient will be needed): the forward
    keeps A = Linv K_ZX and the clamp mask, which the adjoint reads; else the state is empty.
    Z (O, M, D): vmean (O, M), vchol (O, M, M), the other arguments as gpk::variational_fwd."""
    hyper = _pack_hyper(x, Z, s2, ls, w, b0, jitter)
    forward = ops.variational_chol_forward_batched if Z.dim() == 3 else ops.variational_chol_forward
    out = forward(x, Z, Linv, vmean, vchol, hyper, save=save)
    saved = out.saved if out.saved is not None else x.new_empty(0)
    return out.mean, out.var, out.flags, hyper, saved


@variational_chol_fwd.register_fake
def _(x, Linv, Z, vmean, vchol, s2, ls, w, b0, jitter, save=False):
    B, N, D = x.shape[-3:]
    lead = Z.shape[:-2]
    return (x.new_empty(*lead, B, N), x.new_empty(*lead, B, N), x.new_empty(1, dtype=torch.int32),
            x.new_empty(*lead, 4 + 2 * D), x.new_empty(_chol_saved_numel(x, Z, save)))


@torch.library.custom_op("gpk::variational_chol_adj", mutates_args=(), device_types="cuda")
def variational_chol_adj(x: Tensor, Linv: Tensor, Z: Tensor, vmean: Tensor, vchol: Tensor, hyper: Tensor,
                         gmean: Tensor, gvar: Tensor,
                         saved: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (dX, dLinv, dZ (K_ZX part), dpar = [dvmean (M), ds2, dls (D), dw (D), db0], dchol (M, M)
    lower) from the forward's ``saved`` state. Z (O, M, D): dX (O, B, N, D) per output and every
    other array with a leading O."""
    adjoint = ops.variational_chol_adjoint_batched if Z.dim() == 3 else ops.variational_chol_adjoint
    return adjoint(x, Z, Linv, vmean, vchol, hyper, gmean, gvar, saved)


@variational_chol_adj.register_fake
def _(x, Linv, Z, vmean, vchol, hyper, gmean, gvar, saved):
    M, D = Z.shape[-2:]
    lead = Z.shape[:-2]
    return (x.new_empty(*lead, *x.shape[-3:]), torch.empty_like(Linv), torch.empty_like(Z),
            x.new_empty(*lead, M + 2 * D + 2), x.new_empty(*lead, M, M))


def _vchol_setup(ctx, inputs, output):
    x, Linv, Z, vmean, vchol, s2, ls, w, b0, jitter = inputs[:10]
    ctx.save_for_backward(x, Linv, Z, vmean, vchol, s2, ls, w, b0, output[3], output[4])
    ctx.mark_non_differentiable(output[2], output[3], output[4])


def _vchol_backward(ctx, gmean, gvar, _gflags, _ghyper, _gsaved):
    x, Linv, Z, vmean, vchol, s2, ls, w, b0, hyper, saved = ctx.saved_tensors
    M, D = Z.shape[-2:]
    lead = Z.shape[:-2]
    B, N = x.shape[-3], x.shape[-2]
    if saved.numel() == 0 and B > 0:
        raise RuntimeError("gpk::variational_chol_fwd was called with save=False; no backward")
    if gmean is None:
        gmean = x.new_zeros(*lead, B, N)
    if gvar is None:
        gvar = x.new_zeros(*lead, B, N)
    if B == 0:
        dX, dLinv, dZ = x.new_zeros(*lead, B, N, D), torch.zeros_like(Linv), torch.zeros_like(Z)
        dpar, dchol = x.new_zeros(*lead, M + 2 * D + 2), x.new_zeros(*lead, M, M)
    else:
        dX, dLinv, dZ, dpar, dchol = torch.ops.gpk.variational_chol_adj(
            x, Linv, Z, vmean, vchol, hyper, gmean.contiguous(), gvar.contiguous(), saved)
    dX = _fold_x(dX, x, Z)
    dls = _fold_ls(dpar[..., M + 1:M + 1 + D], ls, Z)
    dw, db0 = _fold_mean(dpar[..., M + 1 + D:M + 1 + 2 * D], dpar[..., M + 1 + 2 * D], w, b0, Z)
    return (dX, dLinv, dZ, dpar[..., :M].reshape(vmean.shape), dchol.reshape(vchol.shape),
            dpar[..., M].reshape(s2.shape), dls, dw, db0, None, None)


variational_chol_fwd.register_autograd(_vchol_backward, setup_context=_vchol_setup)


@torch.library.custom_op("gpk::cholesky_kl", mutates_args=(), device_types="cuda")
def cholesky_kl(m: Tensor, chol: Tensor) -> Tensor:
    """(1,) KL(N(m, L L^T) || N(0, I)), L = tril(chol), of the whitened Cholesky q(u); m (O, M),
    chol (O, M, M): the (O,) KLs of the outputs in one launch."""
    if m.dim() == 2:
        return ops.cholesky_kl_batched(m, chol)
    return ops.cholesky_kl(m.contiguous().float(), chol.contiguous().float())


@cholesky_kl.register_fake
def _(m, chol):
    return m.new_empty(m.shape[0] if m.dim() == 2 else 1)


@torch.library.custom_op("gpk::cholesky_kl_grad", mutates_args=(), device_types="cuda")
def cholesky_kl_grad(m: Tensor, chol: Tensor, gkl: Tensor) -> Tuple[Tensor, Tensor]:
    if m.dim() == 2:
        return ops.cholesky_kl_grad_batched(m, chol, gkl)
    return ops.cholesky_kl_grad(m.contiguous().float(), chol.contiguous().float(),
                                gkl.reshape(1).contiguous().float())


@cholesky_kl_grad.register_fake
def _(m, chol, gkl):
    return torch.empty_like(m), torch.empty_like(chol)


def _ckl_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _ckl_backward(ctx, gkl):
    m, chol = ctx.saved_tensors
    dm, dchol = torch.ops.gpk.cholesky_kl_grad(m, chol, gkl.contiguous())
    return dm, dchol


cholesky_kl.register_autograd(_ckl_backward, setup_context=_ckl_setup)
