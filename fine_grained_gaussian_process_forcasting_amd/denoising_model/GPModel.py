"""ExactGPModel on the gfx950 kernels (reference denoising_model/GPModel.py:4-13).

Training mode: ``model(x)`` returns the prior MultivariateNormal(mean_x, covar_x)
lazily; ``ExactMarginalLogLikelihood(likelihood, model)(model(train_x), train_y)``
evaluates the per-window marginal log likelihood / N with ONE fused kernel (RBF Gram +
jittered Cholesky + forward solve + logdet): include/gpk.h::gpk_exact_mll_f32.

Eval mode: ``model(x)`` is the posterior of f at x (upstream
models/exact_gp.py __call__ -> exact_prediction_strategies.py): the training factor L
and z = L^{-1}(y - c) come from gpk_exact_mll_f32 once and are cached until a
parameter or the training data changes or ``train()`` is called (GPyTorch's
``prediction_strategy`` cache); mean and variance at x come from
gpk_exact_posterior_f32, and the joint covariance (``covariance_matrix``, ``rsample``,
``log_prob``) lazily from gpk_exact_posterior_cov_f32 on the same cached factor.
When a gradient can flow (a parameter, x or the training data requires grad), the same
quantities come from one gpk::exact_posterior_train call on the live parameters and the
backward is gpk_exact_posterior_grad_f32 (N <= 256 and up to 256 test points; beyond that the
differentiable torch restatement of ``_posterior_autograd``).
``likelihood(model(x))`` adds the noise. As in GPyTorch,
calling the model in eval mode on the training inputs warns (GPInputWarning) and
returns the posterior there.

``model.get_fantasy_model(new_x, new_y)`` conditions a model that has predicted on later
observations without fitting again: gpk_exact_append_f32 extends the cached factor by the new
points and the returned model starts with that cache. ``model.forget_oldest(m)`` is the other half
of a streaming look-back: gpk_exact_drop_f32 takes the m oldest points out of the cached factor
(a rank-m update of the trailing block), and ``model.get_sliding_model(new_x, new_y)`` does both,
so a window of constant N slides over a stream with no factorisation launch, also at N = 800
where ``get_fantasy_model`` alone has no room.

Inputs may be batched (B, N, D) windows, a single (N, D) window or 1-D (N,) points,
as GPyTorch accepts; targets follow (B, N) / (N,).

Hyper-parameters: by default ONE set {outputscale, noise, constant, lengthscale} shared by the B
windows (the reference's model). ``ExactGPModel(train_x, train_y, likelihood, batch_shape=
torch.Size([B]))`` with ``GaussianLikelihood(batch_shape=torch.Size([B]))`` is GPyTorch's
batch-independent exact GP: every window owns its set (``mean_module.constant`` (B, 1),
``raw_outputscale`` (B,), ``raw_lengthscale`` (B, 1, n), ``raw_noise`` (B, 1)), the B sets travel
as one (B, 3 + n_ls) matrix and every call is still one launch each way
(include/gpk.h, the *_perwin_f32 entry points). A shared likelihood with a batched model (or the
other way round) is a mixed model and works the same way.
"""
from __future__ import annotations

import copy
import warnings
import weakref

import torch
import torch.nn as nn

from .. import ops
from ..errors import GPInputWarning
from ..gp import ConstantMean, MultivariateNormal, RBFKernel, ScaleKernel, _per_window, psd_safe_cholesky


# forget_oldest uses the rank-m update when more than this many points are kept; up to it one fused
# forward on the kept data seeds the cache faster (measured: DESIGN.md §4.6c)
EXACT_DROP_MIN_KEPT = ops.EXACT_REG_MAX_N


def _as_batch(x: torch.Tensor) -> torch.Tensor:
    """(N,) -> (1, N, 1); (N, D) -> (1, N, D); (B, N, D) unchanged."""
    if x.dim() == 1:
        return x.reshape(1, -1, 1)
    if x.dim() == 2:
        return x.unsqueeze(0)
    if x.dim() == 3:
        return x
    raise ValueError(f"inputs must be (N,), (N, D) or (B, N, D), got {tuple(x.shape)}")


class _PredictionCacheHandle:
    """Lets ops_autograd.invalidate_caches() drop a model's prediction cache (HIP graph
    replays change parameters without bumping the version counters it is keyed on)."""

    def __init__(self, model):
        self._model = weakref.ref(model)

    def clear(self):
        m = self._model()
        if m is not None:
            m._prediction_cache = None


_NO_CACHE_MSG = ("Fantasy observations can only be added after making predictions with a model so "
                 "that all test independent caches exist. Call the model on some data first!")


def _version_key(*ts):
    return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in ts)


class ExactGPModel(nn.Module):
    def __init__(self, train_x, train_y, likelihood, batch_shape=torch.Size([]), ard_num_dims=None):
        super().__init__()
        batch_shape = torch.Size(batch_shape)
        if len(batch_shape) > 1:
            raise ValueError(f"batch_shape must be [] or [B], got {tuple(batch_shape)}")
        self.batch_shape = batch_shape
        self._check_windows(train_x)
        self.train_inputs = (train_x,)
        self.train_targets = train_y
        self.likelihood = likelihood
        if len(batch_shape) == 0 and ard_num_dims is None:
            self.mean_module = ConstantMean()
            self.covar_module = ScaleKernel(RBFKernel())
        else:
            self.mean_module = ConstantMean(batch_shape=batch_shape)
            self.covar_module = ScaleKernel(RBFKernel(ard_num_dims=ard_num_dims, batch_shape=batch_shape),
                                            batch_shape=batch_shape)
        self._prediction_cache = None
        self._cache_handle = _PredictionCacheHandle(self)
        from ..ops_autograd import register_cache
        register_cache(self._cache_handle)

    def _check_windows(self, x):
        """A batch-independent model owns one hyper-parameter set per window: its batch_shape [B]
        must be the windows of the inputs."""
        if len(self.batch_shape) == 0 or x is None:
            return
        windows = _as_batch(x).shape[:1]
        if windows != self.batch_shape:
            raise RuntimeError(f"batch_shape {tuple(self.batch_shape)} does not match the windows of the inputs: "
                               f"inputs of shape {tuple(x.shape)} hold {tuple(windows)} window(s)")

    def set_train_data(self, inputs=None, targets=None, strict=True):
        if inputs is not None:
            x = inputs[0] if isinstance(inputs, (tuple, list)) else inputs
            self._check_windows(x)
            if strict and x.shape != self.train_inputs[0].shape:
                raise RuntimeError("Cannot modify the shape of train inputs with strict=True")
            self.train_inputs = (x,)
        if targets is not None:
            if strict and targets.shape != self.train_targets.shape:
                raise RuntimeError("Cannot modify the shape of train targets with strict=True")
            self.train_targets = targets
        self._prediction_cache = None

    def train(self, mode: bool = True):
        self._prediction_cache = None       # GPyTorch drops its prediction strategy here
        return super().train(mode)

    def get_fantasy_model(self, inputs, targets, **kwargs):
        """A new model conditioned on the training data plus the observations (inputs, targets),
        without fitting again (upstream models/exact_gp.py ExactGP.get_fantasy_model): the cached
        training factor L and z = L^{-1}(y - c) are extended by the m new points in O(N^2 m) with
        one gpk::exact_append call (include/gpk.h::gpk_exact_append_f32) and seed the new model's
        prediction cache, so its first ``model(x)`` under ``no_grad`` launches no factorisation.
        Up to N + m = 256 the cache is seeded by the fused forward on the concatenated data instead,
        which is faster there than the update's launch chain.

        ``inputs`` is (m,), (m, D) or (B, m, D) (or a list / tuple of one such tensor), ``targets``
        (m,) or (B, m); an unbatched one is expanded to every window. The model must have been
        called in eval mode since the last ``train()`` / ``set_train_data`` (the test-independent
        caches must exist); otherwise RuntimeError, in upstream's words (GPyTorch 1.9 as
        remembered, unpinned). Upstream's batch of fantasies (``targets`` with one more leading
        dimension than the inputs) and the ``noise=`` keyword of FixedNoiseGaussianLikelihood
        raise NotImplementedError.

        Returns a deep copy of the modules (parameters included; the training data and the cached
        factor are taken off before the copy) with the concatenated ``train_inputs`` /
        ``train_targets``; this model and its cache are left untouched, and fantasies chain.
        With gradients the new model behaves as any model with that training data (the eval path
        under grad refits from the live parameters). More than 256 new points at once
        (gpk_mvn_root_max_n) give the new model without a seeded cache: its first eval call
        factors from scratch. The Schur complement's factorisation runs psd_safe_cholesky's jitter
        ladder (NumericalWarning per retry, NanError, NotPSDError)."""
        x, xn, yn, m = self._fantasy_args(inputs, targets, kwargs)
        train_x, train_y = self.train_inputs[0], self.train_targets
        Xb, L, z, hyper = self._train_factor()         # the cache, or a refit if it went stale
        B, N, D = Xb.shape
        from .. import _native
        if N + m > _native.lib().gpk_exact_max_n():
            _native.check(-6, ops._exact_name("mll", hyper.dim() - 1))    # what ops.exact_mll raises for N + m

        new_x = torch.cat([_as_batch(train_x), xn.to(train_x.dtype)], dim=1)
        new_x = new_x.reshape(-1) if train_x.dim() == 1 else (new_x.squeeze(0) if train_x.dim() == 2 else new_x)
        new_y = torch.cat([train_y.reshape(B, N), yn.to(train_y.dtype)], dim=1)
        new_y = new_y.reshape(-1) if train_y.dim() == 1 else new_y

        fm = self._clone_with_data(new_x, new_y)
        if m > _native.lib().gpk_mvn_root_max_n():
            return fm
        if N + m <= ops.EXACT_REG_MAX_N:
            # measured: up to N' = 256 the fused forward factors the concatenated
            # data faster than the update's launch chain, so the cache is seeded from scratch
            fm._train_factor()
            return fm
        from .. import library  # noqa: F401  (registers torch.ops.gpk)
        from ..gp import _exact_append_ladder
        xn_f = xn.detach().float().contiguous()
        yn_f = yn.detach().float().contiguous()
        L2, z2 = _exact_append_ladder(Xb, L, z, hyper, xn_f, yn_f)
        fm._seed_cache(L2, z2, hyper)
        return fm

    def _fantasy_args(self, inputs, targets, kwargs):
        """get_fantasy_model's argument checks, before any launch: -> (x, xn (B, m, D), yn (B, m), m)."""
        if kwargs.get("noise") is not None:
            raise NotImplementedError("get_fantasy_model(noise=...) belongs to FixedNoiseGaussianLikelihood, "
                                      "which this package does not have")
        x = inputs[0] if isinstance(inputs, (tuple, list)) else inputs
        xn = _as_batch(x)
        lead = 0 if x.dim() < 3 else 1                 # batch dimensions of the inputs
        if targets.dim() == lead + 2:
            raise NotImplementedError("a batch of fantasies (targets with one more leading dimension than the "
                                      "inputs) is not supported: add one set of observations per window")
        if targets.dim() != lead + 1 and not (lead == 1 and targets.dim() == 1):
            raise ValueError(f"targets must be (m,) or (B, m), got {tuple(targets.shape)}")
        if self._prediction_cache is None:
            raise RuntimeError(_NO_CACHE_MSG)
        self._check_windows(x)
        train_x = self.train_inputs[0]
        B, N, D = _as_batch(train_x).shape
        if xn.shape[-1] != D or xn.shape[0] not in (1, B):
            raise ValueError(f"inputs of shape {tuple(x.shape)} do not match the training inputs "
                             f"{tuple(train_x.shape)}")
        m = xn.shape[1]
        xn = xn.expand(B, m, D)
        if targets.shape[-1] != m or (targets.dim() == 2 and targets.shape[0] != B):
            raise ValueError(f"targets of shape {tuple(targets.shape)} do not match {m} new point(s) in {B} "
                             "window(s)")
        yn = targets.expand(B, m) if targets.dim() == 1 else targets
        return x, xn, yn, m

    def _clone_with_data(self, new_x, new_y):
        """A deep copy of the modules (parameters included) with (new_x, new_y) as training data, a
        prediction-cache handle of its own and no cache; the B N^2 factor and the training data are
        taken off before the copy."""
        saved = (self.train_inputs, self.train_targets, self._prediction_cache, self._cache_handle)
        self.train_inputs = self.train_targets = self._prediction_cache = self._cache_handle = None
        try:
            fm = copy.deepcopy(self)
        finally:
            self.train_inputs, self.train_targets, self._prediction_cache, self._cache_handle = saved
        fm.train_inputs = (new_x,)
        fm.train_targets = new_y
        fm._cache_handle = _PredictionCacheHandle(fm)
        from ..ops_autograd import register_cache
        register_cache(fm._cache_handle)
        return fm

    def _seed_cache(self, L, z, hyper):
        """Start with (L, z) as the prediction cache of the current training data and parameters."""
        train_x, train_y = self.train_inputs[0], self.train_targets
        kern = self.covar_module
        key = _version_key(train_x, train_y, kern.raw_outputscale, kern.base_kernel.raw_lengthscale,
                           self.mean_module.constant, self.likelihood.noise_covar.raw_noise)
        self._prediction_cache = (key, (_as_batch(train_x).detach().float(), L, z, hyper))

    def forget_oldest(self, m):
        """A new model whose training data are the last N - m points of every window (the oldest
        are the first along the point axis, the end ``get_fantasy_model`` does not append to),
        without fitting again: one gpk::exact_drop call (include/gpk.h::gpk_exact_drop_f32) turns
        the cached factor L and z = L^{-1}(y - c) into those of the kept points, a rank-m update of
        the trailing block in O((N - m)^2 m) that cannot fail, and seeds the new model's prediction
        cache. Upstream GPyTorch has no counterpart; with ``get_fantasy_model`` it makes a look-back
        of constant length (``get_sliding_model``).

        ``get_fantasy_model``'s contract: the model must have been called in eval mode since the
        last ``train()`` / ``set_train_data`` (RuntimeError otherwise); the result is a deep copy of
        the modules with contiguous copies of the kept ``train_inputs`` / ``train_targets`` and a
        cache handle of its own; this model and its cache are left untouched. 1 <= m < N, otherwise
        ValueError. The update is used for m <= 64 (gpk_exact_drop_max_m) where it was measured
        faster than factoring the kept points (N - m > 256); otherwise the cache
        is seeded by one factorisation of the kept data. With gradients the new model behaves as
        any model with that training data (the eval path under grad refits from the live
        parameters)."""
        if self._prediction_cache is None:
            raise RuntimeError(_NO_CACHE_MSG)
        m = int(m)
        train_x, train_y = self.train_inputs[0], self.train_targets
        N = _as_batch(train_x).shape[1]
        if m < 1 or m >= N:
            raise ValueError(f"m must be in 1 .. N - 1 = {N - 1}, got {m}")
        Xb, L, z, hyper = self._train_factor()         # the cache, or a refit if it went stale
        new_x = (train_x[:, m:] if train_x.dim() == 3 else train_x[m:]).clone()
        new_y = train_y[..., m:].clone()
        fm = self._clone_with_data(new_x, new_y)
        from .. import _native
        if m > _native.lib().gpk_exact_drop_max_m() or N - m <= EXACT_DROP_MIN_KEPT:
            fm._train_factor()
            return fm
        from .. import library  # noqa: F401  (registers torch.ops.gpk)
        L2, z2 = torch.ops.gpk.exact_drop(L, z, m)
        fm._seed_cache(L2, z2, hyper)
        return fm

    def get_sliding_model(self, inputs, targets, **kwargs):
        """``forget_oldest(m).get_fantasy_model(inputs, targets)`` with m the number of new points:
        the look-back keeps its length N while it takes the m newest observations and forgets the m
        oldest, with no factorisation launch where both updates apply. Works at N = 800
        (gpk_exact_max_n), where ``get_fantasy_model`` alone raises. Arguments and errors as
        ``get_fantasy_model``, checked before any launch; m < N."""
        _, _, _, m = self._fantasy_args(inputs, targets, kwargs)
        N = _as_batch(self.train_inputs[0]).shape[1]
        if m >= N:
            raise ValueError(f"{m} new point(s) would replace all {N} training point(s) of a window")
        return self.forget_oldest(m).get_fantasy_model(inputs, targets, **kwargs)

    def forward(self, x):
        self._check_windows(x)
        xb = _as_batch(x)
        mean_x = self.mean_module(x if x.dim() > 1 else x.unsqueeze(-1))
        return MultivariateNormal(mean_x, None,
                                  exact=(xb, self.covar_module.base_kernel.lengthscale,
                                         self.covar_module.outputscale, self.mean_module.constant))

    def __call__(self, x=None):
        if x is None:
            x = self.train_inputs[0]
        if self.training:
            return self.forward(x)
        train_x = self.train_inputs[0]
        if x.shape == train_x.shape and torch.equal(x, train_x):
            warnings.warn("The input matches the stored training data. Did you forget to call "
                          "model.train()?", GPInputWarning)
        return self._posterior(x)

    # ---- eval mode -------------------------------------------------------------
    def _per_window(self) -> bool:
        """Whether any hyper-parameter carries a window dimension (the model's batch_shape [B], or a
        batched likelihood on a shared model)."""
        kern = self.covar_module
        B = _as_batch(self.train_inputs[0]).shape[0]
        return ops.exact_hyper_per_window(kern.raw_outputscale, self.likelihood.noise_covar.raw_noise,
                                          self.mean_module.constant, kern.base_kernel.raw_lengthscale, B)

    def _hyper(self, device):
        """The packed hyper-parameters, detached: (3 + n_ls,) shared, or (B, 3 + n_ls) per window."""
        kern = self.covar_module
        if self._per_window():
            B = _as_batch(self.train_inputs[0]).shape[0]
            return ops.pack_exact_hyper_windows(kern.outputscale, self.likelihood.noise, self.mean_module.constant,
                                                kern.base_kernel.lengthscale, B).detach().to(device).contiguous()
        return ops.pack_exact_hyper(kern.outputscale, self.likelihood.noise, self.mean_module.constant,
                                    kern.base_kernel.lengthscale, device)

    def _hyper_live(self):
        """The same, built differentiably (dhyp reaches the parameters through the constraints)."""
        kern = self.covar_module
        if self._per_window():
            B = _as_batch(self.train_inputs[0]).shape[0]
            return ops.pack_exact_hyper_windows(kern.outputscale, self.likelihood.noise, self.mean_module.constant,
                                                kern.base_kernel.lengthscale, B)
        return ops.pack_exact_hyper_live(kern.outputscale, self.likelihood.noise, self.mean_module.constant,
                                         kern.base_kernel.lengthscale)

    def _train_factor(self):
        train_x, train_y = self.train_inputs[0], self.train_targets
        kern = self.covar_module
        key = _version_key(train_x, train_y, kern.raw_outputscale, kern.base_kernel.raw_lengthscale,
                           self.mean_module.constant, self.likelihood.noise_covar.raw_noise)
        cache = self._prediction_cache
        if cache is not None and cache[0] == key:
            return cache[1]
        Xb = _as_batch(train_x).detach().float()
        yb = train_y.detach().reshape(Xb.shape[0], Xb.shape[1]).float()
        hyper = self._hyper(Xb.device).detach()
        out = ops.exact_mll(Xb, yb, None, None, None, None, want_L=True, want_z=True, hyper=hyper)
        ops.check_cholesky_info(out.info, 1e-6, inputs=(Xb, yb))
        entry = (Xb, out.L, out.z, hyper)
        self._prediction_cache = (key, entry)
        return entry

    def _posterior(self, x):
        self._check_windows(x)
        params = [p for p in self.parameters()] + [x, self.train_inputs[0], self.train_targets]
        if torch.is_grad_enabled() and any(t.requires_grad for t in params):
            if self._grad_on_kernels(x):
                return self._posterior_kernels_grad(x)
            return self._posterior_autograd(x)
        Xb, L, z, hyper = self._train_factor()
        xs = _as_batch(x).float()
        if xs.shape[0] != Xb.shape[0]:
            xs = xs.expand(Xb.shape[0], *xs.shape[1:])
        from .. import library  # noqa: F401  (registers torch.ops.gpk)
        xs = xs.contiguous()
        mean, var = torch.ops.gpk.exact_posterior(Xb, L, z, hyper, xs)
        if x.dim() == 3 or Xb.shape[0] > 1:
            shape = mean.shape                    # (B, Ns): one posterior per training window
        else:
            shape = x.shape[:-1] if x.dim() > 1 else x.shape
        xs_d = xs.detach()
        memo = []

        def cov():
            # the joint posterior, lazily as upstream (exact_predictive_covar): one
            # gpk_exact_posterior_cov_f32 call on the cached factor, on first use only
            if not memo:
                memo.append(torch.ops.gpk.exact_posterior_cov(Xb, L, z, hyper, xs_d)[2])
            return memo[0]

        return MultivariateNormal(mean.reshape(shape), var.reshape(shape), covar_fn=cov)

    def _grad_on_kernels(self, x) -> bool:
        """Whether the differentiable posterior runs on the HIP kernels (gpk::exact_posterior_train,
        backward gpk_exact_posterior_grad_f32): CUDA fp32 tensors of a shape the adjoint's workspace
        query accepts (N <= 256, Ns <= 256, D <= 64)."""
        train_x, train_y = self.train_inputs[0], self.train_targets
        ts = [x, train_x, train_y] + [p for p in self.parameters()]
        if not all(t.is_cuda and t.dtype == torch.float32 for t in ts):
            return False
        Xb, xs = _as_batch(train_x), _as_batch(x)
        if xs.shape[-1] != Xb.shape[-1] or xs.shape[0] not in (1, Xb.shape[0]):
            return False
        from .. import _native
        B, N, D = Xb.shape
        return _native.lib().gpk_exact_posterior_grad_workspace_bytes(B, N, xs.shape[1], D) > 0

    def _posterior_kernels_grad(self, x):
        """The eval posterior WITH gradients on the kernels: the factor, mean, variance and joint
        covariance of one gpk::exact_posterior_train call on the live parameters (the packed hyper
        vector is built differentiably, so the softplus constraints chain through torch), whose
        backward is gpk_exact_posterior_grad_f32. The prediction cache is not used, as GPyTorch
        does not cache through autograd either."""
        from .. import library  # noqa: F401  (registers torch.ops.gpk)
        train_x, train_y = self.train_inputs[0], self.train_targets
        Xb = _as_batch(train_x)
        yb = train_y.reshape(Xb.shape[0], Xb.shape[1])
        xs = _as_batch(x)
        if xs.shape[0] != Xb.shape[0]:
            xs = xs.expand(Xb.shape[0], *xs.shape[1:])
        # pack_exact_hyper's layout, but not detached (it detaches): dhyp must reach the parameters
        hyper = self._hyper_live()
        mean, var, cov, _L, _z, _state, info = torch.ops.gpk.exact_posterior_train(
            Xb.contiguous(), yb.contiguous(), hyper, xs.contiguous(), 1e-6, 3)
        ops.check_cholesky_info(info, 1e-6, inputs=(Xb, yb))
        if x.dim() == 3 or Xb.shape[0] > 1:
            shape = mean.shape
        else:
            shape = x.shape[:-1] if x.dim() > 1 else x.shape
        return MultivariateNormal(mean.reshape(shape), var.reshape(shape), covar_fn=lambda: cov)

    def _posterior_autograd(self, x):
        """The eval posterior WITH gradients where gpk_exact_posterior_grad_f32 does not reach
        (N > 256 or more than 256 test points, other dtypes; CPU tensors raise) (GPyTorch allows
        them; upstream
        exact_prediction_strategies.py): the same quantities as gpk_exact_posterior_f32,
        restated in differentiable torch ops on the caller's device -- K_hat = s2 RBF(X, X) +
        noise I, L = psd_safe_cholesky(K_hat) (the fp32 jitter ladder), K* = s2 RBF(X, x) over the
        joint inputs in upstream ``_sq_dist``'s centred GEMM form, V = L^{-1} K*,
        z = L^{-1} (y - c), mean = c + V^T z, var = s2 - colsum(V o V). Taken only when a
        gradient will flow (a parameter, the inputs or the training data require grad): the
        prediction cache is not used, as GPyTorch does not cache through autograd either.
        Off the hot path: no HIP kernel serves these shapes."""
        train_x, train_y = self.train_inputs[0], self.train_targets
        if not (x.is_cuda and train_x.is_cuda):
            raise ValueError("ExactGPModel runs on the GPU: move the model and inputs to a cuda device")
        Xb = _as_batch(train_x)
        yb = train_y.reshape(Xb.shape[0], Xb.shape[1])
        xs = _as_batch(x)
        if xs.shape[0] != Xb.shape[0]:
            xs = xs.expand(Xb.shape[0], *xs.shape[1:])
        kern = self.covar_module
        B = Xb.shape[0]

        def hyp(t, shared, min_dim=1):
            # a per-window hyper-parameter (leading size B) broadcasts over its window's matrix
            return t.reshape(B, 1, -1) if _per_window(t, B, min_dim) else t.reshape(shared)

        ls = hyp(kern.base_kernel.lengthscale, (-1,), 2)
        s2 = hyp(kern.outputscale, ())
        c = hyp(self.mean_module.constant, ())
        noise = hyp(self.likelihood.noise, ())
        n = Xb.shape[-2]
        full = torch.cat([Xb, xs], -2) / ls
        a = full - full.mean(-2, keepdim=True)
        nrm = a.pow(2).sum(-1, keepdim=True)
        d = (nrm + nrm.transpose(-1, -2) - 2.0 * a @ a.transpose(-1, -2)).clamp_min(0.0)
        K = s2 * torch.exp(-0.5 * d)
        eye = torch.eye(n, dtype=K.dtype, device=K.device)
        Kxx = K[..., :n, :n] * (1.0 - eye) + s2 * eye        # exact diagonal, as _sq_dist zeroes it
        L = psd_safe_cholesky(Kxx + noise * eye)
        V = torch.linalg.solve_triangular(L, K[..., :n, n:], upper=False)
        zz = torch.linalg.solve_triangular(L, yb.unsqueeze(-1) - c, upper=False)
        mean = (c + (V * zz).sum(-2, keepdim=True)).squeeze(-2)
        var = (s2 - (V * V).sum(-2, keepdim=True)).squeeze(-2)
        if x.dim() == 3 or Xb.shape[0] > 1:
            shape = mean.shape
        else:
            shape = x.shape[:-1] if x.dim() > 1 else x.shape
        # the joint posterior of the same restatement, differentiable: K** - V^T V
        return MultivariateNormal(mean.reshape(shape), var.reshape(shape),
                                  covar_fn=lambda: K[..., n:, n:] - V.transpose(-1, -2) @ V)
