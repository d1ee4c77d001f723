"""gpytorch-free building blocks of the reference GP path, backed by the gfx950 kernels.

Mirrors the GPyTorch 1.9.x objects the reference touches with
the same module / parameter names, so the reference's call sites
(denoising_model/DeepGP.py, GPModel.py, denoise_model_2.py, forecast_denoising.py:86-89,
train.py:20) read the same and its state_dicts keep their keys:

  settings.num_likelihood_samples        gpytorch.settings.num_likelihood_samples
  Positive / GreaterThan                 gpytorch.constraints (softplus transform)
  RBFKernel / ScaleKernel                gpytorch.kernels (raw_lengthscale, raw_outputscale)
  ConstantMean / LinearMean              gpytorch.means
  GaussianLikelihood                     gpytorch.likelihoods (noise_covar.raw_noise)
  MultivariateNormal                     gpytorch.distributions (mean, variance clamp)
  MeanFieldVariationalDistribution       gpytorch.variational
  CholeskyVariationalDistribution        gpytorch.variational (chol_variational_covar)
  VariationalStrategy                    gpytorch.variational (whitened)
  VariationalELBO / DeepApproximateMLL   gpytorch.mlls
  ExactMarginalLogLikelihood             gpytorch.mlls

All arithmetic of the hot path runs in libgpk.so (ops.py); torch is used for
parameters, the tiny constrained-value transforms and elementwise glue on the
device. Gradients: see ops_autograd.py.
"""
from __future__ import annotations

import contextlib
import math
import threading
import warnings
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .errors import NumericalWarning

LOG_2PI = math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------
# settings (upstream gpytorch/settings.py)
# ---------------------------------------------------------------------------
class _Setting:
    """One process-wide value, like GPyTorch's ``_value_context``: entering the context
    stores the value once for the whole process (``_global_value`` is a class
    attribute there), so a value set on the main thread (train.py:20) is what the
    Optuna worker threads (train.py:86, n_jobs=4) read. Exit restores the value that
    was current on entry."""

    _lock = threading.Lock()
    _UNSET = object()

    def __init__(self, default):
        self._default = default
        self._value = self._UNSET

    def value(self, dtype=None):
        v = self._value
        if v is not self._UNSET:
            return v
        if isinstance(self._default, dict):
            return self._default.get(dtype, self._default.get(None))
        return self._default

    @contextlib.contextmanager
    def __call__(self, value):
        with self._lock:
            prev = self._value
            self._value = value
        try:
            yield
        finally:
            with self._lock:
                self._value = prev


class settings:
    """The gpytorch.settings used on this path (process-global like GPyTorch's)."""
    num_likelihood_samples = _Setting(10)          # train.py:20 sets 1
    cholesky_jitter = _Setting({torch.float32: 1e-6, torch.float64: 1e-8, None: 1e-6})
    cholesky_max_tries = _Setting(3)
    variational_cholesky_jitter = _Setting({torch.float32: 1e-4, torch.float64: 1e-6, None: 1e-4})
    min_variance = _Setting({torch.float32: 1e-6, torch.float64: 1e-10, None: 1e-6})
    max_cholesky_size = _Setting(800)


# ---------------------------------------------------------------------------
# constraints (upstream constraints/constraints.py)
# ---------------------------------------------------------------------------
class Interval(nn.Module):
    def __init__(self, lower_bound, upper_bound):
        super().__init__()
        self.register_buffer("lower_bound", torch.as_tensor(float(lower_bound)))
        self.register_buffer("upper_bound", torch.as_tensor(float(upper_bound)))

    def transform(self, raw):
        return F.softplus(raw) + self.lower_bound.to(raw.dtype)

    def inverse_transform(self, value):
        v = torch.as_tensor(value) - self.lower_bound
        return torch.where(v > 20, v, torch.log(torch.expm1(v)))


class Positive(Interval):
    def __init__(self):
        super().__init__(0.0, math.inf)


class GreaterThan(Interval):
    def __init__(self, lower_bound):
        super().__init__(lower_bound, math.inf)


# ---------------------------------------------------------------------------
# kernels / means (upstream kernels/rbf_kernel.py, scale_kernel.py, means/*)
# ---------------------------------------------------------------------------
class RBFKernel(nn.Module):
    """Lengthscale holder of gpytorch.kernels.RBFKernel; shape (*batch, 1, ard or 1)."""

    def __init__(self, ard_num_dims: Optional[int] = None, batch_shape=torch.Size([])):
        super().__init__()
        self.ard_num_dims = ard_num_dims
        n = 1 if ard_num_dims is None else ard_num_dims
        self.register_parameter("raw_lengthscale", nn.Parameter(torch.zeros(*batch_shape, 1, n)))
        self.register_module("raw_lengthscale_constraint", Positive())

    @property
    def lengthscale(self):
        return self.raw_lengthscale_constraint.transform(self.raw_lengthscale)


class ScaleKernel(nn.Module):
    def __init__(self, base_kernel: RBFKernel, batch_shape=torch.Size([]), ard_num_dims=None):
        super().__init__()
        self.base_kernel = base_kernel
        self.register_parameter("raw_outputscale", nn.Parameter(torch.zeros(torch.Size(batch_shape))))
        self.register_module("raw_outputscale_constraint", Positive())

    @property
    def outputscale(self):
        return self.raw_outputscale_constraint.transform(self.raw_outputscale)


class ConstantMean(nn.Module):
    def __init__(self, batch_shape=torch.Size([])):
        super().__init__()
        self.register_parameter("constant", nn.Parameter(torch.zeros(*batch_shape, 1)))

    def forward(self, x):
        return self.constant.expand(*x.shape[:-1])


class LinearMean(nn.Module):
    def __init__(self, input_size: int, batch_shape=torch.Size([]), bias: bool = True):
        super().__init__()
        self.register_parameter("weights", nn.Parameter(torch.randn(*batch_shape, input_size, 1)))
        if bias:
            self.register_parameter("bias", nn.Parameter(torch.randn(*batch_shape, 1)))
        else:
            self.bias = None

    def forward(self, x):
        res = x.matmul(self.weights).squeeze(-1)
        return res + self.bias if self.bias is not None else res


# ---------------------------------------------------------------------------
# distributions (upstream distributions/multivariate_normal.py)
# ---------------------------------------------------------------------------
def warn_if_clamped(flag: torch.Tensor, min_var: float) -> None:
    """GPyTorch's NumericalWarning when the variational kernel clamped a variance."""
    if int(flag.item()) & 1:
        warnings.warn(f"Negative variance values detected. This is likely due to numerical "
                      f"instabilities. Rounding negative variances up to {min_var}.",
                      NumericalWarning)


class MultivariateNormal:
    """Diagonal-query MVN of the hot path.

    Holds what the reference reads from the GP output: ``mean`` and the marginal
    ``variance`` (clamped at settings.min_variance with GPyTorch's
    NumericalWarning), batch_shape / event_shape semantics and ``expand``. Exact-GP
    priors also carry the window inputs so ``log_prob`` can run the fused kernel.
    """

    def __init__(self, mean: torch.Tensor, variance: Optional[torch.Tensor] = None,
                 exact=None, added_noise=None, clamp_flag: Optional[torch.Tensor] = None,
                 preclamped: bool = False, covar_fn=None):
        self._mean = mean
        self._variance = variance
        self._exact = exact                # (X, kernel hyper) for exact-GP priors
        self._added_noise = added_noise    # likelihood noise folded in by GaussianLikelihood
        self._clamp_flag = clamp_flag      # (1,) int32 from gpk_variational_f32: clamp fired
        self._preclamped = preclamped      # variance already clamped by the kernel, no flag
        # () -> dense (..., N, N) covariance of a variational output (its lazy covariance, as
        # GPyTorch's VariationalStrategy builds it); materialised only by covariance_matrix /
        # rsample, never on the hot path
        self._covar_fn = covar_fn

    @property
    def mean(self):
        return self._mean

    @property
    def loc(self):
        return self._mean

    @property
    def batch_shape(self):
        return self._mean.shape[:-1]

    @property
    def event_shape(self):
        return self._mean.shape[-1:]

    def _over_points(self, t):
        """A hyper-parameter against the (..., N) marginals: one value, or one per window (the
        batch entries of the mean) as (..., 1)."""
        if not torch.is_tensor(t) or t.numel() == 1:
            return t.reshape(()) if torch.is_tensor(t) else t
        if t.numel() == self._mean.shape[:-1].numel():
            return t.reshape(*self._mean.shape[:-1], 1)
        return t

    @property
    def variance(self):
        if self._variance is None:
            if self._exact is None:
                raise NotImplementedError("this distribution carries no variance")
            # exact-GP prior: diag K(x, x) = outputscale (the RBF is 1 on the diagonal), as
            # GPyTorch's lazy kernel diagonal returns it
            # (a per-window outputscale (B,) of a batch-independent model: one value per window)
            var = self._over_points(self._exact[2]).expand(self._mean.shape)
        else:
            var = self._variance
        if self._added_noise is not None:
            var = var + self._over_points(self._added_noise)
        min_var = settings.min_variance.value(var.dtype)
        if self._preclamped and self._added_noise is None:
            # a point slice of a kernel output: a clamped entry is exactly min_var
            from .ops import record_or_run
            flag = (var <= min_var).any().to(torch.int32).reshape(1)
            record_or_run("clamp", (flag, min_var), lambda: warn_if_clamped(flag, min_var))
            return var
        if self._clamp_flag is not None and self._added_noise is None:
            # the kernel already clamped (fp32 min_variance); it tells us whether it did:
            # one host read of the flag, as GPyTorch's own .lt(min_var).any() sync
            # (recorded instead while a HIP graph is captured, ops.DeferredChecks)
            from .ops import record_or_run
            flag = self._clamp_flag
            record_or_run("clamp", (flag, min_var), lambda: warn_if_clamped(flag, min_var))
            return var
        if bool((var < min_var).any()):
            warnings.warn(f"Negative variance values detected. This is likely due to numerical "
                          f"instabilities. Rounding negative variances up to {min_var}.",
                          NumericalWarning)
            var = var.clamp_min(min_var)
        return var

    @property
    def stddev(self):
        return self.variance.sqrt()

    @property
    def covariance_matrix(self):
        """Dense covariance, materialised on request (GPyTorch keeps it lazy and evaluates it
        here), + the added likelihood noise on the diagonal. Exact-GP / layer priors:
        outputscale * RBF with upstream ``_sq_dist`` semantics (inputs centred by their mean,
        clamp at 0, exact 0 on the diagonal). Distributions with a ``covar_fn``: what it
        returns -- the exact posterior's K** - K*^T K_hat^{-1} K* (gpk_exact_posterior_cov_f32;
        its diagonal is the unclamped variance, min_variance applies to ``.variance`` only, as
        upstream) and the variational outputs' lazy covariance. Not on the hot path: no
        reference caller reads it. A distribution built from a mean and marginal variances
        alone carries no covariance."""
        if self._exact is None and self._covar_fn is None:
            raise NotImplementedError("this distribution carries only marginal variances; "
                                      "covariance_matrix is provided for exact-GP / layer priors, "
                                      "the exact posterior and variational outputs")
        if self._exact is not None:
            X, lengthscale, outputscale, _ = self._exact
            K = rbf_covariance(X, lengthscale, outputscale)
        else:
            K = self._covar_fn()
        if self._added_noise is not None:
            noise = torch.as_tensor(self._added_noise, dtype=K.dtype, device=K.device)
            if _per_window(noise, K.shape[0]):
                noise = noise.reshape(-1, 1)          # (B, 1): one noise per window
            K = K + torch.diag_embed(noise.expand(K.shape[:-1]))
        n = self._mean.shape[-1]
        if K.numel() != self._mean.numel() * n:   # an expanded distribution: its batch is a view
            K = K.expand(*self._mean.shape, n)
        return K.reshape(*self._mean.shape, n)

    @property
    def lazy_covariance_matrix(self):
        return self.covariance_matrix

    def confidence_region(self):
        """(mean - 2 stddev, mean + 2 stddev), as upstream MultivariateNormal.confidence_region."""
        std2 = self.stddev.mul(2)
        return self._mean.sub(std2), self._mean.add(std2)

    def rsample(self, sample_shape=torch.Size(), base_samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Reparameterised sample mean + chol(Sigma) eps (upstream MultivariateNormal.rsample: the
        covariance root by psd_safe_cholesky with the jitter ladder). Off the hot path: the dense
        covariance is materialised (covariance_matrix). A CUDA fp32 distribution of n <= 256 points
        draws by gpk_mvn_root_f32 (factor and mean + R eps in one launch, leading sample dimensions
        as S), with or without gradients: its backward is gpk_mvn_root_grad_f32. Every other case
        (CPU, fp64, n > 256, empty) is torch arithmetic."""
        cov = self.covariance_matrix
        shape = torch.Size(sample_shape) + self._mean.shape
        if base_samples is None:
            base_samples = torch.randn(shape, dtype=self._mean.dtype, device=self._mean.device)
        elif base_samples.shape != shape:
            raise RuntimeError(f"base_samples shape {tuple(base_samples.shape)} != {tuple(shape)}")
        if (_mvn_root_eligible(cov) and self._mean.dtype == torch.float32 and base_samples.numel() > 0
                and base_samples.is_cuda and base_samples.dtype == torch.float32):
            # the factor and mean + R eps in one launch (gpk_mvn_root_f32), the leading sample
            # dimensions as its S; psd_safe_cholesky's ladder around it
            n = self._mean.shape[-1]
            nb = self._mean.numel() // n
            _, smp = _mvn_root_ladder(cov.reshape(nb, n, n), None, self._mean.reshape(nb, n),
                                      base_samples.reshape(-1, nb, n), want_R=False)
            return smp.reshape(shape)
        root = psd_safe_cholesky(cov)
        return self._mean + (root @ base_samples.unsqueeze(-1)).squeeze(-1)

    def sample(self, sample_shape=torch.Size(), base_samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        with torch.no_grad():
            return self.rsample(sample_shape, base_samples)

    def expand(self, batch_size):
        batch_size = torch.Size(batch_size)
        mean = self._mean.expand(*batch_size, *self.event_shape)
        var = self._variance.expand(*batch_size, *self.event_shape) if self._variance is not None else None
        exact = self._exact
        if exact is not None:
            # the prior's inputs follow the mean's batch, so covariance_matrix / log_prob of the
            # expanded distribution see one input set per batch entry (GPyTorch expands the lazy
            # kernel tensor the same way)
            X = exact[0]
            n, d = X.shape[-2:]
            if X.numel() != self.batch_shape.numel() * n * d:
                raise NotImplementedError("expand of an exact prior whose inputs do not follow its batch")
            Xe = X.reshape(*self.batch_shape, n, d).expand(*batch_size, n, d).reshape(-1, n, d)
            # per-window hyper-parameters (a batch-independent model) follow their windows
            nb, ne = self.batch_shape.numel(), Xe.shape[0]

            def follow(t, min_dim=1):
                if not _per_window(t, nb, min_dim):
                    return t
                rest = t.shape[1:]
                return t.reshape(*self.batch_shape, *rest).expand(*batch_size, *rest).reshape(ne, *rest)

            exact = (Xe, follow(exact[1], 2)) + tuple(follow(t) for t in exact[2:])
            noise = follow(self._added_noise)
            return MultivariateNormal(mean, var, exact, noise, self._clamp_flag, self._preclamped, self._covar_fn)
        return MultivariateNormal(mean, var, exact, self._added_noise, self._clamp_flag,
                                  self._preclamped, self._covar_fn)

    def add_noise(self, noise):
        total = noise if self._added_noise is None else self._added_noise + noise
        return MultivariateNormal(self._mean, self._variance, self._exact, total, self._clamp_flag,
                                  self._preclamped, self._covar_fn)

    def slice_points(self, start, stop):
        """The marginals of points [start, stop) (diagonal-query outputs of the variational
        path only): the clamp warning then reflects exactly the sliced points."""
        if self._exact is not None or self._variance is None:
            raise NotImplementedError("point slices are defined for variational outputs")
        sl = (Ellipsis, slice(start, stop))
        cf = self._covar_fn
        sub = (lambda: cf()[..., start:stop, start:stop]) if cf is not None else None
        return MultivariateNormal(self._mean[sl], self._variance[sl], None, self._added_noise, None,
                                  preclamped=self._clamp_flag is not None or self._preclamped, covar_fn=sub)

    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        """Exact-GP priors: the marginal log density by the fused RBF + Cholesky + solve + logdet
        kernel. Distributions that carry a dense covariance (``covar_fn``: the exact posterior,
        variational outputs): the Gaussian log density through R = psd_safe_cholesky(Sigma),
        -0.5 (|R^{-1}(value - mean)|^2 + 2 sum log R_ii + n log 2 pi), as upstream
        MultivariateNormal.log_prob (off the hot path: Sigma is materialised). Where the root is
        the HIP one (CUDA fp32, n <= 256) the whitening solve is gpk_tri_solve_f32; elsewhere
        torch.linalg.solve_triangular."""
        if self._exact is None and self._covar_fn is not None:
            cov = self.covariance_matrix
            root = psd_safe_cholesky(cov)
            diff = (value - self._mean).unsqueeze(-1)
            if diff.shape[:-2] != root.shape[:-2]:   # leading sample dimensions of value
                root = root.expand(*diff.shape[:-2], *root.shape[-2:])
            n = self._mean.shape[-1]
            if _mvn_root_eligible(root) and diff.dtype == torch.float32 and diff.is_cuda and diff.numel() > 0:
                # the root came from gpk_mvn_root_f32; the whitening is gpk_tri_solve_f32 (differentiable)
                from . import library  # noqa: F401  (registers torch.ops.gpk)
                w = torch.ops.gpk.tri_solve(root.reshape(-1, n, n).contiguous(), diff.reshape(-1, n).contiguous(),
                                            False).reshape(diff.shape[:-1])
            else:
                w = torch.linalg.solve_triangular(root, diff.to(root.dtype), upper=False).squeeze(-1)
            logdet = 2.0 * root.diagonal(dim1=-2, dim2=-1).log().sum(-1)
            return -0.5 * (w.pow(2).sum(-1) + logdet + n * math.log(2.0 * math.pi))
        if self._exact is None:
            raise NotImplementedError("log_prob needs a covariance: an exact-GP prior (GPModel.py) "
                                      "or a distribution with a dense covariance (covar_fn)")
        X, lengthscale, outputscale, constant = self._exact
        noise = self._added_noise if self._added_noise is not None else torch.zeros((), device=X.device)
        from .ops_autograd import exact_log_prob
        n = X.shape[-2]
        target = value.reshape(X.shape[:-1])
        if constant is None:
            # a general (e.g. LinearMean) prior mean: the fused kernel's constant mean is 0 and
            # the residual value - mean(x) is its target (the same MVN density)
            target = target - self._mean.reshape(X.shape[:-1])
            constant = torch.zeros((), device=X.device)
        res = exact_log_prob(X, target, lengthscale, outputscale, constant, noise) * n
        return res.reshape(value.shape[:-1])      # (N,) targets of an unbatched model -> scalar


def _per_window(t, B: int, min_dim: int = 1) -> bool:
    """Whether a hyper-parameter carries a window dimension: a tensor whose leading size is the
    B > 1 windows ((B,), (B, 1); the lengthscale, ``min_dim`` 2: (B, 1, n)), as the parameters of a
    batch-independent model (batch_shape = [B]) have. A shared one holds 1 (n) values, leading size 1."""
    return torch.is_tensor(t) and B > 1 and t.dim() >= min_dim and t.shape[0] == B


def rbf_covariance(X: torch.Tensor, lengthscale, outputscale) -> torch.Tensor:
    """outputscale * exp(-||x_i - x_j||^2 / (2 l^2)) for X (B, N, D), as GPyTorch's
    ScaleKernel(RBFKernel) evaluates a lazy kernel tensor (upstream kernels/rbf_kernel.py,
    kernel.py ``_sq_dist``: inputs divided by the lengthscale and centred by their mean,
    ||a||^2 + ||b||^2 - 2 a.b clamped at 0, the x1 == x2 diagonal set to exactly 0).
    Per-window hyper-parameters: lengthscale (B, 1, n) and / or outputscale (B,) give window b
    its own kernel."""
    B = X.shape[0] if X.dim() == 3 else 1
    ls = torch.as_tensor(lengthscale, device=X.device, dtype=X.dtype)
    ls = ls.reshape(B, 1, -1) if _per_window(ls, B, 2) else ls.reshape(-1)
    xs = X / ls
    xs = xs - xs.mean(-2, keepdim=True)
    nrm = xs.pow(2).sum(-1)
    d = (nrm.unsqueeze(-1) + nrm.unsqueeze(-2) - 2.0 * xs @ xs.transpose(-1, -2)).clamp_min(0.0)
    d = d * (1.0 - torch.eye(X.shape[-2], device=X.device, dtype=X.dtype))
    s2 = torch.as_tensor(outputscale, device=X.device, dtype=X.dtype)
    s2 = s2.reshape(B, 1, 1) if _per_window(s2, B) else s2.reshape(())
    return s2 * torch.exp(-0.5 * d)


def _no_grad_flows(*tensors) -> bool:
    """No gradient can flow through an op on these tensors: grad mode is off, or none of them
    requires grad."""
    return not torch.is_grad_enabled() or not any(torch.is_tensor(t) and t.requires_grad for t in tensors)


# Size rule of the HIP root: gpk_mvn_root_f32 keeps one matrix in one workgroup's LDS.
MVN_ROOT_MAX_N = ops.MVN_ROOT_MAX_N


def _mvn_root_eligible(A: torch.Tensor) -> bool:
    """A dense covariance (batch) the HIP Cholesky root takes: CUDA, fp32, 1 <= n <= 256, with
    or without a gradient through it (gpk::mvn_root carries its adjoint)."""
    return (torch.is_tensor(A) and A.is_cuda and A.dtype == torch.float32 and A.dim() >= 2
            and A.shape[-1] == A.shape[-2] and 1 <= A.shape[-1] <= MVN_ROOT_MAX_N)


def _mvn_root_ladder(A: torch.Tensor, max_tries: Optional[int], mean: Optional[torch.Tensor] = None,
                     eps: Optional[torch.Tensor] = None, want_R: bool = True):
    """psd_safe_cholesky's sequence on gpk::mvn_root for A (B, n, n): jitter 0; on any failure
    the NaN check (NanError), then up to max_tries relaunches of the WHOLE batch with
    cholesky_jitter * 10^t (upstream adds the jitter to every matrix of the batch), each warning
    NumericalWarning; NotPSDError after the last. Returns (R or None, samples or None). When a
    gradient can flow the op also writes R, which its backward needs."""
    keep_R = want_R or not _no_grad_flows(A, mean, eps)

    def launch(jit):
        R, smp, info = torch.ops.gpk.mvn_root(A, float(jit), mean, eps, keep_R)
        ok = not bool((info > 0).any())
        return ok, (R if want_R else None), (smp if eps is not None else None)

    ok, R, smp = launch(0.0)
    if ok:
        return R, smp
    if torch.isnan(A).any():
        from .errors import NanError
        raise NanError(f"cholesky_cpu: {torch.isnan(A).sum().item()} of {A.numel()} elements of the "
                       f"{tuple(A.shape)} tensor are NaN.")
    jitter = settings.cholesky_jitter.value(A.dtype)
    tries = settings.cholesky_max_tries.value() if max_tries is None else max_tries
    jitter_new = 0.0
    for i in range(tries):
        jitter_new = jitter * (10 ** i)
        warnings.warn(f"A not p.d., added jitter of {jitter_new:.1e} to the diagonal", NumericalWarning)
        ok, R, smp = launch(jitter_new)
        if ok:
            return R, smp
    from .errors import NotPSDError
    raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to {jitter_new:.1e}.")


def _exact_append_ladder(X, L, z, hyper, Xn, yn, max_tries: Optional[int] = None):
    """psd_safe_cholesky's sequence on gpk::exact_append, as ``_mvn_root_ladder`` runs it on
    gpk::mvn_root: jitter 0; on any failure the NaN check (NanError), then up to max_tries
    relaunches of the WHOLE batch with cholesky_jitter * 10^t on the Schur complement's diagonal,
    each warning NumericalWarning; NotPSDError after the last. Returns (L2, z2). One host read of
    ``info`` per launch."""
    def launch(jit):
        L2, z2, info = torch.ops.gpk.exact_append(X, L, z, hyper, Xn, yn, float(jit))
        return not bool((info > 0).any()), L2, z2

    ok, L2, z2 = launch(0.0)
    if ok:
        return L2, z2
    for A in (Xn, yn, X, L, z):
        if torch.isnan(A).any():
            from .errors import NanError
            raise NanError(f"cholesky_cpu: {torch.isnan(A).sum().item()} of {A.numel()} elements of the "
                           f"{tuple(A.shape)} tensor are NaN.")
    jitter = settings.cholesky_jitter.value(L.dtype)
    tries = settings.cholesky_max_tries.value() if max_tries is None else max_tries
    jitter_new = 0.0
    for i in range(tries):
        jitter_new = jitter * (10 ** i)
        warnings.warn(f"A not p.d., added jitter of {jitter_new:.1e} to the diagonal", NumericalWarning)
        ok, L2, z2 = launch(jitter_new)
        if ok:
            return L2, z2
    from .errors import NotPSDError
    raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to {jitter_new:.1e}.")


def psd_safe_cholesky(A: torch.Tensor, max_tries: Optional[int] = None) -> torch.Tensor:
    """Upstream linear_operator utils/cholesky.py psd_safe_cholesky for a dense matrix (the
    covariance roots of rsample; the hot path's factorisations run in the gfx950 kernels):
    torch.linalg.cholesky_ex, then up to max_tries retries with jitter 1e-6, 1e-5, ... (fp32;
    1e-8.. for fp64) added to the diagonal, each retry warning NumericalWarning. A CUDA fp32
    matrix of n <= 256 runs the same ladder on gpk_mvn_root_f32 (each rung one launch over the
    whole batch; differentiable through gpk_mvn_root_grad_f32); everything else takes the torch
    path."""
    if _mvn_root_eligible(A) and A.numel() > 0:
        n = A.shape[-1]
        R, _ = _mvn_root_ladder(A.reshape(-1, n, n), max_tries)
        return R.reshape(A.shape)
    L, info = torch.linalg.cholesky_ex(A)
    if not bool((info > 0).any()):
        return L
    if torch.isnan(A).any():
        from .errors import NanError
        raise NanError(f"cholesky_cpu: {torch.isnan(A).sum().item()} of {A.numel()} elements of the "
                       f"{tuple(A.shape)} tensor are NaN.")
    jitter = settings.cholesky_jitter.value(A.dtype)
    tries = settings.cholesky_max_tries.value() if max_tries is None else max_tries
    Aprime = A.clone()
    jitter_prev = 0.0
    for i in range(tries):
        jitter_new = jitter * (10 ** i)
        Aprime.diagonal(dim1=-2, dim2=-1).add_(jitter_new - jitter_prev)
        jitter_prev = jitter_new
        warnings.warn(f"A not p.d., added jitter of {jitter_new:.1e} to the diagonal", NumericalWarning)
        L, info = torch.linalg.cholesky_ex(Aprime)
        if not bool((info > 0).any()):
            return L
    from .errors import NotPSDError
    raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to {jitter_new:.1e}.")


class MultitaskMultivariateNormal:
    """Upstream distributions/multitask_multivariate_normal.py as a multi-output DeepGP layer
    returns it (DeepGPLayer.__call__: ``MultitaskMultivariateNormal(output.loc.transpose(-1, -2),
    BlockDiagLinearOperator(output.lazy_covariance_matrix, block_dim=-3), interleaved=False)``):
    a batch of O independent per-output MultivariateNormals (batch (..., O), event N) viewed with
    event shape (N, O). mean / variance are the per-output marginals transposed; the dense
    covariance is block diagonal in task-major (non-interleaved) order; rsample draws every
    output from its own full covariance."""

    def __init__(self, base: MultivariateNormal):
        self._base = base      # batch (..., O), event N

    @classmethod
    def from_batch_mvn(cls, batch_mvn: MultivariateNormal, task_dim: int = -1):
        if task_dim not in (-1, batch_mvn._mean.dim() - 2):
            raise NotImplementedError("the task dimension is the last batch dimension")
        return cls(batch_mvn)

    @property
    def num_tasks(self):
        return self._base.mean.shape[-2]

    @property
    def mean(self):
        return self._base.mean.transpose(-1, -2)

    @property
    def loc(self):
        return self.mean

    @property
    def variance(self):
        return self._base.variance.transpose(-1, -2)

    @property
    def stddev(self):
        return self.variance.sqrt()

    @property
    def batch_shape(self):
        return self._base.mean.shape[:-2]

    @property
    def event_shape(self):
        return self.mean.shape[-2:]

    @property
    def covariance_matrix(self):
        blocks = self._base.covariance_matrix          # (..., O, N, N)
        return torch.block_diag(*blocks.unbind(-3)) if blocks.dim() == 3 else \
            torch.stack([torch.block_diag(*b.unbind(-3)) for b in blocks.reshape(-1, *blocks.shape[-3:])]) \
            .reshape(*blocks.shape[:-3], blocks.shape[-3] * blocks.shape[-1], blocks.shape[-3] * blocks.shape[-1])

    @property
    def lazy_covariance_matrix(self):
        return self.covariance_matrix

    def expand(self, batch_size):
        return MultitaskMultivariateNormal(self._base.expand(torch.Size(batch_size) + self._base.mean.shape[-2:-1]))

    def add_noise(self, noise):
        return MultitaskMultivariateNormal(self._base.add_noise(noise))

    def rsample(self, sample_shape=torch.Size(), base_samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        if base_samples is not None:
            base_samples = base_samples.transpose(-1, -2)
        return self._base.rsample(sample_shape, base_samples).transpose(-1, -2)

    def sample(self, sample_shape=torch.Size(), base_samples: Optional[torch.Tensor] = None) -> torch.Tensor:
        with torch.no_grad():
            return self.rsample(sample_shape, base_samples)


# ---------------------------------------------------------------------------
# likelihood (upstream likelihoods/gaussian_likelihood.py, noise_models.py)
# ---------------------------------------------------------------------------
class HomoskedasticNoise(nn.Module):
    def __init__(self, batch_shape=torch.Size([])):
        super().__init__()
        self.register_parameter("raw_noise", nn.Parameter(torch.zeros(*batch_shape, 1)))
        self.register_module("raw_noise_constraint", GreaterThan(1e-4))

    @property
    def noise(self):
        return self.raw_noise_constraint.transform(self.raw_noise)


class GaussianLikelihood(nn.Module):
    def __init__(self, batch_shape=torch.Size([])):
        super().__init__()
        self.noise_covar = HomoskedasticNoise(batch_shape)

    @property
    def noise(self):
        return self.noise_covar.noise

    def forward(self, function_dist: MultivariateNormal) -> MultivariateNormal:
        """Marginal p(y) = q(f) + noise (only the diagonal is ever read on this path)."""
        noise = self.noise
        # batch_shape [B]: one noise per window, (B, 1) against the (B, N) marginals
        return function_dist.add_noise(noise.reshape(()) if noise.numel() == 1 else noise)

    def expected_log_prob(self, target: torch.Tensor, input: MultivariateNormal) -> torch.Tensor:
        mean, variance = input.mean, input.variance
        noise = self.noise.reshape(())
        res = ((target - mean) ** 2 + variance) / noise + noise.log() + LOG_2PI
        return res.mul(-0.5)

    def expected_log_prob_sum(self, target: torch.Tensor, input: MultivariateNormal) -> torch.Tensor:
        """expected_log_prob(target, input).sum(-1) -- what VariationalELBO reads -- as ONE
        gfx950 launch forward and one backward (gpk::gauss_ell) instead of ~10 elementwise
        kernels each way; the per-point form above stays GPyTorch's API."""
        mean, variance = input.mean, input.variance
        if not (mean.is_cuda and mean.dtype == torch.float32 and variance.shape == mean.shape
                and self.noise.numel() == 1):
            # (a batched noise model has one noise per batch entry: the unfused expression)
            return self.expected_log_prob(target, input).sum(-1)
        shape = mean.shape
        N = shape[-1]
        y = torch.broadcast_to(target, shape).to(torch.float32)
        ell = torch.ops.gpk.gauss_ell(y.reshape(-1, N), mean.reshape(-1, N), variance.reshape(-1, N),
                                      self.noise.reshape(1))
        return ell.reshape(shape[:-1])


# ---------------------------------------------------------------------------
# variational distribution / strategy (upstream variational/*.py, whitened)
# ---------------------------------------------------------------------------
class MeanFieldVariationalDistribution(nn.Module):
    def __init__(self, num_inducing_points: int, batch_shape=torch.Size([]), mean_init_std=1e-3):
        super().__init__()
        self.num_inducing_points = num_inducing_points
        self.mean_init_std = mean_init_std
        self.register_parameter("variational_mean", nn.Parameter(torch.zeros(*batch_shape, num_inducing_points)))
        self.register_parameter("_variational_stddev", nn.Parameter(torch.ones(*batch_shape, num_inducing_points)))

    def initialize_variational_distribution(self):
        # prior N(0, I) (whitened): m = 0 + mean_init_std * randn, stddev = 1
        with torch.no_grad():
            self.variational_mean.data.zero_()
            self.variational_mean.data.add_(torch.randn_like(self.variational_mean), alpha=self.mean_init_std)
            self._variational_stddev.data.fill_(1.0)

    def kl_divergence(self) -> torch.Tensor:
        """KL(N(m, diag s^2) || N(0, I)) = 1/2 (sum s^2 + sum m^2 - M - sum log s^2)
        (one gfx950 launch each way, gpk::meanfield_kl, for the unbatched fp32 layer)."""
        m = self.variational_mean
        s = self._variational_stddev
        if m.is_cuda and m.dim() == 1 and m.dtype == torch.float32:
            return torch.ops.gpk.meanfield_kl(m, s).reshape(())
        s2 = s.pow(2)
        return 0.5 * (s2.sum(-1) + m.pow(2).sum(-1) - m.shape[-1] - s2.log().sum(-1))


class CholeskyVariationalDistribution(nn.Module):
    """q(u) = N(m, L_q L_q^T), L_q = tril(chol_variational_covar): upstream
    variational/cholesky_variational_distribution.py (GPyTorch's default distribution). The
    strict upper triangle of the parameter is never read and gets exactly zero gradient; its
    diagonal is unconstrained (a negative entry is legal: the covariance and the log-determinant
    see its square)."""

    def __init__(self, num_inducing_points: int, batch_shape=torch.Size([]), mean_init_std=1e-3):
        super().__init__()
        self.num_inducing_points = num_inducing_points
        self.mean_init_std = mean_init_std
        mean_init = torch.zeros(num_inducing_points).repeat(*batch_shape, 1)
        covar_init = torch.eye(num_inducing_points, num_inducing_points).repeat(*batch_shape, 1, 1)
        self.register_parameter("variational_mean", nn.Parameter(mean_init))
        self.register_parameter("chol_variational_covar", nn.Parameter(covar_init))

    def initialize_variational_distribution(self):
        # prior N(0, I) (whitened): m = 0 + mean_init_std * randn, L_q = I
        with torch.no_grad():
            self.variational_mean.data.zero_()
            self.variational_mean.data.add_(torch.randn_like(self.variational_mean), alpha=self.mean_init_std)
            C = self.chol_variational_covar.data
            C.zero_()
            C.diagonal(dim1=-2, dim2=-1).fill_(1.0)

    def kl_divergence(self) -> torch.Tensor:
        """KL(q || N(0, I)) = 1/2 (|L_q|_F^2 + |m|^2 - M - sum_k log L_q,kk^2): one gfx950 launch
        each way for a CUDA fp32 layer (gpk::cholesky_kl: () for one output, (O,) for the (O, M) mean
        of a multi-output layer), the closed form in torch elsewhere."""
        m = self.variational_mean
        C = self.chol_variational_covar
        if m.is_cuda and m.dtype == torch.float32 and C.dtype == torch.float32:
            if m.dim() == 1:
                return torch.ops.gpk.cholesky_kl(m, C).reshape(())
            if m.dim() == 2 and 1 <= m.shape[0] <= 65535 and m.shape[1] <= 16384:
                return torch.ops.gpk.cholesky_kl(m, C)
        return cholesky_kl_closed_form(m, C)


def cholesky_kl_closed_form(m, C):
    """KL(N(m, L L^T) || N(0, I)) with L = tril(C), batched over leading dimensions (torch)."""
    L = torch.tril(C)
    logdet = L.diagonal(dim1=-2, dim2=-1).pow(2).log().sum(-1)
    return 0.5 * (L.pow(2).sum((-1, -2)) + m.pow(2).sum(-1) - m.shape[-1] - logdet)


def _variational_interp(x, Z, Linv, outputscale, lengthscale):
    """A = L^{-1} K_ZX (B', M, N) as upstream's whitened strategy forms it: the solve in fp64,
    cast back to the dtype of x."""
    ls = lengthscale.reshape(-1)
    s2 = outputscale.reshape(())
    zs = (Z / ls).double()
    xs = (x / ls).double()
    d = (zs.pow(2).sum(-1)[:, None] + xs.pow(2).sum(-1).unsqueeze(-2)
         - 2.0 * zs @ xs.transpose(-1, -2)).clamp_min(0.0)             # (B', M, N)
    Kzx = s2.double() * torch.exp(-0.5 * d)
    return (Linv.double() @ Kzx).to(x.dtype)


def variational_chol_predict(x, Z, Linv, vmean, vchol, outputscale, lengthscale, weights, bias, jitter):
    """(mean, unclamped variance) of q(f) at x (B', N, D) for the whitened strategy with a Cholesky
    q(u) = N(vmean, L_q L_q^T), L_q = tril(vchol), written out in differentiable torch:
      A = Linv K_ZX   W = L_q^T A   mean = A^T m + x w + b0   var = s2 + jitter - sum A^2 + sum W^2
    The formulas of gpk_variational_chol_f32 / its adjoint: the fallback for shapes the kernels
    refuse and for multi-output layers, and the tests' fp64 reference. ``weights`` (D,) or None."""
    A = _variational_interp(x, Z, Linv, outputscale, lengthscale)
    Lq = torch.tril(vchol).to(x.dtype)
    W = Lq.transpose(-1, -2) @ A
    mean = (A * vmean.reshape(-1).to(x.dtype)[:, None]).sum(-2) + bias
    if weights is not None:
        mean = mean + x @ weights.reshape(-1).to(x.dtype)
    var = outputscale.reshape(()) + jitter - A.pow(2).sum(-2) + W.pow(2).sum(-2)
    return mean, var


def variational_chol_dense_covariance(x, Z, Linv, vchol, outputscale, lengthscale, jitter):
    """The full predictive covariance K_XX + jitter I + W^T W - A^T A of q(f) with a Cholesky q(u)
    (dense torch arithmetic, on request: covariance_matrix / rsample)."""
    ls = lengthscale.reshape(-1)
    s2 = outputscale.reshape(())
    A = _variational_interp(x, Z, Linv, s2, ls)
    W = torch.tril(vchol).to(x.dtype).transpose(-1, -2) @ A
    eye = torch.eye(x.shape[-2], dtype=x.dtype, device=x.device)
    return (rbf_covariance(x, ls, s2) + jitter * eye + W.transpose(-1, -2) @ W
            - A.transpose(-1, -2) @ A)


def variational_dense_covariance(x, Z, Linv, vstd, outputscale, lengthscale, jitter):
    """The full predictive covariance of q(f) at x (B', N, D), as upstream
    VariationalStrategy.forward (whitened) builds it lazily: K_XX + jitter I + A^T (S - I) A with
    A = L^{-1} K_ZX solved in fp64 and cast back (``L.solve(induc_data_covar.double())``),
    S = diag(stddev^2). Dense torch arithmetic on request (covariance_matrix / rsample) -- the
    hot path reads the marginals from the kernels and never calls this."""
    ls = lengthscale.reshape(-1)
    s2 = outputscale.reshape(())
    Kxx = rbf_covariance(x, ls, s2)
    A = _variational_interp(x, Z, Linv, s2, ls)
    mid = (vstd.reshape(-1).pow(2) - 1.0).to(x.dtype)
    eye = torch.eye(x.shape[-2], dtype=x.dtype, device=x.device)
    return Kxx + jitter * eye + A.transpose(-1, -2) @ (mid[:, None] * A)


def _variational_cov_on_kernels(x, Z, Linv, vstd, outputscale, lengthscale) -> bool:
    """The dense covariance of q(f) runs on gpk_variational_cov_f32 when no gradient can flow
    (grad mode off, or none of the tensors requires grad) and the inputs are CUDA fp32; the
    differentiable covariance is _variational_cov_grad_on_kernels' case, and every CPU path
    stays the dense torch restatement."""
    return (x.is_cuda and x.dtype == torch.float32 and Z.dtype == torch.float32 and x.numel() > 0
            and _no_grad_flows(x, Z, Linv, vstd, outputscale, lengthscale))


def _variational_cov_grad_on_kernels(x, Z, Linv, vstd, outputscale, lengthscale) -> bool:
    """The differentiable dense covariance of q(f) runs on gpk::variational_cov_train
    (gpk_variational_cov_f32 keeping A, its adjoint gpk_variational_cov_grad_f32) when a gradient
    can flow, the inputs are CUDA fp32 and the adjoint's workspace query accepts the shape
    (M <= 256, D <= 64, N <= 256); the dense torch restatement stays for CPU tensors, other
    dtypes and refused shapes. Z (O, M, D): the batched form, x (B, N, D) or (O, B, N, D)."""
    if not (x.is_cuda and x.dtype == torch.float32 and Z.dtype == torch.float32 and x.numel() > 0):
        return False
    if _no_grad_flows(x, Z, Linv, vstd, outputscale, lengthscale):
        return False
    from . import _native
    B, N, D = x.shape[-3:]
    M = Z.shape[-2]
    if Z.dim() == 3:
        return _native.lib().gpk_variational_cov_grad_batched_workspace_bytes(Z.shape[0], B, N, M, D) > 0
    return _native.lib().gpk_variational_cov_grad_workspace_bytes(B, N, M, D) > 0


def _chol_cov_kernel_inputs(x, Z, vchol) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and Z.dtype == torch.float32
            and vchol.dtype == torch.float32 and x.numel() > 0)


def _variational_chol_cov_on_kernels(x, Z, Linv, vchol, outputscale, lengthscale) -> bool:
    """The dense covariance of q(f) with a Cholesky q(u) runs on gpk_variational_chol_cov_f32 when
    no gradient can flow (grad mode off, or none of the tensors requires grad), the inputs are
    CUDA fp32 and the workspace query accepts the shape (M <= 256, D <= 64); the differentiable
    covariance is _variational_chol_cov_grad_on_kernels' case, and every CPU path stays
    variational_chol_dense_covariance. Z (O, M, D): the batched form."""
    if not _chol_cov_kernel_inputs(x, Z, vchol):
        return False
    if not _no_grad_flows(x, Z, Linv, vchol, outputscale, lengthscale):
        return False
    from . import _native
    B, N, D = x.shape[-3:]
    M = Z.shape[-2]
    if D > 64:
        return False
    if Z.dim() == 3:
        return _native.lib().gpk_variational_chol_cov_batched_workspace_bytes(Z.shape[0], B, N, M) > 0
    return _native.lib().gpk_variational_chol_cov_workspace_bytes(B, N, M) > 0


def _variational_chol_cov_grad_on_kernels(x, Z, Linv, vchol, outputscale, lengthscale) -> bool:
    """The differentiable form runs on gpk::variational_chol_cov_train (the same forward keeping
    its stacked [W; A] panels, its adjoint gpk_variational_chol_cov_grad_f32) when a gradient can
    flow, the inputs are CUDA fp32 and the adjoint's workspace query accepts the shape (M <= 256,
    D <= 64, N <= 256); variational_chol_dense_covariance stays for CPU tensors, other dtypes and
    refused shapes. Z (O, M, D): the batched form, x (B, N, D) or (O, B, N, D)."""
    if not _chol_cov_kernel_inputs(x, Z, vchol):
        return False
    if _no_grad_flows(x, Z, Linv, vchol, outputscale, lengthscale):
        return False
    from . import _native
    B, N, D = x.shape[-3:]
    M = Z.shape[-2]
    if Z.dim() == 3:
        return _native.lib().gpk_variational_chol_cov_grad_batched_workspace_bytes(Z.shape[0], B, N, M, D) > 0
    return _native.lib().gpk_variational_chol_cov_grad_workspace_bytes(B, N, M, D) > 0


class VariationalStrategy(nn.Module):
    """Whitened VariationalStrategy for one DeepGP layer: one output (output_dims=None, inducing
    points (M, D)) or O outputs (inducing points (O, M, D)), mean-field or Cholesky q(u).

    __call__(x) with x (..., N, D) returns q(f) as a MultivariateNormal (mean, var)
    computed by gpk_kzz_chol_f64 (ONE fp64 factorisation of the shared K_ZZ, cached across
    the calls of a step / eval batches, ops_autograd.KzzCache) + gpk_variational_f32
    (column-tiled fp64-MFMA L^{-1} K_ZX, mean, variance), or their batched / Cholesky-q(u) forms.
    """

    def __init__(self, model, inducing_points: torch.Tensor, variational_distribution,
                 learn_inducing_locations: bool = True, jitter_val: Optional[float] = None):
        super().__init__()
        object.__setattr__(self, "model", model)
        ip = inducing_points.clone()
        if learn_inducing_locations:
            self.register_parameter("inducing_points", nn.Parameter(ip))
        else:
            self.register_buffer("inducing_points", ip)
        self._variational_distribution = variational_distribution
        self.register_buffer("variational_params_initialized", torch.tensor(0))
        self.register_buffer("updated_strategy", torch.tensor(True))
        self.jitter_val = jitter_val
        self._initialized = False     # host mirror of the buffer: no device sync per call
        from .ops_autograd import KzzCache
        self._kzz_cache = KzzCache()     # multi-output layers: the (O, M, M) factor is one entry

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._initialized = bool(int(self.variational_params_initialized))
        self._kzz_cache.clear()

    def train(self, mode: bool = True):
        self._kzz_cache.clear()      # GPyTorch clears its cholesky cache on mode switches
        return super().train(mode)

    @property
    def variational_distribution(self):
        return self._variational_distribution

    def _jitter(self, dtype):
        return self.jitter_val if self.jitter_val is not None else settings.variational_cholesky_jitter.value(dtype)

    def kl_divergence(self) -> torch.Tensor:
        return self._variational_distribution.kl_divergence()

    def __call__(self, x: torch.Tensor) -> MultivariateNormal:
        """q(f) at x. One flow for both layer forms and both q(u) kinds:

        1. Normalise to ``lead`` = () -- inducing points (M, D), x (..., N, D) -- or (O,) -- a
           multi-output layer (output_dims = O, DeepGP.py:24-26): inducing points (O, M, D), q(u) batch
           (O,), kernel hyper-parameters per output, x (..., O, N, D) as DeepGPLayer.__call__ expands
           it. That stride-0 expansion (or O == 1) is read in place as one (B', N, D) tensor shared by
           the outputs: no (O, B', N, D) copy.
        2. The marginals on the kernels (ops_autograd.variational_predict*): one launch chain each
           way whatever O is, the K_ZZ factor(s) one KzzCache entry, the per-output dLinv flowing
           into one K_ZZ adjoint. A mean-field q(u) has no other route (CPU tensors raise). A Cholesky
           q(u) needs CUDA fp32 inputs and a shape the kernels' queries accept (M <= 256, D <= 64;
           N <= 256 when a gradient can flow); every other case is variational_chol_predict in torch
           from the same cached factor, one evaluation per output.
        3. Reshape back to (..., N) or (..., O, N).
        4. The dense covariance behind covariance_matrix / rsample, materialised on request
           (_lazy_covariance)."""
        if not self._initialized:
            self._variational_distribution.initialize_variational_distribution()
            self.variational_params_initialized.fill_(1)
            self._initialized = True
        from . import ops_autograd
        model = self.model
        kern = model.covar_module
        q = self._variational_distribution
        chol = isinstance(q, CholeskyVariationalDistribution)
        Z = self.inducing_points
        jitter = self._jitter(x.dtype)
        key = (Z, kern.raw_outputscale, kern.base_kernel.raw_lengthscale)
        N, D = x.shape[-2:]
        M = Z.shape[-2]
        if Z.dim() == 3:
            O = Z.shape[0]
            if x.dim() < 3 or x.shape[-3] != O:
                raise RuntimeError(f"a layer with {O} outputs takes inputs (..., {O}, N, D); got {tuple(x.shape)}")
            lead, batch = (O,), x.shape[:-3]
            if x.stride(-3) == 0 or O == 1:     # DeepGPLayer's expansion: one (B', N, D) tensor for all outputs
                xk = x[..., 0, :, :].reshape(-1, N, D)
            else:
                xk = x.movedim(-3, 0).reshape(O, -1, N, D)
        else:
            O, lead, batch = None, (), x.shape[:-2]
            xk = x.reshape(-1, N, D)
        s2, ls, vm = kern.outputscale, kern.base_kernel.lengthscale, q.variational_mean
        vq = q.chol_variational_covar if chol else q._variational_stddev
        if lead:
            # one view of each parameter for all its consumers. A single output hands the parameters
            # on as the modules hold them: each consumer takes its own view, so the contributions to
            # a parameter's gradient (marginals, covariance, KL) are summed in the order they arrive
            s2, ls, vm = s2.reshape(O), ls.reshape(O, -1), vm.reshape(O, M)
            vq = vq.reshape(O, M, M) if chol else vq.reshape(O, M)

        on_kernels = True
        if chol:
            grad = torch.is_grad_enabled()
            nwin = xk.shape[-3]
            on_kernels = (x.is_cuda and x.dtype == torch.float32 and Z.dtype == torch.float32
                          and vq.dtype == torch.float32
                          and (ops.variational_chol_batched_supported(O, nwin, N, M, D, adjoint=grad) if lead
                               else ops.variational_chol_supported(nwin, N, M, D, adjoint=grad)))
        hyper = None
        if on_kernels:
            if chol:
                predict = (ops_autograd.variational_predict_chol_batched if lead
                           else ops_autograd.variational_predict_chol)
                mean, var, flag, Linv = predict(xk, Z, vm, vq, s2, ls, model.mean_module, jitter,
                                                cache=self._kzz_cache, key_tensors=key, return_linv=True)
            else:
                predict = ops_autograd.variational_predict_batched if lead else ops_autograd.variational_predict
                mean, var, flag, Linv, hyper = predict(xk, Z, vm, vq, s2, ls, model.mean_module, jitter,
                                                       cache=self._kzz_cache, key_tensors=key,
                                                       return_linv=True, return_hyper=True)
        else:
            flag = None
            if lead:
                Linv = self._kzz_cache.factor(Z, s2, ls, jitter, key)
                w, b0 = ops_autograd._mean_params_batched(model.mean_module, O, D, x.device)
                xo = x.movedim(-3, 0).reshape(O, -1, N, D)     # a view of an expanded x
                outs = [variational_chol_predict(xo[o], Z[o], Linv[o], vm[o], vq[o], s2[o], ls[o],
                                                 w[o] if w.dim() == 2 else w, b0[o] if b0.numel() == O else b0[0],
                                                 jitter) for o in range(O)]
                mean, var = torch.stack([m for m, _ in outs]), torch.stack([v for _, v in outs])
            else:
                Linv = self._kzz_cache.factor(Z, s2.reshape(()), ls.reshape(-1), jitter, key)
                w, b0 = ops_autograd._mean_params(model.mean_module, D, x.device)
                mean, var = variational_chol_predict(xk, Z, Linv, vm, vq, s2, ls, w, b0, jitter)
            self._kzz_cache.note_consumers(mean, var)
            self._kzz_cache.check_pending()

        if lead:
            mean = mean.reshape(O, *batch, N).movedim(0, -2).contiguous()
            var = var.reshape(O, *batch, N).movedim(0, -2).contiguous()
        else:
            mean, var = mean.reshape(*batch, N), var.reshape(*batch, N)
        cov = self._lazy_covariance(chol, x, xk, Z, Linv, vq, s2, ls, jitter, hyper, batch)
        return MultivariateNormal(mean, var, clamp_flag=flag, covar_fn=cov)

    @staticmethod
    def _lazy_covariance(chol, x, xk, Z, Linv, vq, s2, ls, jitter, hyper, batch):
        """The closure behind covariance_matrix / rsample (upstream VariationalStrategy.forward's
        predictive_covar) for a mean-field (``vq`` the stddevs) or Cholesky (``chol``: ``vq`` the factor)
        q(u): on the kernels when no gradient can flow (gpk::variational_cov / _chol_cov) and, with
        their HIP adjoint, when one can (gpk::variational_cov_train / _chol_cov_train; dLinv then
        flows into the same Linv as the marginals' and the layer still runs one K_ZZ adjoint per step),
        all outputs of a multi-output layer on one launch chain; as dense torch arithmetic from
        Linv[o] for CPU tensors, other dtypes and shapes the queries refuse."""
        N, D = x.shape[-2:]
        lead = tuple(Z.shape[:-2])

        def op_hypers():     # the ops take s2 (), ls (D,); a multi-output layer's are (O,), (O, D) already
            return (s2, ls) if lead else (s2.reshape(()), ls.reshape(-1))

        def cov():
            if chol:
                on_kernels, grad_on_kernels = _variational_chol_cov_on_kernels, _variational_chol_cov_grad_on_kernels
                cov_op, train_op = torch.ops.gpk.variational_chol_cov, torch.ops.gpk.variational_chol_cov_train
                dense = variational_chol_dense_covariance
            else:
                on_kernels, grad_on_kernels = _variational_cov_on_kernels, _variational_cov_grad_on_kernels
                cov_op, train_op = torch.ops.gpk.variational_cov, torch.ops.gpk.variational_cov_train
                dense = variational_dense_covariance
            if on_kernels(xk, Z, Linv, vq, s2, ls):
                h = hyper
                if h is None:     # the Cholesky forward's vector is not kept: packed on request
                    from .library import _cov_hyper
                    h = _cov_hyper(xk, Z, *op_hypers(), float(jitter))
                c = cov_op(xk, Linv, Z, vq, h)                         # (*lead, B', N, N)
            elif grad_on_kernels(xk, Z, Linv, vq, s2, ls):
                c = train_op(xk, Linv, Z, vq, *op_hypers(), float(jitter))[0]
            elif not lead:
                c = dense(xk, Z, Linv, vq, s2, ls, jitter)
            else:
                xo = x.movedim(-3, 0).reshape(lead[0], -1, N, D)
                return torch.stack([dense(xo[o], Z[o], Linv[o], vq[o], s2[o], ls[o], jitter).reshape(*batch, N, N)
                                    for o in range(lead[0])], dim=-3)
            c = c.reshape(*lead, *batch, N, N)
            return c.movedim(0, -3) if lead else c
        return cov


# ---------------------------------------------------------------------------
# marginal log likelihoods (upstream mlls/*.py)
# ---------------------------------------------------------------------------
class _ApproximateMarginalLogLikelihood(nn.Module):
    def __init__(self, likelihood, model, num_data: int, beta: float = 1.0, combine_terms: bool = True):
        super().__init__()
        self.likelihood = likelihood
        self.model = model
        self.num_data = num_data
        self.beta = beta
        self.combine_terms = combine_terms

    def _log_likelihood_term(self, approximate_dist_f, target, **kwargs):
        raise NotImplementedError

    def forward(self, approximate_dist_f: MultivariateNormal, target: torch.Tensor, **kwargs):
        num_batch = approximate_dist_f.event_shape[0]
        log_likelihood = self._log_likelihood_term(approximate_dist_f, target, **kwargs).div(num_batch)
        kl_divergence = self.model.variational_strategy.kl_divergence().div(self.num_data / self.beta)
        if self.combine_terms:
            return log_likelihood - kl_divergence
        return log_likelihood, kl_divergence, torch.zeros_like(log_likelihood)


class VariationalELBO(_ApproximateMarginalLogLikelihood):
    def forward(self, approximate_dist_f: MultivariateNormal, target: torch.Tensor, **kwargs):
        fused = self._fused(approximate_dist_f, target)
        return fused if fused is not None else super().forward(approximate_dist_f, target, **kwargs)

    def _fused(self, dist, target):
        """ELL / N - KL / (num_data / beta) for every row in ONE launch each way
        (gpk::variational_elbo) when the terms are the hot path's: a Gaussian likelihood, a
        variational output of the kernels, one unbatched mean-field strategy. Same warnings as
        the unfused expression (the variance clamp flag)."""
        if (not self.combine_terms or not isinstance(self.likelihood, GaussianLikelihood)
                or not isinstance(dist, MultivariateNormal)):
            return None
        # the fused op takes one scalar noise and returns no target gradient: a batched noise
        # model or a target that requires grad takes the unfused path
        if self.likelihood.noise.numel() != 1 or (torch.is_tensor(target) and target.requires_grad):
            return None
        mean, var = dist._mean, dist._variance
        if (var is None or dist._exact is not None or dist._added_noise is not None or not mean.is_cuda
                or mean.dtype != torch.float32 or var.shape != mean.shape
                or (dist._clamp_flag is None and not dist._preclamped)):
            return None
        strategies = [m for m in self.model.modules() if isinstance(m, VariationalStrategy)]
        if len(strategies) != 1:
            return None
        q = strategies[0].variational_distribution
        if not isinstance(q, MeanFieldVariationalDistribution) or q.variational_mean.dim() != 1:
            return None
        shape = mean.shape
        N = shape[-1]
        y = torch.broadcast_to(target, shape).to(torch.float32)
        min_var = settings.min_variance.value(var.dtype)
        elbo, flag = torch.ops.gpk.variational_elbo(
            y.reshape(-1, N), mean.reshape(-1, N), var.reshape(-1, N), self.likelihood.noise.reshape(1),
            q.variational_mean, q._variational_stddev, float(self.beta) / float(self.num_data), float(min_var))
        # MultivariateNormal.variance's clamp warning: the variational kernel's own flag when the
        # distribution carries it, else the rows' flag computed with the ELBO
        from .ops import record_or_run
        f = dist._clamp_flag if dist._clamp_flag is not None else (flag if dist._preclamped else None)
        if f is not None:
            record_or_run("clamp", (f, min_var), lambda: warn_if_clamped(f, min_var))
        return elbo.reshape(shape[:-1])

    def _log_likelihood_term(self, variational_dist_f, target, **kwargs):
        if hasattr(self.likelihood, "expected_log_prob_sum"):
            return self.likelihood.expected_log_prob_sum(target, variational_dist_f)
        return self.likelihood.expected_log_prob(target, variational_dist_f).sum(-1)


class DeepApproximateMLL(nn.Module):
    def __init__(self, base_mll):
        super().__init__()
        self.base_mll = base_mll

    def forward(self, approximate_dist_f, target, **kwargs):
        return self.base_mll(approximate_dist_f, target, **kwargs).mean(0)


class ExactMarginalLogLikelihood(nn.Module):
    def __init__(self, likelihood, model):
        super().__init__()
        self.likelihood = likelihood
        self.model = model

    def forward(self, function_dist: MultivariateNormal, target: torch.Tensor, *params):
        output = self.likelihood(function_dist)
        res = output.log_prob(target)
        num_data = function_dist.event_shape.numel()
        return res.div(num_data)


class _DeepGPVariationalStrategy:
    """DeepGP.variational_strategy: KL summed over the sub-strategies of the model."""

    def __init__(self, model):
        self._model = model

    def kl_divergence(self):
        strategies = [m for m in self._model.modules() if isinstance(m, VariationalStrategy)]
        return sum(s.kl_divergence().sum() for s in strategies)
