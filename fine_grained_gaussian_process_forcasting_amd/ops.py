"""Torch-facing launchers for the gfx950 GP kernels (no compute happens here).

Each function validates shapes/dtypes/devices on the host, allocates outputs with
torch (device memory, caller stream), and enqueues ONE C-ABI call on
``torch.cuda.current_stream()``. Tensors must live on a ROCm device; there is
no CPU path.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Optional

import torch

from . import _native
from .errors import GpkInternalError, NanError, NotPSDError, NumericalWarning


def _require_device(*ts: torch.Tensor) -> None:
    for t in ts:
        if not t.is_cuda:
            raise ValueError("gpk ops run only on a ROCm device (tensor.is_cuda must be True); "
                             "there is no CPU fallback")


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _scalar_tensor(v, device) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        return v.detach().reshape(-1).to(device=device, dtype=torch.float32)
    # a fill kernel, not a host->device copy: graph-capture safe
    return torch.full((1,), float(v), device=device, dtype=torch.float32)


def pack_exact_hyper(outputscale, noise, mean_constant, lengthscale, device) -> torch.Tensor:
    """Device vector {s2, noise, c, lengthscale...} consumed by gpk_exact_mll_f32."""
    parts = [_scalar_tensor(outputscale, device)[:1], _scalar_tensor(noise, device)[:1],
             _scalar_tensor(mean_constant, device)[:1], _scalar_tensor(lengthscale, device)]
    return torch.cat(parts).contiguous()


def pack_exact_hyper_live(outputscale, noise, mean_constant, lengthscale) -> torch.Tensor:
    """The same vector {s2, noise, c, lengthscale...} from tensors WITHOUT detaching them, for the
    ops with a registered backward: their dhyp flows on to the parameters (and through the softplus
    constraints) by torch autograd. ``pack_exact_hyper`` detaches and is for the no-grad callers."""
    return torch.cat([outputscale.reshape(1), noise.reshape(1), mean_constant.reshape(1),
                      lengthscale.reshape(-1)]).float()


def _hyper_piece(v, B: int, width: int, name: str, device=None) -> torch.Tensor:
    """One hyper-parameter as (B, width): shared (``width`` values in any shape: expanded over the
    windows, so autograd sums its gradient over them) or per-window (leading size B)."""
    if not isinstance(v, torch.Tensor):
        v = torch.full((1,), float(v), device=device, dtype=torch.float32)
    if v.numel() == width:
        return v.reshape(1, width).expand(B, width)
    if v.dim() >= 1 and v.shape[0] == B and v.numel() == B * width:
        return v.reshape(B, width)
    raise ValueError(f"{name} must hold {width} shared value(s) or have a leading window dimension "
                     f"B = {B} with {width} value(s) per window, got shape {tuple(v.shape)}")


def pack_exact_hyper_windows(outputscale, noise, mean_constant, lengthscale, B: int) -> torch.Tensor:
    """Per-window hyper matrix (B, 3 + n_ls), row b = {s2, noise, c, lengthscale...} of window b, for
    the exact ops' 2-D ``hyper`` (include/gpk.h, the *_perwin_f32 entry points). Each argument is
    shared (one value in any shape; the lengthscale: 1 or n_ls values) or per-window (leading size
    B: (B,), (B, 1), (B, 1, n_ls)), so mixed models pack too. A 1-D lengthscale is the shared (n_ls,)
    vector; a per-window one has at least two dimensions, as GPyTorch's (B, 1, n_ls). Built with
    expand / cat only: differentiable, a shared entry's gradient sums over the windows through
    autograd, and no host sync (HIP-graph capturable)."""
    B = int(B)
    dev = next((t.device for t in (outputscale, noise, mean_constant, lengthscale)
                if isinstance(t, torch.Tensor)), None)
    if isinstance(lengthscale, torch.Tensor):
        per_window = lengthscale.dim() >= 2 and lengthscale.shape[0] == B
        n_ls = lengthscale.numel() // max(B, 1) if per_window else lengthscale.numel()
    else:
        n_ls = 1
    parts = [_hyper_piece(outputscale, B, 1, "outputscale", dev), _hyper_piece(noise, B, 1, "noise", dev),
             _hyper_piece(mean_constant, B, 1, "mean_constant", dev),
             _hyper_piece(lengthscale, B, n_ls, "lengthscale", dev)]
    return torch.cat(parts, dim=1).float()


def exact_hyper_per_window(outputscale, noise, mean_constant, lengthscale, B: int) -> bool:
    """Whether any of the hyper-parameters carries a window dimension (leading size B > 1: (B,),
    (B, 1); the lengthscale (B, 1, n_ls)), i.e. the model is GPyTorch's batch-independent one and
    packs with ``pack_exact_hyper_windows``. Shapes only: no host sync."""
    def lead(t, min_dim):
        return isinstance(t, torch.Tensor) and B > 1 and t.dim() >= min_dim and t.shape[0] == B
    return lead(outputscale, 1) or lead(noise, 1) or lead(mean_constant, 1) or lead(lengthscale, 2)


def _exact_hyper_layout(hyper: torch.Tensor, B: int):
    """-> (hyper, n_ls, hyp_stride) of an exact op's ``hyper``: 1-D {s2, noise, c, lengthscale...}
    shared by every window (stride 0), or (B, 3 + n_ls) with one row per window."""
    if hyper.dim() == 1:
        return hyper, hyper.shape[-1] - 3, 0
    if hyper.dim() != 2:
        raise ValueError(f"hyper must be 1-D (3 + n_ls,) or 2-D (B, 3 + n_ls), got {tuple(hyper.shape)}")
    if hyper.shape[0] != B:
        raise ValueError(f"a 2-D hyper must have one row per window: (B, 3 + n_ls) with B = {B}, "
                         f"got {tuple(hyper.shape)}")
    hyper = hyper.detach().contiguous().float()
    return hyper, hyper.shape[-1] - 3, hyper.shape[-1]


def _exact_name(base: str, stride: int) -> str:
    return f"gpk_exact_{base}_perwin_f32" if stride else f"gpk_exact_{base}_f32"


def _exact_prologue(X, L, z, hyper, Xs, xs: str = "Xs", ns: str = "Ns", others=(), check=None,
                    layout_first: bool = False):
    """The shared head of the exact ops that run from a cached factor: shape checks of X, the second
    input set ``Xs`` (named ``xs``, (B, ``ns``, D)), L and z; ``check(B, N, D, n_ls)`` for the op's own
    checks (``n_ls`` only with ``layout_first``: the hyper layout is read before the device check,
    otherwise after the tensors are made contiguous); the device check of these and ``others``.
    -> (X, L, z, hyper, Xs) detached, contiguous, float32, and (B, N, D, n_ls, hyp_stride)."""
    if X.dim() != 3 or Xs.dim() != 3:
        raise ValueError(f"X and {xs} must be (B, N, D) and (B, {ns}, D)")
    B, N, D = X.shape
    if Xs.shape[0] != B or Xs.shape[2] != D:
        raise ValueError(f"{xs} must be (B, {ns}, D) = ({B}, {ns}, {D}), got {tuple(Xs.shape)}")
    if L.shape != (B, N, N) or z.shape != (B, N):
        raise ValueError("L / z do not match X")
    n_ls = stride = None
    if layout_first:
        hyper, n_ls, stride = _exact_hyper_layout(hyper, B)
    if check is not None:
        check(B, N, D, n_ls)
    _require_device(X, L, z, hyper, Xs, *others)
    X, Xs, L, z = (t.detach().contiguous().float() for t in (X, Xs, L, z))
    if not layout_first:
        hyper, n_ls, stride = _exact_hyper_layout(hyper, B)
    return X, L, z, hyper, Xs, (B, N, D, n_ls, stride)


@dataclass
class ExactMLLOut:
    mll: torch.Tensor            # (B,)
    L: Optional[torch.Tensor]    # (B, N, N) lower Cholesky factor of K + noise I (+ jitter)
    z: Optional[torch.Tensor]    # (B, N)   L^{-1}(y - c)
    info: torch.Tensor           # (B,) int32 (0 / -t / k, see include/gpk.h)


EXACT_REG_MAX_N = 256   # largest N of the register / LDS-resident exact kernels (gpk_internal.h)


def exact_mll(X: torch.Tensor, y: torch.Tensor, lengthscale, outputscale, mean_constant, noise,
              jitter: float = 1e-6, max_tries: int = 3, want_L: bool = True,
              want_z: bool = False, hyper: Optional[torch.Tensor] = None,
              mll_out: Optional[torch.Tensor] = None, info_out: Optional[torch.Tensor] = None,
              L_out: Optional[torch.Tensor] = None) -> ExactMLLOut:
    """Fused exact-GP log marginal likelihood per window (one gfx950 kernel launch).

    X: (B, N, D) float32, y: (B, N) float32 on the same ROCm device. ``lengthscale``
    is a scalar or a length-D vector (ARD). Hyperparameters may be python floats or
    device tensors (no host sync either way). See include/gpk.h::gpk_exact_mll_f32.
    ``hyper``: the packed vector (3 + n_ls,) shared by every window, or (B, 3 + n_ls) with one row
    per window (``pack_exact_hyper_windows``; gpk_exact_mll_perwin_f32).
    """
    if X.dim() != 3:
        raise ValueError(f"X must be (B, N, D), got {tuple(X.shape)}")
    B, N, D = X.shape
    if y.shape != (B, N):
        raise ValueError(f"y must be (B, N) = {(B, N)}, got {tuple(y.shape)}")
    _require_device(X, y)
    X = X.contiguous().float()
    y = y.contiguous().float()
    dev = X.device
    if hyper is None:
        hyper = pack_exact_hyper(outputscale, noise, mean_constant, lengthscale, dev)
    if hyper.dim() == 1:     # one vector shared by the windows: the per-step launch of a training loop,
        n_ls, stride = hyper.numel() - 3, 0      # so nothing is added to its host path
    else:
        hyper, n_ls, stride = _exact_hyper_layout(hyper, B)
    if n_ls not in (1, D):
        raise ValueError(f"lengthscale must have 1 or D={D} entries, got {n_ls}")
    if mll_out is not None and (mll_out.shape != (B,) or mll_out.dtype != torch.float32
                                or not mll_out.is_contiguous() or mll_out.device != dev):
        raise ValueError("mll_out must be a contiguous (B,) float32 tensor on X's device")
    if info_out is not None and (info_out.shape != (B,) or info_out.dtype != torch.int32
                                 or not info_out.is_contiguous() or info_out.device != dev):
        raise ValueError("info_out must be a contiguous (B,) int32 tensor on X's device")
    mll = mll_out if mll_out is not None else torch.empty(B, device=dev, dtype=torch.float32)
    info = info_out if info_out is not None else torch.empty(B, device=dev, dtype=torch.int32)
    if L_out is not None and (L_out.shape != (B, N, N) or L_out.dtype != torch.float32
                              or not L_out.is_contiguous() or L_out.device != dev):
        raise ValueError("L_out must be a contiguous (B, N, N) float32 tensor on X's device")
    # Above EXACT_REG_MAX_N the blocked kernels (gpk_exact_large.hip) factor in place in L, so
    # it is allocated even when the caller does not keep it.
    need_L = want_L or N > EXACT_REG_MAX_N
    L = (L_out if L_out is not None else torch.empty(B, N, N, device=dev, dtype=torch.float32)) if need_L else None
    z = torch.empty(B, N, device=dev, dtype=torch.float32) if want_z else None
    if stride == 0:
        rc = _native.lib().gpk_exact_mll_f32(
            X.data_ptr(), y.data_ptr(), hyper.data_ptr(), n_ls, B, N, D, float(jitter), int(max_tries),
            L.data_ptr() if L is not None else None, z.data_ptr() if z is not None else None,
            mll.data_ptr(), info.data_ptr(), _stream_ptr(dev))
    else:
        rc = _native.lib().gpk_exact_mll_perwin_f32(
            X.data_ptr(), y.data_ptr(), hyper.data_ptr(), n_ls, stride, B, N, D, float(jitter), int(max_tries),
            L.data_ptr() if L is not None else None, z.data_ptr() if z is not None else None,
            mll.data_ptr(), info.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        _native.check(rc, _exact_name("mll", stride))
    return ExactMLLOut(mll, L if want_L else None, z, info)


@dataclass
class ExactMLLGrad:
    dX: Optional[torch.Tensor]   # (B, N, D)
    dy: Optional[torch.Tensor]   # (B, N)
    dhyp: torch.Tensor           # (B, 3 + n_ls): per-window d/d{s2, noise, c, lengthscale...}


def exact_mll_grad(X: torch.Tensor, L: torch.Tensor, z: torch.Tensor, hyper: torch.Tensor,
                   gout: torch.Tensor, want_dX: bool = True, want_dy: bool = True) -> ExactMLLGrad:
    """Analytic backward of ``exact_mll`` (one gfx950 kernel launch, see
    include/gpk.h::gpk_exact_mll_grad_f32). ``L`` and ``z`` are the forward's outputs,
    ``gout`` (B,) the incoming gradient of each window's MLL. With a 2-D ``hyper`` (B, 3 + n_ls)
    row b of ``dhyp`` is the gradient of hyper row b."""
    B, N, D = X.shape
    _require_device(X, L, z, hyper, gout)
    X = X.contiguous().float()
    L = L.contiguous().float()
    z = z.contiguous().float()
    gout = gout.reshape(B).contiguous().float()
    dev = X.device
    hyper, n_ls, stride = _exact_hyper_layout(hyper, B)
    lib = _native.lib()
    ws = torch.empty(max(1, lib.gpk_exact_grad_workspace_bytes(B, N) // 4), device=dev,
                     dtype=torch.float32)
    dX = torch.empty(B, N, D, device=dev, dtype=torch.float32) if want_dX else None
    dy = torch.empty(B, N, device=dev, dtype=torch.float32) if want_dy else None
    dhyp = torch.empty(B, 3 + n_ls, device=dev, dtype=torch.float32)
    rc = lib.gpk_exact_mll_grad_perwin_f32(
        X.data_ptr(), L.data_ptr(), z.data_ptr(), hyper.data_ptr(), n_ls, stride, B, N, D, gout.data_ptr(),
        ws.data_ptr(), dX.data_ptr() if dX is not None else None,
        dy.data_ptr() if dy is not None else None, dhyp.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        _native.check(rc, _exact_name("mll_grad", stride))
    return ExactMLLGrad(dX, dy, dhyp)


@dataclass
class ExactPosterior:
    mean: torch.Tensor   # (B, Ns) posterior mean of f
    var: torch.Tensor    # (B, Ns) posterior variance of f (unclamped)


def exact_posterior(X: torch.Tensor, L: torch.Tensor, z: torch.Tensor, hyper: torch.Tensor,
                    Xs: torch.Tensor) -> ExactPosterior:
    """Exact-GP posterior at the test inputs ``Xs`` (B, Ns, D) from the training factor
    ``L`` and ``z = L^{-1}(y - c)`` of ``exact_mll`` (one gfx950 kernel launch, see
    include/gpk.h::gpk_exact_posterior_f32). ``hyper`` is the exact path's device vector, or
    (B, 3 + n_ls) with one row per window."""
    X, L, z, hyper, Xs, (B, N, D, n_ls, stride) = _exact_prologue(X, L, z, hyper, Xs)
    Ns = Xs.shape[1]
    dev = X.device
    mean = torch.empty(B, Ns, device=dev, dtype=torch.float32)
    var = torch.empty(B, Ns, device=dev, dtype=torch.float32)
    rc = _native.lib().gpk_exact_posterior_perwin_f32(
        X.data_ptr(), L.data_ptr(), z.data_ptr(), hyper.data_ptr(), n_ls, stride, Xs.data_ptr(),
        B, N, Ns, D, mean.data_ptr(), var.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        _native.check(rc, _exact_name("posterior", stride))
    return ExactPosterior(mean, var)


@dataclass
class ExactPosteriorCov:
    mean: torch.Tensor   # (B, Ns) posterior mean of f
    var: torch.Tensor    # (B, Ns) posterior variance of f (unclamped) == diagonal(cov)
    cov: torch.Tensor    # (B, Ns, Ns) posterior covariance of f, symmetric


def exact_posterior_cov(X: torch.Tensor, L: torch.Tensor, z: torch.Tensor, hyper: torch.Tensor,
                        Xs: torch.Tensor, return_state: bool = False):
    """Joint exact-GP posterior at the test inputs ``Xs`` (B, Ns, D): ``exact_posterior``'s mean
    and variance plus the dense covariance K(xs, xs) - V^T V, V = L^{-1} K* (two gfx950 kernel
    launches of one C-ABI call, see include/gpk.h::gpk_exact_posterior_cov_f32). The V
    workspace (B * N * Ns floats) lives only for the call, unless ``return_state``:
    -> (ExactPosteriorCov, workspace), the saved state ``exact_posterior_grad`` runs from."""
    X, L, z, hyper, Xs, (B, N, D, n_ls, stride) = _exact_prologue(X, L, z, hyper, Xs)
    Ns = Xs.shape[1]
    dev = X.device
    lib = _native.lib()
    nbytes = lib.gpk_exact_posterior_cov_workspace_bytes(B, N, Ns)
    if nbytes == 0 and B > 0 and Ns > 0:
        raise ValueError(f"gpk_exact_posterior_cov_f32 does not support B={B}, N={N}, Ns={Ns}")
    ws = torch.empty(max(1, nbytes // 4), device=dev, dtype=torch.float32)
    mean = torch.empty(B, Ns, device=dev, dtype=torch.float32)
    var = torch.empty(B, Ns, device=dev, dtype=torch.float32)
    cov = torch.empty(B, Ns, Ns, device=dev, dtype=torch.float32)
    if B == 0 or Ns == 0:
        return (ExactPosteriorCov(mean, var, cov), ws) if return_state else ExactPosteriorCov(mean, var, cov)
    rc = lib.gpk_exact_posterior_cov_perwin_f32(
        X.data_ptr(), L.data_ptr(), z.data_ptr(), hyper.data_ptr(), n_ls, stride, Xs.data_ptr(),
        B, N, Ns, D, ws.data_ptr(), mean.data_ptr(), var.data_ptr(), cov.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        _native.check(rc, _exact_name("posterior_cov", stride))
    return (ExactPosteriorCov(mean, var, cov), ws) if return_state else ExactPosteriorCov(mean, var, cov)


def exact_append(X: torch.Tensor, L: torch.Tensor, z: torch.Tensor, hyper: torch.Tensor, Xn: torch.Tensor,
                 yn: torch.Tensor, jitter: float = 0.0):
    """Append the m observations ``Xn`` (B, m, D), ``yn`` (B, m) to the training factor ``L`` and
    ``z = L^{-1}(y - c)`` of ``exact_mll``: -> (L2 (B, N + m, N + m), z2 (B, N + m), info (B,) int32),
    the factor and whitened targets of the concatenated data in O(N^2 m), with L2[:, :N, :N] and
    z2[:, :N] bit-exact copies (one C-ABI call, see include/gpk.h::gpk_exact_append_f32).
    ``jitter`` is added to the diagonal of the Schur complement beside the noise: one rung of the
    jitter ladder, which the caller runs (``info[b] > 0``: window b did not factor). ``hyper`` is
    the exact path's device vector, or (B, 3 + n_ls) with one row per window."""
    def check_yn(B, N, D, _):
        if yn.shape != (B, Xn.shape[1]):
            raise ValueError(f"yn must be (B, m) = {(B, Xn.shape[1])}, got {tuple(yn.shape)}")

    X, L, z, hyper, Xn, (B, N, D, n_ls, stride) = _exact_prologue(X, L, z, hyper, Xn, "Xn", "m", (yn,), check_yn)
    m = Xn.shape[1]
    yn = yn.detach().contiguous().float()
    dev = X.device
    lib = _native.lib()
    nbytes = lib.gpk_exact_append_workspace_bytes(B, N, m)
    if nbytes == 0 and B > 0:
        raise ValueError(f"gpk_exact_append_f32 does not support B={B}, N={N}, m={m}")
    ws = torch.empty(max(1, nbytes // 4), device=dev, dtype=torch.float32)
    L2 = torch.empty(B, N + m, N + m, device=dev, dtype=torch.float32)
    z2 = torch.empty(B, N + m, device=dev, dtype=torch.float32)
    info = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0:
        return L2, z2, info
    rc = lib.gpk_exact_append_perwin_f32(
        X.data_ptr(), L.data_ptr(), z.data_ptr(), hyper.data_ptr(), n_ls, stride, Xn.data_ptr(), yn.data_ptr(),
        B, N, m, D, float(jitter), ws.data_ptr(), L2.data_ptr(), z2.data_ptr(), info.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        _native.check(rc, _exact_name("append", stride))
    return L2, z2, info


def exact_drop(L: torch.Tensor, z: torch.Tensor, m: int):
    """Drop the m oldest (first) observations from the training factor ``L`` (B, N, N) and
    ``z = L^{-1}(y - c)`` (B, N) of ``exact_mll`` / ``exact_append``: -> (L2 (B, N - m, N - m),
    z2 (B, N - m)), the factor and whitened targets of the last N - m points in O((N - m)^2 m), a
    positive rank-m update of the trailing block that cannot fail (one C-ABI call, see
    include/gpk.h::gpk_exact_drop_f32). Neither the inputs nor the hyper-parameters enter.
    1 <= m <= min(gpk_exact_drop_max_m() = 64, N - 1), otherwise ValueError."""
    if L.dim() != 3 or L.shape[1] != L.shape[2]:
        raise ValueError(f"L must be (B, N, N), got {tuple(L.shape)}")
    B, N, _ = L.shape
    if z.shape != (B, N):
        raise ValueError(f"z must be (B, N) = {(B, N)}, got {tuple(z.shape)}")
    _require_device(L, z)
    m = int(m)
    lib = _native.lib()
    if m < 1 or m > min(lib.gpk_exact_drop_max_m(), N - 1):
        raise ValueError(f"m must be in 1 .. min(gpk_exact_drop_max_m() = {lib.gpk_exact_drop_max_m()}, N - 1 = "
                         f"{N - 1}), got {m}")
    L = L.detach().contiguous().float()
    z = z.detach().contiguous().float()
    dev = L.device
    L2 = torch.empty(B, N - m, N - m, device=dev, dtype=torch.float32)
    z2 = torch.empty(B, N - m, device=dev, dtype=torch.float32)
    if B == 0:
        return L2, z2
    rc = lib.gpk_exact_drop_f32(L.data_ptr(), z.data_ptr(), B, N, m, L2.data_ptr(), z2.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        _native.check(rc, "gpk_exact_drop_f32")
    return L2, z2


@dataclass
class ExactPosteriorGrad:
    dX: Optional[torch.Tensor]    # (B, N, D)
    dy: Optional[torch.Tensor]    # (B, N)
    dXs: Optional[torch.Tensor]   # (B, Ns, D)
    dhyp: torch.Tensor            # (B, 3 + n_ls): per-window d/d{s2, noise, c, lengthscale...}


def exact_posterior_grad(X: torch.Tensor, L: torch.Tensor, z: torch.Tensor, hyper: torch.Tensor,
                         Xs: torch.Tensor, state: torch.Tensor, gmean: Optional[torch.Tensor] = None,
                         gvar: Optional[torch.Tensor] = None, gcov: Optional[torch.Tensor] = None,
                         want_dX: bool = True, want_dy: bool = True,
                         want_dXs: bool = True) -> ExactPosteriorGrad:
    """Adjoint of ``exact_posterior_cov`` (include/gpk.h::gpk_exact_posterior_grad_f32, up to six
    gfx950 launches of one C-ABI call): from gmean (B, Ns), gvar (B, Ns) and gcov (B, Ns, Ns, any
    matrix), each optional, and the forward's workspace ``state`` returns the gradients with
    respect to the training inputs and targets, the test inputs and, per window, the packed
    hyper-parameters. 1 <= N, Ns <= 256, D <= 64. The workspace lives only for the call."""
    def check_grads(B, N, D, n_ls):
        Ns = Xs.shape[1]
        if n_ls not in (1, D):
            raise ValueError(f"hyper must have 3 + 1 or 3 + D entries per vector, got {hyper.shape[-1]}")
        if gmean is None and gvar is None and gcov is None:
            raise ValueError("at least one of gmean, gvar, gcov must be given")
        for name, g, shape in (("gmean", gmean, (B, Ns)), ("gvar", gvar, (B, Ns)), ("gcov", gcov, (B, Ns, Ns))):
            if g is not None and tuple(g.shape) != shape:
                raise ValueError(f"{name} must be {shape}, got {tuple(g.shape)}")

    X, L, z, hyper, Xs, (B, N, D, n_ls, stride) = _exact_prologue(
        X, L, z, hyper, Xs, others=(state, *[g for g in (gmean, gvar, gcov) if g is not None]), check=check_grads,
        layout_first=True)
    Ns = Xs.shape[1]
    dev = X.device
    hyper = hyper.detach().contiguous().float()
    gmean, gvar, gcov = (g.detach().contiguous().float() if g is not None else None for g in (gmean, gvar, gcov))
    lib = _native.lib()
    nbytes = lib.gpk_exact_posterior_grad_workspace_bytes(B, N, Ns, D)
    if nbytes == 0 and B > 0:
        raise ValueError(f"gpk_exact_posterior_grad_f32 does not support B={B}, N={N}, Ns={Ns}, D={D}")
    dX = torch.empty(B, N, D, device=dev, dtype=torch.float32) if want_dX else None
    dy = torch.empty(B, N, device=dev, dtype=torch.float32) if want_dy else None
    dXs = torch.empty(B, Ns, D, device=dev, dtype=torch.float32) if want_dXs else None
    dhyp = torch.empty(B, 3 + n_ls, device=dev, dtype=torch.float32)
    if B == 0:
        return ExactPosteriorGrad(dX, dy, dXs, dhyp)
    want = lib.gpk_exact_posterior_cov_workspace_bytes(B, N, Ns) // 4
    if state.dtype != torch.float32 or state.device != dev or state.numel() != max(1, want):
        raise ValueError(f"state must be the {want} float32 values of exact_posterior_cov(return_state=True)'s "
                         f"workspace on {dev}, got {state.numel()} {state.dtype} on {state.device}")
    state = state.detach().contiguous()
    ws = torch.empty(max(1, nbytes // 4), device=dev, dtype=torch.float32)
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.gpk_exact_posterior_grad_perwin_f32(
        X.data_ptr(), L.data_ptr(), z.data_ptr(), hyper.data_ptr(), n_ls, stride, Xs.data_ptr(), state.data_ptr(),
        ptr(gmean), ptr(gvar), ptr(gcov), B, N, Ns, D, ws.data_ptr(), ptr(dX), ptr(dy), ptr(dXs),
        dhyp.data_ptr(), _stream_ptr(dev))
    if rc != 0:
        _native.check(rc, _exact_name("posterior_grad", stride))
    return ExactPosteriorGrad(dX, dy, dXs, dhyp)


INFO_TIMEOUT = 1 << 20   # gpk_exact.hip kInfoTimeout: a bounded LDS spin-wait expired


class DeferredChecks:
    """Host-side verdicts recorded while a HIP graph is being captured.

    A captured step cannot read device memory on the host (the capture would break),
    so psd_safe_cholesky's info check and the variance-clamp flag are RECORDED instead.
    Each recorded check is condensed IN THE GRAPH into a 3-int verdict (max info,
    ladder steps, NaN in the inputs / clamp bit) by one gpk_record_check launch, written
    into slot ``replay % slots`` of a device ring; ``finalize()`` (captured at the end of
    the step) advances the replay counter. ``check(n)`` after n replays reads the ring with ONE device->host copy and
    warns / raises for each of the n replays in order, exactly as the eager calls would
    have -- so a block of ``slots`` replays costs one host sync, not one per check.
    """

    MAX_ITEMS = 16   # recorded checks per step (the cfg-3 step records 2-3)

    def __init__(self, device=None, slots: int = 1):
        self.items = []
        self.slots = max(1, int(slots))
        self.ring = None
        # (1,) int32 device flag: any hard failure since reset_sticky(); (1,) int64 replay
        # counter. Allocated before the capture (a tensor created inside it would be
        # re-zeroed by every replay)
        self.sticky = torch.zeros(1, dtype=torch.int32, device=device) if device is not None else None
        self.counter = torch.zeros(1, dtype=torch.int64, device=device) if device is not None else None
        self._ring = (torch.zeros(self.slots, self.MAX_ITEMS, 3, dtype=torch.int32, device=device)
                      if device is not None else None)
        self._keep = []   # tensors the recorded verdict launches read (kept alive with the graph)

    def add(self, kind: str, args: tuple) -> None:
        """Record a check; in a capture also its in-graph verdict (include/gpk.h::
        gpk_record_check: one small kernel per check, the ring slot of this replay)."""
        self.items.append((kind, args))
        if self.sticky is None:
            if kind == "cholesky":
                raise RuntimeError("DeferredChecks used in a capture without a device flag "
                                   "(construct it with device=...)")
            return
        if not self.sticky.is_cuda:   # host tensors (tests of the bookkeeping): torch ops
            if kind == "cholesky":
                self.sticky.copy_(torch.maximum(self.sticky, (args[0] > 0).any().to(torch.int32).reshape(1)))
            return
        item = len(self.items) - 1
        if item >= self.MAX_ITEMS:
            raise RuntimeError(f"more than {self.MAX_ITEMS} numerical checks recorded in one step")
        t = args[0]
        if kind == "cholesky":
            info = t.reshape(-1)
            ins = [x.detach().reshape(-1).float() for x in args[4] if x is not None][:2]
            ins = [x if x.is_contiguous() else x.contiguous() for x in ins]
            p = [(x.data_ptr(), x.numel()) for x in ins] + [(None, 0)] * (2 - len(ins))
            rc = _native.lib().gpk_record_check(info.data_ptr(), info.numel(), p[0][0], p[0][1], p[1][0],
                                                p[1][1], 0, self._ring.data_ptr(), self.counter.data_ptr(),
                                                self.slots, item, self.MAX_ITEMS, self.sticky.data_ptr(),
                                                _stream_ptr(info.device))
            self._keep.append(ins)
        else:
            flag = t.reshape(-1).to(torch.int32)
            rc = _native.lib().gpk_record_check(flag.data_ptr(), 1, None, 0, None, 0, 1, self._ring.data_ptr(),
                                                self.counter.data_ptr(), self.slots, item, self.MAX_ITEMS,
                                                None, _stream_ptr(flag.device))
            self._keep.append([flag])
        _native.check(rc, "gpk_record_check")

    def finalize(self) -> None:
        """Captured at the end of the step: advance the replay counter (the ring slot)."""
        if not self.items or self.counter is None or not self.counter.is_cuda:
            return
        rc = _native.lib().gpk_record_check(None, 0, None, 0, None, 0, 2, None, self.counter.data_ptr(),
                                            self.slots, 0, self.MAX_ITEMS, None,
                                            _stream_ptr(self.counter.device))
        _native.check(rc, "gpk_record_check")
        self.ring = self._ring[:, :len(self.items)]

    def reset_sticky(self) -> None:
        if self.sticky is not None:
            self.sticky.zero_()

    def _replay_verdicts(self, n: int):
        """Host copy of the last n replays' verdicts, oldest first (one sync)."""
        both = torch.cat([self.ring.reshape(-1).to(torch.int64), self.counter.reshape(-1)]).cpu()
        cnt = int(both[-1])
        ring = both[:-1].reshape(self.ring.shape)
        n = min(n, self.slots, cnt)
        return [ring[(cnt - n + r) % self.slots] for r in range(n)]

    def check(self, n: int = 1) -> None:
        if self.ring is None:        # nothing condensed (e.g. recorded outside GraphedStep)
            for kind, args in self.items:
                if kind == "cholesky":
                    info, jitter, what, max_tries, inputs = args
                    check_cholesky_info(info, jitter, inputs, what, max_tries)
                else:
                    from .gp import warn_if_clamped
                    warn_if_clamped(*args)
        else:
            for verdicts in self._replay_verdicts(n):
                for (kind, args), v in zip(self.items, verdicts.tolist()):
                    if kind == "cholesky":
                        _raise_or_warn_verdict(v, args[1], args[2], args[3])
                    elif v[0] & 1:
                        from .gp import warn_if_clamped
                        warn_if_clamped(torch.ones(1, dtype=torch.int32), args[1])
        if self.sticky is not None and int(self.sticky.item()) != 0:
            raise NotPSDError("a replay of this check block failed psd_safe_cholesky (not PD after "
                              "the jitter ladder, or NaN inputs); state rolled back to the block start")


def _raise_or_warn_verdict(v, jitter: float, what: str, max_tries: int) -> None:
    """check_cholesky_info from a condensed verdict [max info, ladder steps, NaN inputs]."""
    max_info, steps, nan = v
    if max_info >= INFO_TIMEOUT:
        raise GpkInternalError(f"{what}: kernel spin-wait timed out (info = 1<<20)")
    failed = max_info > 0
    if failed and nan:
        raise NanError(f"{what}: NaN elements in the inputs.")
    if failed:
        steps = max_tries
    for i in range(steps):
        warnings.warn(f"A not p.d., added jitter of {jitter * (10 ** i):.1e} to the diagonal",
                      NumericalWarning)
    if failed:
        raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to "
                          f"{jitter * 10 ** (max_tries - 1):.1e}.")


_RECORDERS: list = []


def record_or_run(kind: str, args: tuple, run) -> None:
    """Run a host-side check now, or record it when the current stream is capturing."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        if not _RECORDERS:
            raise RuntimeError("gpk: a HIP graph capture reached a host-side numerical check; "
                               "capture through graphs.GraphedStep, which defers the checks")
        _RECORDERS[-1].add(kind, args)
        return
    run()


def check_cholesky_info(info: torch.Tensor, jitter: float, inputs=(), what: str = "cholesky",
                        max_tries: int = 3) -> None:
    """GPyTorch's psd_safe_cholesky bookkeeping, from the per-window info codes.

    One device->host sync (GPyTorch pays the same: ``torch.any(info)``). Emits the
    same NumericalWarning text per ladder step and raises NanError / NotPSDError.
    When any window is still not PD, psd_safe_cholesky has walked the whole ladder
    (``max_tries`` warnings) before raising, whatever the other windows needed.
    Under HIP graph capture the check is recorded (DeferredChecks) instead.
    """
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        record_or_run("cholesky", (info, jitter, what, max_tries, tuple(inputs)), None)
        return
    info_h = info.detach().to("cpu")
    if not bool((info_h != 0).any()):
        return
    if bool((info_h >= INFO_TIMEOUT).any()):
        raise GpkInternalError(f"{what}: kernel spin-wait timed out (info = 1<<20) in windows "
                               f"{torch.nonzero(info_h >= INFO_TIMEOUT).flatten().tolist()[:16]}")
    failed = bool((info_h > 0).any())
    if failed:
        for t in inputs:
            if t is not None and bool(torch.isnan(t).any()):
                raise NanError(f"{what}: {int(torch.isnan(t).sum())} of {t.numel()} elements of the "
                               f"{tuple(t.shape)} tensor are NaN.")
    steps = int((-info_h[info_h < 0]).max()) if bool((info_h < 0).any()) else 0
    if failed:
        steps = max_tries
    for i in range(steps):
        warnings.warn(f"A not p.d., added jitter of {jitter * (10 ** i):.1e} to the diagonal",
                      NumericalWarning)
    if failed:
        raise NotPSDError(
            f"Matrix not positive definite after repeatedly adding jitter up to "
            f"{jitter * 10 ** (max_tries - 1):.1e}. Failing windows: "
            f"{torch.nonzero(info_h > 0).flatten().tolist()[:16]}")


LOG_2PI = math.log(2 * math.pi)


# ---------------------------------------------------------------------------
# Variational (DeepGP) path. One body per operation: the rank of Z selects the form -- Z (M, D) is
# one GP, Z (O, M, D) the O independent output GPs of a multi-output layer in one launch of every
# kernel (include/gpk.h::gpk_*_batched; ToyDeepGPHiddenLayer(output_dims=O), DeepGP.py:24-31) --
# ``lead`` = () or (O,) is the leading shape of every per-output array, and the C entry point is
# chosen at one place in the body. The public single and ``_batched`` names check their rank and
# call the body.
# ---------------------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _single_output(Z: torch.Tensor) -> None:
    if Z.dim() != 2:
        raise ValueError(f"Z must be (M, D), got {tuple(Z.shape)}")


def _multi_output(Z: torch.Tensor) -> None:
    if Z.dim() != 3:
        raise ValueError(f"Z must be (O, M, D), got {tuple(Z.shape)}")


def _batched_x(X: torch.Tensor, O: int):
    """(contiguous float X, shared flag): X (B, N, D) is read by every output; an (O, B, N, D)
    tensor whose output dimension is an expansion (stride 0) too, without a copy."""
    if X.dim() == 3:
        return X.detach().contiguous().float(), True
    if X.dim() != 4 or X.shape[0] != O:
        raise ValueError(f"X must be (B, N, D) or (O, B, N, D) with O = {O}, got {tuple(X.shape)}")
    if O > 1 and X.stride(0) == 0:
        return X[0].detach().contiguous().float(), True
    return X.detach().contiguous().float(), False


def _var_args(X, Z, Linv, hyper, cast_linv: bool = False):
    """Checked, contiguous arguments of a variational op -> (X, shared, Z, Linv, hyper, lead, O or
    None, B, N, M, D). ``hyper`` is pack_variational_hyper's vector, one row per output. The
    forwards require a float64 Linv; the adjoints (``cast_linv``) convert it."""
    if Z.dim() == 3:
        O, M, D = Z.shape
        X, shared = _batched_x(X, O)
        lead = (O,)
    elif Z.dim() == 2:
        O, (M, D) = None, Z.shape
        if X.dim() != 3:
            raise ValueError(f"X must be (B, N, D), got {tuple(X.shape)}")
        X, shared, lead = X.detach().contiguous().float(), True, ()
    else:
        raise ValueError(f"Z must be (M, D) or (O, M, D), got {tuple(Z.shape)}")
    B, N = X.shape[-3], X.shape[-2]
    if X.shape[-1] != D:
        raise ValueError(f"Z must be (..., M, {X.shape[-1]}), got {tuple(Z.shape)}")
    if cast_linv:
        Linv = Linv.double()
    if tuple(Linv.shape) != lead + (M, M) or Linv.dtype != torch.float64:
        raise ValueError(f"Linv must be {lead + (M, M)} float64 from kzz_cholesky")
    if tuple(hyper.shape) != lead + (4 + 2 * D,):
        raise ValueError(f"hyper must be {lead + (4 + 2 * D,)}, got {tuple(hyper.shape)}")
    return (X, shared, Z.detach().contiguous().float(), Linv.detach().contiguous(),
            hyper.detach().contiguous().float(), lead, O, B, N, M, D)


def _per_output(t: torch.Tensor, *shape) -> torch.Tensor:
    """A q(u) parameter or an incoming gradient as a contiguous float32 array of ``shape``."""
    return t.detach().reshape(shape).contiguous().float()


def _vchol_arg(vchol: torch.Tensor, lead, M: int) -> torch.Tensor:
    if tuple(vchol.shape) != lead + (M, M):
        raise ValueError(f"chol_variational_covar must be {lead + (M, M)}, got {tuple(vchol.shape)}")
    return vchol.detach().contiguous().float()


def _abi(X, shared, O, *sizes):
    """The two places where a batched entry point's argument list differs from the single one: the
    input pointer is followed by its shared flag, and the sizes are preceded by O."""
    if O is None:
        return (X.data_ptr(),), sizes
    return (X.data_ptr(), int(shared)), (O,) + sizes


@dataclass
class KzzFactor:
    L: torch.Tensor      # (M, M) float64 lower Cholesky factor of K_ZZ + jitter; (O, M, M) for O outputs
    Linv: torch.Tensor   # (M, M) float64 L^{-1}; (O, M, M)
    info: torch.Tensor   # (1,) int32; (O,)


def _kzz_cholesky(Z, hyper, jitter, chol_jitter, max_tries) -> KzzFactor:
    """Z (float32, contiguous) and hyper = {outputscale, lengthscale[D]} per output, both checked."""
    lead, (M, D) = tuple(Z.shape[:-2]), Z.shape[-2:]
    dev = Z.device
    L = torch.empty(*lead, M, M, device=dev, dtype=torch.float64)
    Linv = torch.empty(*lead, M, M, device=dev, dtype=torch.float64)
    info = torch.empty(lead or (1,), device=dev, dtype=torch.int32)
    name = "gpk_kzz_chol_f64_batched" if lead else "gpk_kzz_chol_f64"
    rc = getattr(_native.lib(), name)(Z.data_ptr(), hyper.data_ptr(), *lead, M, D, float(jitter),
                                      float(chol_jitter), int(max_tries), L.data_ptr(), Linv.data_ptr(),
                                      info.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return KzzFactor(L, Linv, info)


def kzz_cholesky(Z: torch.Tensor, outputscale, lengthscale, jitter: float = 1e-4,
                 chol_jitter: float = 1e-8, max_tries: int = 3,
                 hyper: Optional[torch.Tensor] = None) -> KzzFactor:
    """Shared inducing-point factorisation (include/gpk.h::gpk_kzz_chol_f64)."""
    _single_output(Z)
    _require_device(Z)
    Z = Z.detach().contiguous().float()
    D = Z.shape[1]
    if hyper is None:
        ls = _scalar_tensor(lengthscale, Z.device)
        hyper = torch.cat([_scalar_tensor(outputscale, Z.device)[:1],
                           ls.expand(D) if ls.numel() == 1 else ls]).contiguous()
    if hyper.numel() != 1 + D:
        raise ValueError(f"kzz hyper must hold 1 + D = {1 + D} values, got {hyper.numel()}")
    return _kzz_cholesky(Z, hyper, jitter, chol_jitter, max_tries)


def kzz_cholesky_batched(Z: torch.Tensor, hyper: torch.Tensor, jitter: float = 1e-4,
                         chol_jitter: float = 1e-8, max_tries: int = 3) -> KzzFactor:
    """The K_ZZ factors of O outputs (include/gpk.h::gpk_kzz_chol_f64_batched): Z (O, M, D),
    hyper (O, 1 + D) = {outputscale, lengthscale[D]} per output -> L, Linv (O, M, M) float64
    and info (O,), bit-identical to O ``kzz_cholesky`` calls."""
    _multi_output(Z)
    _require_device(Z, hyper)
    O, _, D = Z.shape
    if tuple(hyper.shape) != (O, 1 + D):
        raise ValueError(f"kzz hyper must be (O, 1 + D) = {(O, 1 + D)}, got {tuple(hyper.shape)}")
    return _kzz_cholesky(Z.detach().contiguous().float(), hyper.detach().contiguous().float(), jitter,
                         chol_jitter, max_tries)


def _kzz_backward(dLinv, L, Linv, Z, hyper):
    """-> (dZ (..., M, D) float, dhyp (..., 1 + D) = {ds2, dlengthscale[D]} per output)."""
    _require_device(dLinv, L, Linv, Z, hyper)
    lead, (M, D) = tuple(Z.shape[:-2]), Z.shape[-2:]
    dev = Z.device
    lib = _native.lib()
    if lead:
        name = "gpk_kzz_backward_f64_batched"
        nbytes = lib.gpk_kzz_backward_batched_workspace_bytes(*lead, M, D)
        if nbytes == 0:
            raise ValueError(f"unsupported K_ZZ shape O={lead[0]} M={M} D={D}")
    else:
        name = "gpk_kzz_backward_f64"
        nbytes = lib.gpk_kzz_backward_workspace_bytes(M, D)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dZ = torch.empty(*lead, M, D, device=dev, dtype=torch.float32)
    dhyp = torch.empty(*lead, 1 + D, device=dev, dtype=torch.float32)
    rc = getattr(lib, name)(
        dLinv.detach().contiguous().double().data_ptr(), L.detach().contiguous().double().data_ptr(),
        Linv.detach().contiguous().double().data_ptr(), Z.detach().contiguous().float().data_ptr(),
        hyper.detach().contiguous().float().data_ptr(), *lead, M, D, ws.data_ptr(), dZ.data_ptr(),
        dhyp.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return dZ, dhyp


def kzz_backward(dLinv: torch.Tensor, L: torch.Tensor, Linv: torch.Tensor, Z: torch.Tensor,
                 outputscale: torch.Tensor, lengthscale: torch.Tensor):
    """Back-propagate dObjective/dLinv (lower, fp64) through Linv = chol(K_ZZ + jitter)^{-1}
    to (dZ, d outputscale, d lengthscale): once per optimizer step for all GP calls that
    shared the factor (include/gpk.h::gpk_kzz_backward_f64: five fp64-MFMA tile GEMMs
    Lbar = -tril(Linv^T G Linv^T), S = Linv^T Phi(L^T Lbar) Linv, then the RBF adjoint over
    K_ZZ with Kbar = (S + S^T)/2). Returns (dZ (M, D) float, ds2 (), dls (D,)) -- dls per
    dimension even for a shared lengthscale (the caller sums)."""
    _single_output(Z)
    D = Z.shape[1]
    ls = lengthscale.detach().reshape(-1).float()
    hyper = torch.cat([outputscale.detach().reshape(1).float(), ls.expand(D) if ls.numel() == 1 else ls])
    dZ, dhyp = _kzz_backward(dLinv, L, Linv, Z, hyper)
    return dZ, dhyp[0], dhyp[1:]


def kzz_backward_batched(dLinv: torch.Tensor, L: torch.Tensor, Linv: torch.Tensor, Z: torch.Tensor,
                         hyper: torch.Tensor):
    """``kzz_backward`` for O outputs, every launch once (gpk_kzz_backward_f64_batched):
    dLinv, L, Linv (O, M, M) float64, Z (O, M, D), hyper (O, 1 + D) -> (dZ (O, M, D),
    dhyp (O, 1 + D) = {ds2, dlengthscale[D]} per output)."""
    _multi_output(Z)
    O, M, D = Z.shape
    for name, t in (("dLinv", dLinv), ("L", L), ("Linv", Linv)):
        if tuple(t.shape) != (O, M, M):
            raise ValueError(f"{name} must be (O, M, M) = {(O, M, M)}, got {tuple(t.shape)}")
    if tuple(hyper.shape) != (O, 1 + D):
        raise ValueError(f"kzz hyper must be (O, 1 + D) = {(O, 1 + D)}, got {tuple(hyper.shape)}")
    return _kzz_backward(dLinv, L, Linv, Z, hyper)


@dataclass
class VariationalOut:
    mean: torch.Tensor           # (B, N); (O, B, N) for O outputs
    var: torch.Tensor            # as mean, clamped at 1e-6
    ell: Optional[torch.Tensor]  # (B,) sum over N of the expected log likelihood (one output, with y)
    flags: Optional[torch.Tensor]  # (1,) int32: bit 0 = the variance clamp fired (one word for all outputs)
    saved: Optional[torch.Tensor] = None  # training state for variational_adjoint (M > 64), or None


_CONST_PAIRS: dict = {}


def _const_pair(a: float, b: float, device) -> torch.Tensor:
    """Device tensor [a, b] for python-float hyper entries, cached per (device, a, b) so a
    step packs its hyper vector with ONE cat kernel. Never cached while a HIP graph is being
    captured (the tensor would live in the graph's private pool): GraphedStep's eager
    warm-up steps populate the cache first."""
    key = (str(torch.device(device)), float(a), float(b))
    t = _CONST_PAIRS.get(key)
    if t is not None:
        return t
    t = torch.stack([torch.full((), float(a), device=device), torch.full((), float(b), device=device)])
    if not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        _CONST_PAIRS[key] = t
    return t


def pack_variational_hyper(outputscale, noise, jitter, bias, weights, lengthscale, D, device):
    ls = _scalar_tensor(lengthscale, device)
    if ls.numel() == 1:
        ls = ls.expand(D)
    w = _scalar_tensor(weights, device).reshape(-1)
    if w.numel() != D:
        raise ValueError(f"LinearMean weights must have D={D} entries, got {w.numel()}")
    if not isinstance(noise, torch.Tensor) and not isinstance(jitter, torch.Tensor):
        mid = _const_pair(noise, jitter, device)
    else:
        mid = torch.cat([_scalar_tensor(noise, device)[:1], _scalar_tensor(jitter, device)[:1]])
    return torch.cat([_scalar_tensor(outputscale, device)[:1], mid, _scalar_tensor(bias, device)[:1],
                      w, ls]).contiguous()


def _variational_forward(X, Z, Linv, vmean, vstd, hyper, y, want_flags, save) -> VariationalOut:
    _require_device(X, Z, Linv, vmean, vstd, hyper)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper)
    dev = X.device
    vmean = _per_output(vmean, *lead, M)
    vstd = _per_output(vstd, *lead, M)
    if y is not None:
        if y.shape != (B, N):
            raise ValueError(f"y must be (B, N) = {(B, N)}, got {tuple(y.shape)}")
        _require_device(y)
        y = y.detach().contiguous().float()
    mean = torch.empty(*lead, B, N, device=dev, dtype=torch.float32)
    var = torch.empty(*lead, B, N, device=dev, dtype=torch.float32)
    ell = torch.empty(B, device=dev, dtype=torch.float32) if y is not None else None
    flags = torch.empty(1, device=dev, dtype=torch.int32) if want_flags else None
    lib = _native.lib()
    nsaved = lib.gpk_variational_saved_bytes(B, N, M, D) if (save and B > 0) else 0
    saved = torch.empty((O or 1) * (nsaved // 4), device=dev, dtype=torch.float32) if nsaved > 0 else None
    ins = (Z.data_ptr(), Linv.data_ptr(), vmean.data_ptr(), vstd.data_ptr(), hyper.data_ptr())
    if O is not None:        # one entry point, the state or NULL; no y / ell
        name = "gpk_variational_batched_f32"
        rc = lib.gpk_variational_batched_f32(X.data_ptr(), int(shared), *ins, O, B, N, M, D, mean.data_ptr(),
                                             var.data_ptr(), _ptr(flags), _ptr(saved), _stream_ptr(dev))
    elif saved is not None:
        name = "gpk_variational_train_f32"
        rc = lib.gpk_variational_train_f32(X.data_ptr(), *ins, _ptr(y), B, N, M, D, mean.data_ptr(),
                                           var.data_ptr(), _ptr(ell), _ptr(flags), saved.data_ptr(),
                                           _stream_ptr(dev))
    else:
        name = "gpk_variational_f32"
        rc = lib.gpk_variational_f32(X.data_ptr(), *ins, _ptr(y), B, N, M, D, mean.data_ptr(),
                                     var.data_ptr(), _ptr(ell), _ptr(flags), _stream_ptr(dev))
    _native.check(rc, name)
    return VariationalOut(mean, var, ell, flags, saved)


def variational_forward(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vmean: torch.Tensor,
                        vstd: torch.Tensor, outputscale=None, noise=None, jitter=None, bias=None,
                        weights=None, lengthscale=None, y: Optional[torch.Tensor] = None,
                        hyper: Optional[torch.Tensor] = None, want_flags: bool = True,
                        save: bool = False) -> VariationalOut:
    """Batched q(f) mean / variance (+ expected log likelihood sum when y is given)
    for the whitened mean-field VariationalStrategy (include/gpk.h::gpk_variational_f32).
    ``save=True`` (training): where the saved-state adjoint serves the shape (M > 64), the
    forward also keeps A = Linv K_ZX and the clamp mask (gpk_variational_train_f32) in
    ``out.saved`` for ``variational_adjoint(..., saved=out.saved)``; None elsewhere."""
    _single_output(Z)
    if hyper is None:
        hyper = pack_variational_hyper(outputscale, noise, jitter, bias, weights, lengthscale, X.shape[-1],
                                       X.device)
    return _variational_forward(X, Z, Linv, vmean, vstd, hyper, y, want_flags, save)


def variational_forward_batched(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vmean: torch.Tensor,
                                vstd: torch.Tensor, hyper: torch.Tensor, want_flags: bool = True,
                                save: bool = False) -> VariationalOut:
    """``variational_forward`` for O outputs in one launch (gpk_variational_batched_f32): X
    (B, N, D) shared by every output or (O, B, N, D), Z (O, M, D), Linv (O, M, M) float64,
    vmean / vstd (O, M), hyper (O, 4 + 2D) -> mean, var (O, B, N), one clamp flag word for all
    outputs and, with ``save`` where the saved-state adjoint serves the shape, the O training
    states in ``out.saved``. Bit-identical to O single-output calls."""
    _multi_output(Z)
    return _variational_forward(X, Z, Linv, vmean, vstd, hyper, None, want_flags, save)


@dataclass
class VariationalAdjoint:
    dX: torch.Tensor      # (B, N, D)
    dLinv: torch.Tensor   # (M, M) float64, lower: sum over points of dA K_ZX^T
    dpar: torch.Tensor    # (2M + 2D + 2,) the packed parameter gradients below
    dZ: torch.Tensor      # (M, D) the K_ZX part of dZ
    dvmean: torch.Tensor  # (M,)
    dvstd: torch.Tensor   # (M,)
    ds2: torch.Tensor     # () K_ZX + variance parts
    dls: torch.Tensor     # (D,) the K_ZX part
    dw: torch.Tensor      # (D,) LinearMean weights
    db0: torch.Tensor     # () LinearMean bias


@dataclass
class VariationalAdjointBatched:
    dX: torch.Tensor      # (O, B, N, D) per output (shared inputs: the caller sums over O)
    dLinv: torch.Tensor   # (O, M, M) float64, lower
    dZ: torch.Tensor      # (O, M, D) the K_ZX part of dZ
    dpar: torch.Tensor    # (O, 2M + 2D + 2): dvmean (M), dvstd (M), ds2, dls (D), dw (D), db0


def _variational_adjoint(X, Z, Linv, vmean, vstd, hyper, gmean, gvar, saved):
    """-> (dX, dLinv, dZ, dpar), every array with ``lead``."""
    _require_device(X, Z, Linv, vmean, vstd, hyper, gmean, gvar)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper, cast_linv=True)
    dev = X.device
    vmean = _per_output(vmean, *lead, M)
    vstd = _per_output(vstd, *lead, M)
    gmean = _per_output(gmean, *lead, B, N)
    gvar = _per_output(gvar, *lead, B, N)
    lib = _native.lib()
    if saved is not None:
        # the C entry point receives a bare pointer: the dtype, device and size are checked here
        if saved.dtype != torch.float32 or saved.device != dev:
            raise ValueError(f"saved state must be float32 on {dev} (got {saved.dtype} on {saved.device}): "
                             f"pass the forward's (save=True) ``saved`` unchanged")
        if saved.numel() * 4 != (O or 1) * lib.gpk_variational_saved_bytes(B, N, M, D):
            raise ValueError("saved state does not match this shape (the forward's, with save=True)")
        saved = saved.detach().contiguous()
    # one output: an entry point and a workspace query per way; O outputs: one of each, has_saved
    if O is not None:
        name = "gpk_variational_adjoint_batched_f32"
        nbytes = lib.gpk_variational_adjoint_batched_workspace_bytes(O, B, N, M, D, int(saved is not None))
    elif saved is not None:
        name = "gpk_variational_adjoint_saved_f32"
        nbytes = lib.gpk_variational_adjoint_saved_workspace_bytes(B, N, M, D)
    else:
        name = "gpk_variational_adjoint_f32"
        nbytes = lib.gpk_variational_adjoint_workspace_bytes(B, N, M, D)
    if nbytes == 0:
        raise ValueError(f"unsupported variational shape O={O} B={B} N={N} M={M} D={D}")
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dX = torch.empty(*lead, B, N, D, device=dev, dtype=torch.float32)
    dLinv = torch.empty(*lead, M, M, device=dev, dtype=torch.float64)
    dZ = torch.empty(*lead, M, D, device=dev, dtype=torch.float32)
    dpar = torch.empty(*lead, 2 * M + 2 * D + 2, device=dev, dtype=torch.float32)
    x, dims = _abi(X, shared, O, B, N, M, D)
    state = (_ptr(saved),) if (O is not None or saved is not None) else ()
    rc = getattr(lib, name)(*x, Z.data_ptr(), Linv.data_ptr(), vmean.data_ptr(), vstd.data_ptr(),
                            hyper.data_ptr(), gmean.data_ptr(), gvar.data_ptr(), *state, *dims, ws.data_ptr(),
                            dX.data_ptr(), dLinv.data_ptr(), dZ.data_ptr(), dpar.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return dX, dLinv, dZ, dpar


def variational_adjoint(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vmean: torch.Tensor,
                        vstd: torch.Tensor, hyper: torch.Tensor, gmean: torch.Tensor,
                        gvar: torch.Tensor, saved: Optional[torch.Tensor] = None) -> VariationalAdjoint:
    """Adjoint of ``variational_forward`` except the shared K_ZZ factor (fused gfx950
    kernels behind include/gpk.h::gpk_variational_adjoint_f32; from the training forward's
    ``saved`` state: gpk_variational_adjoint_saved_f32)."""
    _single_output(Z)
    M, D = Z.shape
    dX, dLinv, dZ, dpar = _variational_adjoint(X, Z, Linv, vmean, vstd, hyper, gmean, gvar, saved)
    return VariationalAdjoint(dX, dLinv, dpar, dZ, dpar[:M], dpar[M:2 * M], dpar[2 * M],
                              dpar[2 * M + 1:2 * M + 1 + D], dpar[2 * M + 1 + D:2 * M + 1 + 2 * D],
                              dpar[2 * M + 1 + 2 * D])


def variational_adjoint_batched(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vmean: torch.Tensor,
                                vstd: torch.Tensor, hyper: torch.Tensor, gmean: torch.Tensor,
                                gvar: torch.Tensor,
                                saved: Optional[torch.Tensor] = None) -> VariationalAdjointBatched:
    """``variational_adjoint`` for O outputs, every launch once
    (gpk_variational_adjoint_batched_f32); arguments as ``variational_forward_batched`` plus
    gmean / gvar (O, B, N) and the forward's ``saved`` state (None: recompute)."""
    _multi_output(Z)
    return VariationalAdjointBatched(*_variational_adjoint(X, Z, Linv, vmean, vstd, hyper, gmean, gvar, saved))


def _variational_cov(X, Z, Linv, vstd, hyper, return_state):
    _require_device(X, Z, Linv, vstd, hyper)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper)
    dev = X.device
    vstd = _per_output(vstd, *lead, M)
    lib = _native.lib()
    if O is None:
        name = "gpk_variational_cov_f32"
        nbytes = lib.gpk_variational_cov_workspace_bytes(B, N, M)
    else:
        name = "gpk_variational_cov_batched_f32"
        nbytes = lib.gpk_variational_cov_batched_workspace_bytes(O, B, N, M)
    if nbytes == 0 and B > 0:
        raise ValueError(f"{name} does not support O={O}, B={B}, N={N}, M={M}")
    cov = torch.empty(*lead, B, N, N, device=dev, dtype=torch.float32)
    if B == 0:
        return (cov, torch.empty(0, device=dev, dtype=torch.float32)) if return_state else cov
    ws = torch.empty(max(1, nbytes // 4), device=dev, dtype=torch.float32)
    x, dims = _abi(X, shared, O, B, N, M, D)
    rc = getattr(lib, name)(*x, Z.data_ptr(), Linv.data_ptr(), vstd.data_ptr(), hyper.data_ptr(), *dims,
                            ws.data_ptr(), cov.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return (cov, ws) if return_state else cov


def variational_cov(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vstd: torch.Tensor,
                    hyper: torch.Tensor, return_state: bool = False):
    """Dense covariance of q(f) at X (B, N, D): K_XX + jitter I + A^T diag(vstd^2 - 1) A with
    A = Linv K_ZX (two gfx950 kernel launches of one C-ABI call, see
    include/gpk.h::gpk_variational_cov_f32). ``hyper`` is the variational path's packed device
    vector (pack_variational_hyper). Memory per call: the A workspace (B * M * N floats, N
    rounded up to 64, + 64 B) lives only for the call; the result is B * N^2 floats.
    ``return_state``: -> (cov, workspace), the saved state ``variational_cov_grad`` runs from."""
    _single_output(Z)
    return _variational_cov(X, Z, Linv, vstd, hyper, return_state)


def variational_cov_batched(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vstd: torch.Tensor,
                            hyper: torch.Tensor, return_state: bool = False):
    """``variational_cov`` for O outputs in one launch chain (gpk_variational_cov_batched_f32): X
    (B, N, D) shared by every output or (O, B, N, D), Z (O, M, D), Linv (O, M, M) float64, vstd
    (O, M), hyper (O, 4 + 2D) -> cov (O, B, N, N). Bit-identical to O single-output calls.
    Memory per call: O workspaces of ``variational_cov`` + the O * B * N^2 floats of cov.
    ``return_state``: -> (cov, workspace), the saved state of ``variational_cov_grad_batched``."""
    _multi_output(Z)
    return _variational_cov(X, Z, Linv, vstd, hyper, return_state)


def _cov_grad_state(state, nfloats, dev, source: str):
    """The forward's workspace, as ``source`` (return_state=True) returned it: the C entry point
    receives a bare pointer, so its dtype, device and size are checked here."""
    if state.dtype != torch.float32 or state.device != dev or state.numel() != max(1, nfloats):
        raise ValueError(f"state must be the {nfloats} float32 values on {dev} that {source}(return_state=True) "
                         f"returned for this shape, got {state.numel()} {state.dtype} on {state.device}")
    return state.detach().contiguous()


def _variational_cov_grad(X, Z, Linv, vstd, hyper, state, gcov):
    _require_device(X, Z, Linv, vstd, hyper, state, gcov)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper)
    dev = X.device
    if tuple(gcov.shape) != lead + (B, N, N):
        raise ValueError(f"gcov must be {lead + (B, N, N)}, got {tuple(gcov.shape)}")
    vstd = _per_output(vstd, *lead, M)
    gcov = gcov.detach().contiguous().float()
    lib = _native.lib()
    if O is None:
        name = "gpk_variational_cov_grad_f32"
        nbytes = lib.gpk_variational_cov_grad_workspace_bytes(B, N, M, D)
    else:
        name = "gpk_variational_cov_grad_batched_f32"
        nbytes = lib.gpk_variational_cov_grad_batched_workspace_bytes(O, B, N, M, D)
    if nbytes == 0 and B > 0:
        raise ValueError(f"{name} does not support O={O}, B={B}, N={N}, M={M}, D={D}")
    dX = torch.empty(*lead, B, N, D, device=dev, dtype=torch.float32)
    dLinv = torch.empty(*lead, M, M, device=dev, dtype=torch.float64)
    dZ = torch.empty(*lead, M, D, device=dev, dtype=torch.float32)
    dpar = torch.empty(*lead, M + 1 + D, device=dev, dtype=torch.float32)
    if B == 0:
        return dX, dLinv.zero_(), dZ.zero_(), dpar.zero_()
    state = _cov_grad_state(state, (O or 1) * (lib.gpk_variational_cov_workspace_bytes(B, N, M) // 4), dev,
                            "variational_cov")
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    x, dims = _abi(X, shared, O, B, N, M, D)
    rc = getattr(lib, name)(*x, Z.data_ptr(), Linv.data_ptr(), vstd.data_ptr(), hyper.data_ptr(),
                            state.data_ptr(), gcov.data_ptr(), *dims, ws.data_ptr(), dX.data_ptr(),
                            dLinv.data_ptr(), dZ.data_ptr(), dpar.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return dX, dLinv, dZ, dpar


def variational_cov_grad(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vstd: torch.Tensor,
                         hyper: torch.Tensor, state: torch.Tensor, gcov: torch.Tensor):
    """Adjoint of ``variational_cov`` (include/gpk.h::gpk_variational_cov_grad_f32, six gfx950
    launches of one C-ABI call): from gcov (B, N, N) = dObjective / dcov and the forward's
    workspace ``state`` returns (dX (B, N, D), dLinv (M, M) float64 lower, dZ (M, D), dpar
    (M + 1 + D) = [dvstd, ds2, dlengthscale]). Memory per call: the workspace (2 B M N floats, N
    rounded up to 64, + min(B, 32) M^2 doubles) lives only for the call."""
    _single_output(Z)
    return _variational_cov_grad(X, Z, Linv, vstd, hyper, state, gcov)


def variational_cov_grad_batched(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vstd: torch.Tensor,
                                 hyper: torch.Tensor, state: torch.Tensor, gcov: torch.Tensor):
    """``variational_cov_grad`` for O outputs, every launch once
    (gpk_variational_cov_grad_batched_f32): arguments as ``variational_cov_batched`` plus its
    workspace ``state`` and gcov (O, B, N, N) -> (dX (O, B, N, D) per output, also with shared
    inputs: the caller sums over O; dLinv (O, M, M) float64, dZ (O, M, D), dpar (O, M + 1 + D)).
    Bit-identical to O single-output calls."""
    _multi_output(Z)
    return _variational_cov_grad(X, Z, Linv, vstd, hyper, state, gcov)


MVN_ROOT_MAX_N = 256   # gpk_mvn_root_max_n(): the matrix lives in one workgroup's LDS


def mvn_root(cov: torch.Tensor, jitter: float = 0.0, mean: Optional[torch.Tensor] = None,
             eps: Optional[torch.Tensor] = None, want_R: bool = True):
    """Lower Cholesky factor R of cov + jitter I for a batch (B, n, n) of dense covariances and,
    with ``mean`` (B, n) and ``eps`` (S, B, n), the draws mean + R eps, in ONE gfx950 launch
    (include/gpk.h::gpk_mvn_root_f32; n <= 256). Returns (R or None, samples (S, B, n) or None,
    info (B,) int32); info[b] > 0: matrix b is not positive definite at this jitter, R[b] and
    its samples must not be read. One rung of psd_safe_cholesky's ladder: the caller retries the
    whole batch. Memory per call: only the outputs (B * n^2 floats of R when asked, S * B * n of
    samples); the matrix is factored in LDS."""
    if cov.dim() != 3 or cov.shape[-1] != cov.shape[-2]:
        raise ValueError(f"cov must be (B, n, n), got {tuple(cov.shape)}")
    B, n, _ = cov.shape
    if not 1 <= n <= MVN_ROOT_MAX_N:
        raise ValueError(f"gpk_mvn_root_f32 takes 1 <= n <= {MVN_ROOT_MAX_N}, got n = {n}")
    if (mean is None) != (eps is None):
        raise ValueError("mean and eps are given together")
    _require_device(cov)
    dev = cov.device
    cov = cov.detach().contiguous().float()
    S = 0
    samples = None
    if eps is not None:
        _require_device(mean, eps)
        if eps.dim() != 3 or tuple(eps.shape[1:]) != (B, n) or tuple(mean.shape) != (B, n):
            raise ValueError(f"mean must be (B, n) = {(B, n)} and eps (S, B, n); got {tuple(mean.shape)}, "
                             f"{tuple(eps.shape)}")
        S = eps.shape[0]
        mean = mean.detach().contiguous().float()
        eps = eps.detach().contiguous().float()
        samples = torch.empty(S, B, n, device=dev, dtype=torch.float32)
    R = torch.empty(B, n, n, device=dev, dtype=torch.float32) if want_R else None
    info = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0:
        return R, samples, info
    rc = _native.lib().gpk_mvn_root_f32(
        cov.data_ptr(), mean.data_ptr() if S > 0 else None, eps.data_ptr() if S > 0 else None, B, n, S,
        float(jitter), R.data_ptr() if R is not None else None,
        samples.data_ptr() if S > 0 else None, info.data_ptr(), _stream_ptr(dev))
    _native.check(rc, "gpk_mvn_root_f32")
    return R, samples, info


def tri_solve(R: torch.Tensor, d: torch.Tensor, trans: bool = False) -> torch.Tensor:
    """w with R w = d (or R^T w = d when ``trans``) for lower-triangular R (B, n, n) and d (B, n):
    one gfx950 launch (include/gpk.h::gpk_tri_solve_f32), 1 <= n <= 256."""
    if R.dim() != 3 or R.shape[-1] != R.shape[-2]:
        raise ValueError(f"R must be (B, n, n), got {tuple(R.shape)}")
    B, n, _ = R.shape
    if tuple(d.shape) != (B, n):
        raise ValueError(f"d must be (B, n) = {(B, n)}, got {tuple(d.shape)}")
    if not 1 <= n <= MVN_ROOT_MAX_N:
        raise ValueError(f"gpk_tri_solve_f32 takes 1 <= n <= {MVN_ROOT_MAX_N}, got n={n}")
    _require_device(R, d)
    R = R.detach().contiguous().float()
    d = d.detach().contiguous().float()
    w = torch.empty(B, n, device=R.device, dtype=torch.float32)
    rc = _native.lib().gpk_tri_solve_f32(R.data_ptr(), d.data_ptr(), B, n, int(bool(trans)), w.data_ptr(),
                                         _stream_ptr(R.device))
    _native.check(rc, "gpk_tri_solve_f32")
    return w


def mvn_root_refine(cov: torch.Tensor, jitter: float, R: torch.Tensor) -> torch.Tensor:
    """One refinement step of the fp32 root R of cov + jitter I with an fp64 residual
    (include/gpk.h::gpk_mvn_root_refine_f32): (B, n, n) -> (B, n, n), for the adjoint of a
    near-singular covariance. Memory per call: the workspace (B * T (T + 1) KiB) + the output."""
    if cov.dim() != 3 or cov.shape[-1] != cov.shape[-2] or cov.shape != R.shape:
        raise ValueError(f"cov and R must be (B, n, n), got {tuple(cov.shape)}, {tuple(R.shape)}")
    B, n, _ = cov.shape
    if not 1 <= n <= MVN_ROOT_MAX_N:
        raise ValueError(f"gpk_mvn_root_refine_f32 takes 1 <= n <= {MVN_ROOT_MAX_N}, got n = {n}")
    _require_device(cov, R)
    dev = cov.device
    cov = cov.detach().contiguous().float()
    R = R.detach().contiguous().float()
    out = torch.empty_like(R)
    if B == 0:
        return out
    lib = _native.lib()
    ws = torch.empty(max(1, lib.gpk_mvn_root_refine_workspace_bytes(B, n) // 4), device=dev, dtype=torch.float32)
    rc = lib.gpk_mvn_root_refine_f32(cov.data_ptr(), R.data_ptr(), B, n, float(jitter), ws.data_ptr(),
                                     out.data_ptr(), _stream_ptr(dev))
    _native.check(rc, "gpk_mvn_root_refine_f32")
    return out


def mvn_root_grad(R: torch.Tensor, gR: Optional[torch.Tensor] = None, gsamples: Optional[torch.Tensor] = None,
                  eps: Optional[torch.Tensor] = None, want_dmean: bool = True):
    """Adjoint of ``mvn_root`` in ONE gfx950 launch (include/gpk.h::gpk_mvn_root_grad_f32): from
    the forward's factor R (B, n, n), the gradient gR (B, n, n; lower triangle read) of R and / or
    the gradient gsamples (S, B, n) of the draws made with eps (S, B, n), returns (dcov (B, n, n)
    symmetric, dmean (B, n) or None). gR None and no gsamples gives zeros. Memory per call: the
    workspace (B * T (T + 1) / 2 KiB, T = ceil(n / 16)) + the outputs."""
    if R.dim() != 3 or R.shape[-1] != R.shape[-2]:
        raise ValueError(f"R must be (B, n, n), got {tuple(R.shape)}")
    B, n, _ = R.shape
    if not 1 <= n <= MVN_ROOT_MAX_N:
        raise ValueError(f"gpk_mvn_root_grad_f32 takes 1 <= n <= {MVN_ROOT_MAX_N}, got n = {n}")
    if (gsamples is None) != (eps is None):
        raise ValueError("gsamples and eps are given together")
    _require_device(R)
    dev = R.device
    R = R.detach().contiguous().float()
    if gR is not None:
        _require_device(gR)
        if tuple(gR.shape) != (B, n, n):
            raise ValueError(f"gR must be (B, n, n) = {(B, n, n)}, got {tuple(gR.shape)}")
        gR = gR.detach().contiguous().float()
    S = 0
    if gsamples is not None:
        _require_device(gsamples, eps)
        if gsamples.dim() != 3 or tuple(gsamples.shape[1:]) != (B, n) or gsamples.shape != eps.shape:
            raise ValueError(f"gsamples and eps must be (S, B, n) with (B, n) = {(B, n)}; got "
                             f"{tuple(gsamples.shape)}, {tuple(eps.shape)}")
        S = gsamples.shape[0]
        gsamples = gsamples.detach().contiguous().float()
        eps = eps.detach().contiguous().float()
    dcov = torch.empty(B, n, n, device=dev, dtype=torch.float32)
    dmean = torch.empty(B, n, device=dev, dtype=torch.float32) if want_dmean else None
    if B == 0:
        return dcov, dmean
    lib = _native.lib()
    nbytes = lib.gpk_mvn_root_grad_workspace_bytes(B, n)
    ws = torch.empty(max(1, nbytes // 4), device=dev, dtype=torch.float32)
    rc = lib.gpk_mvn_root_grad_f32(
        R.data_ptr(), gR.data_ptr() if gR is not None else None, gsamples.data_ptr() if S > 0 else None,
        eps.data_ptr() if S > 0 else None, B, n, S, ws.data_ptr(), dcov.data_ptr(),
        dmean.data_ptr() if dmean is not None else None, _stream_ptr(dev))
    _native.check(rc, "gpk_mvn_root_grad_f32")
    return dcov, dmean


# ---------------------------------------------------------------------------
# ELBO terms (gpk_gauss_ell_f32 / gpk_meanfield_kl_f32)
# ---------------------------------------------------------------------------
def gauss_ell(y: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """Per-row sum of GaussianLikelihood.expected_log_prob for (R, N) rows (one launch)."""
    R, N = mean.shape
    _require_device(y, mean, var, noise)
    dev = mean.device
    ell = torch.empty(R, device=dev, dtype=torch.float32)
    rc = _native.lib().gpk_gauss_ell_f32(y.data_ptr(), mean.data_ptr(), var.data_ptr(), noise.data_ptr(),
                                         R, N, ell.data_ptr(), _stream_ptr(dev))
    _native.check(rc, "gpk_gauss_ell_f32")
    return ell


def gauss_ell_grad(y, mean, var, noise, gell):
    """(dy, dmean, dvar, dnoise (1,)) of sum_r gell_r ell_r (one launch + one sum)."""
    R, N = mean.shape
    _require_device(y, mean, var, noise, gell)
    dev = mean.device
    dy = torch.empty(R, N, device=dev, dtype=torch.float32)
    dmean = torch.empty(R, N, device=dev, dtype=torch.float32)
    dvar = torch.empty(R, N, device=dev, dtype=torch.float32)
    part = torch.empty(R, device=dev, dtype=torch.float32)
    rc = _native.lib().gpk_gauss_ell_grad_f32(y.data_ptr(), mean.data_ptr(), var.data_ptr(), noise.data_ptr(),
                                              gell.data_ptr(), R, N, dy.data_ptr(), dmean.data_ptr(),
                                              dvar.data_ptr(), part.data_ptr(), _stream_ptr(dev))
    _native.check(rc, "gpk_gauss_ell_grad_f32")
    return dy, dmean, dvar, part.sum().reshape(1)


def meanfield_kl(m: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """KL(N(m, diag s^2) || N(0, I)) as a (1,) tensor (one launch)."""
    _require_device(m, s)
    kl = torch.empty(1, device=m.device, dtype=torch.float32)
    rc = _native.lib().gpk_meanfield_kl_f32(m.data_ptr(), s.data_ptr(), m.numel(), kl.data_ptr(), None,
                                            None, None, _stream_ptr(m.device))
    _native.check(rc, "gpk_meanfield_kl_f32")
    return kl


def meanfield_kl_grad(m, s, gkl):
    _require_device(m, s, gkl)
    dm = torch.empty_like(m)
    ds = torch.empty_like(s)
    rc = _native.lib().gpk_meanfield_kl_f32(m.data_ptr(), s.data_ptr(), m.numel(), None, gkl.data_ptr(),
                                            dm.data_ptr(), ds.data_ptr(), _stream_ptr(m.device))
    _native.check(rc, "gpk_meanfield_kl_f32")
    return dm, ds


def _rows(t: torch.Tensor):
    """(tensor, leading dimension) of a (R, N) float32 view with unit column stride."""
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32:
        t = t.contiguous().float()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def variational_elbo(y, mean, var, noise, vmean, vstd, kl_scale: float, min_var: float):
    """(elbo (R,), clamp flag (1,) int32) of include/gpk.h::gpk_variational_elbo_f32."""
    _require_device(y, mean, var, noise, vmean, vstd)
    R, N = mean.shape
    y, ldy = _rows(y)
    mean, ldm = _rows(mean)
    var, ldv = _rows(var)
    dev = mean.device
    elbo = torch.empty(R, device=dev, dtype=torch.float32)
    flag = torch.empty(1, device=dev, dtype=torch.int32)
    m = vmean.detach().reshape(-1).contiguous().float()
    s = vstd.detach().reshape(-1).contiguous().float()
    rc = _native.lib().gpk_variational_elbo_f32(y.data_ptr(), ldy, mean.data_ptr(), ldm, var.data_ptr(), ldv,
                                                noise.data_ptr(), m.data_ptr(), s.data_ptr(), m.numel(), R, N,
                                                float(kl_scale), float(min_var), elbo.data_ptr(), flag.data_ptr(),
                                                _stream_ptr(dev))
    _native.check(rc, "gpk_variational_elbo_f32")
    return elbo, flag


def variational_elbo_grad(y, mean, var, noise, vmean, vstd, kl_scale: float, gelbo):
    """(dmean, dvar, dnoise (1,), dvmean, dvstd) for the objective sum_r gelbo_r elbo_r."""
    R, N = mean.shape
    y, ldy = _rows(y)
    mean, ldm = _rows(mean)
    var, ldv = _rows(var)
    dev = mean.device
    m = vmean.detach().reshape(-1).contiguous().float()
    s = vstd.detach().reshape(-1).contiguous().float()
    dmean = torch.empty(R, N, device=dev, dtype=torch.float32)
    dvar = torch.empty(R, N, device=dev, dtype=torch.float32)
    part = torch.empty(R, device=dev, dtype=torch.float32)
    dm = torch.empty_like(m)
    ds = torch.empty_like(s)
    g = gelbo.reshape(-1).contiguous().float()
    rc = _native.lib().gpk_variational_elbo_grad_f32(y.data_ptr(), ldy, mean.data_ptr(), ldm, var.data_ptr(),
                                                     ldv, noise.data_ptr(), m.data_ptr(), s.data_ptr(), m.numel(),
                                                     R, N, float(kl_scale), g.data_ptr(), dmean.data_ptr(),
                                                     dvar.data_ptr(), part.data_ptr(), dm.data_ptr(),
                                                     ds.data_ptr(), _stream_ptr(dev))
    _native.check(rc, "gpk_variational_elbo_grad_f32")
    return dmean, dvar, part.sum().reshape(1), dm, ds


# ---------------------------------------------------------------------------
# Cholesky (full-covariance) q(u): gpk_variational_chol_f32 / _adjoint_f32, gpk_cholesky_kl_f32 and
# their batched forms (the output index on grid y of every launch); the same convention as above
# ---------------------------------------------------------------------------
def variational_chol_supported(B: int, N: int, M: int, D: int, adjoint: bool = False) -> bool:
    """Whether the Cholesky-q(u) kernels serve the shape (the *_bytes queries of include/gpk.h:
    forward M <= 256, D <= 64; the adjoint additionally N <= 256)."""
    if B < 1:
        return False
    lib = _native.lib()
    if adjoint:
        return lib.gpk_variational_chol_adjoint_workspace_bytes(B, N, M, D) > 0
    return lib.gpk_variational_chol_saved_bytes(B, N, M, D) > 0


def variational_chol_batched_supported(O: int, B: int, N: int, M: int, D: int, adjoint: bool = False) -> bool:
    """Whether the batched Cholesky-q(u) kernels serve the shape (the two batched *_bytes
    queries: 1 <= O <= 65535 and the single-output bounds)."""
    if B < 1:
        return False
    lib = _native.lib()
    if adjoint:
        return lib.gpk_variational_chol_adjoint_batched_workspace_bytes(O, B, N, M, D) > 0
    return lib.gpk_variational_chol_batched_saved_bytes(O, B, N, M, D) > 0


@dataclass
class VariationalCholOut:
    mean: torch.Tensor             # (B, N); (O, B, N) for O outputs
    var: torch.Tensor              # as mean, clamped at 1e-6
    flags: Optional[torch.Tensor]  # (1,) int32: bit 0 = the variance clamp fired
    saved: Optional[torch.Tensor]  # A = Linv K_ZX (B, M, as) and the clamp mask (B, as) per output, or None


def _chol_saved_bytes(lib, O, B, N, M, D) -> int:
    if O is None:
        return lib.gpk_variational_chol_saved_bytes(B, N, M, D)
    return lib.gpk_variational_chol_batched_saved_bytes(O, B, N, M, D)


def _variational_chol_forward(X, Z, Linv, vmean, vchol, hyper, want_flags, save) -> VariationalCholOut:
    _require_device(X, Z, Linv, vmean, vchol, hyper)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper)
    dev = X.device
    vmean = _per_output(vmean, *lead, M)
    vchol = _vchol_arg(vchol, lead, M)
    mean = torch.empty(*lead, B, N, device=dev, dtype=torch.float32)
    var = torch.empty(*lead, B, N, device=dev, dtype=torch.float32)
    flags = torch.zeros(1, device=dev, dtype=torch.int32) if want_flags else None
    lib = _native.lib()
    name = "gpk_variational_chol_f32" if O is None else "gpk_variational_chol_batched_f32"
    saved = None
    if B > 0:
        nsaved = _chol_saved_bytes(lib, O, B, N, M, D)
        if nsaved == 0:
            raise ValueError(f"{name} does not support O={O}, B={B}, N={N}, M={M}, D={D}")
        if save:
            saved = torch.empty(nsaved // 4, device=dev, dtype=torch.float32)
    x, dims = _abi(X, shared, O, B, N, M, D)
    rc = getattr(lib, name)(*x, Z.data_ptr(), Linv.data_ptr(), vmean.data_ptr(), vchol.data_ptr(),
                            hyper.data_ptr(), *dims, mean.data_ptr(), var.data_ptr(), _ptr(flags), _ptr(saved),
                            _stream_ptr(dev))
    _native.check(rc, name)
    return VariationalCholOut(mean, var, flags, saved)


def variational_chol_forward(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vmean: torch.Tensor,
                             vchol: torch.Tensor, hyper: torch.Tensor, want_flags: bool = True,
                             save: bool = False) -> VariationalCholOut:
    """Batched q(f) mean / variance of the whitened VariationalStrategy with a Cholesky q(u)
    (include/gpk.h::gpk_variational_chol_f32); ``hyper`` is pack_variational_hyper's vector.
    ``save=True`` keeps A and the clamp mask for ``variational_chol_adjoint``."""
    _single_output(Z)
    return _variational_chol_forward(X, Z, Linv, vmean, vchol, hyper, want_flags, save)


def variational_chol_forward_batched(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vmean: torch.Tensor,
                                     vchol: torch.Tensor, hyper: torch.Tensor, want_flags: bool = True,
                                     save: bool = False) -> VariationalCholOut:
    """``variational_chol_forward`` for O outputs in one launch (gpk_variational_chol_batched_f32):
    X (B, N, D) shared by every output or (O, B, N, D), Z (O, M, D), Linv (O, M, M) float64, vmean
    (O, M), vchol (O, M, M), hyper (O, 4 + 2D) -> mean, var (O, B, N), one clamp flag word for all
    outputs and, with ``save``, the O states. Bit-identical to O single-output calls."""
    _multi_output(Z)
    return _variational_chol_forward(X, Z, Linv, vmean, vchol, hyper, want_flags, save)


def _variational_chol_adjoint(X, Z, Linv, vmean, vchol, hyper, gmean, gvar, saved):
    _require_device(X, Z, Linv, vmean, vchol, hyper, gmean, gvar, saved)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper, cast_linv=True)
    dev = X.device
    lib = _native.lib()
    if saved.dtype != torch.float32 or saved.device != dev:
        raise ValueError(f"saved state must be float32 on {dev} (got {saved.dtype} on {saved.device})")
    if saved.numel() * 4 != _chol_saved_bytes(lib, O, B, N, M, D):
        raise ValueError("saved state does not match this shape (the forward's, with save=True)")
    if O is None:
        name = "gpk_variational_chol_adjoint_f32"
        nbytes = lib.gpk_variational_chol_adjoint_workspace_bytes(B, N, M, D)
    else:
        name = "gpk_variational_chol_adjoint_batched_f32"
        nbytes = lib.gpk_variational_chol_adjoint_batched_workspace_bytes(O, B, N, M, D)
    if nbytes == 0:
        raise ValueError(f"{name} does not support O={O}, B={B}, N={N}, M={M}, D={D}")
    vmean = _per_output(vmean, *lead, M)
    vchol = _vchol_arg(vchol, lead, M)
    gmean = _per_output(gmean, *lead, B, N)
    gvar = _per_output(gvar, *lead, B, N)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dX = torch.empty(*lead, B, N, D, device=dev, dtype=torch.float32)
    dLinv = torch.empty(*lead, M, M, device=dev, dtype=torch.float64)
    dZ = torch.empty(*lead, M, D, device=dev, dtype=torch.float32)
    dpar = torch.empty(*lead, M + 2 * D + 2, device=dev, dtype=torch.float32)
    dchol = torch.empty(*lead, M, M, device=dev, dtype=torch.float32)
    x, dims = _abi(X, shared, O, B, N, M, D)
    rc = getattr(lib, name)(*x, Z.data_ptr(), Linv.data_ptr(), vmean.data_ptr(), vchol.data_ptr(),
                            hyper.data_ptr(), gmean.data_ptr(), gvar.data_ptr(),
                            saved.detach().contiguous().data_ptr(), *dims, ws.data_ptr(), dX.data_ptr(),
                            dLinv.data_ptr(), dZ.data_ptr(), dpar.data_ptr(), dchol.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return dX, dLinv, dZ, dpar, dchol


def variational_chol_adjoint(X, Z, Linv, vmean, vchol, hyper, gmean, gvar, saved):
    """Adjoint of ``variational_chol_forward`` except the shared K_ZZ factor
    (include/gpk.h::gpk_variational_chol_adjoint_f32) -> (dX (B, N, D), dLinv (M, M) float64 lower,
    dZ (M, D), dpar (M + 2D + 2) = [dvmean, ds2, dls, dw, db0], dchol (M, M) lower)."""
    _single_output(Z)
    return _variational_chol_adjoint(X, Z, Linv, vmean, vchol, hyper, gmean, gvar, saved)


def variational_chol_adjoint_batched(X, Z, Linv, vmean, vchol, hyper, gmean, gvar, saved):
    """``variational_chol_adjoint`` for O outputs, every launch once
    (gpk_variational_chol_adjoint_batched_f32) -> (dX (O, B, N, D) per output also with shared
    inputs, dLinv (O, M, M) float64 lower, dZ (O, M, D), dpar (O, M + 2D + 2), dchol (O, M, M))."""
    _multi_output(Z)
    return _variational_chol_adjoint(X, Z, Linv, vmean, vchol, hyper, gmean, gvar, saved)


def _cholesky_kl(m, chol, gkl=None):
    """The KL (gkl None) or its gradient (dm, dchol) for m (M,), chol (M, M), or with a leading O."""
    lead, M = tuple(m.shape[:-1]), m.shape[-1]
    dev = m.device
    if gkl is None:
        kl = torch.empty(lead or (1,), device=dev, dtype=torch.float32)
        outs = (kl.data_ptr(), None, None, None)
    else:
        dm, dchol = torch.empty_like(m), torch.empty_like(chol)
        outs = (None, gkl.data_ptr(), dm.data_ptr(), dchol.data_ptr())
    name = "gpk_cholesky_kl_batched_f32" if lead else "gpk_cholesky_kl_f32"
    rc = getattr(_native.lib(), name)(m.data_ptr(), chol.data_ptr(), *lead, M, *outs, _stream_ptr(dev))
    _native.check(rc, name)
    return kl if gkl is None else (dm, dchol)


def _kl_single(m: torch.Tensor) -> None:
    if m.dim() != 1:
        raise ValueError(f"m must be (M,), got {tuple(m.shape)}")


def cholesky_kl(m: torch.Tensor, chol: torch.Tensor) -> torch.Tensor:
    """KL(N(m, L L^T) || N(0, I)), L = tril(chol), as a (1,) tensor (one launch)."""
    _require_device(m, chol)
    _kl_single(m)
    return _cholesky_kl(m, chol)


def cholesky_kl_grad(m, chol, gkl):
    _require_device(m, chol, gkl)
    _kl_single(m)
    return _cholesky_kl(m, chol, gkl)


def _kl_batched_args(m, chol):
    if m.dim() != 2 or tuple(chol.shape) != (m.shape[0], m.shape[1], m.shape[1]):
        raise ValueError(f"m must be (O, M) and chol (O, M, M), got {tuple(m.shape)} and {tuple(chol.shape)}")
    return m.detach().contiguous().float(), chol.detach().contiguous().float()


def cholesky_kl_batched(m: torch.Tensor, chol: torch.Tensor) -> torch.Tensor:
    """KL(N(m_o, L_o L_o^T) || N(0, I)), L_o = tril(chol_o), per output as an (O,) tensor (one launch)."""
    _require_device(m, chol)
    return _cholesky_kl(*_kl_batched_args(m, chol))


def cholesky_kl_grad_batched(m, chol, gkl):
    _require_device(m, chol, gkl)
    m, chol = _kl_batched_args(m, chol)
    return _cholesky_kl(m, chol, gkl.detach().reshape(m.shape[0]).contiguous().float())


# ---------------------------------------------------------------------------
# Dense covariance of q(f) for a Cholesky q(u): gpk_variational_chol_cov_f32 / _grad_f32 and their
# batched forms (Z (M, D): one output; Z (O, M, D): O outputs on one launch chain)
# ---------------------------------------------------------------------------
def variational_chol_cov(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vchol: torch.Tensor,
                         hyper: torch.Tensor, return_state: bool = False):
    """Dense covariance of q(f) with a Cholesky q(u): K_XX + jitter I + W^T W - A^T A, A = Linv K_ZX,
    W = tril(vchol)^T A (two gfx950 launches, include/gpk.h::gpk_variational_chol_cov_f32). Z (M, D):
    X (B, N, D) -> cov (B, N, N). Z (O, M, D): X (B, N, D) shared or (O, B, N, D), every other array
    with a leading O -> cov (O, B, N, N), output o bit-identical to a single-output call.
    ``return_state``: -> (cov, workspace), the stacked [W; A] panels and window means that
    ``variational_chol_cov_grad`` runs from (2 B M N floats, N rounded up to 64, per output)."""
    _require_device(X, Z, Linv, vchol, hyper)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper)
    dev = X.device
    vchol = _vchol_arg(vchol, lead, M)
    lib = _native.lib()
    if O is None:
        name = "gpk_variational_chol_cov_f32"
        nbytes = lib.gpk_variational_chol_cov_workspace_bytes(B, N, M)
    else:
        name = "gpk_variational_chol_cov_batched_f32"
        nbytes = lib.gpk_variational_chol_cov_batched_workspace_bytes(O, B, N, M)
    if (nbytes == 0 and B > 0) or D > 64:
        raise ValueError(f"{name} does not support O={O}, B={B}, N={N}, M={M}, D={D}")
    cov = torch.empty(*lead, B, N, N, device=dev, dtype=torch.float32)
    if B == 0:
        return (cov, torch.empty(0, device=dev, dtype=torch.float32)) if return_state else cov
    ws = torch.empty(max(1, nbytes // 4), device=dev, dtype=torch.float32)
    x, dims = _abi(X, shared, O, B, N, M, D)
    rc = getattr(lib, name)(*x, Z.data_ptr(), Linv.data_ptr(), vchol.data_ptr(), hyper.data_ptr(), *dims,
                            ws.data_ptr(), cov.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return (cov, ws) if return_state else cov


def variational_chol_cov_grad(X: torch.Tensor, Z: torch.Tensor, Linv: torch.Tensor, vchol: torch.Tensor,
                              hyper: torch.Tensor, state: torch.Tensor, gcov: torch.Tensor):
    """Adjoint of ``variational_chol_cov`` (include/gpk.h::gpk_variational_chol_cov_grad_f32): from
    gcov = dObjective / dcov (any matrix per window) and the forward's workspace ``state`` ->
    (dX, dLinv float64 lower, dZ (the K_ZX part), dpar = [ds2, dlengthscale (D)], dchol lower).
    Z (O, M, D): every array with a leading O, dX (O, B, N, D) per output also with shared inputs
    (the caller sums over O). M <= 256, D <= 64, N <= 256."""
    _require_device(X, Z, Linv, vchol, hyper, state, gcov)
    X, shared, Z, Linv, hyper, lead, O, B, N, M, D = _var_args(X, Z, Linv, hyper)
    dev = X.device
    vchol = _vchol_arg(vchol, lead, M)
    if tuple(gcov.shape) != lead + (B, N, N):
        raise ValueError(f"gcov must be {lead + (B, N, N)}, got {tuple(gcov.shape)}")
    gcov = gcov.detach().contiguous().float()
    lib = _native.lib()
    if O is None:
        name = "gpk_variational_chol_cov_grad_f32"
        nbytes = lib.gpk_variational_chol_cov_grad_workspace_bytes(B, N, M, D)
        nstate = lib.gpk_variational_chol_cov_workspace_bytes(B, N, M)
    else:
        name = "gpk_variational_chol_cov_grad_batched_f32"
        nbytes = lib.gpk_variational_chol_cov_grad_batched_workspace_bytes(O, B, N, M, D)
        nstate = lib.gpk_variational_chol_cov_batched_workspace_bytes(O, B, N, M)
    if nbytes == 0 and B > 0:
        raise ValueError(f"{name} does not support O={O}, B={B}, N={N}, M={M}, D={D}")
    dX = torch.empty(*lead, B, N, D, device=dev, dtype=torch.float32)
    dLinv = torch.empty(*lead, M, M, device=dev, dtype=torch.float64)
    dZ = torch.empty(*lead, M, D, device=dev, dtype=torch.float32)
    dpar = torch.empty(*lead, 1 + D, device=dev, dtype=torch.float32)
    dchol = torch.empty(*lead, M, M, device=dev, dtype=torch.float32)
    if B == 0:
        return dX, dLinv.zero_(), dZ.zero_(), dpar.zero_(), dchol.zero_()
    state = _cov_grad_state(state, nstate // 4, dev, "variational_chol_cov")
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    x, dims = _abi(X, shared, O, B, N, M, D)
    rc = getattr(lib, name)(*x, Z.data_ptr(), Linv.data_ptr(), vchol.data_ptr(), hyper.data_ptr(),
                            state.data_ptr(), gcov.data_ptr(), *dims, ws.data_ptr(), dX.data_ptr(),
                            dLinv.data_ptr(), dZ.data_ptr(), dpar.data_ptr(), dchol.data_ptr(), _stream_ptr(dev))
    _native.check(rc, name)
    return dX, dLinv, dZ, dpar, dchol
