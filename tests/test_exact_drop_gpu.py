"""Dropping the oldest observations from a cached exact-GP factor: gpk_exact_drop_f32 through
ops.exact_drop, gpk::exact_drop, and ExactGPModel.forget_oldest / get_sliding_model.

Reference: an fp64 NumPy Cholesky of the KEPT data (X[:, m:], y[:, m:]) with plain pairwise squared
distances, L' = chol(K + noise I), z' = L'^{-1}(y - c); each use first ties the posterior that
(L', z') give at a few probe points to oracle.exact_predict at 1e-12 relative, as
test_exact_append_gpu.py ties its factor. The pure linear-algebra test has no kernel matrix behind
it: a random lower-triangular L with a positive diagonal and a random z, against fp64
chol((L L^T)[m:, m:]) and L'^{-1}((L z)[m:]).

Tolerance: the project's 1e-4 relative, norm-wise (Frobenius) per window, over ALL of L' and of z'
(every entry of the output is recomputed, nothing is copied). An fp32 NumPy emulation of the
kernel's recurrence started from the fp64 factor reaches 7e-8 ... 2.5e-7 in L' and 1.0e-7 ...
5.8e-7 in z' at (N, m) = (40, 7), (300, 16), (2, 1), (80, 64), the size of an fp32 refit's own error.
Measured on an MI355X (factors from ops.exact_mll, so the fp32 factorisation's error is included):
see MEASURED below.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
LN2 = math.log(2.0)
NOISE = LN2 + 1e-4

# Measured maxima on an MI355X (relative Frobenius error per window, the largest over the windows):
MEASURED = """
parity (B, N, m), L' / z' against the fp64 factor of the kept data:
  (3, 2, 1) 6.5e-8 / 8.0e-8      (3, 17, 1) 1.0e-7 / 1.8e-7     (2, 40, 7) 1.3e-7 / 1.7e-7
  (2, 33, 17) 1.0e-7 / 2.5e-7    (2, 80, 64) 1.5e-7 / 3.4e-7    (2, 273, 17) 3.1e-7 / 4.5e-7
  (2, 300, 16) 3.1e-7 / 4.3e-7   (2, 321, 1) 5.4e-7 / 6.7e-7    (2, 800, 16) 4.9e-7 / 6.8e-7
  (300, 40, 3) 2.3e-7 / 3.6e-7
pure linear algebra: (3, 70, 9) 6.7e-8 / 1.4e-7, (2, 330, 40) 1.4e-7 / 3.3e-7
slide (drop 16, append 16 at N = 300): 3.2e-7 / 4.5e-7
consumers on the dropped factor: mean 2.9e-6, variance 5.3e-7, Sigma 2.8e-6 (n = 256);
  2.3e-6, 3.7e-7, 2.4e-6 (n = 284)
models against a fresh fit of the same data (mean / variance / Sigma): forget 16 at N = 300
  4.0e-6 / 1.4e-5 / 3.4e-5 at the worst of the three input layouts; three slides of 16 at N = 300
  3.9e-6 / 2.8e-6 / 1.3e-5; three slides of 8 at N = 800 4.4e-6 / 1.3e-5 / 4.5e-5
window model against fp64: mean <= 4.3e-6, variance <= 4.9e-6
"""


def _rel(a, b):
    a = np.asarray(a, np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, np.float64).reshape(b.shape[0], -1)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _sqdist(A, Bm, ls):
    d = (A[:, None, :] - Bm[None, :, :]) / np.asarray(ls, np.float64)
    return (d * d).sum(-1)


def _posterior_fp64(X, L, z, Xs, ls, s2, c):
    """(mean, cov) of the latent posterior at Xs from one window's fp64 factor."""
    V = np.linalg.solve(L, s2 * np.exp(-0.5 * _sqdist(X, Xs, ls)))
    return c + V.T @ z, s2 * np.exp(-0.5 * _sqdist(Xs, Xs, ls)) - V.T @ V


def _factor_fp64(X, y, ls=LN2, s2=LN2, c=0.3, noise=NOISE):
    """fp64 (L, z) of the data, window by window, tied to oracle.exact_predict through the posterior
    they give at probe points."""
    X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
    B, N, _ = X.shape
    L, z = np.empty((B, N, N)), np.empty((B, N))
    for b in range(B):
        L[b] = np.linalg.cholesky(s2 * np.exp(-0.5 * _sqdist(X[b], X[b], ls)) + noise * np.eye(N))
        z[b] = np.linalg.solve(L[b], y[b] - c)
        probe = X[b, :4] + 0.1
        pm, pc = _posterior_fp64(X[b], L[b], z[b], probe, ls, s2, c)
        rm, rv = O.exact_predict(X[b:b + 1], y[b:b + 1], probe[None], ls, s2, c, noise)
        assert _rel(pm[None], rm).max() <= 1e-12
        assert _rel(np.diagonal(pc)[None], rv).max() <= 1e-12
    return L, z


@functools.lru_cache(maxsize=None)
def _case(B, N, m, D, extra=0):
    """Seeded data (N points and `extra` later ones per window) and the fp64 factor of the points
    [m, N + extra). Cached: the tests share it and leave it unchanged."""
    g = torch.Generator().manual_seed(1000 * N + 10 * m + D)
    X = torch.randn(B, N + extra, D, generator=g) / math.sqrt(D)
    y = torch.randn(B, N + extra, generator=g)
    Lr, zr = _factor_fp64(X[:, m:].numpy(), y[:, m:].numpy())
    return X, y, Lr, zr


def _hyper(dev):
    from fine_grained_gaussian_process_forcasting_amd import ops
    return ops.pack_exact_hyper(LN2, NOISE, 0.3, torch.as_tensor(LN2, dtype=torch.float32), dev)


def _fit(dev, X, y, hyper):
    from fine_grained_gaussian_process_forcasting_amd import ops
    f = ops.exact_mll(X.to(dev).contiguous(), y.to(dev).contiguous(), None, None, None, None, want_L=True,
                      want_z=True, hyper=hyper)
    assert int(f.info.abs().max()) == 0
    return f.L, f.z


def _assert_close(L2, z2, Lr, zr, what):
    eL, ez = _rel(L2.cpu().numpy(), Lr), _rel(z2.cpu().numpy(), zr)
    print(f"{what}: L' {eL.max():.2e}, z' {ez.max():.2e}")
    assert eL.max() <= 1e-4 and ez.max() <= 1e-4


def _assert_layout(L2, z2, B, n):
    assert L2.shape == (B, n, n) and z2.shape == (B, n)
    assert L2.dtype == torch.float32 and z2.dtype == torch.float32
    assert L2.is_contiguous() and z2.is_contiguous()
    assert int(torch.count_nonzero(torch.triu(L2, diagonal=1))) == 0      # exactly zero, -0.0 included
    assert not bool(torch.signbit(torch.triu(L2, diagonal=1)).any())
    assert bool((torch.diagonal(L2, dim1=-2, dim2=-1) > 0).all())


SHAPES = [(3, 2, 1, 1),        # n = 1
          (3, 17, 1, 2),
          (2, 40, 7, 3),
          (2, 33, 17, 4),      # m past 16
          (2, 80, 64, 8),      # the largest m: two passes
          (2, 273, 17, 5),     # n = 256 exactly
          (2, 300, 16, 6),     # a blocked-path factor; n not a multiple of 16
          (2, 321, 1, 1),
          (2, 800, 16, 8),     # the largest N
          (300, 40, 3, 2)]     # more windows than CUs


@pytest.mark.parametrize("B,N,m,D", SHAPES)
def test_drop_parity(cuda_device, B, N, m, D):
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    X, y, Lr, zr = _case(B, N, m, D)
    L, z = _fit(dev, X, y, _hyper(dev))
    L0, z0 = L.clone(), z.clone()
    L2, z2 = ops.exact_drop(L, z, m)
    L3, z3 = ops.exact_drop(L, z, m)
    _assert_layout(L2, z2, B, N - m)
    _assert_close(L2, z2, Lr, zr, f"(B={B}, N={N}, m={m})")
    assert torch.equal(L2, L3) and torch.equal(z2, z3)          # a second call: the same bits
    assert torch.equal(L, L0) and torch.equal(z, z0)            # the inputs are only read


@pytest.mark.parametrize("B,N,m", [(3, 70, 9), (2, 330, 40)])
def test_drop_is_pure_linear_algebra(cuda_device, B, N, m):
    """Any lower-triangular factor with a positive diagonal, e.g. one that carries ladder jitter: no
    kernel matrix, inputs or hyper-parameters behind it. The upper triangle of the input is not read."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    g = torch.Generator().manual_seed(N + m)
    L = torch.tril(torch.randn(B, N, N, generator=g, dtype=torch.float64), -1) / math.sqrt(N)
    L = L + torch.diag_embed(1.0 + torch.rand(B, N, generator=g, dtype=torch.float64))
    L, z = L.float(), torch.randn(B, N, generator=g)
    Ln, zn = L.double().numpy(), z.double().numpy()
    K = Ln @ Ln.transpose(0, 2, 1)
    Lr = np.linalg.cholesky(K[:, m:, m:])
    rhs = np.einsum("bij,bj->bi", Ln, zn)[:, m:]
    zr = np.stack([np.linalg.solve(Lr[b], rhs[b]) for b in range(B)])
    L2, z2 = ops.exact_drop(L.to(dev), z.to(dev), m)
    _assert_layout(L2, z2, B, N - m)
    _assert_close(L2, z2, Lr, zr, f"random factor (B={B}, N={N}, m={m})")
    junk = L + torch.triu(torch.full((N, N), float("nan")), diagonal=1)
    L3, z3 = ops.exact_drop(junk.to(dev), z.to(dev), m)
    assert torch.equal(L3, L2) and torch.equal(z3, z2)


@pytest.mark.parametrize("B,N,m,D", [(4, 40, 7, 3), (3, 300, 16, 6), (3, 80, 64, 8)])
def test_windows_are_independent(cuda_device, B, N, m, D):
    """A permutation of the windows permutes the outputs bitwise; a NaN in one window's factor stays
    in that window, and the others are bit-identical to the clean call."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    g = torch.Generator().manual_seed(5)
    X = torch.randn(B, N, D, generator=g) / math.sqrt(D)
    y = torch.randn(B, N, generator=g)
    L, z = _fit(dev, X, y, _hyper(dev))
    L2, z2 = ops.exact_drop(L, z, m)
    perm = torch.tensor([2, 0, 3, 1][:B] if B == 4 else [2, 0, 1], device=dev)
    Lp, zp = ops.exact_drop(L[perm].contiguous(), z[perm].contiguous(), m)
    assert torch.equal(Lp, L2[perm]) and torch.equal(zp, z2[perm])
    L1, z1 = ops.exact_drop(L[1:2].contiguous(), z[1:2].contiguous(), m)      # ... and whatever B is
    assert torch.equal(L1, L2[1:2]) and torch.equal(z1, z2[1:2])
    bad = L.clone()
    bad[1, m + 3, 2] = float("nan")
    Lb, zb = ops.exact_drop(bad, z, m)
    assert bool(torch.isnan(Lb[1]).any()) and bool(torch.isnan(zb[1]).any())
    for b in range(B):
        if b != 1:
            assert torch.equal(Lb[b], L2[b]) and torch.equal(zb[b], z2[b])


def test_drop_argument_errors(cuda_device):
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    L, z = torch.eye(70, device=dev).expand(2, 70, 70).contiguous(), torch.zeros(2, 70, device=dev)
    for m in (0, -1, 65, 70, 71):
        with pytest.raises(ValueError, match="m must be in 1"):
            ops.exact_drop(L, z, m)
    with pytest.raises(ValueError, match="m must be in 1"):
        ops.exact_drop(L[:, :1, :1].contiguous(), z[:, :1].contiguous(), 1)
    L2, z2 = ops.exact_drop(L[:0], z[:0], 5)                                   # B = 0
    assert L2.shape == (0, 65, 65) and z2.shape == (0, 65)
    L2, z2 = ops.exact_drop(L, z, 64)                                          # the identity stays one
    assert torch.equal(L2, torch.eye(6, device=dev).expand(2, 6, 6)) and int(torch.count_nonzero(z2)) == 0


@pytest.mark.parametrize("B,N,m,D", [(2, 273, 17, 5), (2, 300, 16, 6)])
def test_consumers_accept_the_dropped_factor(cuda_device, B, N, m, D):
    """The regular (n = 256) and the blocked (n > 256) posterior read a dropped factor."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    X, y, Lr, zr = _case(B, N, m, D)
    hyper = _hyper(dev)
    L, z = _fit(dev, X, y, hyper)
    L2, z2 = ops.exact_drop(L, z, m)
    Xk = X[:, m:].to(dev).contiguous()
    g = torch.Generator().manual_seed(7)
    Xs = torch.randn(B, 33, D, generator=g) / math.sqrt(D)
    p = ops.exact_posterior(Xk, L2, z2, hyper, Xs.to(dev))
    q = ops.exact_posterior_cov(Xk, L2, z2, hyper, Xs.to(dev))
    ref = [_posterior_fp64(X[b, m:].double().numpy(), Lr[b], zr[b], Xs[b].double().numpy(), LN2, LN2, 0.3)
           for b in range(B)]
    rm, rc = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    rv = np.diagonal(rc, axis1=1, axis2=2)
    errs = {"mean": _rel(p.mean.cpu().numpy(), rm), "var": _rel(p.var.cpu().numpy(), rv),
            "cov mean": _rel(q.mean.cpu().numpy(), rm), "cov": _rel(q.cov.cpu().numpy(), rc)}
    print({k: f"{v.max():.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v.max() <= 1e-4, k


def test_slide_is_drop_then_append(cuda_device):
    """ops.exact_append on a dropped factor: the factor of X[:, m : N + m]."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    B, N, m, D = 2, 300, 16, 6
    X, y, Lr, zr = _case(B, N, m, D, extra=m)
    hyper = _hyper(dev)
    Xd, yd = X.to(dev), y.to(dev)
    L, z = _fit(dev, X[:, :N], y[:, :N], hyper)
    L2, z2 = ops.exact_drop(L, z, m)
    L3, z3, info = ops.exact_append(Xd[:, m:N].contiguous(), L2, z2, hyper, Xd[:, N:].contiguous(),
                                    yd[:, N:].contiguous())
    assert int(info.abs().max()) == 0 and L3.shape == (B, N, N)
    _assert_close(L3, z3, Lr, zr, "slide")


# ---- the model surface ------------------------------------------------------------------------

def _surface_data(dev, shape, n_new=0, seed=3):
    """train (shape), test (41 points) and n_new later observations per window."""
    g = torch.Generator().manual_seed(seed)
    one_d = len(shape) == 1
    full = shape + (1,) if one_d else shape
    f = lambda x: torch.sin(6.0 * x.sum(-1))  # noqa: E731
    train_x = torch.rand(*full, generator=g)
    test_x = torch.rand(*full[:-2], 41, full[-1], generator=g)
    new_x = torch.rand(*full[:-2], n_new, full[-1], generator=g)
    out = [train_x, f(train_x), test_x, new_x, f(new_x)]
    if one_d:
        out = [t.squeeze(-1) if i in (0, 2, 3) else t for i, t in enumerate(out)]
    return [t.to(dev) for t in out]


def _count_factorisations(monkeypatch):
    from fine_grained_gaussian_process_forcasting_amd import ops
    calls = []
    real = ops.exact_mll

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "exact_mll", counted)
    return calls


def _norm_rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _model(dev, train_x, train_y, like=None, **kw):
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    from fine_grained_gaussian_process_forcasting_amd.gp import GaussianLikelihood
    like = GaussianLikelihood().to(dev) if like is None else like
    return ExactGPModel(train_x, train_y, like, **kw).to(dev)


def _against_fresh(dev, model, got, train_x, train_y, test_x, what):
    """Mean, variance and Sigma of `got` against a fresh model with `model`'s parameters on the data."""
    fresh = _model(dev, train_x, train_y)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    r = fresh(test_x)
    errs = (_norm_rel(got.mean, r.mean), _norm_rel(got.variance, r.variance),
            _norm_rel(got.covariance_matrix, r.covariance_matrix))
    print(f"{what} against a fresh fit: mean {errs[0]:.2e} var {errs[1]:.2e} cov {errs[2]:.2e}")
    assert max(errs) <= 1e-4


@pytest.mark.parametrize("shape", [(300,), (300, 3), (3, 300, 3)])
def test_forget_oldest_updates_the_cache(cuda_device, monkeypatch, shape):
    """N = 300, m = 16: no factorisation, the new cache is the op's output bit for bit, the new data
    are contiguous copies of the kept points, and the old model is untouched."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    train_x, train_y, test_x, _, _ = _surface_data(dev, shape)
    model = _model(dev, train_x, train_y)
    model.eval()
    with torch.no_grad():
        before = model(test_x)
        b_mean, b_cov = before.mean.clone(), before.covariance_matrix.clone()
        old_cache = model._prediction_cache
        _, L, z, hyp = old_cache[1]
        calls = _count_factorisations(monkeypatch)
        fm = model.forget_oldest(16)
        assert len(calls) == 0 and fm is not model
        kept_x = train_x[:, 16:] if len(shape) == 3 else train_x[16:]
        assert fm.train_inputs[0].shape == kept_x.shape and torch.equal(fm.train_inputs[0], kept_x)
        assert torch.equal(fm.train_targets, train_y[..., 16:])
        assert fm.train_inputs[0].is_contiguous() and fm.train_targets.is_contiguous()
        assert fm.train_inputs[0].data_ptr() != kept_x.data_ptr()
        assert fm._cache_handle is not model._cache_handle and fm.likelihood is not model.likelihood
        assert all(p is not q and torch.equal(p, q) for p, q in zip(fm.parameters(), model.parameters()))
        Ld, zd = ops.exact_drop(L, z, 16)
        X2, L2, z2, hyp2 = fm._prediction_cache[1]
        assert torch.equal(L2, Ld) and torch.equal(z2, zd) and torch.equal(hyp2, hyp)
        assert X2.shape == (L.shape[0], 284, train_x.shape[-1] if len(shape) > 1 else 1)
        got = fm(test_x)
        assert got.mean.shape == b_mean.shape
        _against_fresh(dev, model, got, kept_x.contiguous(), train_y[..., 16:].contiguous(), test_x, f"forget {shape}")
        assert len(calls) == 1                               # ... the fresh model's own
        # self still predicts as before, from the same cache
        assert model._prediction_cache is old_cache and model.train_inputs[0] is train_x
        again = model(test_x)
        assert torch.equal(again.mean, b_mean) and torch.equal(again.covariance_matrix, b_cov)
        assert len(calls) == 1


def test_sliding_model_at_the_largest_n(cuda_device, monkeypatch):
    """N = 800: get_fantasy_model alone has no room; get_sliding_model slides by 8 points three
    times with no factorisation launch and predicts as a fresh fit of the last 800 points."""
    from fine_grained_gaussian_process_forcasting_amd import _native
    dev = cuda_device
    train_x, train_y, test_x, new_x, new_y = _surface_data(dev, (800, 3), n_new=24)
    model = _model(dev, train_x, train_y)
    model.eval()
    with torch.no_grad():
        model(test_x)
        calls = _count_factorisations(monkeypatch)
        with pytest.raises(_native.GpkError, match="code -6"):
            model.get_fantasy_model(new_x[:8], new_y[:8])
        sm = model
        for k in range(3):
            sm = sm.get_sliding_model(new_x[8 * k:8 * k + 8], new_y[8 * k:8 * k + 8])
            assert sm.train_inputs[0].shape == (800, 3) and sm.train_targets.shape == (800,)
            assert sm._prediction_cache[1][1].shape == (1, 800, 800)
        got = sm(test_x)
        got.covariance_matrix
        assert len(calls) == 0
        all_x, all_y = torch.cat([train_x, new_x]), torch.cat([train_y, new_y])
        assert torch.equal(sm.train_inputs[0], all_x[24:]) and torch.equal(sm.train_targets, all_y[24:])
        _against_fresh(dev, model, got, all_x[24:].contiguous(), all_y[24:].contiguous(), test_x, "three slides, N = 800")
        assert model.train_inputs[0] is train_x and model._prediction_cache[1][1].shape == (1, 800, 800)


def test_sliding_model_chain_of_windows(cuda_device, monkeypatch):
    """Three slides of 16 at N = 300 over three windows: zero factorisations, and mean, variance
    and Sigma within the bar of a fresh model on the same data."""
    dev = cuda_device
    train_x, train_y, test_x, new_x, new_y = _surface_data(dev, (3, 300, 3), n_new=48)
    model = _model(dev, train_x, train_y)
    model.eval()
    with torch.no_grad():
        model(test_x)
        calls = _count_factorisations(monkeypatch)
        sm = model
        for k in range(3):
            sm = sm.get_sliding_model(new_x[:, 16 * k:16 * k + 16], new_y[:, 16 * k:16 * k + 16])
        got = sm(test_x)
        got.covariance_matrix
        assert len(calls) == 0
        all_x, all_y = torch.cat([train_x, new_x], 1), torch.cat([train_y, new_y], 1)
        assert torch.equal(sm.train_inputs[0], all_x[:, 48:])
        _against_fresh(dev, model, got, all_x[:, 48:].contiguous(), all_y[:, 48:].contiguous(), test_x,
                       "three slides, N = 300")


def test_forget_oldest_refits_where_the_update_does_not_apply(cuda_device, monkeypatch):
    """N - m <= 256 and m > 64: exactly one factorisation of the kept data seeds the cache."""
    dev = cuda_device
    train_x, train_y, test_x, _, _ = _surface_data(dev, (2, 400, 3))
    model = _model(dev, train_x, train_y)
    model.eval()
    with torch.no_grad():
        model(test_x)
        for m in (144, 70):                              # n = 256 (m > 64 too), m > 64
            calls = _count_factorisations(monkeypatch)
            fm = model.forget_oldest(m)
            assert len(calls) == 1 and fm._prediction_cache is not None
            assert fm._prediction_cache[1][1].shape == (2, 400 - m, 400 - m)
            got = fm(test_x)
            assert len(calls) == 1
            monkeypatch.undo()
            if m == 70:
                _against_fresh(dev, model, got, train_x[:, m:].contiguous(), train_y[:, m:].contiguous(), test_x,
                               "forget 70 by a refit")
        small = _model(dev, train_x[:, :270].contiguous(), train_y[:, :270].contiguous())
        small.eval()
        small(test_x)
        calls = _count_factorisations(monkeypatch)
        fm = small.forget_oldest(16)                     # n = 254 <= 256 with a small m
        assert len(calls) == 1 and fm._prediction_cache[1][1].shape == (2, 254, 254)
        fm = small.forget_oldest(13)                     # n = 257: the update
        assert len(calls) == 1 and fm._prediction_cache[1][1].shape == (2, 257, 257)


def test_window_model_forgets_and_slides(cuda_device, monkeypatch):
    """A batch_shape=[3] model with a batched likelihood: the (B, 3 + n_ls) hyper matrix travels with
    the cache, and every window's predictions are those of its own hyper-parameters on the kept data.
    The noises keep every window where the fp32 posterior itself resolves the 1e-4 bar (the figures
    at a smaller noise: test_exact_append_gpu.py's window-model docstring)."""
    from fine_grained_gaussian_process_forcasting_amd.gp import GaussianLikelihood
    dev = cuda_device
    train_x, train_y, test_x, new_x, new_y = _surface_data(dev, (3, 300, 3), n_new=16)
    bs = torch.Size([3])
    with torch.no_grad():
        lik = GaussianLikelihood(batch_shape=bs).to(dev)
        wm = _model(dev, train_x, train_y, like=lik, batch_shape=bs)
        wm.covar_module.raw_outputscale.copy_(torch.tensor([0.2, -0.3, 0.9]))
        wm.covar_module.base_kernel.raw_lengthscale.copy_(torch.tensor([-0.5, 0.1, 0.4]).reshape(3, 1, 1))
        wm.mean_module.constant.copy_(torch.tensor([0.1, -0.2, 0.3]).reshape(wm.mean_module.constant.shape))
        lik.noise_covar.raw_noise.copy_(torch.tensor([-1.0, 0.0, 0.5]).reshape(3, 1))
        wm.eval()
        wm(test_x)
        calls = _count_factorisations(monkeypatch)
        fw = wm.forget_oldest(16)
        sw = wm.get_sliding_model(new_x, new_y)
        assert fw.batch_shape == bs and sw.batch_shape == bs
        assert fw._prediction_cache[1][3].shape == (3, 4) and sw.train_inputs[0].shape == (3, 300, 3)
        g_f, g_s = fw(test_x), sw(test_x)
        assert len(calls) == 0
        s2, ls, c, nz = ([float(v) for v in t.double().reshape(3)] for t in
                         (wm.covar_module.outputscale, wm.covar_module.base_kernel.lengthscale,
                          wm.mean_module.constant, lik.noise))
        for got, X, y in ((g_f, train_x[:, 16:], train_y[:, 16:]),
                          (g_s, torch.cat([train_x[:, 16:], new_x], 1), torch.cat([train_y[:, 16:], new_y], 1))):
            Xn, yn = X.double().cpu().numpy(), y.double().cpu().numpy()
            for b in range(3):
                Lr, zr = _factor_fp64(Xn[b:b + 1], yn[b:b + 1], ls[b], s2[b], c[b], nz[b])
                pm, pc = _posterior_fp64(Xn[b], Lr[0], zr[0], test_x[b].double().cpu().numpy(), ls[b], s2[b], c[b])
                em = _rel(got.mean[b:b + 1].cpu().numpy(), pm[None]).max()
                ev = _rel(got.variance[b:b + 1].cpu().numpy(), np.diagonal(pc)[None]).max()
                print(f"window {b}: mean {em:.2e} var {ev:.2e}")
                assert em <= 1e-4 and ev <= 1e-4


def test_model_errors_and_grad(cuda_device):
    dev = cuda_device
    train_x, train_y, test_x, new_x, new_y = _surface_data(dev, (300, 3), n_new=4)
    model = _model(dev, train_x, train_y)
    model.eval()
    with pytest.raises(RuntimeError, match="Call the model on some data first"):
        model.forget_oldest(4)
    with pytest.raises(RuntimeError, match="Call the model on some data first"):
        model.get_sliding_model(new_x, new_y)
    with torch.no_grad():
        model(test_x)
        for bad in (0, -3, 300, 301):
            with pytest.raises(ValueError, match="m must be in 1"):
                model.forget_oldest(bad)
        with pytest.raises(ValueError, match="do not match the training inputs"):
            model.get_sliding_model(new_x[:, :2], new_y)
        with pytest.raises(ValueError, match="do not match 4 new point"):
            model.get_sliding_model(new_x, new_y[:3])
        assert model.get_sliding_model(new_x, new_y).train_inputs[0].shape == (300, 3)
    # with gradients the new model is any model with that data: the eval path refits from the live parameters
    small = _model(dev, train_x[:80].contiguous(), train_y[:80].contiguous())
    small.eval()
    with torch.no_grad():
        small(test_x)
        sm = small.get_sliding_model(new_x, new_y)
    sm.zero_grad()
    sm(test_x).mean.sum().backward()
    params = list(sm.parameters())
    assert params and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert all(p.grad is None for p in small.parameters())


def test_exact_drop_opcheck(cuda_device):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    dev = cuda_device
    X, y, _, _ = _case(2, 40, 7, 3)
    L, z = _fit(dev, X, y, _hyper(dev))
    torch.library.opcheck(torch.ops.gpk.exact_drop.default, (L, z, 7), test_utils=("test_schema", "test_faketensor"))
