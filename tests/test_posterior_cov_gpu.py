"""Joint exact-GP posterior (eval mode): gpk_exact_posterior_cov_f32, gpk::exact_posterior_cov
and the covariance / sampling / log_prob / confidence_region surface of ExactGPModel.eval().

The oracle has no joint covariance, so this file carries its own fp64 NumPy restatement,
Sigma = K(xs, xs) - V^T V with V = L^{-1} K* and plain pairwise squared distances (no centring
tricks); each use first ties its mean and diagonal to oracle.exact_predict at 1e-12 relative.

Tolerance: 1e-4 relative, norm-wise (Frobenius) per window (north_star, test_posterior_gpu.py).
A CPU fp32 emulation of the kernel's arithmetic reaches <= 2.8e-5 on every shape below (worst:
N = 250, D = 1; all others <= 4e-6).
"""
import math

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
LN2 = math.log(2.0)


def _rel(a, b):
    a = np.asarray(a, np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, np.float64).reshape(b.shape[0], -1)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _sqdist(A, Bm, ls):
    d = (A[:, :, None, :] - Bm[:, None, :, :]) / np.asarray(ls, np.float64)
    return (d * d).sum(-1)


def _joint_fp64(X, y, Xs, ls, s2, c, noise):
    """fp64 (mean, cov) of the latent posterior, tied to the oracle's mean and variance."""
    X, y, Xs = (np.asarray(t, np.float64) for t in (X, y, Xs))
    B, N, _ = X.shape
    mean = np.empty(Xs.shape[:2])
    cov = np.empty((B, Xs.shape[1], Xs.shape[1]))
    for b in range(B):
        K = s2 * np.exp(-0.5 * _sqdist(X[b:b + 1], X[b:b + 1], ls)[0]) + noise * np.eye(N)
        L = np.linalg.cholesky(K)
        Ks = s2 * np.exp(-0.5 * _sqdist(X[b:b + 1], Xs[b:b + 1], ls)[0])
        V = np.linalg.solve(L, Ks)
        zz = np.linalg.solve(L, y[b] - c)
        mean[b] = c + V.T @ zz
        cov[b] = s2 * np.exp(-0.5 * _sqdist(Xs[b:b + 1], Xs[b:b + 1], ls)[0]) - V.T @ V
    rm, rv = O.exact_predict(X, y, Xs, ls, s2, c, noise)
    assert _rel(mean, rm).max() <= 1e-12
    assert _rel(np.diagonal(cov, axis1=1, axis2=2), rv).max() <= 1e-12
    return mean, cov


def _run(dev, X, y, Xs, ls, s2, c, noise):
    from fine_grained_gaussian_process_forcasting_amd import ops
    hyper = ops.pack_exact_hyper(s2, noise, c, torch.as_tensor(ls, dtype=torch.float32), dev)
    Xd, yd, Xsd = X.to(dev), y.to(dev), Xs.to(dev)
    f = ops.exact_mll(Xd, yd, None, None, None, None, want_L=True, want_z=True, hyper=hyper)
    p = ops.exact_posterior_cov(Xd, f.L, f.z, hyper, Xsd)
    p2 = ops.exact_posterior_cov(Xd, f.L, f.z, hyper, Xsd)
    q = ops.exact_posterior(Xd, f.L, f.z, hyper, Xsd)
    torch.cuda.synchronize()
    assert int(f.info.abs().max()) == 0
    return p, p2, q


@pytest.mark.parametrize("B,N,Ns,D", [(3, 16, 1, 4), (2, 16, 17, 3), (2, 33, 65, 4), (4, 37, 50, 5),
                                      (2, 128, 64, 32), (3, 250, 77, 1), (2, 256, 200, 32),
                                      (2, 96, 130, 64), (8, 64, 70, 8), (2, 300, 77, 5),
                                      (3, 257, 16, 64)])
def test_posterior_cov_parity(cuda_device, B, N, Ns, D):
    g = torch.Generator().manual_seed(N + Ns + D)
    X = torch.randn(B, N, D, generator=g) / math.sqrt(D)
    Xs = torch.randn(B, Ns, D, generator=g) / math.sqrt(D)
    y = torch.randn(B, N, generator=g)
    p, p2, q = _run(cuda_device, X, y, Xs, LN2, LN2, 0.3, LN2 + 1e-4)
    rm, rc = _joint_fp64(X.numpy(), y.numpy(), Xs.numpy(), LN2, LN2, 0.3, LN2 + 1e-4)
    assert p.cov.shape == (B, Ns, Ns) and p.mean.shape == (B, Ns) and p.var.shape == (B, Ns)
    err = _rel(p.cov.cpu().numpy(), rc)
    print(f"cov rel (B={B}, N={N}, Ns={Ns}, D={D}): {err.max():.2e}")
    assert err.max() <= 1e-4
    assert _rel(p.mean.cpu().numpy(), rm).max() <= 1e-4
    assert torch.equal(p.cov, p.cov.transpose(-1, -2))
    assert torch.equal(torch.diagonal(p.cov, dim1=-2, dim2=-1), p.var)
    assert torch.equal(p.mean, q.mean) and torch.equal(p.var, q.var)
    assert torch.equal(p.cov, p2.cov) and torch.equal(p.mean, p2.mean) and torch.equal(p.var, p2.var)


def test_posterior_cov_ard_offset_small_noise(cuda_device):
    """ARD lengthscales, inputs far from the origin (the centring matters), noise 1e-2, and the
    first 20 test points equal to training points: the covariance block there is tiny
    (|cov_ij| <= sqrt(var_i var_j) < 2e-2, Cauchy-Schwarz on test_posterior_gpu.py's bound)."""
    B, N, D = 3, 64, 6
    g = torch.Generator().manual_seed(5)
    X = torch.randn(B, N, D, generator=g) + 25.0
    Xs = torch.cat([X[:, :20], torch.randn(B, 30, D, generator=g) + 25.0], 1)
    y = torch.randn(B, N, generator=g)
    ls = np.linspace(0.8, 2.0, D)
    p, _, _ = _run(cuda_device, X, y, Xs, ls, 1.3, -0.2, 1e-2)
    _, rc = _joint_fp64(X.numpy(), y.numpy(), Xs.numpy(), ls, 1.3, -0.2, 1e-2)
    cov = p.cov.cpu().numpy()
    err = _rel(cov, rc)
    print(f"cov rel (ARD, offset): {err.max():.2e}")
    assert err.max() <= 1e-4
    assert np.abs(cov[:, :20, :20]).max() <= 2e-2


def _model(dev, batched=False):
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    from fine_grained_gaussian_process_forcasting_amd.gp import GaussianLikelihood
    g = torch.Generator().manual_seed(3)
    N, D = 80, 3
    shape = (3, N, D) if batched else (N, D)
    train_x = torch.rand(*shape, generator=g).to(dev)
    train_y = torch.sin(6.0 * train_x.sum(-1)).to(dev)
    test_x = torch.rand(*shape[:-2], 41, D, generator=g).to(dev)
    test_y = torch.sin(6.0 * test_x.sum(-1)).to(dev)
    lik = GaussianLikelihood().to(dev)
    model = ExactGPModel(train_x, train_y, lik).to(dev)
    model.eval()
    lik.eval()
    return model, lik, train_x, train_y, test_x, test_y, g


def _ref_of(model, lik, train_x, train_y, test_x):
    s2 = float(model.covar_module.outputscale)
    ls = float(model.covar_module.base_kernel.lengthscale)
    noise = float(lik.noise)
    c = float(model.mean_module.constant)
    f = lambda t: t.detach().reshape(-1, *t.shape[-2:]).cpu().double().numpy()  # noqa: E731
    yb = train_y.detach().reshape(-1, train_y.shape[-1]).cpu().double().numpy()
    rm, rc = _joint_fp64(f(train_x), yb, f(test_x), ls, s2, c, noise)
    return rm, rc, noise


def test_exact_gp_model_joint_posterior(cuda_device):
    """ExactGPModel.eval(): covariance_matrix, likelihood noise, rsample / sample, log_prob and
    confidence_region of the joint posterior, unbatched and batched."""
    dev = cuda_device
    model, lik, train_x, train_y, test_x, test_y, g = _model(dev)
    with torch.no_grad():
        d = model(test_x)
        L1 = model._prediction_cache[1][1]
        cov = d.covariance_matrix
        assert cov.shape == (41, 41)
        assert model._prediction_cache[1][1] is L1          # nothing is refactored
        rm, rc, noise = _ref_of(model, lik, train_x, train_y, test_x)
        assert _rel(cov[None].cpu().numpy(), rc).max() <= 1e-4
        p = lik(d)
        pc = p.covariance_matrix
        assert torch.equal(pc, cov + noise_eye(lik, 41, dev))
        S = rc[0] + noise * np.eye(41)
        R = np.linalg.cholesky(S)
        eps = torch.randn(5, 41, generator=g)
        draws = p.rsample(torch.Size([5]), base_samples=eps.to(dev))
        want = rm[0] + eps.double().numpy() @ R.T
        assert draws.shape == (5, 41)
        assert _rel(draws.cpu().numpy(), want).max() <= 1e-4
        assert p.sample(torch.Size([3])).shape == (3, 41)
        ty = test_y.cpu().double().numpy()
        w = np.linalg.solve(R, ty - rm[0])
        lp = -0.5 * (w @ w + 2.0 * np.log(np.diag(R)).sum() + 41 * math.log(2.0 * math.pi))
        got = p.log_prob(test_y)
        assert got.shape == ()
        assert abs(float(got) - lp) <= 1e-4 * abs(lp)
        lo, hi = p.confidence_region()
        assert torch.equal(lo, p.mean - 2.0 * p.stddev) and torch.equal(hi, p.mean + 2.0 * p.stddev)
        assert model._prediction_cache[1][1] is L1
    model, lik, train_x, train_y, test_x, test_y, g = _model(dev, batched=True)
    with torch.no_grad():
        cov = model(test_x).covariance_matrix
        assert cov.shape == (3, 41, 41)
        _, rc, _ = _ref_of(model, lik, train_x, train_y, test_x)
        assert _rel(cov.cpu().numpy(), rc).max() <= 1e-4


def noise_eye(lik, n, dev):
    return torch.diag_embed(lik.noise.detach().reshape(1).expand(n).to(dev))


def test_exact_gp_model_joint_posterior_gradients(cuda_device):
    """With the test inputs requiring grad the joint posterior is the differentiable restatement:
    it matches the kernel covariance and carries a gradient to the inputs."""
    dev = cuda_device
    model, lik, train_x, train_y, test_x, _, _ = _model(dev)
    with torch.no_grad():
        ref = model(test_x).covariance_matrix
    xr = test_x.clone().requires_grad_(True)
    cov = model(xr).covariance_matrix
    assert cov.shape == (41, 41) and cov.requires_grad
    assert _rel(cov[None].detach().cpu().numpy(), ref[None].cpu().double().numpy()).max() <= 1e-4
    cov.sum().backward()
    assert xr.grad is not None and bool(torch.isfinite(xr.grad).all())
    assert float(xr.grad.abs().max()) > 0.0


def test_exact_posterior_cov_opcheck(cuda_device):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    g = torch.Generator().manual_seed(0)
    B, N, D = 2, 24, 4
    X = (torch.randn(B, N, D, generator=g) / 2).to(dev)
    y = torch.randn(B, N, generator=g).to(dev)
    h = ops.pack_exact_hyper(LN2, LN2 + 1e-4, 0.1, torch.tensor(LN2), dev)
    _, L, z, _ = torch.ops.gpk.exact_mll(X, y, h, 1e-6, 3, True)
    Xs = (torch.randn(B, 30, D, generator=g) / 2).to(dev)
    torch.library.opcheck(torch.ops.gpk.exact_posterior_cov.default, (X, L, z, h, Xs),
                          test_utils=("test_schema", "test_faketensor"))
