"""CPU: the Cholesky (full-covariance) variational distribution -- the class surface, the KL closed
form, the torch reference of gpk_variational_chol_f32 (gp.variational_chol_predict) against the
mean-field oracle and autograd, the closed-form adjoint of include/gpk.h, and the argument
validation / size queries of the three new C entry points (no device is touched)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O


def _problem(B, N, M, D, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(B, N, D, generator=g) / np.sqrt(D)).to(dtype)
    Z = (torch.randn(M, D, generator=g) / np.sqrt(D)).to(dtype)
    ls = (0.5 + 0.5 * torch.rand(D, generator=g)).to(dtype)
    s2 = torch.tensor(0.8, dtype=dtype)
    m = (0.5 * torch.randn(M, generator=g)).to(dtype)
    C = torch.diag(0.5 + torch.rand(M, generator=g)) + torch.tril(0.3 * torch.randn(M, M, generator=g) / np.sqrt(M), -1)
    C[0, 0] = -C[0, 0]
    C = (C + torch.triu(torch.randn(M, M, generator=g), 1)).to(dtype)   # garbage above the diagonal
    w = torch.randn(D, generator=g).to(dtype)
    b0 = torch.tensor(0.3, dtype=dtype)
    gmean = torch.randn(B, N, generator=g).to(dtype)
    gvar = torch.randn(B, N, generator=g).to(dtype)
    return X, Z, ls, s2, m, C, w, b0, gmean, gvar


def _linv(Z, ls, s2, jitter):
    zs = Z.double() / ls.double()
    d = (zs[:, None, :] - zs[None, :, :]).pow(2).sum(-1)
    K = s2.double() * torch.exp(-0.5 * d) + jitter * torch.eye(Z.shape[0], dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    return torch.linalg.solve_triangular(L, torch.eye(Z.shape[0], dtype=torch.float64), upper=False)


def test_class_surface_and_state_dict():
    import fine_grained_gaussian_process_forcasting_amd as pkg
    from fine_grained_gaussian_process_forcasting_amd import gp
    assert pkg.CholeskyVariationalDistribution is gp.CholeskyVariationalDistribution
    for name in ("CholeskyVariationalDistribution", "variational_chol_predict",
                 "variational_chol_dense_covariance", "cholesky_kl_closed_form"):
        assert hasattr(gp, name), name
    q = gp.CholeskyVariationalDistribution(6)
    assert dict((k, tuple(v.shape)) for k, v in q.named_parameters()) == {
        "variational_mean": (6,), "chol_variational_covar": (6, 6)}
    assert torch.equal(q.variational_mean, torch.zeros(6))
    assert torch.equal(q.chol_variational_covar, torch.eye(6))
    qb = gp.CholeskyVariationalDistribution(5, batch_shape=torch.Size([3]))
    assert qb.variational_mean.shape == (3, 5) and qb.chol_variational_covar.shape == (3, 5, 5)
    assert torch.equal(qb.chol_variational_covar, torch.eye(5).expand(3, 5, 5))

    # inside a layer: GPyTorch's key names, and a round trip
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.DeepGP import ToyDeepGPHiddenLayer
    layer = ToyDeepGPHiddenLayer(3, None, 0, num_inducing=6)
    layer.variational_strategy._variational_distribution = gp.CholeskyVariationalDistribution(6)
    sd = layer.state_dict()
    assert "variational_strategy._variational_distribution.variational_mean" in sd
    assert "variational_strategy._variational_distribution.chol_variational_covar" in sd
    assert "variational_strategy._variational_distribution._variational_stddev" not in sd
    g = torch.Generator().manual_seed(1)
    upstream = {k: v.clone() for k, v in sd.items()}
    upstream["variational_strategy._variational_distribution.variational_mean"] = torch.randn(6, generator=g)
    upstream["variational_strategy._variational_distribution.chol_variational_covar"] = torch.randn(6, 6, generator=g)
    layer.load_state_dict(upstream)
    q = layer.variational_strategy.variational_distribution
    assert torch.equal(q.chol_variational_covar,
                       upstream["variational_strategy._variational_distribution.chol_variational_covar"])
    again = ToyDeepGPHiddenLayer(3, None, 5, num_inducing=6)
    again.variational_strategy._variational_distribution = gp.CholeskyVariationalDistribution(6)
    again.load_state_dict(layer.state_dict())
    for k, v in layer.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k


def test_initialize_consumes_the_rng_as_mean_field():
    from fine_grained_gaussian_process_forcasting_amd import gp
    for batch in (torch.Size([]), torch.Size([3])):
        qc = gp.CholeskyVariationalDistribution(7, batch)
        qm = gp.MeanFieldVariationalDistribution(7, batch)
        with torch.no_grad():
            qc.chol_variational_covar.add_(1.5)
        torch.manual_seed(11)
        qc.initialize_variational_distribution()
        after_c = torch.rand(1)
        torch.manual_seed(11)
        qm.initialize_variational_distribution()
        after_m = torch.rand(1)
        assert torch.equal(qc.variational_mean, qm.variational_mean)
        assert float(qc.variational_mean.detach().abs().max()) > 0
        assert torch.equal(qc.chol_variational_covar, torch.eye(7).expand(*batch, 7, 7))
        assert torch.equal(after_c, after_m)     # the same number of draws


@pytest.mark.parametrize("M", [1, 5, 20])
def test_kl_closed_form_vs_torch_distributions(M):
    from fine_grained_gaussian_process_forcasting_amd import gp
    g = torch.Generator().manual_seed(M)
    m = torch.randn(M, generator=g, dtype=torch.float64)
    C = torch.diag(0.5 + torch.rand(M, generator=g, dtype=torch.float64)) + \
        torch.tril(0.3 * torch.randn(M, M, generator=g, dtype=torch.float64), -1)
    prior = torch.distributions.MultivariateNormal(torch.zeros(M, dtype=torch.float64),
                                                   scale_tril=torch.eye(M, dtype=torch.float64))
    ref = torch.distributions.kl_divergence(torch.distributions.MultivariateNormal(m, scale_tril=C), prior)
    q = gp.CholeskyVariationalDistribution(M).double()
    with torch.no_grad():
        q.variational_mean.copy_(m)
        q.chol_variational_covar.copy_(C)
    assert abs(float(q.kl_divergence().detach() - ref)) <= 1e-12 * max(1.0, abs(float(ref)))
    # one negative diagonal entry: the same covariance as with that column's sign flipped
    k = M // 2
    Cn = C.clone()
    Cn[:, k] = -Cn[:, k]
    assert Cn[k, k] < 0
    with torch.no_grad():
        q.chol_variational_covar.copy_(Cn)
    assert abs(float(q.kl_divergence().detach() - ref)) <= 1e-12 * max(1.0, abs(float(ref)))
    # batched
    qb = gp.CholeskyVariationalDistribution(M, torch.Size([2])).double()
    with torch.no_grad():
        qb.variational_mean.copy_(torch.stack([m, 2 * m]))
        qb.chol_variational_covar.copy_(torch.stack([C, Cn]))
    kl = qb.kl_divergence().detach()
    assert kl.shape == (2,) and abs(float(kl[0] - ref)) <= 1e-12 * max(1.0, abs(float(ref)))


def test_strict_upper_triangle_is_never_read():
    from fine_grained_gaussian_process_forcasting_amd import gp
    X, Z, ls, s2, m, C, w, b0, gmean, gvar = _problem(2, 9, 6, 3, 5)
    Linv = _linv(Z, ls, s2, 1e-4)
    clean = torch.tril(C)
    Cg = C.clone().requires_grad_(True)
    mean, var = gp.variational_chol_predict(X, Z, Linv, m, Cg, s2, ls, w, b0, 1e-4)
    mean0, var0 = gp.variational_chol_predict(X, Z, Linv, m, clean, s2, ls, w, b0, 1e-4)
    # (torch.matmul folds the batch differently when an operand requires grad: the bitwise
    # comparison is between two calls that do not)
    mean1, var1 = gp.variational_chol_predict(X, Z, Linv, m, C, s2, ls, w, b0, 1e-4)
    assert torch.equal(mean1, mean0) and torch.equal(var1, var0)
    kl = gp.cholesky_kl_closed_form(m, Cg)
    assert torch.equal(kl.detach(), gp.cholesky_kl_closed_form(m, clean))
    ((gmean * mean).sum() + (gvar * var).sum() + 0.7 * kl).backward()
    assert torch.equal(torch.triu(Cg.grad, 1), torch.zeros(6, 6, dtype=torch.float64))
    assert float(Cg.grad[torch.tril(torch.ones(6, 6)) > 0].abs().min()) > 0
    cov = gp.variational_chol_dense_covariance(X, Z, Linv, C, s2, ls, 1e-4)
    assert torch.equal(cov, gp.variational_chol_dense_covariance(X, Z, Linv, clean, s2, ls, 1e-4))
    assert torch.allclose(cov.diagonal(dim1=-2, dim2=-1), var0, rtol=0, atol=1e-12)


def test_reference_reduces_to_the_mean_field_oracle():
    from fine_grained_gaussian_process_forcasting_amd import gp
    B, N, M, D = 3, 20, 8, 4
    X, Z, ls, s2, m, _, w, b0, _, _ = _problem(B, N, M, D, 3)
    g = torch.Generator().manual_seed(9)
    s = (0.5 + torch.rand(M, generator=g)).double()
    ref = O.variational_forward(X.numpy(), Z.numpy(), ls.numpy(), float(s2), w.numpy(), float(b0), m.numpy(),
                                s.numpy(), jitter=1e-4, dtype=np.float64)
    Linv = _linv(Z, ls, s2, 1e-4)
    mean, var = gp.variational_chol_predict(X, Z, Linv, m, torch.diag(s), s2, ls, w, b0, 1e-4)
    assert float((mean - torch.as_tensor(ref.mean)).abs().max()) <= 1e-12
    assert float((var - torch.as_tensor(ref.var)).abs().max()) <= 1e-12
    assert float(var.min()) > 1e-6     # the oracle's clamp did not fire


def test_reference_gradcheck():
    from fine_grained_gaussian_process_forcasting_amd import gp
    X, Z, ls, s2, m, C, w, b0, _, _ = _problem(1, 5, 4, 2, 2)
    Linv = _linv(Z, ls, s2, 1e-4)
    args = [t.clone().requires_grad_(True) for t in (X, Z, Linv, m, torch.tril(C), s2, ls, w, b0)]

    def fn(X, Z, Linv, m, C, s2, ls, w, b0):
        return gp.variational_chol_predict(X, Z, Linv, m, C, s2, ls, w, b0, 1e-4)
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_closed_form_adjoint_equals_autograd():
    """dA, dm and dC as include/gpk.h states them, against autograd of the reference."""
    B, N, M, D = 2, 17, 8, 3
    g = torch.Generator().manual_seed(8)
    A = torch.randn(B, M, N, generator=g, dtype=torch.float64, requires_grad=True)
    m = torch.randn(M, generator=g, dtype=torch.float64, requires_grad=True)
    C = torch.randn(M, M, generator=g, dtype=torch.float64, requires_grad=True)
    gmean = torch.randn(B, N, generator=g, dtype=torch.float64)
    gvar = torch.randn(B, N, generator=g, dtype=torch.float64)
    Lq = torch.tril(C)
    W = Lq.T @ A
    mean = (A * m[:, None]).sum(-2)
    var = 0.8 - A.pow(2).sum(-2) + W.pow(2).sum(-2)
    dA, dm, dC = torch.autograd.grad((gmean * mean).sum() + (gvar * var).sum(), [A, m, C])
    with torch.no_grad():
        Y = Lq @ W
        dA_cf = gmean[:, None, :] * m[:, None] + 2.0 * gvar[:, None, :] * (Y - A)
        dm_cf = (A * gmean[:, None, :]).sum((0, 2))
        dC_cf = 2.0 * torch.tril(torch.einsum("bmi,bki->mk", A * gvar[:, None, :], W))
    assert torch.allclose(dA, dA_cf, rtol=0, atol=1e-12)
    assert torch.allclose(dm, dm_cf, rtol=0, atol=1e-12)
    assert torch.allclose(dC, dC_cf, rtol=0, atol=1e-12)
    assert torch.equal(torch.triu(dC, 1), torch.zeros(M, M, dtype=torch.float64))
    # KL backward
    kl = 0.5 * (Lq.pow(2).sum() + m.pow(2).sum() - M - Lq.diagonal().pow(2).log().sum())
    km, kC = torch.autograd.grad(kl, [m, C])
    assert torch.allclose(km, m.detach(), rtol=0, atol=1e-14)
    assert torch.allclose(kC, (Lq - torch.diag(1.0 / C.diagonal())).detach(), rtol=0, atol=1e-12)


def test_new_symbols_exported_and_ops_registered():
    from fine_grained_gaussian_process_forcasting_amd import _native, ops, ops_autograd
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    lib = _native.lib()
    for n in ("gpk_variational_chol_saved_bytes", "gpk_variational_chol_f32",
              "gpk_variational_chol_adjoint_workspace_bytes", "gpk_variational_chol_adjoint_f32",
              "gpk_cholesky_kl_f32"):
        assert hasattr(lib, n) and n in _native.SIGNATURES, n
    for n in ("variational_chol_forward", "variational_chol_adjoint", "variational_chol_supported",
              "cholesky_kl", "cholesky_kl_grad"):
        assert hasattr(ops, n), n
    assert hasattr(ops_autograd, "variational_predict_chol")
    for n in ("variational_chol_fwd", "variational_chol_adj", "cholesky_kl", "cholesky_kl_grad"):
        assert hasattr(torch.ops.gpk, n), n
    with FakeTensorMode():
        B, N, M, D = 3, 70, 20, 4
        X, Z = torch.empty(B, N, D), torch.empty(M, D)
        Linv = torch.empty(M, M, dtype=torch.float64)
        mean, var, flags, hyp, saved = torch.ops.gpk.variational_chol_fwd(
            X, Linv, Z, torch.empty(M), torch.empty(M, M), torch.empty(()), torch.empty(D), torch.empty(D),
            torch.empty(()), 1e-4, True)
        assert mean.shape == (B, N) and var.shape == (B, N) and flags.dtype == torch.int32
        assert hyp.shape == (4 + 2 * D,) and saved.numel() == B * M * 128 + B * 128
        out = torch.ops.gpk.variational_chol_fwd(X, Linv, Z, torch.empty(M), torch.empty(M, M), torch.empty(()),
                                                 torch.empty(D), torch.empty(D), torch.empty(()), 1e-4)
        assert out[4].numel() == 0
        dX, dL, dZ, dpar, dC = torch.ops.gpk.variational_chol_adj(X, Linv, Z, torch.empty(M), torch.empty(M, M),
                                                                  hyp, mean, var, saved)
        assert dX.shape == X.shape and dL.shape == (M, M) and dL.dtype == torch.float64
        assert dZ.shape == (M, D) and dpar.shape == (M + 2 * D + 2,) and dC.shape == (M, M)
        assert torch.ops.gpk.cholesky_kl(torch.empty(M), torch.empty(M, M)).shape == (1,)


def test_entry_validation_without_device():
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation returns first
    # forward: X Z Linv vmean vchol hyp | B N M D | mean var flags saved stream
    args = [one] * 6 + [2, 16, 8, 4] + [one, one, None, None, None]
    for idx in (0, 1, 2, 3, 4, 5, 10, 11):
        bad = list(args); bad[idx] = None
        assert lib.gpk_variational_chol_f32(*bad) == -(idx + 1), idx
    for idx, val in ((6, -1), (7, 0), (8, 0), (8, 257), (9, 0), (9, 65)):
        bad = list(args); bad[idx] = val
        assert lib.gpk_variational_chol_f32(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[13] = ctypes.c_void_p(8)       # saved not 16-byte aligned
    assert lib.gpk_variational_chol_f32(*bad) == -14
    bad = list(args); bad[6] = 0
    assert lib.gpk_variational_chol_f32(*bad) == 0       # no windows: nothing launched
    # adjoint: X Z Linv vmean vchol hyp gmean gvar saved | B N M D | ws dX dLinv dZ dpar dchol stream
    args = [one] * 9 + [2, 16, 8, 4] + [one] * 6 + [None]
    for idx in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 15, 16, 17, 18):
        bad = list(args); bad[idx] = None
        assert lib.gpk_variational_chol_adjoint_f32(*bad) == -(idx + 1), idx
    for idx, val in ((9, -1), (10, 0), (10, 257), (11, 0), (11, 257), (12, 0), (12, 65)):
        bad = list(args); bad[idx] = val
        assert lib.gpk_variational_chol_adjoint_f32(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[13] = ctypes.c_void_p(8)
    assert lib.gpk_variational_chol_adjoint_f32(*bad) == -14
    bad = list(args); bad[9] = 0
    assert lib.gpk_variational_chol_adjoint_f32(*bad) == 0
    # KL: m chol M kl gkl dm dchol stream
    assert lib.gpk_cholesky_kl_f32(None, one, 4, one, None, None, None, None) == -1
    assert lib.gpk_cholesky_kl_f32(one, None, 4, one, None, None, None, None) == -2
    assert lib.gpk_cholesky_kl_f32(one, one, 0, one, None, None, None, None) == -3
    assert lib.gpk_cholesky_kl_f32(one, one, 4, None, None, None, None, None) == -4
    assert lib.gpk_cholesky_kl_f32(one, one, 4, None, one, None, one, None) == -6
    assert lib.gpk_cholesky_kl_f32(one, one, 4, None, one, one, None, None) == -7


def test_size_queries():
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    for q in (lib.gpk_variational_chol_saved_bytes, lib.gpk_variational_chol_adjoint_workspace_bytes):
        assert q(4, 192, 257, 32) == 0
        assert q(4, 192, 256, 65) == 0
        assert q(0, 192, 256, 32) == 0
        for shape in ((3, 20, 8, 4), (2, 65, 20, 5), (4, 192, 256, 32), (1, 256, 256, 64), (70, 16, 16, 4)):
            n = q(*shape)
            assert n > 0 and n % 16 == 0, (shape, n)
    assert lib.gpk_variational_chol_adjoint_workspace_bytes(4, 257, 64, 32) == 0
    assert lib.gpk_variational_chol_saved_bytes(4, 257, 64, 32) == (4 * 64 * 320 + 4 * 320) * 4
    # A (B, M, as) and the mask (B, as), as = N rounded up to 64
    assert lib.gpk_variational_chol_saved_bytes(2, 65, 20, 5) == (2 * 20 * 128 + 2 * 128) * 4
    # the adjoint's workspace holds the shared pipeline's and W diag(gvar) (B M as floats) on top
    B, N, M, D = 4, 192, 256, 32
    ws = lib.gpk_variational_chol_adjoint_workspace_bytes(B, N, M, D)
    assert ws >= lib.gpk_variational_cov_grad_workspace_bytes(B, N, M, D) + B * M * N * 4
