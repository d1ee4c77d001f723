"""Host-side checks of the variational covariance and the MVN root (no GPU): exported symbols,
argument validation and workspace queries of gpk_variational_cov_f32 / _batched_f32 and
gpk_mvn_root_f32, the FakeTensor shapes of the two custom ops, and that CPU tensors keep the
torch path of psd_safe_cholesky / rsample / covariance_matrix unchanged."""
import ctypes
import math
import warnings

import pytest
import torch


def _lib():
    from fine_grained_gaussian_process_forcasting_amd import _native
    return _native.lib()


def test_new_symbols_and_version():
    lib = _lib()
    for name in ("gpk_variational_cov_workspace_bytes", "gpk_variational_cov_f32",
                 "gpk_variational_cov_batched_workspace_bytes", "gpk_variational_cov_batched_f32",
                 "gpk_mvn_root_max_n", "gpk_mvn_root_f32"):
        assert hasattr(lib, name)
    assert lib.gpk_version() >= 400
    assert lib.gpk_mvn_root_max_n() == 256


def test_variational_cov_validation_without_device():
    lib = _lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation returns first
    #       X    Z    Linv vstd hyp  B  N   M   D  ws   cov  stream
    args = [one, one, one, one, one, 2, 40, 16, 4, one, one, None]
    for idx, code in [(0, -1), (1, -2), (2, -3), (3, -4), (4, -5), (9, -10), (10, -11)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_variational_cov_f32(*bad) == code
    for idx, val, code in [(5, -1, -6), (6, 0, -7), (7, 0, -8), (7, 257, -8), (8, 0, -9), (8, 65, -9),
                           (9, ctypes.c_void_p(8), -10)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_variational_cov_f32(*bad) == code
    bad = list(args); bad[5] = 0
    assert lib.gpk_variational_cov_f32(*bad) == 0      # no windows: nothing launched
    #       X  shared Z    Linv vstd hyp  O  B  N   M   D  ws   cov  stream
    args = [one, 1, one, one, one, one, 3, 2, 40, 16, 4, one, one, None]
    for idx, code in [(0, -1), (2, -3), (3, -4), (4, -5), (5, -6), (11, -12), (12, -13)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_variational_cov_batched_f32(*bad) == code
    for idx, val, code in [(6, 0, -7), (6, 65536, -7), (7, -1, -8), (8, 0, -9), (9, 257, -10), (10, 65, -11),
                           (11, ctypes.c_void_p(4), -12)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_variational_cov_batched_f32(*bad) == code
    bad = list(args); bad[7] = 0
    assert lib.gpk_variational_cov_batched_f32(*bad) == 0


def test_variational_cov_workspace_queries():
    lib = _lib()
    q = lib.gpk_variational_cov_workspace_bytes
    for B, N, M in [(2, 1, 8), (3, 17, 16), (2, 65, 64), (256, 192, 256), (1, 300, 32)]:
        stride = (N + 63) // 64 * 64
        assert q(B, N, M) == 4 * (B * M * stride + 64 * B)     # A (B, M, as), then the means (B, 64)
        assert q(B, N, M) % 16 == 0
        assert lib.gpk_variational_cov_batched_workspace_bytes(3, B, N, M) == 3 * q(B, N, M)
    assert q(2, 0, 8) == 0 and q(2, 16, 0) == 0 and q(2, 16, 257) == 0 and q(-1, 16, 8) == 0
    assert q(0, 16, 8) == 0            # B = 0 is accepted by the call and needs no workspace
    assert lib.gpk_variational_cov_batched_workspace_bytes(0, 2, 16, 8) == 0
    assert lib.gpk_variational_cov_batched_workspace_bytes(65536, 2, 16, 8) == 0


def test_mvn_root_validation_without_device():
    lib = _lib()
    one = ctypes.c_void_p(16)
    #       cov  mean eps  B  n   S  jitter R   samples info stream
    args = [one, one, one, 2, 16, 3, 0.0, one, one, one, None]
    for idx, code in [(0, -1), (1, -2), (2, -3), (8, -9), (9, -10)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_mvn_root_f32(*bad) == code
    for idx, val, code in [(3, -1, -4), (4, 0, -5), (4, 257, -5), (5, -1, -6), (6, -1.0, -7),
                           (6, float("nan"), -7)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_mvn_root_f32(*bad) == code
    bad = list(args); bad[3] = 0
    assert lib.gpk_mvn_root_f32(*bad) == 0             # no matrices: nothing launched
    # S = 0 takes NULL mean / eps / samples (and a NULL R): still valid up to the launch
    assert lib.gpk_mvn_root_f32(one, None, None, 0, 16, 0, 0.0, None, None, one, None) == 0


def test_new_ops_fake_shapes_and_cpu_refusal():
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.gpk, "variational_cov") and hasattr(torch.ops.gpk, "mvn_root")
    with FakeTensorMode():
        x = torch.empty(3, 20, 4)
        c = torch.ops.gpk.variational_cov(x, torch.empty(8, 8, dtype=torch.float64), torch.empty(8, 4),
                                          torch.empty(8), torch.empty(12))
        assert c.shape == (3, 20, 20)
        c = torch.ops.gpk.variational_cov(x, torch.empty(2, 8, 8, dtype=torch.float64), torch.empty(2, 8, 4),
                                          torch.empty(2, 8), torch.empty(2, 12))
        assert c.shape == (2, 3, 20, 20)
        R, s, info = torch.ops.gpk.mvn_root(c[0], 0.0, torch.empty(3, 20), torch.empty(5, 3, 20), True)
        assert R.shape == (3, 20, 20) and s.shape == (5, 3, 20) and info.shape == (3,) and info.dtype == torch.int32
        R, s, info = torch.ops.gpk.mvn_root(c[0], 0.0, None, None, False)
        assert R.numel() == 0 and s.numel() == 0
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.mvn_root(torch.eye(4)[None])
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.variational_cov(torch.zeros(2, 8, 3), torch.zeros(4, 3), torch.eye(4, dtype=torch.float64),
                            torch.ones(4), torch.ones(10))
    with pytest.raises(ValueError, match="n <= 256"):
        ops.mvn_root(torch.zeros(1, 257, 257))


def test_cpu_tensors_keep_the_torch_path():
    from fine_grained_gaussian_process_forcasting_amd import NumericalWarning
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.DeepGP import ToyDeepGPHiddenLayer
    from fine_grained_gaussian_process_forcasting_amd.gp import (MultivariateNormal, psd_safe_cholesky,
                                                                  variational_dense_covariance)
    g = torch.Generator().manual_seed(0)
    W = torch.randn(2, 6, 12, generator=g)
    A = W @ W.mT / 12 + 0.5 * torch.eye(6)
    assert torch.equal(psd_safe_cholesky(A), torch.linalg.cholesky(A))
    # the ladder on a singular CPU matrix: today's sequence and result
    ones = torch.ones(4, 4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        L = psd_safe_cholesky(ones)
    msgs = [str(x.message) for x in w if issubclass(x.category, NumericalWarning)]
    assert msgs[0] == "A not p.d., added jitter of 1.0e-06 to the diagonal" and 1 <= len(msgs) <= 3
    jit = 1e-6 * 10 ** (len(msgs) - 1)
    assert torch.allclose(L, torch.linalg.cholesky(ones + jit * torch.eye(4)), atol=1e-6)
    # rsample of a CPU distribution: mean + cholesky(cov) eps
    mean = torch.randn(2, 6, generator=g)
    eps = torch.randn(3, 2, 6, generator=g)
    d = MultivariateNormal(mean, torch.diagonal(A, dim1=-2, dim2=-1).clone(), covar_fn=lambda: A)
    want = mean + (torch.linalg.cholesky(A) @ eps.unsqueeze(-1)).squeeze(-1)
    assert torch.equal(d.rsample(torch.Size([3]), base_samples=eps), want)
    # the lazy covariance of a variational output built on CPU tensors is the dense restatement
    Z = torch.randn(5, 3, generator=g)
    x = torch.randn(2, 7, 3, generator=g)
    Kzz = torch.exp(-0.5 * torch.cdist(Z.double(), Z.double()) ** 2) + 1e-4 * torch.eye(5, dtype=torch.float64)
    Linv = torch.linalg.inv(torch.linalg.cholesky(Kzz))
    vstd = torch.rand(5, generator=g) + 0.5
    cov = variational_dense_covariance(x, Z, Linv, vstd, torch.tensor(1.0), torch.ones(3), 1e-4)
    from fine_grained_gaussian_process_forcasting_amd.gp import _variational_cov_on_kernels
    assert not _variational_cov_on_kernels(x, Z, Linv, vstd, torch.tensor(1.0), torch.ones(3))
    assert cov.shape == (2, 7, 7) and torch.allclose(cov, cov.mT, atol=1e-6)
    A64 = Linv @ torch.exp(-0.5 * torch.cdist(Z.double()[None], x.double()) ** 2)
    ref = (torch.exp(-0.5 * torch.cdist(x.double(), x.double()) ** 2) + 1e-4 * torch.eye(7, dtype=torch.float64)
           + A64.mT @ ((vstd.double() ** 2 - 1)[:, None] * A64))
    assert torch.allclose(cov.double(), ref, atol=1e-5)
