"""Host-side checks of gpk_tri_solve_f32 (no GPU): argument validation, the FakeTensor shape of
gpk::tri_solve, the refusal of CPU tensors, and that a CPU distribution's log_prob keeps torch's
triangular solve."""
import ctypes

import pytest
import torch


def test_tri_solve_validation_without_device():
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation returns first
    #       R    d    B  n   trans w   stream
    args = [one, one, 2, 40, 0, one, None]
    for idx in (0, 1, 5):
        bad = list(args); bad[idx] = None
        assert lib.gpk_tri_solve_f32(*bad) == -(idx + 1)
    for idx, val in [(2, -1), (3, 0), (3, 257), (4, 2), (4, -1)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_tri_solve_f32(*bad) == -(idx + 1)
    bad = list(args); bad[2] = 0
    assert lib.gpk_tri_solve_f32(*bad) == 0      # no matrices: nothing launched


def test_tri_solve_fake_shape_and_cpu_refusal():
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        w = torch.ops.gpk.tri_solve(torch.empty(3, 20, 20), torch.empty(3, 20), True)
        assert w.shape == (3, 20)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tri_solve(torch.eye(4)[None], torch.ones(1, 4))
    with pytest.raises(ValueError):
        ops.tri_solve(torch.eye(4)[None], torch.ones(1, 5))


def test_cpu_log_prob_keeps_the_torch_solve(monkeypatch):
    from fine_grained_gaussian_process_forcasting_amd.gp import MultivariateNormal
    g = torch.Generator().manual_seed(0)
    A = torch.randn(2, 6, 6, generator=g, dtype=torch.float64)
    cov = A @ A.transpose(-1, -2) + 6.0 * torch.eye(6, dtype=torch.float64)
    mean, val = torch.randn(2, 6, generator=g, dtype=torch.float64), torch.randn(2, 6, generator=g, dtype=torch.float64)
    calls = []
    real = torch.linalg.solve_triangular
    monkeypatch.setattr(torch.linalg, "solve_triangular", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    dist = MultivariateNormal(mean, torch.diagonal(cov, dim1=-2, dim2=-1), covar_fn=lambda: cov)
    got = dist.log_prob(val)
    want = torch.distributions.MultivariateNormal(mean, covariance_matrix=cov).log_prob(val)
    assert calls and torch.allclose(got, want, rtol=1e-12, atol=1e-12)
