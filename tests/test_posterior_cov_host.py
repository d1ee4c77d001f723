"""Host-side checks of the joint exact-GP posterior (no GPU): the argument validation of
gpk_exact_posterior_cov_f32, its workspace query, the FakeTensor shapes of
gpk::exact_posterior_cov, the "no CPU fallback" guard and the log_prob / confidence_region
arithmetic of MultivariateNormal on a hand-built 3 x 3 covariance."""
import ctypes
import math

import pytest
import torch


def test_posterior_cov_entry_validation_without_device():
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation returns first
    #       X    L    z    hyp n_ls Xs  B  N   Ns  D  ws   mean var  cov  stream
    args = [one, one, one, one, 1, one, 2, 16, 40, 4, one, one, one, one, None]
    for idx, code in [(0, -1), (1, -2), (2, -3), (3, -4), (5, -6), (10, -11), (11, -12), (12, -13),
                      (13, -14)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_exact_posterior_cov_f32(*bad) == code
    bad = list(args); bad[4] = 3
    assert lib.gpk_exact_posterior_cov_f32(*bad) == -5
    bad = list(args); bad[4] = 4
    bad[7] = 0
    assert lib.gpk_exact_posterior_cov_f32(*bad) == -8    # n_lengthscale = D is accepted; N < 1
    bad = list(args); bad[7] = 801
    assert lib.gpk_exact_posterior_cov_f32(*bad) == -8
    bad = list(args); bad[9] = 65
    bad[4] = 65
    assert lib.gpk_exact_posterior_cov_f32(*bad) == -10
    bad = list(args); bad[8] = 0
    assert lib.gpk_exact_posterior_cov_f32(*bad) == 0     # no test points: nothing launched
    bad = list(args); bad[6] = 0
    assert lib.gpk_exact_posterior_cov_f32(*bad) == 0     # no windows: nothing launched
    # the blocked path keeps B on the grid's y dimension
    bad = list(args); bad[6] = 65536
    bad[7] = 257
    assert lib.gpk_exact_posterior_cov_f32(*bad) == -7


def test_posterior_cov_workspace_query():
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    q = lib.gpk_exact_posterior_cov_workspace_bytes
    assert q(3, 801, 40) == 0
    assert q(3, 0, 40) == 0
    for B, N, Ns in [(3, 16, 1), (2, 33, 65), (512, 256, 256), (2, 300, 77), (1, 800, 64)]:
        assert q(B, N, Ns) >= 4 * B * N * Ns
    assert q(65536, 257, 16) == 0       # rejected by the call (-7)
    assert q(65536, 256, 16) >= 4 * 65536 * 256 * 16


def test_exact_posterior_cov_fake_shapes():
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.gpk, "exact_posterior_cov")
    with FakeTensorMode():
        X = torch.empty(3, 16, 4)
        L = torch.empty(3, 16, 16)
        z = torch.empty(3, 16)
        h = torch.empty(4)
        m, v, c = torch.ops.gpk.exact_posterior_cov(X, L, z, h, torch.empty(3, 40, 4))
        assert m.shape == (3, 40) and v.shape == (3, 40) and c.shape == (3, 40, 40)


def test_exact_posterior_cov_refuses_cpu_tensors():
    from fine_grained_gaussian_process_forcasting_amd import ops
    X = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.exact_posterior_cov(X, torch.zeros(2, 8, 8), torch.zeros(2, 8), torch.ones(4),
                                torch.zeros(2, 5, 3))


def test_mvn_log_prob_and_confidence_region_closed_form():
    """MultivariateNormal(mean, var, covar_fn=...) on a 3 x 3 covariance with a known factor:
    Sigma = R R^T, log|Sigma| = 2 sum log R_ii, and the quadratic form by hand."""
    from fine_grained_gaussian_process_forcasting_amd.gp import MultivariateNormal
    R = torch.tensor([[2.0, 0.0, 0.0], [0.5, 1.5, 0.0], [-1.0, 0.25, 0.5]], dtype=torch.float64)
    S = R @ R.T
    mean = torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64)
    calls = []

    def cov():
        calls.append(1)
        return S

    d = MultivariateNormal(mean, S.diagonal().clone(), covar_fn=cov)
    assert not calls                                      # lazy until asked
    w = torch.tensor([0.3, -0.7, 1.1], dtype=torch.float64)   # value = mean + R w  ->  R^-1 diff = w
    value = mean + R @ w
    want = -0.5 * (float(w @ w) + 2.0 * (math.log(2.0) + math.log(1.5) + math.log(0.5))
                   + 3 * math.log(2.0 * math.pi))
    got = d.log_prob(value)
    assert got.shape == () and abs(float(got) - want) <= 1e-12 * abs(want)
    # against torch's own density, and with a leading sample dimension
    ref = torch.distributions.MultivariateNormal(mean, covariance_matrix=S)
    vals = torch.stack([value, mean, mean - 1.0])
    assert torch.allclose(d.log_prob(vals), ref.log_prob(vals), rtol=1e-12, atol=0)
    lo, hi = d.confidence_region()
    sd = torch.tensor([2.0, math.sqrt(0.25 + 2.25), math.sqrt(1.0 + 0.0625 + 0.25)], dtype=torch.float64)
    assert torch.allclose(lo, mean - 2.0 * sd, rtol=1e-14, atol=0)
    assert torch.allclose(hi, mean + 2.0 * sd, rtol=1e-14, atol=0)
    # the likelihood's noise lands on the diagonal of the density's covariance
    dn = d.add_noise(torch.tensor(0.3, dtype=torch.float64))
    refn = torch.distributions.MultivariateNormal(mean, covariance_matrix=S + 0.3 * torch.eye(3, dtype=torch.float64))
    assert torch.allclose(dn.log_prob(value), refn.log_prob(value), rtol=1e-12, atol=0)
    # a distribution of marginals alone still has no joint density
    with pytest.raises(NotImplementedError):
        MultivariateNormal(mean, S.diagonal().clone()).log_prob(value)
