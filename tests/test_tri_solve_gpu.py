"""gpk_tri_solve_f32 / gpk::tri_solve: the one-right-hand-side solve against a batch of lower
triangular roots (MultivariateNormal.log_prob's whitening) and its registered backward, against
fp64 torch on the CPU. The roots are Cholesky factors of A A^T / n + I (condition number <= ~5), so
the project's 1e-4 norm-wise relative bound applies to the values and to both gradients."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(B, n, seed=0):
    g = torch.Generator().manual_seed(100 * seed + n)
    A = torch.randn(B, n, n, generator=g, dtype=torch.float64)
    R = torch.linalg.cholesky(A @ A.transpose(-1, -2) / n + torch.eye(n, dtype=torch.float64))
    return R, torch.randn(B, n, generator=g, dtype=torch.float64), torch.randn(B, n, generator=g, dtype=torch.float64)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# n: one element; one block; a padded second block; many blocks with padding; the largest
@pytest.mark.parametrize("B,n", [(2, 1), (3, 16), (2, 17), (2, 100), (2, 256)])
@pytest.mark.parametrize("trans", [False, True])
def test_tri_solve_values_and_gradients(cuda_device, B, n, trans):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    R64, d64, gw = _case(B, n)
    Rq, dq = R64.clone().requires_grad_(), d64.clone().requires_grad_()
    want = torch.linalg.solve_triangular(Rq.transpose(-1, -2) if trans else Rq, dq.unsqueeze(-1),
                                         upper=trans).squeeze(-1)
    wR, wd = torch.autograd.grad((gw * want).sum(), [Rq, dq])
    # junk above the diagonal must not be read
    R = (R64 + torch.triu(torch.full((n, n), 7.0, dtype=torch.float64), 1)).float().to(cuda_device).requires_grad_()
    d = d64.float().to(cuda_device).requires_grad_()
    got = torch.ops.gpk.tri_solve(R, d, trans)
    again = torch.ops.gpk.tri_solve(R, d, trans)
    assert torch.equal(got, again)
    gR, gd = torch.autograd.grad((gw.float().to(cuda_device) * got).sum(), [R, d])
    e = (_rel(got, want), _rel(gd, wd), _rel(gR, wR))
    print(f"tri_solve B={B} n={n} trans={trans}: w {e[0]:.2e} dd {e[1]:.2e} dR {e[2]:.2e}")
    assert max(e) <= 1e-4, e
    assert float(torch.triu(gR, 1).abs().sum()) == 0.0


def test_tri_solve_opcheck(cuda_device):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    R64, d64, _ = _case(2, 20, seed=1)
    R, d = R64.float().to(cuda_device).requires_grad_(), d64.float().to(cuda_device).requires_grad_()
    for trans in (False, True):
        torch.library.opcheck(torch.ops.gpk.tri_solve.default, (R, d, trans),
                              test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


def test_log_prob_of_a_dense_covariance_uses_the_kernel(cuda_device, monkeypatch):
    """CUDA fp32, n <= 256: log_prob's value and gradient against torch.distributions in fp64, with
    torch's triangular solve patched to raise; leading sample dimensions of the value included."""
    from fine_grained_gaussian_process_forcasting_amd.gp import MultivariateNormal
    g = torch.Generator().manual_seed(3)
    B, n = 2, 37
    A = torch.randn(B, n, n, generator=g, dtype=torch.float64)
    cov64 = A @ A.transpose(-1, -2) / n + torch.eye(n, dtype=torch.float64)
    mean64 = torch.randn(B, n, generator=g, dtype=torch.float64)
    val64 = torch.randn(3, B, n, generator=g, dtype=torch.float64)
    cq = cov64.clone().requires_grad_()
    want = torch.distributions.MultivariateNormal(mean64, covariance_matrix=cq).log_prob(val64)
    wc, = torch.autograd.grad(want.sum(), [cq])

    def boom(*a, **k):
        raise AssertionError("log_prob left the kernels")
    monkeypatch.setattr(torch.linalg, "solve_triangular", boom)
    cov = cov64.float().to(cuda_device).requires_grad_()
    dist = MultivariateNormal(mean64.float().to(cuda_device), torch.diagonal(cov, dim1=-2, dim2=-1).detach(),
                              covar_fn=lambda: cov)
    got = dist.log_prob(val64.float().to(cuda_device))
    assert got.shape == want.shape
    gc, = torch.autograd.grad(got.sum(), [cov])
    gc = 0.5 * (gc + gc.transpose(-1, -2))
    wc = 0.5 * (wc + wc.transpose(-1, -2))
    print(f"log_prob on the kernels: value {_rel(got, want):.2e} dcov {_rel(gc, wc):.2e}")
    assert _rel(got, want) <= 1e-4 and _rel(gc, wc) <= 1e-4
