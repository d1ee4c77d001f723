"""gpk_mvn_root_grad_f32: the adjoint of the batched Cholesky root fused with sampling, the
autograd formula of gpk::mvn_root on it, and psd_safe_cholesky / log_prob / the DeepGP skip-input
draw differentiating through the kernels.

References are fp64 torch on the CPU: torch.linalg.cholesky + autograd of
sum gsamples . (mean + R eps) + sum gR . R. Tolerance: 1e-4 relative, norm-wise (Frobenius) per
matrix (the project's parity bar). The well-conditioned matrices have condition
<= 6.2; fp32 LAPACK autograd is <= 5e-7 from fp64 on them. Measured on an MI355X: dcov <= 4.9e-7
over every n and case, log_prob's d/dcov 3.6e-7, the skip model's parameter gradients <= 3.7e-7
from the torch route, the ladder matrix's gradient 5.6e-7.
"""
import math
import warnings

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NS = [1, 15, 16, 17, 33, 100, 255, 256]
_CACHE = {}


def _rel(a, b):
    a = a.detach().cpu().double().reshape(a.shape[0], -1)
    b = b.detach().cpu().double().reshape(b.shape[0], -1)
    return float((torch.linalg.norm(a - b, dim=1) / torch.linalg.norm(b, dim=1)).max())


def _well_conditioned(n):
    g = torch.Generator().manual_seed(1000 + n)
    W = torch.randn(3, n, 2 * n, generator=g, dtype=torch.float64)
    A = W @ W.mT / (2 * n) + 0.5 * torch.eye(n, dtype=torch.float64)
    A = A.float()
    return (0.5 * (A + A.mT)).contiguous()


def _near_singular(n, shift):
    G = np.random.default_rng(n).standard_normal((n, n // 2))
    A = torch.from_numpy(G @ G.T / (n / 2) - shift * np.eye(n)).float()
    return (0.5 * (A + A.mT)).contiguous()


def _case(n):
    """Inputs of size n and the fp64 references of the four gradient cases, computed once."""
    if n in _CACHE:
        return _CACHE[n]
    A = _well_conditioned(n)
    g = torch.Generator().manual_seed(7 * n + 1)
    mean = torch.randn(3, n, generator=g)
    eps = torch.randn(5, 3, n, generator=g)
    gs = torch.randn(5, 3, n, generator=g)
    gR = torch.randn(3, n, n, generator=g)
    ref = {}
    for name, S, use_gR in [("s1", 1, False), ("s5", 5, False), ("gR", 0, True), ("both", 5, True)]:
        A64 = A.double().requires_grad_(True)
        m64 = mean.double().requires_grad_(True)
        R = torch.linalg.cholesky(A64)
        loss = A64.sum() * 0.0 + m64.sum() * 0.0
        if S:
            smp = m64 + torch.einsum("bij,sbj->sbi", R, eps[:S].double())
            loss = loss + (gs[:S].double() * smp).sum()
        if use_gR:
            loss = loss + (gR.double() * R).sum()
        loss.backward()
        ref[name] = (S, use_gR, A64.grad.clone(), m64.grad.clone())
    _CACHE[n] = (A, mean, eps, gs, gR, ref)
    return _CACHE[n]


@pytest.mark.parametrize("n", NS)
def test_mvn_root_grad_vs_fp64(cuda_device, n):
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    A, mean, eps, gs, gR, ref = _case(n)
    R, _, info = ops.mvn_root(A.to(dev))
    assert bool((info == 0).all())
    worst = 0.0
    for name, (S, use_gR, dA, dm) in ref.items():
        a_gR = gR.to(dev) if use_gR else None
        a_gs = gs[:S].to(dev).contiguous() if S else None
        a_eps = eps[:S].to(dev).contiguous() if S else None
        dcov, dmean = ops.mvn_root_grad(R, a_gR, a_gs, a_eps)
        dcov2, dmean2 = ops.mvn_root_grad(R, a_gR, a_gs, a_eps)
        torch.cuda.synchronize()
        e_cov = _rel(dcov, dA)
        worst = max(worst, e_cov)
        print(f"mvn_root_grad n={n} {name}: dcov rel {e_cov:.2e}")
        assert e_cov <= 1e-4
        if S:
            e_mean = _rel(dmean, dm)
            assert e_mean <= 1e-4
        else:
            assert bool((dmean == 0).all())
        assert torch.equal(dcov, dcov.mT)
        assert torch.equal(dcov, dcov2) and torch.equal(dmean, dmean2)     # a second launch: the same bits
        # junk in the upper triangles of R and gR changes nothing
        junk = torch.triu(torch.full_like(R, 7.0), 1)
        dcov3, _ = ops.mvn_root_grad(R + junk, a_gR + junk if use_gR else None, a_gs, a_eps)
        assert torch.equal(dcov3, dcov)
        # no dmean wanted
        dcov4, none = ops.mvn_root_grad(R, a_gR, a_gs, a_eps, want_dmean=False)
        assert none is None and torch.equal(dcov4, dcov)
    print(f"mvn_root_grad n={n}: max dcov rel {worst:.2e}")
    # no gradient arrives: zeros
    z, zm = ops.mvn_root_grad(R)
    assert bool((z == 0).all()) and bool((zm == 0).all())


def test_mvn_root_grad_batch_independence(cuda_device):
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    n, B = 32, 5
    A = _well_conditioned(n)[:1].to(dev).expand(B, n, n).contiguous()
    g = torch.Generator().manual_seed(11)
    eps = torch.randn(2, B, n, generator=g).to(dev)
    gs = torch.randn(2, B, n, generator=g).to(dev)
    R, _, _ = ops.mvn_root(A)
    dcov, dmean = ops.mvn_root_grad(R, None, gs, eps)
    for b in range(B):
        one, onem = ops.mvn_root_grad(R[b:b + 1], None, gs[:, b:b + 1].contiguous(), eps[:, b:b + 1].contiguous())
        assert torch.equal(one[0], dcov[b]) and torch.equal(onem[0], dmean[b])


def test_autograd_through_the_ops(cuda_device):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    n = 33
    A, mean, eps, gs, gR, _ = _case(n)
    cov = A.to(dev).requires_grad_(True)
    m = mean.to(dev).requires_grad_(True)
    e = eps.to(dev)
    R, smp, info = torch.ops.gpk.mvn_root(cov, 0.0, m, e, True)
    assert R.requires_grad and smp.requires_grad and not info.requires_grad
    ((gs.to(dev) * smp).sum() + (gR.to(dev) * R).sum()).backward()
    dcov, dmean = ops.mvn_root_grad(R.detach(), gR.to(dev), gs.to(dev), e)
    assert torch.equal(cov.grad, dcov) and torch.equal(m.grad, dmean)
    # the draws alone; eps with a gradient gets R^T g
    cov2 = A.to(dev).requires_grad_(True)
    e2 = e.clone().requires_grad_(True)
    R2, smp2, _ = torch.ops.gpk.mvn_root(cov2, 0.0, mean.to(dev), e2, True)
    (gs.to(dev) * smp2).sum().backward()
    assert torch.equal(cov2.grad, ops.mvn_root_grad(R2.detach(), None, gs.to(dev), e)[0])
    want = torch.einsum("bji,sbj->sbi", torch.linalg.cholesky(A.double()), gs.double())
    assert _rel(e2.grad.reshape(-1, n), want.reshape(-1, n)) <= 1e-4
    # a backward reached without the factor is an error, not a wrong gradient
    cov3 = A.to(dev).requires_grad_(True)
    _, smp3, _ = torch.ops.gpk.mvn_root(cov3, 0.0, mean.to(dev), e, False)
    with pytest.raises(RuntimeError, match="want_R"):
        smp3.sum().backward()
    # once differentiable
    cov4 = A.to(dev).requires_grad_(True)
    R4, _, _ = torch.ops.gpk.mvn_root(cov4, 0.0, None, None, True)
    (g4,) = torch.autograd.grad(R4.sum(), cov4, create_graph=True)
    with pytest.raises(RuntimeError):
        g4.sum().backward()


def test_mvn_root_autograd_opcheck(cuda_device):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    dev = cuda_device
    n = 17
    A, mean, eps, gs, gR, _ = _case(n)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    cov = A.to(dev).requires_grad_(True)
    m = mean.to(dev).requires_grad_(True)
    torch.library.opcheck(torch.ops.gpk.mvn_root.default, (cov, 0.0, m, eps.to(dev), True), test_utils=tests)
    torch.library.opcheck(torch.ops.gpk.mvn_root.default, (cov, 1e-6, None, None, True), test_utils=tests)
    R = torch.linalg.cholesky(A.double()).float().to(dev)
    torch.library.opcheck(torch.ops.gpk.mvn_root_grad.default, (R, gR.to(dev), gs.to(dev), eps.to(dev)),
                          test_utils=tests)
    torch.library.opcheck(torch.ops.gpk.mvn_root_grad.default, (R, None, None, None), test_utils=tests)


def _boom(*a, **k):
    raise AssertionError("torch.linalg.cholesky_ex must not run on the kernel path")


def test_log_prob_with_grad_on_the_kernel(cuda_device, monkeypatch):
    from fine_grained_gaussian_process_forcasting_amd.gp import MultivariateNormal
    dev = cuda_device
    n = 41
    A = _well_conditioned(n)[0]
    g = torch.Generator().manual_seed(5)
    mean = torch.randn(n, generator=g)
    value = torch.randn(n, generator=g)
    monkeypatch.setattr(torch.linalg, "cholesky_ex", _boom)
    cov = A.to(dev).requires_grad_(True)
    d = MultivariateNormal(mean.to(dev), torch.diagonal(A).clone().to(dev), covar_fn=lambda: cov)
    d.log_prob(value.to(dev)).sum().backward()
    S64 = A.double()
    Sinv = torch.linalg.inv(S64)
    alpha = Sinv @ (value - mean).double()
    want = -0.5 * (Sinv - torch.outer(alpha, alpha))
    err = _rel(cov.grad[None], want[None])
    print(f"log_prob d/dcov rel: {err:.2e}")
    assert err <= 1e-4


def test_ladder_with_grad_on_the_kernel(cuda_device, monkeypatch):
    """The ladder matrix (rank n/2 minus 3e-5 I, factored at jitter 1e-4: condition 6.8e4) with a
    gradient: the three warnings in order, a finite gradient, and the gradient against fp64
    autograd through cholesky(A + 1e-4 I).

    Measured on an MI355X: 5.6e-7. The backward of a rung with jitter refines the fp32 factor once
    with an fp64 residual (gpk_mvn_root_refine_f32) before the adjoint; without that step the
    kernels gave 7.2e-4, as fp32 LAPACK autograd does (7.7e-4): the fp32 factorisation's error,
    amplified by the condition number, not the adjoint's arithmetic."""
    from fine_grained_gaussian_process_forcasting_amd import NumericalWarning
    from fine_grained_gaussian_process_forcasting_amd.gp import psd_safe_cholesky
    dev = cuda_device
    n = 32
    A = _near_singular(n, 3e-5)
    gR = torch.randn(n, n, generator=torch.Generator().manual_seed(9))
    monkeypatch.setattr(torch.linalg, "cholesky_ex", _boom)
    cov = A.to(dev).requires_grad_(True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        L = psd_safe_cholesky(cov)
    msgs = [str(x.message) for x in w if issubclass(x.category, NumericalWarning)]
    assert msgs == [f"A not p.d., added jitter of {j} to the diagonal" for j in ("1.0e-06", "1.0e-05", "1.0e-04")]
    (gR.to(dev) * L).sum().backward()
    monkeypatch.undo()
    A64 = A.double().requires_grad_(True)
    (gR.double() * torch.linalg.cholesky(A64 + 1e-4 * torch.eye(n, dtype=torch.float64))).sum().backward()
    assert bool(torch.isfinite(cov.grad).all())
    err = _rel(cov.grad[None], A64.grad[None])
    print(f"ladder gradient rel: {err:.2e}")
    assert err <= 1e-4


def test_skip_path_trains_through_the_kernels(cuda_device, monkeypatch):
    """l2(l1(x), x) in train mode (DeepGP.py:62-64): the draw between the layers and its backward
    run on gpk_mvn_root_f32 / gpk_mvn_root_grad_f32 (torch.linalg.cholesky_ex patched to raise);
    every l1 parameter gets the gradient of the torch route."""
    from fine_grained_gaussian_process_forcasting_amd import gp, settings
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.DeepGP import ToyDeepGPHiddenLayer
    dev = cuda_device
    d, b, N, M, NO = 6, 3, 16, 20, 2
    l1 = ToyDeepGPHiddenLayer(input_dims=d, output_dims=NO, seed=4, num_inducing=M).to(dev)
    l2 = ToyDeepGPHiddenLayer(input_dims=NO + d, output_dims=None, seed=6, num_inducing=M).to(dev)
    l1.train()
    l2.train()
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(b, N, d, generator=g) / math.sqrt(d)).to(dev)
    with torch.no_grad(), settings.num_likelihood_samples(1):
        # a layer's first call initialises q(u) from the generator (mean_init_std * randn): done
        # here, so both routes below start from the same parameters and the same generator state
        l2(l1(x), x)

    def step():
        for p in list(l1.parameters()) + list(l2.parameters()):
            p.grad = None
        with settings.num_likelihood_samples(1):
            torch.manual_seed(0)
            y = l2(l1(x), x)
            (y.mean.sum() + y.variance.sum()).backward()
        return {k: p.grad.clone() for k, p in l1.named_parameters()}

    real_cholesky_ex = torch.linalg.cholesky_ex
    monkeypatch.setattr(torch.linalg, "cholesky_ex", _boom)
    got = step()
    names = " ".join(got)
    for part in ("inducing_points", "variational_mean", "variational_stddev", "raw_outputscale",
                 "raw_lengthscale", "constant"):
        assert part in names, (part, names)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0.0, k
    # the bound below means something only for a well-conditioned Sigma
    vs1 = l1.variational_strategy
    for o in range(NO):
        S = O.variational_covariance(
            x.cpu().double().numpy(), vs1.inducing_points[o].detach().cpu().double().numpy(),
            l1.covar_module.base_kernel.lengthscale[o].reshape(-1).detach().cpu().double().numpy(),
            float(l1.covar_module.outputscale[o]),
            vs1._variational_distribution._variational_stddev[o].detach().cpu().double().numpy(), jitter=1e-4)
        cond = np.linalg.cond(S)
        print(f"output {o}: cond(Sigma) {cond.min():.0f} .. {cond.max():.0f}")
        assert cond.max() <= 200
    # the same step on the torch route
    monkeypatch.setattr(torch.linalg, "cholesky_ex", real_cholesky_ex)
    monkeypatch.setattr(gp, "_mvn_root_eligible", lambda A: False)
    want = step()
    errs = {k: float(torch.linalg.norm((got[k] - want[k]).double()) / torch.linalg.norm(want[k].double()))
            for k in got}
    for k, err in errs.items():
        print(f"{k}: rel {err:.2e}")
    for k, err in errs.items():
        assert err <= 1e-4, k


@pytest.mark.parametrize("n", [17, 100, 256])
def test_mvn_root_refine_keeps_a_good_factor(cuda_device, n):
    """On a well-conditioned matrix the refined factor stays at fp32 rounding from the fp64 one."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    A = _well_conditioned(n).to(cuda_device)
    R, _, _ = ops.mvn_root(A)
    R1 = ops.mvn_root_refine(A, 0.0, R)
    L = torch.linalg.cholesky(A.cpu().double())
    e0, e1 = _rel(R, L), _rel(R1, L)
    print(f"refine n={n}: R rel {e0:.2e} -> {e1:.2e}")
    assert e1 <= 1e-6      # a few fp32 roundings per entry; the unrefined factor measures <= 1.8e-7
    assert bool((torch.triu(R1, 1) == 0).all())
    assert torch.equal(R1, ops.mvn_root_refine(A, 0.0, R))
    junk = torch.triu(torch.full_like(A, 7.0), 1)
    assert torch.equal(R1, ops.mvn_root_refine(A + junk, 0.0, R + junk))


@pytest.mark.parametrize("n", [32, 100])
def test_mvn_root_refine_on_the_ladder_matrix(cuda_device, n):
    """Near-singular (condition ~ 7e4 at jitter 1e-4): the fp32 factor is ~ cond * 2^-24 = 4e-3 off
    at worst; one step with an fp64 residual leaves the square of that plus fp32 rounding, so
    1e-5 is asked for, and at least ten times better than before."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    A = _near_singular(n, 3e-5)
    R, _, info = ops.mvn_root(A[None].to(cuda_device), jitter=1e-4)
    assert int(info.item()) == 0
    R1 = ops.mvn_root_refine(A[None].to(cuda_device), 1e-4, R)
    L = torch.linalg.cholesky(A.double() + 1e-4 * torch.eye(n, dtype=torch.float64))[None]
    e0, e1 = _rel(R, L), _rel(R1, L)
    print(f"refine ladder n={n}: R rel {e0:.2e} -> {e1:.2e}")
    assert e1 <= 1e-5 and e1 <= 0.1 * e0
