"""Adjoint of the exact-GP posterior on the gfx950 kernels: gpk_exact_posterior_grad_f32 through
ops.exact_posterior_grad, gpk::exact_posterior_train / gpk::exact_posterior_grad, and ExactGPModel
in eval mode under grad.

Reference: fp64 torch autograd of the dense posterior on the CPU (the restatement of
tests/test_posterior_gpu.py::_posterior_fp64, with the joint covariance). Error: norm-wise
relative per gradient block (dX, dy, dXs, dhyp summed over the windows); dX and dXs also per
window. Bound: the project's 1e-4 at the fixtures' hyper-parameters (s2 = ln 2, noise = ln 2 + 1e-4,
c = 0.1, l = ln 2 or per-dimension values in [0.5, 1.5]: cond(K_hat) <= N + 1).
"""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
LN2 = math.log(2.0)
S2, NOISE, C0 = LN2, LN2 + 1e-4, 0.1


def _posterior_fp64(X, y, Xs, ls, s2, c, noise):
    """fp64 torch restatement of the exact posterior (mean, latent variance, joint covariance)."""
    d = (((X.unsqueeze(-2) - X.unsqueeze(-3)) / ls) ** 2).sum(-1)
    n = X.shape[-2]
    K = s2 * torch.exp(-0.5 * d) + noise * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    ds = (((X.unsqueeze(-2) - Xs.unsqueeze(-3)) / ls) ** 2).sum(-1)
    dss = (((Xs.unsqueeze(-2) - Xs.unsqueeze(-3)) / ls) ** 2).sum(-1)
    V = torch.linalg.solve_triangular(L, s2 * torch.exp(-0.5 * ds), upper=False)
    z = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False)
    cov = s2 * torch.exp(-0.5 * dss) - V.transpose(-1, -2) @ V
    return c + (V * z).sum(-2), s2 - (V * V).sum(-2), cov


def _reference(X, y, Xs, ls, s2, c, noise, gm, gv, gc):
    """-> (dX, dy, dXs, dhyp summed over the windows) in fp64 on the CPU."""
    D = lambda t: None if t is None else t.detach().cpu().double()   # noqa: E731
    q = [D(t).clone().requires_grad_() for t in (X, y, Xs)]
    h = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in (s2, noise, c)]
    lsq = torch.as_tensor(ls, dtype=torch.float64).reshape(-1).clone().requires_grad_()
    mean, var, cov = _posterior_fp64(q[0], q[1], q[2], lsq, h[0], h[2], h[1])
    obj = 0.0
    for g, out in ((gm, mean), (gv, var), (gc, cov)):
        if g is not None:
            obj = obj + (D(g) * out).sum()
    gr = torch.autograd.grad(obj, q + h + [lsq], allow_unused=True)
    gr = [g if g is not None else torch.zeros_like(t) for g, t in zip(gr, q + h + [lsq])]
    return gr[0], gr[1], gr[2], torch.cat([gr[3].reshape(1), gr[4].reshape(1), gr[5].reshape(1), gr[6]])


def _inputs(B, N, Ns, D, ard, seed=0, offset=0.0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + Ns + D)
    X = torch.randn(B, N, D, generator=g) / math.sqrt(D) + offset
    Xs = torch.randn(B, Ns, D, generator=g) / math.sqrt(D) + offset
    y = torch.randn(B, N, generator=g)
    ls = (0.5 + torch.rand(D, generator=g)) if ard else torch.tensor([LN2])
    gm, gv, gc = torch.randn(B, Ns, generator=g), torch.randn(B, Ns, generator=g), torch.randn(B, Ns, Ns, generator=g)
    return X, y, Xs, ls, gm, gv, gc


def _kernels(dev, X, y, Xs, ls, s2, c, noise, gm, gv, gc, jitter_ok=False):
    from fine_grained_gaussian_process_forcasting_amd import ops
    T = lambda t: None if t is None else t.to(dev)   # noqa: E731
    hyper = ops.pack_exact_hyper(s2, noise, c, torch.as_tensor(ls, dtype=torch.float32), dev)
    f = ops.exact_mll(T(X), T(y), None, None, None, None, want_L=True, want_z=True, hyper=hyper)
    p, state = ops.exact_posterior_cov(T(X), f.L, f.z, hyper, T(Xs), return_state=True)
    g = ops.exact_posterior_grad(T(X), f.L, f.z, hyper, T(Xs), state, T(gm), T(gv), T(gc))
    torch.cuda.synchronize()
    if not jitter_ok:
        assert int(f.info.abs().max()) == 0
    return g, f.info


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _errors(g, ref, per_window=True):
    """Norm-wise relative error per block; dX and dXs also per window (the worst is kept)."""
    dX, dy, dXs, dhyp = ref
    e = {"dX": _rel(g.dX, dX), "dy": _rel(g.dy, dy) if float(dy.norm()) > 0 else float(g.dy.abs().max()),
         "dXs": _rel(g.dXs, dXs), "dhyp": _rel(g.dhyp.sum(0), dhyp)}
    if per_window:
        for b in range(dX.shape[0]):
            e["dX"] = max(e["dX"], _rel(g.dX[b], dX[b]))
            e["dXs"] = max(e["dXs"], _rel(g.dXs[b], dXs[b]))
    return e


_SHAPES = [(2, 1, 1, 1, False), (2, 16, 16, 4, False), (3, 17, 5, 3, True), (2, 37, 65, 4, False),
           (2, 64, 130, 8, True), (2, 250, 41, 7, False), (1, 256, 256, 32, False), (1, 96, 64, 64, False),
           (71, 5, 8, 2, False)]


@pytest.mark.parametrize("B,N,Ns,D,ard", _SHAPES)
def test_posterior_grad_vs_fp64(cuda_device, B, N, Ns, D, ard):
    X, y, Xs, ls, gm, gv, gc = _inputs(B, N, Ns, D, ard)
    g, _ = _kernels(cuda_device, X, y, Xs, ls, S2, C0, NOISE, gm, gv, gc)
    e = _errors(g, _reference(X, y, Xs, ls, S2, C0, NOISE, gm, gv, gc))
    print(f"posterior_grad B={B} N={N} Ns={Ns} D={D} ard={ard}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for name, v in e.items():
        assert v <= 1e-4, (name, v)


def test_posterior_grad_largest_workgroup_memory(cuda_device):
    """N = Ns = 256 with D = 64: the K* kernel's dynamic LDS at its maximum (H / Q*, both inputs:
    156 KB of the CU's 160), which needs the opt-in above the default limit."""
    B, N, Ns, D = 1, 256, 256, 64
    X, y, Xs, ls, gm, gv, gc = _inputs(B, N, Ns, D, True, seed=6)
    g, _ = _kernels(cuda_device, X, y, Xs, ls, S2, C0, NOISE, gm, gv, gc)
    e = _errors(g, _reference(X, y, Xs, ls, S2, C0, NOISE, gm, gv, gc))
    print(f"posterior_grad B={B} N={N} Ns={Ns} D={D}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for name, v in e.items():
        assert v <= 1e-4, (name, v)


def test_posterior_grad_variants(cuda_device):
    """A non-symmetric gcov is the default; each gradient alone, the absent ones passed as NULL:
    against fp64, and equal to the all-present call with zeros at 1e-6. Inputs offset by +25."""
    B, N, Ns, D = 2, 37, 65, 4
    X, y, Xs, ls, gm, gv, gc = _inputs(B, N, Ns, D, False, seed=1)
    assert float((gc - gc.transpose(-1, -2)).abs().max()) > 0.1
    zm, zc = torch.zeros_like(gm), torch.zeros_like(gc)
    for name, sel, full in (("gmean", (gm, None, None), (gm, zm, zc)), ("gvar", (None, gv, None), (zm, gv, zc)),
                            ("gcov", (None, None, gc), (zm, zm, gc))):
        g, _ = _kernels(cuda_device, X, y, Xs, ls, S2, C0, NOISE, *sel)
        e = _errors(g, _reference(X, y, Xs, ls, S2, C0, NOISE, *sel))
        print(f"posterior_grad {name} only: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= 1e-4, (name, k, v)
        gz, _ = _kernels(cuda_device, X, y, Xs, ls, S2, C0, NOISE, *full)
        for k in ("dX", "dy", "dXs", "dhyp"):
            a, b = getattr(g, k), getattr(gz, k)
            assert float((a - b).norm()) <= 1e-6 * max(float(b.norm()), 1e-30), (name, k)
    Xo, yo, Xso, lso, gm, gv, gc = _inputs(B, N, Ns, D, True, seed=2, offset=25.0)
    g, _ = _kernels(cuda_device, Xo, yo, Xso, lso, S2, C0, NOISE, gm, gv, gc)
    e = _errors(g, _reference(Xo, yo, Xso, lso, S2, C0, NOISE, gm, gv, gc))
    print("posterior_grad offset +25: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= 1e-4, (k, v)


def test_posterior_grad_deterministic_and_per_window(cuda_device):
    """Two launches give the same bits; window b of a B = 3 call is bitwise the B = 1 call."""
    X, y, Xs, ls, gm, gv, gc = _inputs(3, 37, 65, 4, True, seed=3)
    g1, _ = _kernels(cuda_device, X, y, Xs, ls, S2, C0, NOISE, gm, gv, gc)
    g2, _ = _kernels(cuda_device, X, y, Xs, ls, S2, C0, NOISE, gm, gv, gc)
    for k in ("dX", "dy", "dXs", "dhyp"):
        assert torch.equal(getattr(g1, k), getattr(g2, k)), k
    for b in range(3):
        s = slice(b, b + 1)
        gb, _ = _kernels(cuda_device, X[s], y[s], Xs[s], ls, S2, C0, NOISE, gm[s], gv[s], gc[s])
        for k in ("dX", "dy", "dXs", "dhyp"):
            assert torch.equal(getattr(g1, k)[s], getattr(gb, k)), (k, b)


def _parent_route_fp32(dev, X, y, Xs, ls, s2, c, noise, gm, gv, gc):
    """The torch route (ExactGPModel._posterior_autograd, fp32 on the GPU) on leaf hyper-parameters."""
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    leaf = lambda v: torch.as_tensor(v, dtype=torch.float32).to(dev).clone().requires_grad_()   # noqa: E731
    Xl, yl, Xsl = leaf(X), leaf(y), leaf(Xs)
    s2l, nl, cl, lsl = leaf(s2), leaf(noise), leaf(c), leaf(ls)
    stub = types.SimpleNamespace(
        train_inputs=(Xl,), train_targets=yl,
        covar_module=types.SimpleNamespace(base_kernel=types.SimpleNamespace(lengthscale=lsl), outputscale=s2l),
        mean_module=types.SimpleNamespace(constant=cl), likelihood=types.SimpleNamespace(noise=nl))
    dist = ExactGPModel._posterior_autograd(stub, Xsl)
    obj = (gm.to(dev) * dist.mean).sum() + (gv.to(dev) * dist.variance).sum() + \
        (gc.to(dev) * dist.covariance_matrix).sum()
    dX, dy, dXs, ds2, dn, dc, dl = torch.autograd.grad(obj, [Xl, yl, Xsl, s2l, nl, cl, lsl])
    return types.SimpleNamespace(dX=dX, dy=dy, dXs=dXs,
                                 dhyp=torch.cat([ds2.reshape(1), dn.reshape(1), dc.reshape(1), dl.reshape(-1)])[None])


@pytest.mark.parametrize("noise", [1e-2, 1e-3])
def test_posterior_grad_ill_conditioned_vs_fp32_reference(cuda_device, noise):
    """noise 1e-2 / 1e-3 at N = 128: cond(K_hat) up to ~1e5, beyond what fp32 holds at 1e-4. Bound
    per block: max(1e-4, 3 x the error of the torch route in fp32 on the same GPU) against the same
    fp64 reference (the rule of test_exact_grad_ill_conditioned_vs_fp32_reference).
    Measured (kernels / torch fp32), worst block dhyp: 3.8e-6 / 9.6e-6 at 1e-2, 5.0e-5 / 4.2e-5 at
    1e-3; the other blocks <= 9.7e-6 on both routes."""
    B, N, Ns, D = 2, 128, 32, 8
    X, y, Xs, ls, gm, gv, gc = _inputs(B, N, Ns, D, False, seed=4)
    ref = _reference(X, y, Xs, ls, S2, C0, noise, gm, gv, gc)
    g, _ = _kernels(cuda_device, X, y, Xs, ls, S2, C0, noise, gm, gv, gc)
    e = _errors(g, ref, per_window=False)
    e32 = _errors(_parent_route_fp32(cuda_device, X, y, Xs, ls, S2, C0, noise, gm, gv, gc), ref, per_window=False)
    for k in e:
        print(f"ill-conditioned noise={noise:g} {k:5s}: kernels {e[k]:.2e}  torch fp32 {e32[k]:.2e}")
    for k in e:
        assert e[k] <= max(1e-4, 3.0 * e32[k]), (k, e[k], e32[k])


def test_posterior_grad_jitter_ladder(cuda_device):
    """Window 0 holds two identical training points with a noise that fp32 rounds away (s2 + noise
    == s2), so its second pivot is exactly 0 and the ladder adds 1e-6: info = -1. The gradients
    match the fp64 reference with the same jitter on the diagonal. Every coordinate is a small
    dyadic number, the training mean is 0 and l = 0.5, so the Gram entry of the pair is s2 exactly.
    s2 = 2^-14 keeps cond(K_hat + 1e-6 I) <= (8 s2 + 1e-6) / 1e-6 < 500, so the project's 1e-4 holds
    here too (an fp32 solve loses about cond x 2^-24 = 3e-5)."""
    s2, noise, ls = 2.0 ** -14, 1e-12, torch.tensor([0.5])
    pts = torch.tensor([[0., 0.], [0., 0.], [1., 0.], [-1., 0.], [0., 1.], [0., -1.], [1., 1.], [-1., -1.]])
    X = torch.stack([pts, pts.clone()])
    X[1, 1] = torch.tensor([1., -1.])
    X[1, 0] = torch.tensor([-1., 1.])           # window 1: eight distinct points
    g0 = torch.Generator().manual_seed(9)
    Xs = torch.randn(2, 5, 2, generator=g0) * 0.5
    y = torch.randn(2, 8, generator=g0) * 0.01
    gm, gv, gc = torch.randn(2, 5, generator=g0), torch.randn(2, 5, generator=g0), torch.randn(2, 5, 5, generator=g0)
    g, info = _kernels(cuda_device, X, y, Xs, ls, s2, C0, noise, gm, gv, gc, jitter_ok=True)
    info = info.cpu().tolist()
    assert info == [-1, 0], info
    for b, jit in ((0, 1e-6), (1, 0.0)):
        s = slice(b, b + 1)
        ref = _reference(X[s], y[s], Xs[s], ls, s2, C0, noise + jit, gm[s], gv[s], gc[s])
        gb = types.SimpleNamespace(dX=g.dX[s], dy=g.dy[s], dXs=g.dXs[s], dhyp=g.dhyp[s])
        e = _errors(gb, ref)
        print(f"jitter ladder window {b} (info {info[b]}): " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= 1e-4, (b, k, v)


def test_posterior_grad_opcheck(cuda_device):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = cuda_device
    X, y, Xs, ls, gm, gv, gc = (t.to(dev) for t in _inputs(2, 17, 5, 3, True, seed=5))
    hyper = ops.pack_exact_hyper(S2, NOISE, C0, ls, dev)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.gpk.exact_posterior_train.default,
                          (X.requires_grad_(), y.requires_grad_(), hyper.requires_grad_(), Xs.requires_grad_(),
                           1e-6, 3), test_utils=tests)
    mean, var, cov, L, z, state, info = torch.ops.gpk.exact_posterior_train(X.detach(), y.detach(),
                                                                            hyper.detach(), Xs.detach(), 1e-6, 3)
    torch.library.opcheck(torch.ops.gpk.exact_posterior_grad.default,
                          (X.detach(), L, z, hyper.detach(), Xs.detach(), state, gm, gv, gc), test_utils=tests)
    torch.library.opcheck(torch.ops.gpk.exact_posterior_grad.default,
                          (X.detach(), L, z, hyper.detach(), Xs.detach(), state, None, gv, None), test_utils=tests)


# ---- model level ------------------------------------------------------------------------------

def _model(dev, train_x, train_y):
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    from fine_grained_gaussian_process_forcasting_amd.gp import GaussianLikelihood
    lik = GaussianLikelihood().to(dev)
    model = ExactGPModel(train_x.to(dev), train_y.to(dev), lik).to(dev)
    with torch.no_grad():
        model.mean_module.constant.fill_(C0)
    model.eval()
    lik.eval()
    return model, lik


def _raw_params(model):
    return [model.covar_module.raw_outputscale, model.covar_module.base_kernel.raw_lengthscale,
            model.mean_module.constant, model.likelihood.noise_covar.raw_noise]


@pytest.mark.parametrize("batched", [False, True])
def test_model_values_and_gradients(cuda_device, batched):
    """ExactGPModel in eval with test_x.requires_grad_(): the values are the no_grad kernels' (1e-6
    relative), the gradients with respect to x and every raw parameter match fp64 at 1e-4."""
    dev = cuda_device
    g = torch.Generator().manual_seed(11)
    N, D, Ns = 40, 3, 21
    lead = (3,) if batched else ()
    train_x = torch.rand(*lead, N, D, generator=g)
    train_y = torch.sin(6.0 * train_x.sum(-1))
    test_x = torch.rand(*lead, Ns, D, generator=g)
    model, _ = _model(dev, train_x, train_y)
    with torch.no_grad():
        d0 = model(test_x.to(dev))
        m0, v0, c0 = d0.mean.clone(), d0.variance.clone(), d0.covariance_matrix.clone()
    xr = test_x.to(dev).clone().requires_grad_()
    dist = model(xr)
    for a, b in ((dist.mean, m0), (dist.variance, v0), (dist.covariance_matrix, c0)):
        assert a.shape == b.shape
        assert _rel(a, b) <= 1e-6
    gm, gv = torch.randn(*lead, Ns, generator=g), torch.randn(*lead, Ns, generator=g)
    gc = torch.randn(*lead, Ns, Ns, generator=g)
    params = [xr] + _raw_params(model)
    obj = (gm.to(dev) * dist.mean).sum() + (gv.to(dev) * dist.variance).sum() + \
        (gc.to(dev) * dist.covariance_matrix).sum()
    got = torch.autograd.grad(obj, params)
    q = [t.detach().cpu().double().clone().requires_grad_() for t in params]
    F = torch.nn.functional
    s2, ls = F.softplus(q[1]).reshape(()), F.softplus(q[2]).reshape(-1)
    c, noise = q[3].reshape(()), F.softplus(q[4]).reshape(()) + 1e-4
    mean, var, cov = _posterior_fp64(train_x.double(), train_y.double(), q[0], ls, s2, c, noise)
    var = var.clamp_min(1e-6)
    want = torch.autograd.grad((gm.double() * mean).sum() + (gv.double() * var).sum() + (gc.double() * cov).sum(), q)
    for name, a, b in zip(["x", "outputscale", "lengthscale", "constant", "noise"], got, want):
        e = _rel(a.reshape(b.shape), b)
        print(f"model grad batched={batched} {name:12s} {e:.2e}")
        assert e <= 1e-4, (name, e)


def test_model_backward_never_falls_back_to_torch(cuda_device, monkeypatch):
    """rsample(...).backward() and log_prob(y).backward() of the eval posterior under grad run on
    gpk_exact_posterior_cov_f32 / gpk_mvn_root_f32 and their adjoints: the torch route, torch's
    triangular solve and its Cholesky are patched to raise (log_prob's own whitening against the
    root is gpk_tri_solve_f32)."""
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    dev = cuda_device
    g = torch.Generator().manual_seed(12)
    N, D, Ns = 40, 3, 21
    train_x = torch.rand(N, D, generator=g)
    train_y = torch.sin(6.0 * train_x.sum(-1))
    model, _ = _model(dev, train_x, train_y)

    def boom(*a, **k):
        raise AssertionError("the differentiable posterior left the kernels")
    monkeypatch.setattr(ExactGPModel, "_posterior_autograd", boom)
    monkeypatch.setattr(torch.linalg, "solve_triangular", boom)
    monkeypatch.setattr(torch.linalg, "cholesky_ex", boom)

    def check(xr):
        for t in [xr] + _raw_params(model):
            assert t.grad is not None and bool(torch.isfinite(t.grad).all()), t
            assert float(t.grad.abs().max()) > 0
            t.grad = None

    xr = torch.rand(Ns, D, generator=g).to(dev).requires_grad_()
    torch.manual_seed(0)
    model(xr).rsample(torch.Size([2])).sum().backward()
    check(xr)
    yt = torch.randn(Ns, generator=g).to(dev)
    model(xr).log_prob(yt).backward()
    check(xr)


def test_model_range_boundary_keeps_the_torch_route(cuda_device, monkeypatch):
    """N = 300 is inside the forward's range and outside the adjoint's: _posterior_autograd."""
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    dev = cuda_device
    g = torch.Generator().manual_seed(13)
    train_x = torch.rand(300, 2, generator=g)
    model, _ = _model(dev, train_x, torch.sin(6.0 * train_x.sum(-1)))
    calls = []
    real = ExactGPModel._posterior_autograd
    monkeypatch.setattr(ExactGPModel, "_posterior_autograd", lambda self, x: (calls.append(1), real(self, x))[1])
    xr = torch.rand(9, 2, generator=g).to(dev).requires_grad_()
    model(xr).mean.sum().backward()
    assert calls == [1] and xr.grad is not None
    calls.clear()
    model2, _ = _model(dev, train_x[:256], torch.sin(6.0 * train_x[:256].sum(-1)))
    model2(xr).mean.sum().backward()
    assert calls == []
