"""Host-side checks of the adjoint of the exact-GP posterior (no GPU): the workspace query and
argument validation of gpk_exact_posterior_grad_f32, the FakeTensor shapes of
gpk::exact_posterior_train / gpk::exact_posterior_grad, the refusal of CPU tensors, and the
derivation itself: an fp64 torch restatement of the formulas the kernels implement (in the kernels'
own algebra: W, alpha, u, the three centred Grams with the diagonal apart, the row-sum forms)
against torch autograd of the dense posterior."""
import ctypes
import math

import pytest
import torch


def _lib():
    from fine_grained_gaussian_process_forcasting_amd import _native
    return _native.lib()


def test_workspace_query():
    q = _lib().gpk_exact_posterior_grad_workspace_bytes
    for B, N, Ns, D in [(2, 1, 1, 1), (3, 17, 5, 3), (2, 37, 65, 4), (512, 256, 256, 32), (1, 96, 64, 64),
                        (71, 5, 8, 2)]:
        n = q(B, N, Ns, D)
        stride = (Ns + 63) // 64 * 64
        assert n >= 2 * 4 * B * N * stride          # W and T, as the forward stores V
        assert n % 16 == 0
    assert q(0, 16, 16, 4) >= 0
    assert q(2, 257, 16, 4) == 0 and q(2, 16, 257, 4) == 0 and q(2, 16, 16, 65) == 0
    assert q(2, 0, 16, 4) == 0 and q(2, 16, 0, 4) == 0 and q(2, 16, 16, 0) == 0 and q(-1, 16, 16, 4) == 0
    assert q(2, 300, 16, 4) == 0 and q(2, 800, 16, 4) == 0   # the forward's blocked range: out of scope


def test_validation_without_device():
    lib = _lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation returns first
    #       X    L    z    hyp  nls Xs   state gm   gv   gc   B  N   Ns  D  ws   dX   dy   dXs  dhyp stream
    args = [one, one, one, one, 1, one, one, one, one, one, 2, 40, 16, 4, one, one, one, one, one, None]
    f = lib.gpk_exact_posterior_grad_f32
    for idx in (0, 1, 2, 3, 5, 6, 14, 18):
        bad = list(args); bad[idx] = None
        assert f(*bad) == -(idx + 1)
    for idx in (7, 8, 9, 15, 16, 17):        # each optional alone: accepted up to the next check
        ok = list(args); ok[idx] = None; ok[10] = 0
        assert f(*ok) == 0
    bad = list(args); bad[7] = bad[8] = bad[9] = None
    assert f(*bad) == -8                     # no incoming gradient at all
    for idx, val in [(4, 3), (10, -1), (11, 0), (11, 257), (12, 0), (12, 257), (13, 0), (13, 65),
                     (6, ctypes.c_void_p(8)), (14, ctypes.c_void_p(8))]:
        bad = list(args); bad[idx] = val
        assert f(*bad) == -(idx + 1)
    ok = list(args); ok[4] = 4               # n_lengthscale = D
    ok[10] = 0
    assert f(*ok) == 0                       # no windows: nothing launched


def test_fake_shapes_and_cpu_refusal():
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    B, N, Ns, D = 3, 20, 70, 4
    nstate = _lib().gpk_exact_posterior_cov_workspace_bytes(B, N, Ns) // 4
    with FakeTensorMode():
        X, y, Xs = torch.empty(B, N, D), torch.empty(B, N), torch.empty(B, Ns, D)
        for h in (torch.empty(4), torch.empty(3 + D)):
            mean, var, cov, L, z, state, info = torch.ops.gpk.exact_posterior_train(X, y, h, Xs, 1e-6, 3)
            assert mean.shape == (B, Ns) and var.shape == (B, Ns) and cov.shape == (B, Ns, Ns)
            assert L.shape == (B, N, N) and z.shape == (B, N) and state.shape == (nstate,)
            assert info.shape == (B,) and info.dtype == torch.int32
            dX, dy, dXs, dhyp = torch.ops.gpk.exact_posterior_grad(X, L, z, h, Xs, state, mean, None, cov)
            assert dX.shape == (B, N, D) and dy.shape == (B, N) and dXs.shape == (B, Ns, D)
            assert dhyp.shape == (B, h.numel())
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.exact_posterior_grad(torch.zeros(2, 8, 3), torch.zeros(2, 8, 8), torch.zeros(2, 8), torch.ones(4),
                                 torch.zeros(2, 5, 3), torch.zeros(2 * 8 * 64 + 128), torch.zeros(2, 5))
    with pytest.raises(ValueError, match="at least one"):
        ops.exact_posterior_grad(torch.zeros(2, 8, 3), torch.zeros(2, 8, 8), torch.zeros(2, 8), torch.ones(4),
                                 torch.zeros(2, 5, 3), torch.zeros(2 * 8 * 64 + 128))


def test_cpu_model_under_grad_still_raises():
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    from fine_grained_gaussian_process_forcasting_amd.gp import GaussianLikelihood
    model = ExactGPModel(torch.rand(8, 2), torch.rand(8), GaussianLikelihood())
    model.eval()
    x = torch.rand(3, 2).requires_grad_()
    assert not model._grad_on_kernels(x)
    with pytest.raises(ValueError, match="runs on the GPU"):
        model(x)


# ---- the derivation ---------------------------------------------------------------------------

def _dense_posterior(X, y, Xs, ls, s2, c, noise):
    d = (((X.unsqueeze(-2) - X.unsqueeze(-3)) / ls) ** 2).sum(-1)
    n = X.shape[-2]
    K = s2 * torch.exp(-0.5 * d) + noise * torch.eye(n, dtype=X.dtype)
    L = torch.linalg.cholesky(K)
    ds = (((X.unsqueeze(-2) - Xs.unsqueeze(-3)) / ls) ** 2).sum(-1)
    dss = (((Xs.unsqueeze(-2) - Xs.unsqueeze(-3)) / ls) ** 2).sum(-1)
    V = torch.linalg.solve_triangular(L, s2 * torch.exp(-0.5 * ds), upper=False)
    z = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False)
    mean = c + (V * z).sum(-2)
    cov = s2 * torch.exp(-0.5 * dss) - V.transpose(-1, -2) @ V
    return mean, torch.diagonal(cov, dim1=-2, dim2=-1), cov, L, z.squeeze(-1), V


def _block(dK, a, b, s2, square):
    """Q = dK o K for K = s2 E(a, b) by the centred Gram; da, db in the row-sum forms; sum Q."""
    na, nb = (a * a).sum(-1), (b * b).sum(-1)
    d2 = (na.unsqueeze(-1) + nb.unsqueeze(-2) - 2.0 * a @ b.transpose(-1, -2)).clamp_min(0.0)
    Q = dK * s2 * torch.exp(-0.5 * d2)
    if square:   # the diagonal apart: K_ii is s2 (+ noise) exactly and gives no dX
        Q = Q - torch.diag_embed(torch.diagonal(Q, dim1=-2, dim2=-1))
    da = Q @ b - Q.sum(-1, keepdim=True) * a
    db = Q.transpose(-1, -2) @ a - Q.sum(-2).unsqueeze(-1) * b
    return da, db, Q.sum((-1, -2))


def posterior_grad_algebra(X, y, Xs, ls, s2, c, noise, gmean=None, gvar=None, gcov=None):
    """The formulas of gpk_exact_posterior_grad_f32 in the dtype of the inputs, in the kernels'
    order of operations. -> (dX, dy, dXs, dhyp (B, 3 + n_ls))."""
    B, N, D = X.shape
    Ns = Xs.shape[1]
    with torch.no_grad():
        _, _, _, L, z, V = _dense_posterior(X, y, Xs, ls, s2, c, noise)
        W = torch.linalg.solve_triangular(L.transpose(-1, -2), V, upper=True)
        alpha = torch.linalg.solve_triangular(L.transpose(-1, -2), z.unsqueeze(-1), upper=True).squeeze(-1)
        G = torch.zeros(B, Ns, Ns, dtype=X.dtype)
        if gcov is not None:
            G = G + gcov
        if gvar is not None:
            G = G + torch.diag_embed(gvar)
        H = G + G.transpose(-1, -2)
        gm = gmean if gmean is not None else torch.zeros(B, Ns, dtype=X.dtype)
        u = (W @ gm.unsqueeze(-1)).squeeze(-1)
        T = W @ H
        dKs = -T + alpha.unsqueeze(-1) * gm.unsqueeze(-2)
        ua = u.unsqueeze(-1) * alpha.unsqueeze(-2)
        dKh = 0.5 * T @ W.transpose(-1, -2) - 0.5 * (ua + ua.transpose(-1, -2))
        dKss = 0.5 * H
        mu = (X / ls).mean(-2, keepdim=True)        # the forward's centring: the training mean of x / l
        a, bs = X / ls - mu, Xs / ls - mu
        da_s, db_s, q_s = _block(dKs, a, bs, s2, False)
        da_h, db_h, q_h = _block(dKh, a, a, s2, True)
        da_ss, db_ss, q_ss = _block(dKss, bs, bs, s2, True)
        da = da_s + da_h + db_h
        db = db_s + da_ss + db_ss
        tr_h = torch.diagonal(dKh, dim1=-2, dim2=-1).sum(-1)
        tr_ss = torch.diagonal(dKss, dim1=-2, dim2=-1).sum(-1)
        dl = -((a * da).sum(-2) + (bs * db).sum(-2)) / ls
        if torch.as_tensor(ls).numel() == 1:
            dl = dl.sum(-1, keepdim=True)
        ds2 = (q_s + q_h + q_ss) / s2 + tr_h + tr_ss
        dc = gm.sum(-1) - u.sum(-1)
        dhyp = torch.cat([ds2.unsqueeze(-1), tr_h.unsqueeze(-1), dc.unsqueeze(-1), dl], -1)
        return da / ls, u, db / ls, dhyp


def _case(B, N, Ns, D, ard, offset=0.0, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * N + Ns)
    X = torch.randn(B, N, D, generator=g, dtype=torch.float64) / math.sqrt(D) + offset
    Xs = torch.randn(B, Ns, D, generator=g, dtype=torch.float64) / math.sqrt(D) + offset
    y = torch.randn(B, N, generator=g, dtype=torch.float64)
    ls = (0.5 + torch.rand(D, generator=g, dtype=torch.float64)) if ard else torch.tensor([math.log(2.0)],
                                                                                          dtype=torch.float64)
    gm = torch.randn(B, Ns, generator=g, dtype=torch.float64)
    gv = torch.randn(B, Ns, generator=g, dtype=torch.float64)
    gc = torch.randn(B, Ns, Ns, generator=g, dtype=torch.float64)
    return X, y, Xs, ls, gm, gv, gc


def _autograd(X, y, Xs, ls, s2, c, noise, gm, gv, gc):
    q = [t.clone().requires_grad_() for t in (X, y, Xs, s2, noise, c, ls)]
    mean, var, cov, *_ = _dense_posterior(q[0], q[1], q[2], q[6], q[3], q[5], q[4])
    obj = 0.0
    if gm is not None:
        obj = obj + (gm * mean).sum()
    if gv is not None:
        obj = obj + (gv * var).sum()
    if gc is not None:
        obj = obj + (gc * cov).sum()
    gr = torch.autograd.grad(obj, q, allow_unused=True)   # without gmean, y and c are not reached
    dX, dy, dXs, ds2, dn, dc, dl = (g if g is not None else torch.zeros_like(t) for g, t in zip(gr, q))
    return dX, dy, dXs, torch.cat([ds2.reshape(1), dn.reshape(1), dc.reshape(1), dl.reshape(-1)])


def _check(case, gm, gv, gc, bound=1e-10):
    X, y, Xs, ls = case
    s2 = torch.tensor(math.log(2.0), dtype=torch.float64)
    noise = torch.tensor(math.log(2.0) + 1e-4, dtype=torch.float64)
    c = torch.tensor(0.1, dtype=torch.float64)
    dX, dy, dXs, dhyp = posterior_grad_algebra(X, y, Xs, ls, s2, c, noise, gm, gv, gc)
    want = _autograd(X, y, Xs, ls, s2, c, noise, gm, gv, gc)
    worst = 0.0
    for name, a, b in zip(("dX", "dy", "dXs", "dhyp"), (dX, dy, dXs, dhyp.sum(0)), want):
        e = float((a - b).norm() / b.norm().clamp_min(1e-300))
        if float(b.norm()) == 0.0:
            e = float((a - b).norm())
        worst = max(worst, e)
        assert e <= bound, (name, e)
    return worst


@pytest.mark.parametrize("B,N,Ns,D,ard,offset", [(2, 1, 1, 1, False, 0.0), (2, 17, 5, 3, True, 0.0),
                                                 (3, 37, 41, 4, False, 0.0), (2, 16, 70, 2, False, 0.0),
                                                 (1, 64, 20, 3, False, 25.0)])
def test_algebra_against_fp64_autograd(B, N, Ns, D, ard, offset):
    X, y, Xs, ls, gm, gv, gc = _case(B, N, Ns, D, ard, offset)
    worst = _check((X, y, Xs, ls), gm, gv, gc)           # gc is not symmetric
    print(f"algebra B={B} N={N} Ns={Ns} D={D} offset={offset}: {worst:.2e}")


def test_algebra_single_gradients_and_symmetric_gcov():
    X, y, Xs, ls, gm, gv, gc = _case(2, 16, 70, 2, True)
    _check((X, y, Xs, ls), gm, None, None)
    _check((X, y, Xs, ls), None, gv, None)
    _check((X, y, Xs, ls), None, None, gc)
    _check((X, y, Xs, ls), gm, gv, 0.5 * (gc + gc.transpose(-1, -2)))
