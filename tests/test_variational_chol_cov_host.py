"""CPU: the dense covariance of a Cholesky q(u) layer -- the adjoint algebra the kernels implement
restated in fp64 torch against fp64 autograd of gp.variational_chol_dense_covariance, the bound
symbols and registered ops, the size queries, the argument validation that returns before any HIP
call (no device is touched, nothing is launched), and the torch route a CPU layer still takes."""
import ctypes
import math

import pytest
import torch

NEW_SYMBOLS = ("gpk_variational_chol_cov_workspace_bytes", "gpk_variational_chol_cov_f32",
               "gpk_variational_chol_cov_batched_workspace_bytes", "gpk_variational_chol_cov_batched_f32",
               "gpk_variational_chol_cov_grad_workspace_bytes", "gpk_variational_chol_cov_grad_f32",
               "gpk_variational_chol_cov_grad_batched_workspace_bytes",
               "gpk_variational_chol_cov_grad_batched_f32")
JIT = 1e-4


def _case(B, N, M, D, seed, identity=False):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, N, D, generator=g, dtype=torch.float64) / math.sqrt(D)
    Z = torch.randn(M, D, generator=g, dtype=torch.float64) / math.sqrt(D)
    ls = torch.rand(D, generator=g, dtype=torch.float64) * 0.5 + 0.6
    s2 = torch.tensor(1.3, dtype=torch.float64)
    if identity:
        C = torch.eye(M, dtype=torch.float64)
    else:
        C = torch.diag(0.5 + torch.rand(M, generator=g, dtype=torch.float64)) + \
            torch.tril(0.3 * torch.randn(M, M, generator=g, dtype=torch.float64) / math.sqrt(M), -1)
        C[M // 2, M // 2] *= -1.0                                                   # a negative diagonal entry
        C = C + torch.triu(torch.randn(M, M, generator=g, dtype=torch.float64), 1)  # junk above the diagonal
    zs = Z / ls
    K = s2 * torch.exp(-0.5 * (zs[:, None] - zs[None]).pow(2).sum(-1)) + JIT * torch.eye(M, dtype=torch.float64)
    Linv = torch.linalg.solve_triangular(torch.linalg.cholesky(K), torch.eye(M, dtype=torch.float64), upper=False)
    gc = torch.randn(B, N, N, generator=g, dtype=torch.float64)                     # not symmetric
    return X, Z, Linv, C, s2, ls, gc


def _kzx(X, Z, s2, ls):
    zs, xs = Z / ls, X / ls
    d = (zs.pow(2).sum(-1)[:, None] + xs.pow(2).sum(-1).unsqueeze(-2) - 2.0 * zs @ xs.mT).clamp_min(0.0)
    return s2 * torch.exp(-0.5 * d)


def _rel(a, b):
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


@pytest.mark.parametrize("B,N,M,D,identity", [(3, 17, 12, 4, False), (2, 1, 8, 3, False), (2, 9, 6, 1, False),
                                              (2, 9, 6, 3, True)])
def test_adjoint_algebra_against_autograd(B, N, M, D, identity):
    """T_W = W H, T_A = A H, dA = L_q T_W - T_A, dC = tril(sum_b A T_W^T) (no factor 2),
    dLinv = tril(sum_b dA K_ZX^T); diag(cov) is the unclamped marginal variance."""
    from fine_grained_gaussian_process_forcasting_amd import gp
    X, Z, Linv, C, s2, ls, gc = _case(B, N, M, D, seed=3 * N + M, identity=identity)
    li, c = Linv.clone().requires_grad_(), C.clone().requires_grad_()
    cov = gp.variational_chol_dense_covariance(X, Z, li, c, s2, ls, JIT)
    (cov * gc).sum().backward()
    assert int(torch.count_nonzero(torch.triu(c.grad, 1))) == 0      # exactly 0 above the diagonal

    K = _kzx(X, Z, s2, ls)
    A = Linv @ K
    Lq = torch.tril(C)
    W = Lq.mT @ A
    H = gc + gc.mT
    TW, TA = W @ H, A @ H
    dA = Lq @ TW - TA
    dC = torch.tril((A @ TW.mT).sum(0))
    dLinv = torch.tril((dA @ K.mT).sum(0))
    # dA itself, with A as the leaf of the product term
    a = A.clone().requires_grad_()
    w = Lq.mT @ a
    ((w.mT @ w - a.mT @ a) * gc).sum().backward()
    assert _rel(dC, c.grad) <= 1e-12
    if identity:      # L_q = I: W = A, the product term vanishes, nothing flows to A
        assert float(dA.abs().max()) <= 1e-12 and float(a.grad.abs().max()) <= 1e-12
        assert float(torch.tril(li.grad).abs().max()) <= 1e-10
    else:
        assert _rel(dA, a.grad) <= 1e-12
        assert _rel(dLinv, torch.tril(li.grad)) <= 1e-12
    # one weighted SYRK over the stacked panel gives the product term
    S = torch.cat([W, A], dim=-2)
    sign = torch.cat([torch.ones(M), -torch.ones(M)]).double()
    assert torch.allclose(S.mT @ (sign[:, None] * S), W.mT @ W - A.mT @ A, rtol=0, atol=1e-13)
    _, var = gp.variational_chol_predict(X, Z, Linv, torch.zeros(M, dtype=torch.float64), C, s2, ls, None, 0.0, JIT)
    assert torch.allclose(cov.detach().diagonal(dim1=-2, dim2=-1), var, rtol=0, atol=1e-13)


def test_diagonal_lq_is_the_mean_field_covariance():
    from fine_grained_gaussian_process_forcasting_amd import gp
    X, Z, Linv, C, s2, ls, gc = _case(2, 9, 6, 3, seed=5)
    s = C.diagonal().clone()
    a = gp.variational_chol_dense_covariance(X, Z, Linv, torch.diag(s), s2, ls, JIT)
    b = gp.variational_dense_covariance(X, Z, Linv, s, s2, ls, JIT)
    assert torch.allclose(a, b, rtol=0, atol=1e-13)


def test_new_symbols_bound_and_ops_registered():
    from fine_grained_gaussian_process_forcasting_amd import _native, gp, ops
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    lib = _native.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _native.SIGNATURES, n
    for n in ("variational_chol_cov", "variational_chol_cov_grad"):
        assert hasattr(ops, n), n
    for n in ("_variational_chol_cov_on_kernels", "_variational_chol_cov_grad_on_kernels"):
        assert hasattr(gp, n), n
    for n in ("variational_chol_cov", "variational_chol_cov_train", "variational_chol_cov_grad"):
        assert hasattr(torch.ops.gpk, n), n
    with FakeTensorMode():
        O, B, N, M, D = 3, 2, 70, 20, 4
        for lead, xs in (((), [(B, N, D)]), ((O,), [(B, N, D), (O, B, N, D)])):
            Z, Linv = torch.empty(*lead, M, D), torch.empty(*lead, M, M, dtype=torch.float64)
            vc, hyp = torch.empty(*lead, M, M), torch.empty(*lead, 4 + 2 * D)
            s2, ls = torch.empty(lead), torch.empty(*lead, D)
            for xshape in xs:
                X = torch.empty(*xshape)
                cov = torch.ops.gpk.variational_chol_cov(X, Linv, Z, vc, hyp)
                assert cov.shape == (*lead, B, N, N) and cov.dtype == torch.float32
                cov, hy, state = torch.ops.gpk.variational_chol_cov_train(X, Linv, Z, vc, s2, ls, JIT)
                assert cov.shape == (*lead, B, N, N) and hy.shape == (*lead, 4 + 2 * D)
                assert state.numel() == max(1, len(lead) and O) * (B * 2 * M * 128 + B * 64)
                assert state.dtype == torch.float32
                dX, dL, dZ, dpar, dC = torch.ops.gpk.variational_chol_cov_grad(X, Linv, Z, vc, hy, state, cov)
                assert dX.shape == (*lead, B, N, D) and dL.shape == (*lead, M, M) and dL.dtype == torch.float64
                assert dZ.shape == (*lead, M, D) and dpar.shape == (*lead, 1 + D) and dC.shape == (*lead, M, M)
                assert dC.dtype == torch.float32


def test_queries():
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    f1, fb = lib.gpk_variational_chol_cov_workspace_bytes, lib.gpk_variational_chol_cov_batched_workspace_bytes
    g1 = lib.gpk_variational_chol_cov_grad_workspace_bytes
    gb = lib.gpk_variational_chol_cov_grad_batched_workspace_bytes
    shapes = ((3, 20, 8, 4), (2, 70, 20, 5), (33, 24, 12, 6), (71, 5, 8, 2), (2, 40, 256, 32),
              (256, 192, 256, 32), (1024, 256, 64, 32), (1, 256, 256, 64))
    for B, N, M, D in shapes:
        asz = (N + 63) // 64 * 64
        assert f1(B, N, M) == (2 * B * M * asz + 64 * B) * 4
        one = g1(B, N, M, D)
        # the shared pipeline's plan, T over the stacked rows, the dchol partials
        assert one > lib.gpk_variational_cov_grad_workspace_bytes(B, N, M, D) + 2 * B * M * asz * 4
        assert one % 16 == 0
        for O in (1, 2, 3, 65535):
            assert fb(O, B, N, M) == O * f1(B, N, M) and gb(O, B, N, M, D) == O * one
    for O in (0, -1, 65536):
        assert fb(O, 4, 192, 64) == 0 and gb(O, 4, 192, 64, 32) == 0
    assert f1(4, 192, 257) == 0 and fb(2, 4, 192, 257) == 0
    assert g1(4, 192, 257, 32) == 0 and gb(2, 4, 192, 257, 32) == 0
    assert g1(4, 192, 256, 65) == 0 and gb(2, 4, 192, 256, 65) == 0
    assert g1(4, 257, 64, 32) == 0 and gb(2, 4, 257, 64, 32) == 0      # N > 256: the shared pipeline
    assert f1(4, 257, 64) > 0                                           # the forward serves it


def test_entry_validation_without_device():
    """Only cases the shim refuses before its first HIP call."""
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation returns first
    # forward: X Z Linv vchol hyp | B N M D | workspace cov stream
    args = [one] * 5 + [2, 16, 8, 4] + [one, one, None]
    fwd = lib.gpk_variational_chol_cov_f32
    for idx in (0, 1, 2, 3, 4, 9, 10):
        bad = list(args); bad[idx] = None
        assert fwd(*bad) == -(idx + 1), idx
    for idx, val in ((5, -1), (6, 0), (7, 0), (7, 257), (8, 0), (8, 65)):
        bad = list(args); bad[idx] = val
        assert fwd(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[9] = ctypes.c_void_p(8)
    assert fwd(*bad) == -10
    bad = list(args); bad[5] = 0
    assert fwd(*bad) == 0                                # no windows: nothing launched
    # batched forward: X shared Z Linv vchol hyp | O B N M D | workspace cov stream
    args = [one, 1] + [one] * 4 + [2, 2, 16, 8, 4] + [one, one, None]
    fwd = lib.gpk_variational_chol_cov_batched_f32
    for idx in (0, 2, 3, 4, 5, 11, 12):
        bad = list(args); bad[idx] = None
        assert fwd(*bad) == -(idx + 1), idx
    for idx, val in ((6, 0), (6, 65536), (7, -1), (8, 0), (9, 0), (9, 257), (10, 0), (10, 65)):
        bad = list(args); bad[idx] = val
        assert fwd(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[11] = ctypes.c_void_p(8)
    assert fwd(*bad) == -12
    bad = list(args); bad[7] = 0
    assert fwd(*bad) == 0
    # adjoint: X Z Linv vchol hyp state gcov | B N M D | workspace dX dLinv dZ dpar dchol stream
    args = [one] * 7 + [2, 16, 8, 4] + [one] * 6 + [None]
    adj = lib.gpk_variational_chol_cov_grad_f32
    for idx in (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16):
        bad = list(args); bad[idx] = None
        assert adj(*bad) == -(idx + 1), idx
    for idx, val in ((7, -1), (8, 0), (8, 257), (9, 0), (9, 257), (10, 0), (10, 65)):
        bad = list(args); bad[idx] = val
        assert adj(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[5] = ctypes.c_void_p(8)
    assert adj(*bad) == -6
    bad = list(args); bad[11] = ctypes.c_void_p(8)
    assert adj(*bad) == -12
    bad = list(args); bad[7] = 0
    assert adj(*bad) == 0
    # batched adjoint: X shared Z Linv vchol hyp state gcov | O B N M D | ws dX dLinv dZ dpar dchol stream
    args = [one, 0] + [one] * 6 + [2, 2, 16, 8, 4] + [one] * 6 + [None]
    adj = lib.gpk_variational_chol_cov_grad_batched_f32
    for idx in (0, 2, 3, 4, 5, 6, 7, 13, 14, 15, 16, 17, 18):
        bad = list(args); bad[idx] = None
        assert adj(*bad) == -(idx + 1), idx
    for idx, val in ((8, 0), (8, 65536), (9, -1), (10, 0), (10, 257), (11, 0), (11, 257), (12, 0), (12, 65)):
        bad = list(args); bad[idx] = val
        assert adj(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[6] = ctypes.c_void_p(8)
    assert adj(*bad) == -7
    bad = list(args); bad[13] = ctypes.c_void_p(8)
    assert adj(*bad) == -14
    bad = list(args); bad[9] = 0
    assert adj(*bad) == 0


@pytest.mark.parametrize("O", [None, 2])
def test_cpu_layer_covariance_takes_the_torch_function(monkeypatch, O):
    """CPU tensors: covariance_matrix of a Cholesky layer is gp.variational_chol_dense_covariance,
    once per output, and the predicates never reach their workspace queries (the CUDA-only K_ZZ
    factor op is replaced by its torch restatement)."""
    from fine_grained_gaussian_process_forcasting_amd import _native, gp, settings
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.DeepGP import ToyDeepGPHiddenLayer
    D, M = 5, 12
    n_out = 1 if O is None else O
    batch = torch.Size([]) if O is None else torch.Size([O])
    layer = ToyDeepGPHiddenLayer(D, O, 7, num_inducing=M)
    q = gp.CholeskyVariationalDistribution(M, batch)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        q.variational_mean.copy_(0.5 * torch.randn(*batch, M, generator=g))
        q.chol_variational_covar.copy_(torch.diag_embed(0.5 + torch.rand(*batch, M, generator=g)) +
                                       torch.tril(0.3 * torch.randn(*batch, M, M, generator=g) / math.sqrt(M), -1))
    vs = layer.variational_strategy
    vs._variational_distribution = q
    vs.variational_params_initialized.fill_(1)
    vs._initialized = True
    x = torch.randn(4, 30, D, generator=g) / math.sqrt(D)
    calls = []
    real = gp.variational_chol_dense_covariance
    monkeypatch.setattr(gp, "variational_chol_dense_covariance", lambda *a: (calls.append(1), real(*a))[1])

    def refuse(*a, **k):
        raise AssertionError("the kernels' library is not asked for CPU tensors")
    monkeypatch.setattr(_native, "lib", refuse)

    def torch_factor(Zf, s2f, lsf, jitter, key_tensors):
        Zf, s2f, lsf = Zf.reshape(n_out, M, D), s2f.reshape(n_out), lsf.reshape(n_out, -1)
        zs = (Zf / lsf[:, None, :]).double()
        K = s2f.double()[:, None, None] * torch.exp(-0.5 * (zs[:, :, None] - zs[:, None]).pow(2).sum(-1)) + \
            jitter * torch.eye(M, dtype=torch.float64)
        Li = torch.linalg.solve_triangular(torch.linalg.cholesky(K),
                                           torch.eye(M, dtype=torch.float64).expand(n_out, M, M), upper=False)
        return Li[0] if O is None else Li
    monkeypatch.setattr(vs._kzz_cache, "factor", torch_factor)
    for grad in (False, True):
        del calls[:]
        with torch.set_grad_enabled(grad), settings.num_likelihood_samples(1):
            out = layer(x)
            base = out if O is None else out._base
            cov = base.covariance_matrix
        assert len(calls) == n_out
        assert cov.shape[-2:] == (30, 30) and cov.requires_grad == grad
        assert torch.allclose(cov.diagonal(dim1=-2, dim2=-1), base.variance, rtol=1e-4, atol=1e-5)
