"""CPU: the batched (multi-output) Cholesky q(u) entry points -- the two size queries against the
single-output ones, the bound symbols, the argument validation that returns before any HIP call
(no device is touched, nothing is launched), and the torch loop a multi-output Cholesky layer
still runs on CPU tensors."""
import ctypes

import numpy as np
import torch

NEW_SYMBOLS = ("gpk_variational_chol_batched_saved_bytes", "gpk_variational_chol_batched_f32",
               "gpk_variational_chol_adjoint_batched_workspace_bytes",
               "gpk_variational_chol_adjoint_batched_f32", "gpk_cholesky_kl_batched_f32")


def test_batched_queries_are_o_slices_of_the_single_output_ones():
    from fine_grained_gaussian_process_forcasting_amd import _native, ops
    lib = _native.lib()
    pairs = ((lib.gpk_variational_chol_batched_saved_bytes, lib.gpk_variational_chol_saved_bytes, False),
             (lib.gpk_variational_chol_adjoint_batched_workspace_bytes,
              lib.gpk_variational_chol_adjoint_workspace_bytes, True))
    shapes = ((3, 20, 8, 4), (2, 70, 20, 5), (33, 24, 12, 6), (70, 16, 16, 4), (2, 40, 100, 40), (2, 40, 256, 32),
              (256, 192, 256, 32), (1024, 256, 64, 32), (1, 256, 256, 64))
    for qb, q1, adjoint in pairs:
        for shape in shapes:
            one = q1(*shape)
            assert one > 0, shape
            for O in (1, 2, 3, 4, 65535):
                assert qb(O, *shape) == O * one, (O, shape)
                assert ops.variational_chol_batched_supported(O, *shape, adjoint=adjoint)
        for O in (0, -1, 65536):
            assert qb(O, 4, 192, 64, 32) == 0, O
        assert qb(2, 4, 192, 257, 32) == 0
        assert qb(2, 4, 192, 256, 65) == 0
        assert qb(2, 0, 192, 256, 32) == 0
        assert not ops.variational_chol_batched_supported(2, 4, 192, 257, 32, adjoint=adjoint)
        assert not ops.variational_chol_batched_supported(0, 4, 192, 64, 32, adjoint=adjoint)
    # N > 256: the forward serves it, the adjoint (the shared pipeline) does not
    assert lib.gpk_variational_chol_adjoint_batched_workspace_bytes(2, 4, 257, 64, 32) == 0
    assert lib.gpk_variational_chol_batched_saved_bytes(2, 4, 257, 64, 32) == \
        2 * lib.gpk_variational_chol_saved_bytes(4, 257, 64, 32)
    assert ops.variational_chol_batched_supported(2, 4, 257, 64, 32)
    assert not ops.variational_chol_batched_supported(2, 4, 257, 64, 32, adjoint=True)


def test_new_symbols_bound_and_ops_registered():
    from fine_grained_gaussian_process_forcasting_amd import _native, ops, ops_autograd
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    lib = _native.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _native.SIGNATURES, n
    for n in ("variational_chol_forward_batched", "variational_chol_adjoint_batched", "cholesky_kl_batched",
              "cholesky_kl_grad_batched", "variational_chol_batched_supported"):
        assert hasattr(ops, n), n
    assert hasattr(ops_autograd, "variational_predict_chol_batched")
    for n in ("variational_chol_fwd", "variational_chol_adj", "cholesky_kl", "cholesky_kl_grad"):
        assert hasattr(torch.ops.gpk, n), n
    with FakeTensorMode():
        O, B, N, M, D = 3, 2, 70, 20, 4
        Z, Linv = torch.empty(O, M, D), torch.empty(O, M, M, dtype=torch.float64)
        vm, vc = torch.empty(O, M), torch.empty(O, M, M)
        for X in (torch.empty(B, N, D), torch.empty(O, B, N, D)):
            mean, var, flags, hyp, saved = torch.ops.gpk.variational_chol_fwd(
                X, Linv, Z, vm, vc, torch.empty(O), torch.empty(O, D), torch.empty(D), torch.empty(1), 1e-4, True)
            assert mean.shape == (O, B, N) and var.shape == (O, B, N) and flags.dtype == torch.int32
            assert hyp.shape == (O, 4 + 2 * D) and saved.numel() == O * (B * M * 128 + B * 128)
            dX, dL, dZ, dpar, dC = torch.ops.gpk.variational_chol_adj(X, Linv, Z, vm, vc, hyp, mean, var,
                                                                              saved)
            assert dX.shape == (O, B, N, D) and dL.shape == (O, M, M) and dL.dtype == torch.float64
            assert dZ.shape == (O, M, D) and dpar.shape == (O, M + 2 * D + 2) and dC.shape == (O, M, M)
        out = torch.ops.gpk.variational_chol_fwd(X, Linv, Z, vm, vc, torch.empty(O), torch.empty(O, D),
                                                         torch.empty(D), torch.empty(1), 1e-4)
        assert out[4].numel() == 0
        assert torch.ops.gpk.cholesky_kl(vm, vc).shape == (O,)
        dm, dC = torch.ops.gpk.cholesky_kl_grad(vm, vc, torch.empty(O))
        assert dm.shape == (O, M) and dC.shape == (O, M, M)


def test_entry_validation_without_device():
    """Only cases the shim refuses before its first HIP call."""
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation returns first
    # forward: X shared Z Linv vmean vchol hyp | O B N M D | mean var flags saved stream
    args = [one, 1] + [one] * 5 + [2, 2, 16, 8, 4] + [one, one, None, None, None]
    fwd = lib.gpk_variational_chol_batched_f32
    for idx in (0, 2, 3, 4, 5, 6, 12, 13):
        bad = list(args); bad[idx] = None
        assert fwd(*bad) == -(idx + 1), idx
    for idx, val in ((7, 0), (7, 65536), (8, -1), (9, 0), (10, 0), (10, 257), (11, 0), (11, 65)):
        bad = list(args); bad[idx] = val
        assert fwd(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[15] = ctypes.c_void_p(8)       # saved not 16-byte aligned
    assert fwd(*bad) == -16
    bad = list(args); bad[15] = one; bad[8] = 0          # saved at a shape whose saved size is 0
    assert fwd(*bad) == -16
    bad = list(args); bad[15] = one; bad[8] = 1 << 30; bad[9] = 65     # B ceil(N / 64) past the grid
    assert fwd(*bad) == -16
    bad = list(args); bad[8] = 0
    assert fwd(*bad) == 0                                # no windows: nothing launched
    # adjoint: X shared Z Linv vmean vchol hyp gmean gvar saved | O B N M D | ws dX dLinv dZ dpar dchol stream
    args = [one, 0] + [one] * 8 + [2, 2, 16, 8, 4] + [one] * 6 + [None]
    adj = lib.gpk_variational_chol_adjoint_batched_f32
    for idx in (0, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 18, 19, 20):
        bad = list(args); bad[idx] = None
        assert adj(*bad) == -(idx + 1), idx
    for idx, val in ((10, 0), (10, 65536), (11, -1), (12, 0), (12, 257), (13, 0), (13, 257), (14, 0), (14, 65)):
        bad = list(args); bad[idx] = val
        assert adj(*bad) == -(idx + 1), (idx, val)
    bad = list(args); bad[9] = ctypes.c_void_p(8)
    assert adj(*bad) == -10
    bad = list(args); bad[15] = ctypes.c_void_p(8)
    assert adj(*bad) == -16
    bad = list(args); bad[11] = 0
    assert adj(*bad) == 0
    # KL: m chol O M kl gkl dm dchol stream
    kl = lib.gpk_cholesky_kl_batched_f32
    assert kl(None, one, 2, 4, one, None, None, None, None) == -1
    assert kl(one, None, 2, 4, one, None, None, None, None) == -2
    assert kl(one, one, 0, 4, one, None, None, None, None) == -3
    assert kl(one, one, 65536, 4, one, None, None, None, None) == -3
    assert kl(one, one, 2, 0, one, None, None, None, None) == -4
    assert kl(one, one, 2, 4, None, None, None, None, None) == -5
    assert kl(one, one, 2, 4, None, one, None, one, None) == -7
    assert kl(one, one, 2, 4, None, one, one, None, None) == -8


def test_cpu_layer_still_runs_the_torch_loop(monkeypatch):
    """CPU tensors: a three-output Cholesky layer evaluates one gp.variational_chol_predict per
    output and the closed-form KL, never asks the kernels, and equals the per-output restatement
    (the CUDA-only K_ZZ factor op is replaced by its torch restatement)."""
    from fine_grained_gaussian_process_forcasting_amd import gp, ops, settings
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.DeepGP import ToyDeepGPHiddenLayer
    D, M, O = 5, 12, 3
    layer = ToyDeepGPHiddenLayer(D, O, 7, num_inducing=M)
    q = gp.CholeskyVariationalDistribution(M, torch.Size([O]))
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        q.variational_mean.copy_(0.5 * torch.randn(O, M, generator=g))
        q.chol_variational_covar.copy_(torch.diag_embed(0.5 + torch.rand(O, M, generator=g)) +
                                       torch.tril(0.3 * torch.randn(O, M, M, generator=g) / np.sqrt(M), -1))
    vs = layer.variational_strategy
    vs._variational_distribution = q
    vs.variational_params_initialized.fill_(1)
    vs._initialized = True
    x = torch.randn(4, 30, D, generator=g) / np.sqrt(D)
    calls = []
    real = gp.variational_chol_predict
    monkeypatch.setattr(gp, "variational_chol_predict", lambda *a: (calls.append(1), real(*a))[1])

    def refuse(*a, **k):
        raise AssertionError("the kernels' query is not asked for CPU tensors")
    monkeypatch.setattr(ops, "variational_chol_batched_supported", refuse)

    # the K_ZZ factor op exists for CUDA tensors only: the cache's factor is restated in torch here,
    # so that the routing of _call_chol itself runs without a device
    def torch_factor(Zf, s2f, lsf, jitter, key_tensors):
        zs = (Zf / lsf[:, None, :]).double()
        K = s2f.double()[:, None, None] * torch.exp(-0.5 * (zs[:, :, None] - zs[:, None]).pow(2).sum(-1)) + \
            jitter * torch.eye(M, dtype=torch.float64)
        return torch.linalg.solve_triangular(torch.linalg.cholesky(K), torch.eye(M, dtype=torch.float64).expand(O, M, M),
                                             upper=False)
    monkeypatch.setattr(vs._kzz_cache, "factor", torch_factor)
    with torch.no_grad(), settings.num_likelihood_samples(1):
        out = layer(x)
        kl = vs.kl_divergence()
    assert len(calls) == O and out._base._clamp_flag is None     # the layer wraps the per-output MVN
    assert out.mean.shape == (1, 4, 30, O) and kl.shape == (O,)
    with torch.no_grad():
        Z = vs.inducing_points
        s2 = layer.covar_module.outputscale.reshape(O)
        ls = layer.covar_module.base_kernel.lengthscale.reshape(O, -1)
        c = layer.mean_module.constant.reshape(O)
        jit = vs._jitter(x.dtype)
        for o in range(O):
            zs = (Z[o] / ls[o]).double()
            K = s2[o].double() * torch.exp(-0.5 * (zs[:, None] - zs[None]).pow(2).sum(-1)) + \
                jit * torch.eye(M, dtype=torch.float64)
            Linv = torch.linalg.solve_triangular(torch.linalg.cholesky(K), torch.eye(M, dtype=torch.float64),
                                                 upper=False)
            mean, var = real(x, Z[o], Linv, q.variational_mean[o], q.chol_variational_covar[o], s2[o], ls[o], None,
                             c[o], jit)
            assert torch.allclose(out.mean[0, ..., o], mean, rtol=1e-4, atol=1e-5)
            assert torch.allclose(out.variance[0, ..., o], var, rtol=1e-4, atol=1e-5)
        assert torch.allclose(kl, gp.cholesky_kl_closed_form(q.variational_mean, q.chol_variational_covar))
