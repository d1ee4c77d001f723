"""CPU: the multi-output (batched) entry points of include/gpk.h validate their arguments
before touching the device, their workspace queries scale with the output count O, and the
three batched custom ops propagate shapes under FakeTensorMode."""
import ctypes

import pytest
import torch

ONE = ctypes.c_void_p(16)   # never dereferenced: validation returns first


def _lib():
    from fine_grained_gaussian_process_forcasting_amd import _native
    return _native.lib()


def test_batched_symbols_and_version():
    lib = _lib()
    from fine_grained_gaussian_process_forcasting_amd import _native
    for n in ("gpk_kzz_chol_f64_batched", "gpk_kzz_backward_batched_workspace_bytes",
              "gpk_kzz_backward_f64_batched", "gpk_variational_batched_f32",
              "gpk_variational_adjoint_batched_workspace_bytes", "gpk_variational_adjoint_batched_f32"):
        assert hasattr(lib, n) and n in _native.SIGNATURES, n
    assert lib.gpk_version() >= 200


def test_kzz_chol_batched_validation():
    lib = _lib()
    # (Z, hyp, O, M, D, jitter, chol_jitter, max_tries, L, Linv, info, stream)
    args = [ONE, ONE, 3, 24, 8, 1e-4, 1e-8, 3, ONE, ONE, ONE, None]
    for idx, code in [(0, -1), (1, -2), (8, -9), (9, -10), (10, -11)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_kzz_chol_f64_batched(*bad) == code
    for idx, val, code in [(2, 0, -3), (2, 65536, -3), (3, 257, -4), (3, 0, -4), (4, 65, -5), (7, 13, -8)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_kzz_chol_f64_batched(*bad) == code


def test_kzz_backward_batched_validation_and_workspace():
    lib = _lib()
    one = lib.gpk_kzz_backward_workspace_bytes(96, 4)
    assert one > 0
    for O in (1, 3, 8):
        assert lib.gpk_kzz_backward_batched_workspace_bytes(O, 96, 4) == O * one
    assert lib.gpk_kzz_backward_batched_workspace_bytes(0, 96, 4) == 0
    assert lib.gpk_kzz_backward_batched_workspace_bytes(3, 257, 4) == 0
    assert lib.gpk_kzz_backward_batched_workspace_bytes(3, 96, 65) == 0
    # (dLinv, L, Linv, Z, hyp, O, M, D, workspace, dZ, dhyp, stream)
    args = [ONE, ONE, ONE, ONE, ONE, 3, 24, 8, ONE, ONE, ONE, None]
    for idx, code in [(0, -1), (1, -2), (2, -3), (3, -4), (4, -5), (8, -9), (9, -10), (10, -11)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_kzz_backward_f64_batched(*bad) == code
    for idx, val, code in [(5, 0, -6), (6, 257, -7), (7, 65, -8)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_kzz_backward_f64_batched(*bad) == code


def test_variational_batched_validation():
    lib = _lib()
    # (X, shared_x, Z, Linv, vmean, vstd, hyp, O, B, N, M, D, mean, var, flags, saved, stream)
    args = [ONE, 1, ONE, ONE, ONE, ONE, ONE, 3, 2, 40, 96, 4, ONE, ONE, None, None, None]
    for idx, code in [(0, -1), (2, -3), (3, -4), (4, -5), (5, -6), (6, -7), (12, -13), (13, -14)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_variational_batched_f32(*bad) == code
    for idx, val, code in [(7, 0, -8), (8, -1, -9), (9, 0, -10), (10, 257, -11), (11, 65, -12)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_variational_batched_f32(*bad) == code
    # a saved-state buffer where no saved-state adjoint serves the shape (M <= 64)
    assert lib.gpk_variational_saved_bytes(2, 40, 24, 4) == 0
    bad = list(args); bad[10] = 24; bad[15] = ONE
    assert lib.gpk_variational_batched_f32(*bad) == -16
    # B = 0: nothing to do
    ok = list(args); ok[8] = 0
    assert lib.gpk_variational_batched_f32(*ok) == 0


def test_variational_adjoint_batched_validation_and_workspace():
    lib = _lib()
    B, N, M, D = 2, 40, 96, 4
    rec = lib.gpk_variational_adjoint_workspace_bytes(B, N, M, D)
    sav = lib.gpk_variational_adjoint_saved_workspace_bytes(B, N, M, D)
    assert rec > 0 and sav > 0
    for O in (1, 3, 8):
        assert lib.gpk_variational_adjoint_batched_workspace_bytes(O, B, N, M, D, 0) == O * rec
        assert lib.gpk_variational_adjoint_batched_workspace_bytes(O, B, N, M, D, 1) == O * sav
    assert lib.gpk_variational_adjoint_batched_workspace_bytes(0, B, N, M, D, 0) == 0
    assert lib.gpk_variational_adjoint_batched_workspace_bytes(3, B, N, 257, D, 0) == 0
    assert lib.gpk_variational_adjoint_batched_workspace_bytes(3, B, N, M, 65, 0) == 0
    # no saved-state adjoint at M <= 64: the saved-state workspace query says so
    assert lib.gpk_variational_adjoint_batched_workspace_bytes(3, B, N, 24, D, 1) == 0
    # (X, shared_x, Z, Linv, vmean, vstd, hyp, gmean, gvar, saved, O, B, N, M, D, workspace,
    #  dX, dLinv, dZ, dpar, stream)
    args = [ONE, 1, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, 3, B, N, M, D, ONE, ONE, ONE, ONE, ONE, None]
    for idx, code in [(0, -1), (2, -3), (3, -4), (4, -5), (5, -6), (6, -7), (7, -8), (8, -9), (15, -16),
                      (16, -17), (17, -18), (18, -19), (19, -20)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_variational_adjoint_batched_f32(*bad) == code
    for idx, val, code in [(10, 0, -11), (11, 0, -12), (12, 0, -13), (13, 257, -14), (14, 65, -15)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_variational_adjoint_batched_f32(*bad) == code
    bad = list(args); bad[13] = 24; bad[9] = ONE     # saved given, saved size 0 at this shape
    assert lib.gpk_variational_adjoint_batched_f32(*bad) == -10


def test_batched_ops_refuse_cpu_tensors_and_bad_shapes():
    from fine_grained_gaussian_process_forcasting_amd import ops
    O, M, D = 2, 8, 4
    Z = torch.zeros(O, M, D)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.kzz_cholesky_batched(Z, torch.ones(O, 1 + D))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.variational_forward_batched(torch.zeros(3, 16, D), Z, torch.zeros(O, M, M, dtype=torch.float64),
                                        torch.zeros(O, M), torch.ones(O, M), torch.ones(O, 4 + 2 * D))
    with pytest.raises(ValueError, match=r"\(O, M, D\)"):
        ops.kzz_cholesky_batched(torch.zeros(M, D), torch.ones(1, 1 + D))
    with pytest.raises(ValueError, match=r"\(O, M, D\)"):
        ops.variational_adjoint_batched(torch.zeros(3, 16, D), torch.zeros(M, D), None, None, None, None, None, None)
    with pytest.raises(ValueError, match=r"\(O, M, D\)"):
        ops.kzz_backward_batched(None, None, None, torch.zeros(M, D), None)


def test_batched_custom_ops_fake_shapes():
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for n in ("kzz_factor", "variational_fwd", "variational_adj"):
        assert hasattr(torch.ops.gpk, n), n
    nat = _lib().gpk_variational_saved_bytes(3, 16, 256, 4) // 4
    assert nat == 3 * 1 * (16 * 2 * 256 + 32)
    with FakeTensorMode():
        O, B, N, M, D = 3, 3, 16, 8, 4
        X = torch.empty(B, N, D)
        Z = torch.empty(O, M, D)
        Linv, L, info = torch.ops.gpk.kzz_factor(Z, torch.empty(O), torch.empty(O, D), 1e-4, 1e-8, 3)
        assert Linv.shape == (O, M, M) and Linv.dtype == torch.float64 and L.shape == (O, M, M)
        assert info.shape == (O,) and info.dtype == torch.int32
        mean, var, flags, hyp, saved = torch.ops.gpk.variational_fwd(
            X, Linv, Z, torch.empty(O, M), torch.empty(O, M), torch.empty(O), torch.empty(O, D), torch.empty(D),
            torch.empty(1), 1e-4)
        assert mean.shape == (O, B, N) and var.shape == (O, B, N) and mean.dtype == torch.float32
        assert flags.shape == (1,) and flags.dtype == torch.int32
        assert hyp.shape == (O, 4 + 2 * D) and saved.numel() == 0
        # per-output inputs and a per-output mean
        mean4 = torch.ops.gpk.variational_fwd(
            torch.empty(O, B, N, D), Linv, Z, torch.empty(O, M), torch.empty(O, M), torch.empty(O),
            torch.empty(O, D), torch.empty(O, D), torch.empty(O), 1e-4)[0]
        assert mean4.shape == (O, B, N)
        # training at M = 256: O x the native saved-state size
        Z2 = torch.empty(O, 256, D)
        L2 = torch.empty(O, 256, 256, dtype=torch.float64)
        out = torch.ops.gpk.variational_fwd(X, L2, Z2, torch.empty(O, 256), torch.empty(O, 256),
                                                    torch.empty(O), torch.empty(O, D), torch.empty(D),
                                                    torch.empty(1), 1e-4, True)
        assert out[4].numel() == O * nat and out[4].dtype == torch.float32
        dX, dL, dZ, dpar = torch.ops.gpk.variational_adj(X, L2, Z2, torch.empty(O, 256),
                                                                 torch.empty(O, 256), out[3], out[0], out[1],
                                                                 out[4])
        assert dX.shape == (O, B, N, D) and dL.shape == (O, 256, 256) and dL.dtype == torch.float64
        assert dZ.shape == (O, 256, D) and dpar.shape == (O, 2 * 256 + 2 * D + 2)
