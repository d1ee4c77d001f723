"""CPU: the C ABI of gpk_exact_append_f32 (exports, workspace query, argument validation without a
device), the FakeTensor impl of gpk::exact_append, and the host-side guards of
ExactGPModel.get_fantasy_model."""
import ctypes

import pytest
import torch


def _lib():
    from fine_grained_gaussian_process_forcasting_amd import _native
    return _native.lib()


def test_symbols_exported_and_bound():
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _lib()
    for n in ("gpk_exact_append_workspace_bytes", "gpk_exact_append_f32", "gpk_exact_append_perwin_f32"):
        assert hasattr(lib, n), n
        assert n in _native.SIGNATURES, n
    # the per-window entry point takes hyp_stride (long long) after n_lengthscale
    shared = _native.SIGNATURES["gpk_exact_append_f32"][1]
    perwin = _native.SIGNATURES["gpk_exact_append_perwin_f32"][1]
    assert len(perwin) == len(shared) + 1 and perwin[5] is ctypes.c_longlong
    assert perwin[:5] + perwin[6:] == shared


def test_workspace_query():
    """0 for a refused shape, linear in B otherwise. The query takes (B, N, m): D does not size the
    workspace, so D = 65 is refused by the call itself (-11, test_argument_validation_without_device)."""
    lib = _lib()
    q = lib.gpk_exact_append_workspace_bytes
    assert q(4, 100, 0) == 0
    assert q(4, 100, 257) == 0
    assert q(4, 785, 16) == 0          # N + m = 801
    assert q(4, 0, 16) == 0
    assert q(-1, 100, 16) == 0
    assert q(65536, 300, 16) == 0      # the blocked phase 1 keeps B on gridDim.y
    assert q(65536, 200, 16) > 0
    for N, m in [(1, 1), (37, 5), (250, 16), (96, 256), (784, 16)]:
        one = q(1, N, m)
        # at least V (N x m rounded up to 64 columns), S and R
        assert one >= 4 * (N * 64 * ((m + 63) // 64) + 2 * m * m), (N, m)
        for B in (2, 3, 7, 512):
            assert q(B, N, m) == B * one, (B, N, m)
        # the posterior-covariance workspace at Ns = m is its head
        assert one > lib.gpk_exact_posterior_cov_workspace_bytes(1, N, m)


def test_argument_validation_without_device():
    lib = _lib()
    one = ctypes.c_void_p(16)  # never dereferenced: validation returns first
    # X, L, z, hyp, n_ls, Xn, yn, B, N, m, D, jitter, workspace, Lout, zout, info, stream
    args = [one, one, one, one, 1, one, one, 2, 16, 3, 4, 0.0, one, one, one, one, None]
    for idx, code in [(0, -1), (1, -2), (2, -3), (3, -4), (5, -6), (6, -7), (12, -13), (13, -14), (14, -15),
                      (15, -16)]:
        bad = list(args); bad[idx] = None
        assert lib.gpk_exact_append_f32(*bad) == code, idx
    for idx, val, code in [(4, 3, -5), (7, -1, -8), (8, 0, -9), (8, 801, -9), (9, 0, -10), (9, 257, -10),
                           (10, 0, -11), (10, 65, -11), (11, -1.0, -12), (11, float("nan"), -12),
                           (12, ctypes.c_void_p(20), -13)]:
        bad = list(args); bad[idx] = val
        assert lib.gpk_exact_append_f32(*bad) == code, (idx, val)
    bad = list(args); bad[8], bad[9] = 790, 11      # N + m = 801
    assert lib.gpk_exact_append_f32(*bad) == -10
    bad = list(args); bad[7], bad[8] = 65536, 300   # B on gridDim.y of the blocked phase 1
    assert lib.gpk_exact_append_f32(*bad) == -8
    zero = list(args); zero[7] = 0
    assert lib.gpk_exact_append_f32(*zero) == 0     # B = 0: nothing to do
    # per-window: hyp_stride after n_lengthscale; 0 or >= 3 + n_lengthscale
    pw = args[:5] + [4] + args[5:]
    for stride, code in [(1, -6), (3, -6), (-4, -6)]:
        bad = list(pw); bad[5] = stride
        assert lib.gpk_exact_append_perwin_f32(*bad) == code, stride
    bad = list(pw); bad[0] = None
    assert lib.gpk_exact_append_perwin_f32(*bad) == -1
    bad = list(pw); bad[16] = None
    assert lib.gpk_exact_append_perwin_f32(*bad) == -16
    for stride in (0, 4, 9):
        z = list(pw); z[5] = stride; z[8] = 0
        assert lib.gpk_exact_append_perwin_f32(*z) == 0


def test_custom_op_registered_with_fake():
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.gpk, "exact_append")
    with FakeTensorMode():
        B, N, m, D = 3, 16, 5, 4
        X, L, z = torch.empty(B, N, D), torch.empty(B, N, N), torch.empty(B, N)
        for h in (torch.empty(4), torch.empty(B, 4)):
            L2, z2, info = torch.ops.gpk.exact_append(X, L, z, h, torch.empty(B, m, D), torch.empty(B, m), 0.0)
            assert L2.shape == (B, N + m, N + m) and z2.shape == (B, N + m)
            assert info.shape == (B,) and info.dtype == torch.int32


def test_ops_exact_append_refuses_cpu_and_bad_shapes():
    from fine_grained_gaussian_process_forcasting_amd import ops
    B, N, m, D = 2, 8, 3, 2
    X, L, z, h = torch.zeros(B, N, D), torch.zeros(B, N, N), torch.zeros(B, N), torch.ones(4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.exact_append(X, L, z, h, torch.zeros(B, m, D), torch.zeros(B, m))
    with pytest.raises(ValueError):
        ops.exact_append(X, L, z, h, torch.zeros(B, m, D + 1), torch.zeros(B, m))
    with pytest.raises(ValueError):
        ops.exact_append(X, L, z, h, torch.zeros(B, m, D), torch.zeros(B, m + 1))


def _fake_append(monkeypatch, fail_first, nan=False):
    """Stand in for gpk::exact_append on the host: the first ``fail_first`` launches report a failed
    pivot in window 1; records the jitter of every launch."""
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    jitters = []

    def fake(X, L, z, hyper, Xn, yn, jitter):
        jitters.append(jitter)
        B, n2 = X.shape[0], X.shape[1] + Xn.shape[1]
        info = torch.zeros(B, dtype=torch.int32)
        if len(jitters) <= fail_first:
            info[1] = 3
        return torch.full((B, n2, n2), float(len(jitters))), torch.zeros(B, n2), info

    monkeypatch.setattr(torch.ops.gpk, "exact_append", fake, raising=False)
    B, N, m, D = 2, 4, 3, 2
    Xn = torch.zeros(B, m, D)
    if nan:
        Xn[1, 0, 0] = float("nan")
    return jitters, (torch.zeros(B, N, D), torch.zeros(B, N, N), torch.zeros(B, N), torch.ones(4), Xn,
                     torch.zeros(B, m))


def test_append_ladder_is_psd_safe_choleskys(monkeypatch):
    """jitter 0, then the whole batch again with cholesky_jitter * 10^t, one NumericalWarning per
    retry; NotPSDError after cholesky_max_tries; NanError before any retry when an input holds NaN."""
    import warnings
    from fine_grained_gaussian_process_forcasting_amd.errors import NanError, NotPSDError, NumericalWarning
    from fine_grained_gaussian_process_forcasting_amd.gp import _exact_append_ladder
    jitters, args = _fake_append(monkeypatch, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        L2, _ = _exact_append_ladder(*args)
    assert jitters == [0.0] and float(L2[0, 0, 0]) == 1.0
    jitters, args = _fake_append(monkeypatch, 2)
    with pytest.warns(NumericalWarning) as rec:
        L2, _ = _exact_append_ladder(*args)
    assert jitters == pytest.approx([0.0, 1e-6, 1e-5]) and float(L2[0, 0, 0]) == 3.0
    msgs = [str(w.message) for w in rec if issubclass(w.category, NumericalWarning)]
    assert msgs == ["A not p.d., added jitter of 1.0e-06 to the diagonal",
                    "A not p.d., added jitter of 1.0e-05 to the diagonal"]
    jitters, args = _fake_append(monkeypatch, 99)
    with pytest.warns(NumericalWarning), pytest.raises(NotPSDError, match="up to 1.0e-04"):
        _exact_append_ladder(*args)
    assert jitters == pytest.approx([0.0, 1e-6, 1e-5, 1e-4])
    jitters, args = _fake_append(monkeypatch, 99, nan=True)
    with pytest.raises(NanError, match=r"1 of 12 elements of the \(2, 3, 2\) tensor are NaN"):
        _exact_append_ladder(*args)
    assert jitters == [0.0]


def _cpu_model(batched=False):
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    from fine_grained_gaussian_process_forcasting_amd.gp import GaussianLikelihood
    shape = (3, 7, 2) if batched else (7, 2)
    return ExactGPModel(torch.zeros(*shape), torch.zeros(*shape[:-1]), GaussianLikelihood())


def test_fantasy_needs_the_prediction_cache():
    for batched in (False, True):
        m = _cpu_model(batched)
        m.eval()
        with pytest.raises(RuntimeError, match="Call the model on some data first"):
            m.get_fantasy_model(torch.zeros(4, 2), torch.zeros(4))
        with pytest.raises(RuntimeError, match="Fantasy observations can only be added after making predictions"):
            m.get_fantasy_model([torch.zeros(4, 2)], torch.zeros(4))
        assert m._prediction_cache is None and m.train_inputs[0].shape[-2] == 7


def test_fantasy_refuses_fantasy_batches_and_fixed_noise():
    m = _cpu_model()
    m.eval()
    with pytest.raises(NotImplementedError, match="batch of fantasies"):
        m.get_fantasy_model(torch.zeros(4, 2), torch.zeros(5, 4))
    with pytest.raises(NotImplementedError, match="batch of fantasies"):
        m.get_fantasy_model(torch.zeros(4), torch.zeros(5, 4))
    with pytest.raises(NotImplementedError, match="batch of fantasies"):
        _cpu_model(True).get_fantasy_model(torch.zeros(3, 4, 2), torch.zeros(5, 3, 4))
    with pytest.raises(NotImplementedError, match="FixedNoiseGaussianLikelihood"):
        m.get_fantasy_model(torch.zeros(4, 2), torch.zeros(4), noise=torch.ones(4))
