"""Parity of the variational (DeepGP) backward — the per-window HIP adjoint
gpk_variational_adjoint_f32 plus the GEMM contractions and the K_ZZ adjoint in
ops_autograd — against the fp64 oracle gradients (oracle.variational_grads: torch fp64
autograd of the VariationalStrategy restatement, pinned by finite differences in
tests/test_oracle.py). Tolerance 1e-4 norm-wise per gradient block (north_star bound).
"""
import types

import numpy as np
import pytest
import torch

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _rel(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("B,N,M,D", [(4, 24, 16, 8), (3, 40, 32, 16), (2, 64, 64, 32), (2, 20, 8, 4),
                                     # D in (32, 64] at M <= 64 (DQ = 64 variants)
                                     (3, 40, 48, 48), (2, 30, 64, 64)])
def test_variational_grads_vs_oracle(cuda_device, B, N, M, D):
    from fine_grained_gaussian_process_forcasting_amd import ops_autograd
    g = torch.Generator().manual_seed(B * 1000 + N + M)
    X = torch.randn(B, N, D, generator=g) / np.sqrt(D)
    Z = torch.randn(M, D, generator=g) / np.sqrt(D)
    m = 0.3 * torch.randn(M, generator=g)
    s = 0.5 + 0.5 * torch.rand(M, generator=g)
    w = torch.randn(D, generator=g)
    b0 = 0.3
    ls = np.linspace(0.7, 1.3, D)
    s2 = 0.9
    gmean = torch.randn(B, N, generator=g)
    gvar = torch.randn(B, N, generator=g)
    dev = cuda_device
    P = lambda t: t.clone().to(dev).requires_grad_(True)  # noqa: E731
    Xd, Zd, md, sd, wd = P(X), P(Z), P(m), P(s), P(w)
    b0d = torch.tensor(b0, device=dev, requires_grad=True)
    lsd = torch.tensor(ls, dtype=torch.float32, device=dev, requires_grad=True)
    s2d = torch.tensor(s2, device=dev, requires_grad=True)
    mm = types.SimpleNamespace(weights=wd, bias=b0d)
    mean, var, _ = ops_autograd.variational_predict(Xd, Zd, md, sd, s2d, lsd, mm, 1e-4)
    ((gmean.to(dev) * mean).sum() + (gvar.to(dev) * var).sum()).backward()
    ref = O.variational_grads(X.double().numpy(), Z.double().numpy(), ls, s2, w.double().numpy(), b0,
                              m.double().numpy(), s.double().numpy(), gmean.double().numpy(),
                              gvar.double().numpy(), jitter=1e-4)
    got = {"X": Xd.grad, "Z": Zd.grad, "m": md.grad, "s": sd.grad, "outputscale": s2d.grad,
           "lengthscale": lsd.grad, "weights": wd.grad, "bias": b0d.grad}
    for k, v in got.items():
        e = _rel(v.detach().cpu().numpy(), ref[k])
        print(f"B={B} N={N} M={M} D={D} {k:12s} {e:.2e}")
        assert e <= TOL, (k, e)


def _op_level_grads(dev, X, Z, m, s, w, b0, ls, s2, gmean, gvar, jitter, var_jitter, saved=False):
    """The product backward composed from the op-level entry points (what
    _VariationalPredict + _KzzFactor do), with a separate K_XX jitter (test hook).
    ``saved``: the training pair (forward keeps A, gpk_variational_adjoint_saved_f32) where it
    serves the shape; the recompute adjoint otherwise."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    D = X.shape[-1]
    lst = torch.tensor(ls, dtype=torch.float32, device=dev)
    f = ops.kzz_cholesky(Z.to(dev), s2, lst, jitter=jitter)
    hyper = ops.pack_variational_hyper(s2, 1.0, var_jitter, b0, w.to(dev), lst, D, dev)
    st = None
    if saved:
        st = ops.variational_forward(X.to(dev), Z.to(dev), f.Linv, m.to(dev), s.to(dev), hyper=hyper,
                                     save=True).saved
    adj = ops.variational_adjoint(X.to(dev), Z.to(dev), f.Linv, m.to(dev), s.to(dev), hyper,
                                  gmean.to(dev), gvar.to(dev), saved=st)
    dZk, ds2k, dlsk = ops.kzz_backward(adj.dLinv, f.L, f.Linv, Z.to(dev), torch.tensor(s2, device=dev), lst)
    return {"X": adj.dX, "Z": adj.dZ.double() + dZk, "m": adj.dvmean, "s": adj.dvstd,
            "outputscale": adj.ds2.double() + ds2k, "lengthscale": adj.dls.double() + dlsk}


@pytest.mark.parametrize("M,saved", [(32, False), (96, False), (96, True)])
def test_variance_clamp_gradient_mask(cuda_device, M, saved):
    """Where the variance clamp is active (MVN.variance clamp_min), gvar passes no
    gradient: driven with a negative K_XX jitter (test hook) so ~half the points clamp.
    M = 96 runs the M > 64 adjoints, recompute and saved-state (the forward's clamp mask)."""
    B, N, D = 3, 48, 8
    g = torch.Generator().manual_seed(77)
    X = torch.randn(B, N, D, generator=g) / np.sqrt(D)
    Z = torch.randn(M, D, generator=g) / np.sqrt(D)
    m = 0.3 * torch.randn(M, generator=g)
    s = 0.1 + 0.2 * torch.rand(M, generator=g)
    w = torch.randn(D, generator=g)
    ls = np.linspace(0.7, 1.3, D)
    s2, b0 = 0.69, 0.1
    gmean = torch.randn(B, N, generator=g)
    gvar = torch.randn(B, N, generator=g)
    ref_fwd = O.variational_forward(X.double().numpy(), Z.double().numpy(), ls, s2, w.double().numpy(), b0,
                                    m.double().numpy(), s.double().numpy(), jitter=1e-4,
                                    dtype=np.float64, var_jitter=-0.15)
    frac = float((ref_fwd.var <= 1e-6).mean())
    assert 0.05 < frac < 0.95, frac
    got = _op_level_grads(cuda_device, X, Z, m, s, w, b0, ls, s2, gmean, gvar, 1e-4, -0.15, saved=saved)
    ref = O.variational_grads(X.double().numpy(), Z.double().numpy(), ls, s2, w.double().numpy(), b0,
                              m.double().numpy(), s.double().numpy(), gmean.double().numpy(),
                              gvar.double().numpy(), jitter=1e-4, var_jitter=-0.15)
    for k, v in got.items():
        e = _rel(v.detach().cpu().numpy(), ref[k])
        print(f"clamp-mask {k:12s} {e:.2e}")
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("B,N,M,D", [(8, 192, 256, 32), (16, 256, 64, 32), (5, 96, 256, 16),
                                     # M > 64 register-resident adjoint: every row-block
                                     # count, ragged M / N, D up to the DQ = 64 variant
                                     (3, 70, 100, 7), (2, 50, 96, 20), (2, 33, 180, 30),
                                     (2, 41, 250, 32), (2, 45, 90, 40), (2, 30, 120, 64),
                                     # the LDS-tiled adjoint's instantiations no other test launches:
                                     # gpk_var_adj_kernel<1, 64>, <2, 64>, and <12, 64>, <16, 64> (M > 64
                                     # where the L^{-1} plan does not fit; no saved state either)
                                     (2, 40, 13, 33), (2, 40, 29, 33), (2, 40, 130, 33), (2, 40, 250, 33)])
@pytest.mark.parametrize("saved", [False, True])
def test_variational_grads_reference_shapes(cuda_device, B, N, M, D, saved):
    """The backward at the reference's GP shapes (M=256 default, DeepGP.py:15; cfg 5's
    M=64) on a window sample, every gradient block vs the fp64 oracle; ``saved``: the
    training pair (forward keeps A; M > 64 with D <= 32), else the recompute adjoint."""
    g = torch.Generator().manual_seed(B + N + M)
    X = torch.randn(B, N, D, generator=g) / np.sqrt(D)
    Z = torch.randn(M, D, generator=g) / np.sqrt(D)
    m = 0.3 * torch.randn(M, generator=g)
    s = 0.5 + 0.5 * torch.rand(M, generator=g)
    w = torch.randn(D, generator=g)
    ls = np.linspace(0.7, 1.3, D)
    s2, b0 = 0.9, 0.3
    gmean = torch.randn(B, N, generator=g)
    gvar = torch.randn(B, N, generator=g)
    got = _op_level_grads(cuda_device, X, Z, m, s, w, b0, ls, s2, gmean, gvar, 1e-4, 1e-4, saved=saved)
    ref = O.variational_grads(X.double().numpy(), Z.double().numpy(), ls, s2, w.double().numpy(), b0,
                              m.double().numpy(), s.double().numpy(), gmean.double().numpy(),
                              gvar.double().numpy(), jitter=1e-4)
    for k, v in got.items():
        e = _rel(v.detach().cpu().numpy(), ref[k])
        print(f"B={B} N={N} M={M} D={D} saved={saved} {k:12s} {e:.2e}")
        assert e <= TOL, (k, e)


@pytest.mark.parametrize("M,D", [(12, 5), (64, 32), (100, 7), (256, 32), (250, 64)])
def test_kzz_backward_kernel_vs_torch_fp64(cuda_device, M, D):
    """gpk_kzz_backward_f64 (five fp64-MFMA tile GEMMs + the RBF adjoint) against the
    plain-torch fp64 statement of the same formula (itself checked against autograd
    through cholesky + inverse in tests/test_host_logic.py), on a real K_ZZ factor."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    from tests.test_host_logic import kzz_backward_torch
    dev = cuda_device
    g = torch.Generator().manual_seed(M + D)
    Z = (torch.randn(M, D, generator=g) / np.sqrt(D)).to(dev)
    ls = torch.linspace(0.6, 1.4, D).to(dev)
    s2 = torch.tensor(0.9, device=dev)
    f = ops.kzz_cholesky(Z, s2, ls, jitter=1e-4)
    G = torch.randn(M, M, generator=g, dtype=torch.float64).tril().to(dev)
    dZ, ds2, dls = ops.kzz_backward(G, f.L, f.Linv, Z, s2, ls)
    rZ, rs2, rls = kzz_backward_torch(G, f.L, f.Linv, Z, s2, ls)
    for name, a, b in (("dZ", dZ, rZ), ("ds2", ds2, rs2), ("dls", dls, rls)):
        e = _rel(a.double().cpu().numpy(), b.double().cpu().numpy())
        print(f"M={M} D={D} {name} {e:.2e}")
        assert e <= 1e-6, (name, e)     # fp32 outputs of an fp64 computation


def _fp32_reference_grads(X, Z, ls, s2, w, b0, m, s, gmean, gvar, jitter=1e-4):
    """The reference's own arithmetic for the same objective, with autograd (torch CPU): GPyTorch
    1.9's VariationalStrategy in fp32 (the reference's dtype) -- ONE kernel evaluation over
    full_inputs = cat[Z, x] in upstream ``_sq_dist``'s GEMM form (inputs / l centred by their
    mean, |a|^2 + |b|^2 - 2 a.b clamped at 0; the diagonal is not zeroed since the inputs require
    grad), K_ZZ + jitter, the Cholesky and the A = L^{-1} K_ZX solve in fp64
    (``_linalg_dtype_cholesky``: ``.double()`` in, ``.to(fp32)`` out). The HIP adjoint's error is
    compared with this one's when K_ZZ is ill-conditioned."""
    P = lambda t: torch.as_tensor(t, dtype=torch.float32).clone().requires_grad_(True)  # noqa: E731
    Xt, Zt, mt, st, wt = P(X), P(Z), P(m), P(s), P(w)
    s2t, b0t, lst = P(s2), P(b0), P(np.asarray(ls, np.float32))
    B, N, D = Xt.shape
    M = Zt.shape[0]
    full = torch.cat([Zt.expand(B, M, D), Xt], -2) / lst
    a = full - full.mean(-2, keepdim=True)
    nrm = a.pow(2).sum(-1, keepdim=True)
    d = (nrm + nrm.transpose(-1, -2) - 2.0 * a @ a.transpose(-1, -2)).clamp_min(0.0)
    K = s2t * torch.exp(-0.5 * d)
    Kzz = K[..., :M, :M] + jitter * torch.eye(M)
    Kzx = K[..., :M, M:]
    L = torch.linalg.cholesky(Kzz.double())
    A = torch.linalg.solve_triangular(L, Kzx.double(), upper=False).to(torch.float32)
    mean = (A * mt[:, None]).sum(-2) + Xt @ wt + b0t
    var = (s2t + jitter + (A * A * (st * st - 1.0)[:, None]).sum(-2)).clamp_min(1e-6)
    obj = (torch.as_tensor(gmean, dtype=torch.float32) * mean).sum() + \
        (torch.as_tensor(gvar, dtype=torch.float32) * var).sum()
    gs = torch.autograd.grad(obj, [Xt, Zt, mt, st, s2t, lst, wt, b0t])
    names = ["X", "Z", "m", "s", "outputscale", "lengthscale", "weights", "bias"]
    return {k: v.detach().double().numpy() for k, v in zip(names, gs)}


@pytest.mark.parametrize("M,saved", [(64, False), (96, True), (256, True)])
def test_variational_grads_ill_conditioned_kzz(cuda_device, M, saved):
    """Inducing points in near-duplicate pairs (|dz| ~ 3e-3 l) put cond(K_ZZ + 1e-4 I) near
    2e5-1e6. There the reference's OWN fp32 arithmetic (GPyTorch in fp32 with the fp64
    Cholesky / solve, torch autograd) is ~1e-3 off the fp64 oracle on dZ, so each gradient block
    of the HIP adjoint (whose dK = L^{-T} dA runs on f32 MFMA) must be within 1e-4 of the fp64
    oracle or within 3x of the reference's own fp32 error -- the exact path's rule
    (test_exact_grad_ill_conditioned_vs_fp32_reference). Errors are printed."""
    B, N, D = 4, 64, 8
    g = torch.Generator().manual_seed(4242 + M)
    X = torch.randn(B, N, D, generator=g) / np.sqrt(D)
    base = torch.randn(M // 2, D, generator=g) / np.sqrt(D)
    Z = torch.cat([base, base + 3e-3 * torch.randn(M // 2, D, generator=g)], 0)
    m = 0.3 * torch.randn(M, generator=g)
    s = 0.5 + 0.5 * torch.rand(M, generator=g)
    w = torch.randn(D, generator=g)
    ls = np.linspace(0.7, 1.3, D)
    s2, b0 = 0.9, 0.3
    gmean = torch.randn(B, N, generator=g)
    gvar = torch.randn(B, N, generator=g)
    Kzz = O.rbf(Z.double().numpy(), Z.double().numpy(), ls, s2, x1_eq_x2=True, zero_diag=False) + 1e-4 * np.eye(M)
    print(f"M={M} cond(K_ZZ + jitter) = {np.linalg.cond(Kzz):.2e}")
    got = _op_level_grads(cuda_device, X, Z, m, s, w, b0, ls, s2, gmean, gvar, 1e-4, 1e-4, saved=saved)
    ref = O.variational_grads(X.double().numpy(), Z.double().numpy(), ls, s2, w.double().numpy(), b0,
                              m.double().numpy(), s.double().numpy(), gmean.double().numpy(),
                              gvar.double().numpy(), jitter=1e-4)
    f32 = _fp32_reference_grads(X.numpy(), Z.numpy(), ls, s2, w.numpy(), b0, m.numpy(), s.numpy(),
                                gmean.numpy(), gvar.numpy())
    got = {k: v.detach().cpu().double().numpy().ravel() for k, v in got.items()}
    # the scalar hyper-parameter gradients are compared as ONE vector: a single scalar's rounding
    # error is one draw (the reference's own outputscale error ranges 3e-6..2e-3 over M here)
    for blk in (got, ref, f32):
        blk["hyper"] = np.concatenate([np.ravel(blk["outputscale"]), np.ravel(blk["lengthscale"])])
    for k in ("X", "Z", "m", "s", "hyper"):
        e = _rel(got[k], ref[k])
        e32 = _rel(f32[k], ref[k])
        print(f"ill-conditioned M={M} saved={saved} {k:12s} hip {e:.2e}   reference-fp32 {e32:.2e}")
        assert e <= max(TOL, 3 * e32), (k, e, e32)
