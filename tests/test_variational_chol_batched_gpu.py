"""The Cholesky q(u) of a multi-output layer on one launch chain each way:
gpk_variational_chol_batched_f32, gpk_variational_chol_adjoint_batched_f32 (dLinv chained through the
batched K_ZZ backward) and gpk_cholesky_kl_batched_f32, through ops.* / the gpk:: custom ops /
VariationalStrategy._call_chol, against the fp64 torch reference gp.variational_chol_predict on the
CPU, once per output (Linv from torch.linalg.cholesky of K_ZZ + 1e-4 I, torch autograd), and bit for
bit against the single-output ops on each output's arrays. Tolerance 1e-4 norm-wise per window / per
gradient block, 1e-5 relative for the KL.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
JIT = 1e-4

# (O, B, N, M, D): ragged everything / N over a 64-point block, M no multiple of 16 / B > 32 (window
# splits of 2, ragged last) / the q chunk boundaries per output / two 64-row blocks, D > 32 / M = 256
SHAPES = [(3, 3, 20, 8, 4), (2, 2, 70, 20, 5), (2, 33, 24, 12, 6), (2, 70, 16, 16, 4), (2, 2, 40, 100, 40),
          (2, 2, 40, 256, 32)]
BIT_SHAPES = [(3, 3, 20, 8, 4), (2, 33, 24, 12, 6), (2, 2, 40, 100, 40)]
NAMES = ("X", "Z", "ls", "s2", "m", "C", "w", "b0")


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@functools.lru_cache(maxsize=None)
def _problem(o, B, N, M, D):
    """Output o's problem, drawn in the order of test_variational_chol_gpu._problem."""
    g = torch.Generator().manual_seed(100000 * o + 1000 * B + 100 * N + 10 * M + D)
    X = torch.randn(B, N, D, generator=g) / np.sqrt(D)
    Z = torch.randn(M, D, generator=g) / np.sqrt(D)
    ls = 0.5 + 0.5 * torch.rand(D, generator=g)
    m = 0.5 * torch.randn(M, generator=g)
    C = torch.diag(0.5 + torch.rand(M, generator=g)) + torch.tril(0.3 * torch.randn(M, M, generator=g) / np.sqrt(M), -1)
    C[0, 0] = -C[0, 0]
    C = C + torch.triu(torch.randn(M, M, generator=g), 1)      # never read
    w = torch.randn(D, generator=g)
    gmean = torch.randn(B, N, generator=g)
    gvar = torch.randn(B, N, generator=g)
    return dict(X=X, Z=Z, ls=ls, s2=torch.tensor(0.6 + 0.25 * o), m=m, C=C, w=w, b0=torch.tensor(0.3 - 0.2 * o),
                gmean=gmean, gvar=gvar)


def _output(o, shared, B, N, M, D):
    p = _problem(o, B, N, M, D)
    if shared and o > 0:
        p = dict(p)
        p["X"] = _problem(0, B, N, M, D)["X"]
    return p


@functools.lru_cache(maxsize=None)
def _reference(o, shared, B, N, M, D, var_jitter=JIT):
    """fp64 CPU (mean, unclamped var, gradients of sum gmean mean + sum gvar [var >= 1e-6] var) of
    output o; computed once per case and shared."""
    from fine_grained_gaussian_process_forcasting_amd import gp
    p = _output(o, shared, B, N, M, D)
    t = {k: p[k].double().clone().requires_grad_(True) for k in NAMES}
    zs = t["Z"] / t["ls"]
    Kzz = t["s2"] * torch.exp(-0.5 * (zs[:, None, :] - zs[None, :, :]).pow(2).sum(-1)) + \
        JIT * torch.eye(M, dtype=torch.float64)
    L = torch.linalg.cholesky(Kzz)
    Linv = torch.linalg.solve_triangular(L, torch.eye(M, dtype=torch.float64), upper=False)
    mean, var = gp.variational_chol_predict(t["X"], t["Z"], Linv, t["m"], t["C"], t["s2"], t["ls"], t["w"],
                                            t["b0"], var_jitter)
    keep = (var.detach() >= 1e-6).double()
    obj = (p["gmean"].double() * mean).sum() + (p["gvar"].double() * keep * var).sum()
    gs = torch.autograd.grad(obj, [t[k] for k in NAMES])
    return mean.detach(), var.detach(), dict(zip(NAMES, gs))


def _stacked(dev, shared, O, B, N, M, D, var_jitter=None):
    """The O outputs' arrays with a leading O on the device (X (B, N, D) when shared), the packed
    hyper rows (var_jitter: one K_XX jitter per output) and the batched K_ZZ factor."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    ps = [_output(o, shared, B, N, M, D) for o in range(O)]
    d = {k: torch.stack([p[k] for p in ps]).to(dev) for k in ps[0]}
    if shared:
        d["X"] = ps[0]["X"].to(dev)
    vj = var_jitter if var_jitter is not None else [JIT] * O
    d["hyper"] = torch.stack([ops.pack_variational_hyper(d["s2"][o], 1.0, vj[o], d["b0"][o], d["w"][o], d["ls"][o],
                                                         D, dev) for o in range(O)])
    d["kzz_hyper"] = torch.cat([d["s2"].reshape(O, 1), d["ls"]], dim=1)
    d["f"] = ops.kzz_cholesky_batched(d["Z"], d["kzz_hyper"], jitter=JIT)
    return d


def _batched(d):
    from fine_grained_gaussian_process_forcasting_amd import ops
    out = ops.variational_chol_forward_batched(d["X"], d["Z"], d["f"].Linv, d["m"], d["C"], d["hyper"], save=True)
    adj = ops.variational_chol_adjoint_batched(d["X"], d["Z"], d["f"].Linv, d["m"], d["C"], d["hyper"],
                                               d["gmean"], d["gvar"], out.saved)
    return out, adj


def _grads(d, adj):
    """Per-output gradient blocks, dLinv chained through the batched K_ZZ backward."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    dX, dLinv, dZ, dpar, dC = adj
    O, M, D = d["Z"].shape
    dZk, dhyp = ops.kzz_backward_batched(dLinv, d["f"].L, d["f"].Linv, d["Z"], d["kzz_hyper"])
    return [{"X": dX[o], "Z": dZ[o].double() + dZk[o].double(),
             "ls": dpar[o, M + 1:M + 1 + D].double() + dhyp[o, 1:].double(),
             "s2": dpar[o, M].double() + dhyp[o, 0].double(), "m": dpar[o, :M], "C": dC[o],
             "w": dpar[o, M + 1 + D:M + 1 + 2 * D], "b0": dpar[o, M + 1 + 2 * D]} for o in range(O)]


def _check_grads(tag, got, ref, B):
    for k in ("Z", "ls", "s2", "m", "C", "w", "b0"):
        e = _rel(got[k], ref[k])
        print(f"{tag} d{k:3s} {e:.2e}")
        assert e <= TOL, (tag, k, e)
    for b in range(B):     # dX per window
        e = _rel(got["X"][b], ref["X"][b])
        assert e <= TOL, (tag, "X", b, e)
    print(f"{tag} dX   {_rel(got['X'], ref['X']):.2e}")


@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_output_x"])
@pytest.mark.parametrize("O,B,N,M,D", SHAPES)
def test_parity(cuda_device, O, B, N, M, D, shared):
    d = _stacked(cuda_device, shared, O, B, N, M, D)
    out, adj = _batched(d)
    assert out.mean.shape == (O, B, N) and out.var.shape == (O, B, N)
    assert int(out.flags.item()) == 0
    got = _grads(d, adj)
    for o in range(O):
        rmean, rvar, rg = _reference(o, shared, B, N, M, D)
        assert float(rvar.min()) >= 0.25           # a changed draw cannot clamp silently
        for b in range(B):
            em, ev = _rel(out.mean[o, b], rmean[b]), _rel(out.var[o, b], rvar[b])
            assert em <= TOL and ev <= TOL, (o, b, em, ev)
        print(f"O={O} B={B} N={N} M={M} D={D} output {o}: mean {_rel(out.mean[o], rmean):.2e} "
              f"var {_rel(out.var[o], rvar):.2e}")
        _check_grads(f"output {o}", got[o], rg, B)
        # structure: the strict upper triangles are exactly zero
        assert torch.equal(torch.triu(adj[4][o], 1), torch.zeros_like(adj[4][o]))
        assert torch.equal(torch.triu(adj[1][o], 1), torch.zeros_like(adj[1][o]))


def _single(d, o, shared):
    from fine_grained_gaussian_process_forcasting_amd import ops
    X = d["X"] if shared else d["X"][o]
    Linv = d["f"].Linv[o]
    out = ops.variational_chol_forward(X, d["Z"][o], Linv, d["m"][o], d["C"][o], d["hyper"][o], save=True)
    adj = ops.variational_chol_adjoint(X, d["Z"][o], Linv, d["m"][o], d["C"][o], d["hyper"][o], d["gmean"][o],
                                       d["gvar"][o], out.saved)
    return out, adj


@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "per_output_x"])
@pytest.mark.parametrize("O,B,N,M,D", BIT_SHAPES)
def test_bit_identity(cuda_device, O, B, N, M, D, shared):
    """Every batched output equals the single-output op call on output o's arrays; O = 1 batched
    equals the single-output call; two batched runs are bit-identical."""
    from fine_grained_gaussian_process_forcasting_amd import ops
    d = _stacked(cuda_device, shared, O, B, N, M, D)
    out, adj = _batched(d)
    out2, adj2 = _batched(d)
    assert torch.equal(out.mean, out2.mean) and torch.equal(out.var, out2.var)
    assert torch.equal(out.saved, out2.saved)
    for a, b in zip(adj, adj2):
        assert torch.equal(a, b)
    saved = out.saved.reshape(O, -1)
    names = ("dX", "dLinv", "dZ", "dpar", "dchol")
    for o in range(O):
        so, sa = _single(d, o, shared)
        assert torch.equal(out.mean[o], so.mean) and torch.equal(out.var[o], so.var), o
        assert torch.equal(saved[o], so.saved), o
        for n, a, b in zip(names, adj, sa):
            assert torch.equal(a[o], b), (o, n)
        # O = 1 batched on output o's arrays
        X1 = d["X"] if shared else d["X"][o:o + 1]
        o1 = ops.variational_chol_forward_batched(X1, d["Z"][o:o + 1], d["f"].Linv[o:o + 1], d["m"][o:o + 1],
                                                  d["C"][o:o + 1], d["hyper"][o:o + 1], save=True)
        a1 = ops.variational_chol_adjoint_batched(X1, d["Z"][o:o + 1], d["f"].Linv[o:o + 1], d["m"][o:o + 1],
                                                  d["C"][o:o + 1], d["hyper"][o:o + 1], d["gmean"][o:o + 1],
                                                  d["gvar"][o:o + 1], o1.saved)
        assert torch.equal(o1.mean[0], so.mean) and torch.equal(o1.var[0], so.var), o
        assert torch.equal(o1.saved, so.saved), o
        for n, a, b in zip(names, a1, sa):
            assert torch.equal(a[0], b), (o, n)


def test_clamp_mask_one_output(cuda_device):
    """Output 1's hyp row carries a negative K_XX jitter (chosen as test_clamp_mask chooses it, from
    output 1's fp64 variances) that clamps some but not all of its points; output 0 keeps 1e-4. The
    one flag word is set, output 0 is untouched, output 1's clamped points are exactly 1e-6 and pass
    no gvar, every gradient block of both outputs matches the reference with the same mask."""
    O, B, N, M, D = 2, 3, 48, 40, 8
    _, var0, _ = _reference(1, False, B, N, M, D, 0.0)
    v = var0.reshape(-1).sort().values
    mid = v.numel() // 2
    k = mid - 10 + int((v[mid - 9:mid + 11] - v[mid - 10:mid + 10]).argmax())
    vj = 1e-6 - 0.5 * float(v[k] + v[k + 1])
    refs = [_reference(0, False, B, N, M, D), _reference(1, False, B, N, M, D, vj)]
    rvar1 = refs[1][1]
    share = float((rvar1 < 1e-6).double().mean())
    assert 0.0 < share < 1.0, share
    assert float((rvar1 - 1e-6).abs().min()) > 1e-4    # no point sits on the threshold
    assert float(refs[0][1].min()) >= 0.25
    dev = cuda_device
    d = _stacked(dev, False, O, B, N, M, D, var_jitter=[JIT, vj])
    out, adj = _batched(d)
    assert int(out.flags.item()) & 1
    assert float(out.var[0].min()) > 1e-6              # output 0: no clamped point
    assert _rel(out.var[0], refs[0][1]) <= TOL
    clamped = (rvar1 < 1e-6).to(dev)
    assert torch.equal(out.var[1][clamped], torch.full_like(out.var[1][clamped], 1e-6))
    assert _rel(out.var[1][~clamped], rvar1.to(dev)[~clamped]) <= TOL
    got = _grads(d, adj)
    for o in range(O):
        assert _rel(out.mean[o], refs[o][0]) <= TOL
        _check_grads(f"clamp share={share:.2f} output {o}", got[o], refs[o][2], B)
    # gvar of output 1's clamped points alone moves nothing
    d2 = dict(d)
    d2["gvar"] = d["gvar"].clone()
    d2["gvar"][1] = torch.where(clamped, 7.0 * d["gvar"][1] + 1.0, d["gvar"][1])
    _, adj2 = _batched(d2)
    for a, b in zip(adj, adj2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("O,M", [(3, 1), (2, 20), (2, 256)])
def test_cholesky_kl_batched(cuda_device, O, M):
    import fine_grained_gaussian_process_forcasting_amd  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd import ops
    from fine_grained_gaussian_process_forcasting_amd.gp import cholesky_kl_closed_form
    dev = cuda_device
    ps = [_problem(o, 1, 4, M, 2) for o in range(O)]
    m0, C0 = torch.stack([p["m"] for p in ps]), torch.stack([p["C"] for p in ps])
    gk = torch.tensor([2.5 - 0.75 * o for o in range(O)])
    m = m0.to(dev).requires_grad_(True)
    C = C0.to(dev).requires_grad_(True)
    got = torch.ops.gpk.cholesky_kl(m, C)
    assert got.shape == (O,)
    (gk.to(dev) * got).sum().backward()
    got = got.detach()
    m64 = m0.double().requires_grad_(True)
    C64 = C0.double().requires_grad_(True)
    ref = cholesky_kl_closed_form(m64, C64)
    (gk.double() * ref).sum().backward()
    ref = ref.detach()
    for o in range(O):
        print(f"O={O} M={M} output {o}: kl {float(got[o]):.6f} ref {float(ref[o]):.6f}")
        assert abs(float(got[o]) - float(ref[o])) <= 1e-5 * max(1.0, abs(float(ref[o])))
    assert torch.allclose(m.grad.cpu().double(), m64.grad, rtol=1e-5, atol=1e-6)
    assert torch.allclose(C.grad.cpu().double(), C64.grad, rtol=1e-5, atol=1e-6)
    assert torch.equal(torch.triu(C.grad, 1), torch.zeros_like(C.grad))
    # bit for bit the single-output op per output
    for o in range(O):
        mo, Co = m0[o].to(dev), C0[o].to(dev)
        assert torch.equal(ops.cholesky_kl(mo, Co)[0], got[o])
        dm, dC = ops.cholesky_kl_grad(mo, Co, gk[o:o + 1].to(dev))
        assert torch.equal(dm, m.grad[o]) and torch.equal(dC, C.grad[o])


def _chol_layer(D, seed, M, dev, output_dims, mean_type):
    """ToyDeepGPHiddenLayer with the distribution swapped, as test_variational_chol_gpu._chol_layer."""
    from fine_grained_gaussian_process_forcasting_amd import gp
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.DeepGP import ToyDeepGPHiddenLayer
    layer = ToyDeepGPHiddenLayer(D, output_dims, seed, num_inducing=M, mean_type=mean_type)
    batch = torch.Size([output_dims])
    q = gp.CholeskyVariationalDistribution(M, batch)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        q.variational_mean.copy_(0.5 * torch.randn(q.variational_mean.shape, generator=g))
        C = torch.diag_embed(0.5 + torch.rand(*batch, M, generator=g)) + \
            torch.tril(0.3 * torch.randn(*batch, M, M, generator=g) / np.sqrt(M), -1)
        q.chol_variational_covar.copy_(C + torch.triu(torch.randn(*batch, M, M, generator=g), 1))
    vs = layer.variational_strategy
    vs._variational_distribution = q
    vs.variational_params_initialized.fill_(1)
    vs._initialized = True
    return layer.to(dev)


@pytest.mark.parametrize("mean_type", ["constant", "linear"])
def test_layer_matches_the_torch_fallback(cuda_device, monkeypatch, mean_type):
    """A three-output layer: loss sum gm mean + sum gv variance + sum KL and every parameter gradient,
    x's included, on the kernels against the per-output torch loop on the same device (1e-4); one
    K_ZZ factor per step."""
    from fine_grained_gaussian_process_forcasting_amd import gp, ops, settings
    dev = cuda_device
    D, M, O = 5, 12, 3
    g = torch.Generator().manual_seed(3)
    x0 = (torch.randn(4, 30, D, generator=g) / np.sqrt(D)).to(dev)
    gm = torch.randn(1, 4, 30, O, generator=g).to(dev)
    gv = torch.randn(1, 4, 30, O, generator=g).to(dev)
    predicts, closed, factors = [], [], []
    real_predict, real_closed = gp.variational_chol_predict, gp.cholesky_kl_closed_form
    real_factor = torch.ops.gpk.kzz_factor
    monkeypatch.setattr(gp, "variational_chol_predict", lambda *a: (predicts.append(1), real_predict(*a))[1])
    monkeypatch.setattr(gp, "cholesky_kl_closed_form", lambda *a: (closed.append(1), real_closed(*a))[1])

    class _Counted:
        def __call__(self, *a, **k):
            factors.append(1)
            return real_factor(*a, **k)

        def __getattr__(self, name):
            return getattr(real_factor, name)

    def run(fallback):
        layer = _chol_layer(D, 7, M, dev, O, mean_type)
        x = x0.clone().requires_grad_(True)
        with monkeypatch.context() as mp:
            mp.setattr(torch.ops.gpk, "kzz_factor", _Counted())
            if fallback:
                mp.setattr(ops, "variational_chol_batched_supported", lambda *a, **k: False)
            with settings.num_likelihood_samples(1):
                dist = layer(x)
            kl = layer.variational_strategy.kl_divergence()
            assert dist.mean.shape == (1, 4, 30, O) and kl.shape == (O,)
            val = (gm * dist.mean).sum() + (gv * dist.variance).sum() + kl.sum()
            val.backward()
        grads = {k: v.grad.clone() for k, v in layer.named_parameters()}
        grads["x"] = x.grad.clone()
        return val.detach(), grads, dist

    v1, g1, d1 = run(False)
    assert not predicts and not closed        # the kernels served the layer and the KL
    assert d1._base._clamp_flag is not None   # the layer wraps the per-output MVN, which carries the flag
    assert len(factors) == 1                  # one K_ZZ factor op in the step
    v2, g2, d2 = run(True)
    assert len(predicts) == O                 # the fallback: one torch evaluation per output
    assert d2._base._clamp_flag is None
    print(f"{mean_type}: loss kernels {float(v1):.6f} fallback {float(v2):.6f}")
    assert abs(float(v1) - float(v2)) <= TOL * abs(float(v2))
    assert set(g1) == set(g2) and any("chol_variational_covar" in k for k in g1)
    for k in g1:
        e = _rel(g1[k], g2[k])
        print(f"{k:70s} {e:.2e}")
        assert e <= TOL, (k, e)
    C = [k for k in g1 if "chol_variational_covar" in k][0]
    assert torch.equal(torch.triu(g1[C], 1), torch.zeros_like(g1[C]))


def test_ops_opcheck(cuda_device):
    import fine_grained_gaussian_process_forcasting_amd.library  # noqa: F401
    dev = cuda_device
    O, B, N, M, D = 2, 2, 24, 8, 4
    d = _stacked(dev, True, O, B, N, M, D)
    tests = ("test_schema", "test_autograd_registration", "test_faketensor")
    Linv = torch.ops.gpk.kzz_factor(d["Z"], d["s2"], d["ls"], JIT, 1e-8, 3)[0]
    for X in (d["X"], d["X"].expand(O, B, N, D).contiguous()):
        args = (X, Linv, d["Z"], d["m"], d["C"], d["s2"], d["ls"], d["w"], d["b0"], JIT)
        torch.library.opcheck(torch.ops.gpk.variational_chol_fwd.default, args, test_utils=tests)
        torch.library.opcheck(torch.ops.gpk.variational_chol_fwd.default, args + (True,), test_utils=tests)
        # with gradients requested the registered autograd formula runs
        req = tuple(t.clone().requires_grad_(True) if torch.is_tensor(t) and t.is_floating_point() else t
                    for t in args)
        torch.library.opcheck(torch.ops.gpk.variational_chol_fwd.default, req + (True,),
                              test_utils=tests)
    mean, var, _, hyp, saved = torch.ops.gpk.variational_chol_fwd(*args, True)
    assert saved.numel() == O * (B * M * 64 + B * 64)
    torch.library.opcheck(torch.ops.gpk.variational_chol_adj.default,
                          (X, Linv, d["Z"], d["m"], d["C"], hyp, d["gmean"], d["gvar"], saved),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.gpk.cholesky_kl.default,
                          (d["m"].clone().requires_grad_(True), d["C"].clone().requires_grad_(True)),
                          test_utils=tests)
    torch.library.opcheck(torch.ops.gpk.cholesky_kl_grad.default,
                          (d["m"], d["C"], torch.tensor([1.5, -0.5], device=dev)),
                          test_utils=("test_schema", "test_faketensor"))
