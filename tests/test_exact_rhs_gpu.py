"""Right-hand side of the exact kernel's column-ownership plan (worker_step_col): the forward
solve z = L^{-1}(y - c) runs as VALU matvecs on 16-float rows in LDS, z_k travels as 16 fp32
words, and block row 8 of the right-hand side is summed by several waves.

The column plan serves N in 241..256 only when B exceeds the CU count (two windows per CU), so
every launch here has B = multi_processor_count + 32 at D = 32. The fp64 oracle
(oracle/gp_oracle.py) is evaluated on a fixed sample of ~24 windows that holds window 0, the last
window and windows at and past the CU count; tolerances are tests/test_exact_gpu.py's: 1e-4
relative (norm-wise per window for L and z, per window for the MLL).
"""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))
NOISE0 = LN2 + 1e-4
D = 32
TOL = 1e-4


def _batch(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count + 32


def _sample(B, cus, extra=()):
    """~24 windows: the first, the last, the two around the CU count, an even spread below it
    and everything from the CU count on in steps of 4."""
    s = {0, B - 1, cus - 1, cus, cus + 1} | set(range(0, cus, max(1, cus // 10))) | set(range(cus, B, 4))
    return sorted((s | set(extra)) & set(range(B)))


def _inputs(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, N, D, generator=g) / np.sqrt(D)
    y = torch.randn(B, N, generator=torch.Generator().manual_seed(seed + 1))
    return X, y


def _run(dev, X, y, ls, s2, c, noise, **kw):
    from fine_grained_gaussian_process_forcasting_amd import ops
    kw.setdefault("want_z", True)
    out = ops.exact_mll(X.to(dev), y.to(dev), ls, s2, c, noise, **kw)
    torch.cuda.synchronize()
    return out


def _rel_fro(a, b):
    num = np.linalg.norm((a - b).reshape(a.shape[0], -1), axis=1)
    den = np.linalg.norm(b.reshape(b.shape[0], -1), axis=1)
    return num / den


def _check_sample(out, X, y, sel, ls, s2, c, noise, tag):
    ref = O.exact_mll(X[sel].double().numpy(), y[sel].double().numpy(), ls, s2, c, noise)
    L = out.L[sel].cpu().double().numpy()
    z = out.z[sel].cpu().double().numpy()
    mll = out.mll[sel].cpu().double().numpy()
    eL, ez = _rel_fro(L, ref.L).max(), _rel_fro(z, ref.z).max()
    em = np.max(np.abs(mll - ref.mll) / np.abs(ref.mll))
    print(f"[{tag}] windows {len(sel)}: L {eL:.2e}  z {ez:.2e}  mll {em:.2e}")
    assert np.all(np.triu(L, 1) == 0.0), "upper triangle must be exactly zero"
    assert eL <= TOL and ez <= TOL and em <= TOL, (eL, ez, em)


@pytest.mark.parametrize("N", [256, 250])
def test_rhs_both_instantiations(cuda_device, N):
    """N = 256 (FULL) and N = 250 (padded tiles): L, z and MLL on the sample; every window
    factors (info 0) with a finite MLL."""
    B = _batch(cuda_device)
    X, y = _inputs(B, N, seed=300 + N)
    out = _run(cuda_device, X, y, LN2, LN2, 0.0, NOISE0)
    assert (out.info.cpu().numpy() == 0).all()
    assert bool(torch.isfinite(out.mll).all())
    _check_sample(out, X, y, _sample(B, B - 32), LN2, LN2, 0.0, NOISE0, f"N={N}")


@pytest.mark.parametrize("N", [256, 250])
def test_rhs_large_offset_targets(cuda_device, N):
    """y = 1e3 * randn + 50 with a non-zero constant mean: the right-hand side is far from unit
    scale (it is carried in fp32, never through the f16 split), same bounds."""
    B = _batch(cuda_device)
    X, y = _inputs(B, N, seed=500 + N)
    y = 1e3 * y + 50.0
    c = 37.5
    out = _run(cuda_device, X, y, LN2, LN2, c, NOISE0)
    assert (out.info.cpu().numpy() == 0).all()
    assert bool(torch.isfinite(out.mll).all())
    _check_sample(out, X, y, _sample(B, B - 32), LN2, LN2, c, NOISE0, f"big-y N={N}")


def _ladder_jitter(t):
    """Jitter in force after t rungs of the fp32 ladder: the current rung 1e-6 * 10^(t-1)."""
    return 1e-6 * 10 ** (t - 1) if t > 0 else 0.0


@pytest.mark.parametrize("N", [256, 250])
def test_rhs_jitter_ladder_restart(cuda_device, N):
    """Windows of duplicated points with zero noise restart in-kernel with more jitter: the
    right-hand-side rows (row 8 among them) and the z slots are set up again per attempt. L, z
    and the MLL of regular AND laddered windows are compared with the fp64 oracle at the jitter
    in force, 1e-4 flat; a NaN window and a window that is not positive definite at any rung
    keep reporting info > 0 with a NaN MLL.

    The laddered windows are N copies of one observation (same point, same target) under an
    outputscale of 1e-5. Both choices keep the comparison with an independent fp64 oracle
    meaningful at 1e-4: K = s2 * ones is singular whatever s2 is, so the first attempt fails, but
    the ladder's jitter is absolute, and at s2 = 1e-5 its first rung (1e-6) is a tenth of the
    diagonal, so K + jitter I has condition number ~ N s2 / jitter = 2.6e3 instead of the 2.6e8
    of s2 = 1 (where fp32 cannot even represent the diagonal 1 + 1e-6 to better than 6 % of the
    jitter, and no fp32 factorisation gives z or log|K| to 1e-4); and equal targets are
    consistent with equal points, so z is not dominated by differences of targets divided by
    sqrt(jitter)."""
    B = _batch(cuda_device)
    cus = B - 32
    X, y = _inputs(B, N, seed=700 + N)
    dup = [0, 5, cus - 1, cus + 3, B - 1]          # first, last, both sides of the CU count
    nanw, npdw = 9, cus + 7
    for b in dup:
        X[b] = X[b, :1].expand(N, D)               # all points equal: K = s2 * ones, singular
        y[b] = y[b, :1].expand(N)
    X[nanw, 7, 2] = float("nan")
    X[npdw] = X[npdw] * 1e25                       # squared distances overflow: no rung helps
    ls, s2, c, noise = 0.3, 1e-5, 0.0, 0.0         # regular windows: K close to s2 * I
    out = _run(cuda_device, X, y, ls, s2, c, noise)
    info = out.info.cpu().numpy()
    mll_all = out.mll.cpu().double().numpy()
    print(f"[ladder N={N}] info of dup windows {info[dup]}, NaN window {info[nanw]}, not-PSD window {info[npdw]}")
    assert (info[dup] < 0).all(), info[dup]
    assert info[nanw] > 0 and info[npdw] > 0
    assert np.isnan(mll_all[nanw]) and np.isnan(mll_all[npdw])
    good = [b for b in range(B) if b not in dup and b not in (nanw, npdw)]
    assert (info[good] == 0).all()
    assert np.isfinite(mll_all[good]).all() and np.isfinite(mll_all[dup]).all()
    sel = [b for b in _sample(B, cus) if b in good]
    _check_sample(out, X, y, sel, ls, s2, c, noise, f"ladder-regular N={N}")
    # laddered windows at the jitter in force (jitter on the diagonal == that much more noise)
    for t in sorted({-int(info[b]) for b in dup}):
        at = [b for b in dup if -int(info[b]) == t]
        _check_sample(out, X, y, at, ls, s2, c, noise + _ladder_jitter(t), f"laddered N={N} rungs={t}")


def test_rhs_output_selection(cuda_device):
    """The MLL does not depend on which of L and z are written."""
    N = 256
    B = _batch(cuda_device)
    X, y = _inputs(B, N, seed=901)
    both = _run(cuda_device, X, y, LN2, LN2, 0.1, NOISE0, want_L=True, want_z=True)
    for want_L, want_z in ((False, True), (True, False), (False, False)):
        o = _run(cuda_device, X, y, LN2, LN2, 0.1, NOISE0, want_L=want_L, want_z=want_z)
        assert torch.equal(o.mll, both.mll), (want_L, want_z)
        assert torch.equal(o.info, both.info)
        if want_z:
            assert torch.equal(o.z, both.z)
        if want_L:
            assert torch.equal(o.L, both.L)


@pytest.mark.parametrize("N", [256, 250])
def test_rhs_deterministic(cuda_device, N):
    """Two launches on the same inputs: L, z and the MLL bitwise equal (row 8 of the right-hand
    side is summed by several waves in a fixed order, without atomics)."""
    B = _batch(cuda_device)
    X, y = _inputs(B, N, seed=1100 + N)
    a = _run(cuda_device, X, y, LN2, LN2, 0.0, NOISE0)
    b = _run(cuda_device, X, y, LN2, LN2, 0.0, NOISE0)
    assert torch.equal(a.L, b.L) and torch.equal(a.z, b.z) and torch.equal(a.mll, b.mll)
