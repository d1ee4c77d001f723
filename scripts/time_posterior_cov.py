"""Time the joint exact-GP posterior (gpk_exact_posterior_cov_f32: the V-storing posterior
kernel + the covariance kernel) against gpk_exact_posterior_f32 alone and against the same
arithmetic in torch on the same GPU (K* and K** by ExactGPModel._posterior_autograd's centred
Gram formulae, solve_triangular against the cached L, baddbmm), under no_grad.

Event timing after warm-up; the per-kernel split of the two phases comes from a kernel trace of
this script (rocprofv3 --kernel-trace --stats -- python scripts/time_posterior_cov.py)."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fine_grained_gaussian_process_forcasting_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
LN2 = math.log(2.0)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best


def torch_joint(X, L, z, Xs, ls, s2, c):
    n = X.shape[-2]
    full = torch.cat([X, Xs], -2) / ls
    a = full - full.mean(-2, keepdim=True)
    nrm = a.pow(2).sum(-1, keepdim=True)
    d = (nrm + nrm.transpose(-1, -2) - 2.0 * a @ a.transpose(-1, -2)).clamp_min(0.0)
    K = s2 * torch.exp(-0.5 * d)
    # the batched TRSM in chunks of 64 windows: at B = 512 one call fails in the BLAS library
    # ("Device memory allocation size is too small for TRSM", then an error status)
    Ks = K[..., :n, n:].contiguous()
    V = torch.cat([torch.linalg.solve_triangular(L[i:i + 64], Ks[i:i + 64], upper=False)
                   for i in range(0, L.shape[0], 64)])
    mean = c + (V * z.unsqueeze(-1)).sum(-2)
    var = s2 - (V * V).sum(-2)
    cov = torch.baddbmm(K[..., n:, n:], V.transpose(-1, -2), V, alpha=-1.0)
    return mean, var, cov


with torch.no_grad():
    for B, N, Ns, D in ((512, 256, 256, 32), (64, 256, 64, 32)):
        g = torch.Generator().manual_seed(0)
        X = (torch.randn(B, N, D, generator=g) / math.sqrt(D)).to(dev)
        Xs = (torch.randn(B, Ns, D, generator=g) / math.sqrt(D)).to(dev)
        y = torch.randn(B, N, generator=g).to(dev)
        h = ops.pack_exact_hyper(LN2, LN2 + 1e-4, 0.3, torch.tensor(LN2), dev)
        f = ops.exact_mll(X, y, None, None, None, None, want_L=True, want_z=True, hyper=h)
        reps = 10 if B >= 256 else 50
        t_post = timed(lambda: ops.exact_posterior(X, f.L, f.z, h, Xs), reps)
        t_cov = timed(lambda: ops.exact_posterior_cov(X, f.L, f.z, h, Xs), reps)
        # phase 2's algorithmic bytes: read V once, write cov once
        gb = 4.0 * B * (N * Ns + Ns * Ns) / 1e9
        line = {"B": B, "N": N, "Ns": Ns, "D": D, "posterior_ms": round(t_post, 4),
                "posterior_cov_ms": round(t_cov, 4),
                "cov_minus_posterior_ms": round(t_cov - t_post, 4),
                "phase2_algorithmic_GB": round(gb, 4),
                # (cov - posterior) also holds phase 1's V stores: a lower bound
                "phase2_GBps_lower_bound": round(gb / max(t_cov - t_post, 1e-9) * 1e3, 1)}
        print(json.dumps(line), flush=True)   # the kernels' own times first: the baseline may fail
        t_torch = timed(lambda: torch_joint(X, f.L, f.z, Xs, LN2, LN2, 0.3), reps)
        p = ops.exact_posterior_cov(X, f.L, f.z, h, Xs)
        _, _, tc = torch_joint(X, f.L, f.z, Xs, LN2, LN2, 0.3)
        rel = float(((p.cov - tc).flatten(1).norm(dim=1) / tc.flatten(1).norm(dim=1)).max())
        print(json.dumps({"B": B, "N": N, "Ns": Ns, "D": D, "torch_ms": round(t_torch, 4),
                          "speedup_vs_torch": round(t_torch / t_cov, 2), "cov_vs_torch_rel": rel}),
              flush=True)
