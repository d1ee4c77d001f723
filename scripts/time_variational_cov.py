"""Time the dense covariance of the variational q(f) on the kernels (gpk_variational_cov_f32:
phase 1 A = Linv K_ZX + the covariance kernel's variational mode) and one draw from it
(gpk_mvn_root_f32) against the same work in torch on the same GPU under no_grad
(gp.variational_dense_covariance, then torch.linalg.cholesky_ex and the root matmul).

Event timing after warm-up, best of 3; the per-kernel split comes from a kernel trace of this
script (rocprofv3 --kernel-trace --stats -- python scripts/time_variational_cov.py)."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fine_grained_gaussian_process_forcasting_amd import ops  # noqa: E402
from fine_grained_gaussian_process_forcasting_amd.gp import variational_dense_covariance  # noqa: E402

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


with torch.no_grad():
    for name, B, N, M, D in (("cfg-3", 256, 192, 256, 32), ("cfg-5", 1024, 256, 64, 32)):
        g = torch.Generator().manual_seed(0)
        X = (torch.randn(B, N, D, generator=g) / math.sqrt(D)).to(dev)
        Z = (torch.randn(M, D, generator=g) / math.sqrt(D)).to(dev)
        vstd = (torch.rand(M, generator=g) * 0.5 + 0.5).to(dev)
        mean = torch.randn(B, N, generator=g).to(dev)
        eps = torch.randn(1, B, N, generator=g).to(dev)
        ls = torch.full((D,), LN2, device=dev)
        s2 = torch.tensor(LN2, device=dev)
        Linv = ops.kzz_cholesky(Z, LN2, ls, jitter=1e-4).Linv
        hyper = ops.pack_variational_hyper(LN2, 1.0, 1e-4, 0.0, torch.zeros(D), ls, D, dev)
        reps = 10

        def k_cov():
            return ops.variational_cov(X, Z, Linv, vstd, hyper)

        def k_draw():
            return ops.mvn_root(k_cov(), 0.0, mean, eps, want_R=False)[1]

        def t_cov():
            return variational_dense_covariance(X, Z, Linv, vstd, s2, ls, 1e-4)

        def t_draw():
            R, _ = torch.linalg.cholesky_ex(t_cov())
            return mean + (R @ eps[0].unsqueeze(-1)).squeeze(-1)

        cov = k_cov()
        t_kc = timed(k_cov, reps)
        t_kd = timed(k_draw, reps)
        t_root = timed(lambda: ops.mvn_root(cov, 0.0, mean, eps, want_R=False), reps)
        # phase 2's algorithmic bytes: read A once, write cov once
        gb = 4.0 * B * (M * N + N * N) / 1e9
        print(json.dumps({"shape": name, "B": B, "N": N, "M": M, "D": D, "kernel_cov_ms": round(t_kc, 4),
                          "kernel_cov_draw_ms": round(t_kd, 4), "kernel_root_draw_ms": round(t_root, 4),
                          "phase2_algorithmic_GB": round(gb, 4)}), flush=True)
        t_tc = timed(t_cov, reps)
        t_td = timed(t_draw, reps)
        tc = t_cov()
        rel = float(((cov - tc).flatten(1).norm(dim=1) / tc.flatten(1).norm(dim=1)).max())
        # both draws against the fp64 draw from the kernel covariance
        want = mean.double() + (torch.linalg.cholesky(cov.double()) @ eps[0].double().unsqueeze(-1)).squeeze(-1)
        kd, td = k_draw()[0], t_draw()
        torch.cuda.synchronize()
        dk = float(((kd.double() - want).norm(dim=1) / want.norm(dim=1)).max())
        dt = float(((td.double() - want).norm(dim=1) / want.norm(dim=1)).max())
        print(json.dumps({"shape": name, "torch_cov_ms": round(t_tc, 4), "torch_cov_draw_ms": round(t_td, 4),
                          "cov_speedup_vs_torch": round(t_tc / t_kc, 2),
                          "cov_draw_speedup_vs_torch": round(t_td / t_kd, 2),
                          "cov_vs_torch_rel": rel, "kernel_draw_vs_fp64_rel": dk, "torch_draw_vs_fp64_rel": dt}),
              flush=True)
