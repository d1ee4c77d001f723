"""Time the Cholesky-q(u) variational forward / adjoint (gpk_variational_chol_f32 with its saved
state, gpk_variational_chol_adjoint_f32) beside the mean-field training pair
(gpk_variational_train_f32, gpk_variational_adjoint_saved_f32 or the recompute adjoint where the
saved state does not serve the shape) at the same shapes, in one process:

  cfg5     BASELINE config 5        B = 1024, N = 256, M = 64,  D = 32
  default  the reference's default  B = 256,  N = 192, M = 256, D = 32

HIP events around every call, 10 warm-ups, the median of 50 repetitions. One JSON line per shape
with the four times, the ratios (measured, not targets), the arithmetic the Cholesky q(u) adds
(W = L_q^T A in the forward; W, Y = L_q W and the M x M Gram over all points in the adjoint; a
triangular product counted as M^2 N flops per window, the lower Gram as M^2 B N) and the bytes of
the saved state and the workspace.

  python scripts/var_chol_time.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg5": (1024, 256, 64, 32), "default": (256, 192, 256, 32)}


def _median_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from fine_grained_gaussian_process_forcasting_amd import _native, ops
    dev = torch.device("cuda", 0)
    lib = _native.lib()
    for name, (B, N, M, D) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        X = (torch.randn(B, N, D, generator=g) / math.sqrt(D)).to(dev)
        Z = (torch.randn(M, D, generator=g) / math.sqrt(D)).to(dev)
        ls = (0.5 + 0.5 * torch.rand(D, generator=g)).to(dev)
        m = (0.5 * torch.randn(M, generator=g)).to(dev)
        s = (0.5 + torch.rand(M, generator=g)).to(dev)
        C = (torch.diag(0.5 + torch.rand(M, generator=g))
             + torch.tril(0.3 * torch.randn(M, M, generator=g) / math.sqrt(M), -1)).to(dev)
        w = torch.randn(D, generator=g).to(dev)
        gmean = torch.randn(B, N, generator=g).to(dev)
        gvar = torch.randn(B, N, generator=g).to(dev)
        f = ops.kzz_cholesky(Z, 0.8, ls, jitter=1e-4)
        hyper = ops.pack_variational_hyper(0.8, 1.0, 1e-4, 0.3, w, ls, D, dev)

        chol = ops.variational_chol_forward(X, Z, f.Linv, m, C, hyper, save=True)
        mf = ops.variational_forward(X, Z, f.Linv, m, s, hyper=hyper, save=True)
        t = {
            "chol_fwd_ms": _median_ms(lambda: ops.variational_chol_forward(X, Z, f.Linv, m, C, hyper, save=True),
                                      args.warmup, args.reps),
            "chol_adj_ms": _median_ms(lambda: ops.variational_chol_adjoint(X, Z, f.Linv, m, C, hyper, gmean, gvar,
                                                                           chol.saved), args.warmup, args.reps),
            "meanfield_fwd_ms": _median_ms(lambda: ops.variational_forward(X, Z, f.Linv, m, s, hyper=hyper,
                                                                           save=True), args.warmup, args.reps),
            "meanfield_adj_ms": _median_ms(lambda: ops.variational_adjoint(X, Z, f.Linv, m, s, hyper, gmean, gvar,
                                                                           saved=mf.saved), args.warmup, args.reps),
        }
        tri = float(M) * M * N * B
        out = {"shape": name, "B": B, "N": N, "M": M, "D": D, **{k: round(v, 4) for k, v in t.items()},
               "fwd_ratio": round(t["chol_fwd_ms"] / t["meanfield_fwd_ms"], 3),
               "adj_ratio": round(t["chol_adj_ms"] / t["meanfield_adj_ms"], 3),
               "meanfield_saved_state": mf.saved is not None,
               "added_flops_fwd": tri, "added_flops_adj": 2 * tri + float(M) * M * B * N,
               "chol_saved_bytes": lib.gpk_variational_chol_saved_bytes(B, N, M, D),
               "chol_adjoint_workspace_bytes": lib.gpk_variational_chol_adjoint_workspace_bytes(B, N, M, D),
               "meanfield_saved_bytes": lib.gpk_variational_saved_bytes(B, N, M, D),
               "meanfield_adjoint_workspace_bytes": (lib.gpk_variational_adjoint_saved_workspace_bytes(B, N, M, D)
                                                     if mf.saved is not None else
                                                     lib.gpk_variational_adjoint_workspace_bytes(B, N, M, D))}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
