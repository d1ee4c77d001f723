"""Time the differentiable exact-GP posterior in eval mode, forward + backward with random gmean,
gvar and gcov, on two routes over the same tensors:

  new     ExactGPModel._posterior_kernels_grad: gpk::exact_posterior_train and its registered
          backward (gpk_exact_mll_f32, gpk_exact_posterior_cov_f32 keeping its workspace,
          gpk_exact_posterior_grad_f32)
  parent  ExactGPModel._posterior_autograd + torch autograd (the route of grad mode before the
          adjoint kernels existed), fed in chunks of 64 windows: at B = 512 one batched TRSM call
          fails in the BLAS library (scripts/time_posterior_cov.py)

Both run on a stand-in for the model that holds leaf hyper-parameters. Shapes (B, N, Ns, D):
(512, 256, 256, 32), (64, 256, 64, 32), (1, 64, 20, 3). HIP events after 3 warm-up steps, the mean
of 10 steps; every figure comes from a fresh child process (one route, one shape), five
alternating pairs per shape, each child under its own time limit; the first child that fails ends
the run (nothing is started again). The project's criterion per shape: the slowest new run is
faster than the fastest parent run.

  python scripts/time_exact_posterior_grad.py [--out profiles/exact_posterior_grad_timing.txt]

Per-kernel split: rocprofv3 --kernel-trace --stats -- python scripts/time_exact_posterior_grad.py
--child new big
"""
import argparse
import json
import math
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"big": (512, 256, 256, 32), "mid": (64, 256, 64, 32), "small": (1, 64, 20, 3)}
ROUNDS = 5
CHILD_LIMIT_S = 180
CHUNK = 64


def child(route: str, shape: str) -> None:
    import torch
    sys.path.insert(0, ROOT)
    from fine_grained_gaussian_process_forcasting_amd import library  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd.denoising_model.GPModel import ExactGPModel
    dev = torch.device("cuda", 0)
    B, N, Ns, D = SHAPES[shape]
    ln2 = math.log(2.0)
    g = torch.Generator().manual_seed(0)
    leaf = lambda t: t.to(dev).requires_grad_()   # noqa: E731
    X = leaf(torch.randn(B, N, D, generator=g) / math.sqrt(D))
    Xs = leaf(torch.randn(B, Ns, D, generator=g) / math.sqrt(D))
    y = leaf(torch.randn(B, N, generator=g))
    s2, noise, c = leaf(torch.tensor(ln2)), leaf(torch.tensor(ln2 + 1e-4)), leaf(torch.tensor(0.1))
    ls = leaf(torch.full((1,), ln2))
    gm, gv = torch.randn(B, Ns, generator=g).to(dev), torch.randn(B, Ns, generator=g).to(dev)
    gc = torch.randn(B, Ns, Ns, generator=g).to(dev)
    leaves = (X, Xs, y, s2, noise, c, ls)

    def stub(sl):
        return types.SimpleNamespace(
            train_inputs=(X[sl],), train_targets=y[sl],
            covar_module=types.SimpleNamespace(base_kernel=types.SimpleNamespace(lengthscale=ls), outputscale=s2),
            mean_module=types.SimpleNamespace(constant=c), likelihood=types.SimpleNamespace(noise=noise))

    def run(fn, sl):
        dist = fn(stub(sl), Xs[sl])
        torch.autograd.backward([dist.mean, dist.variance, dist.covariance_matrix], [gm[sl], gv[sl], gc[sl]])

    def step():
        for t in leaves:
            t.grad = None
        if route == "new":
            run(ExactGPModel._posterior_kernels_grad, slice(0, B))
        else:
            for i in range(0, B, CHUNK):
                run(ExactGPModel._posterior_autograd, slice(i, min(B, i + CHUNK)))

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    reps = 10
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        step()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"route": route, "shape": shape, "B": B, "N": N, "Ns": Ns, "D": D,
                      "ms": round(e0.elapsed_time(e1) / reps, 4), "dX_norm": float(X.grad.norm()),
                      "dXs_norm": float(Xs.grad.norm()), "dls": float(ls.grad)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("ROUTE", "SHAPE"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    if args.child:
        child(*args.child)
        return 0
    lines = []
    for shape in args.shapes:
        ms = {"new": [], "parent": []}
        for rnd in range(ROUNDS):
            for route in (("new", "parent") if rnd % 2 == 0 else ("parent", "new")):
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, shape],
                                       capture_output=True, text=True, timeout=CHILD_LIMIT_S)
                except subprocess.TimeoutExpired:
                    print(f"{shape} {route} round {rnd}: time limit; stopping", flush=True)
                    return 2
                if r.returncode != 0:
                    print(f"{shape} {route} round {rnd}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
                    return 2
                info = json.loads(r.stdout.strip().splitlines()[-1])
                ms[route].append(info["ms"])
                print(json.dumps(info), flush=True)
        B, N, Ns, D = SHAPES[shape]
        verdict = "new faster" if max(ms["new"]) < min(ms["parent"]) else "NOT faster"
        lines.append(f"{shape} (B={B} N={N} Ns={Ns} D={D}): new {min(ms['new']):.3f}-{max(ms['new']):.3f} ms, "
                     f"parent {min(ms['parent']):.3f}-{max(ms['parent']):.3f} ms, "
                     f"x{min(ms['parent']) / max(ms['new']):.2f} (fastest parent / slowest new): {verdict}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Exact posterior forward + backward in eval mode, ms per step (HIP events, 10 steps after 3 "
                    "warm-up; five alternating pairs of fresh processes per shape)\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
