"""Time the differentiable dense covariance of the variational q(f), forward + backward with a
random gcov, on two routes over the same tensors:

  new     gpk::variational_cov_train and its registered backward (gpk_variational_cov_f32 keeping
          its workspace, gpk_variational_cov_grad_f32)
  parent  gp.variational_dense_covariance per output + torch autograd (the route of grad mode
          before the adjoint kernels existed)

Shapes: the two-output cfg-3 windows (O = 2, B = 256, N = 192 and 96, M = 256, D = 32) and cfg-5
(B = 1024, N = 256, M = 64, D = 32, one output). HIP events after warm-up; every figure comes from
a fresh child process (one route, one shape), five alternating pairs per shape, each child under
its own time limit; the first child that fails ends the run (nothing is started again). The
project's criterion per shape: the slowest new run is faster than the fastest parent run.

  python scripts/time_variational_cov_grad.py [--out profiles/variational_cov_grad_timing.txt]
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg3_n192": (2, 256, 192, 256, 32), "cfg3_n96": (2, 256, 96, 256, 32), "cfg5": (1, 1024, 256, 64, 32)}
ROUNDS = 5
CHILD_LIMIT_S = 180


def child(route: str, shape: str) -> None:
    import torch
    sys.path.insert(0, ROOT)
    from fine_grained_gaussian_process_forcasting_amd import library, ops  # noqa: F401
    from fine_grained_gaussian_process_forcasting_amd.gp import variational_dense_covariance
    dev = torch.device("cuda", 0)
    O, B, N, M, D = SHAPES[shape]
    ln2 = math.log(2.0)
    g = torch.Generator().manual_seed(0)
    X = (torch.randn(B, N, D, generator=g) / math.sqrt(D)).to(dev).requires_grad_()
    Z = (torch.randn(O, M, D, generator=g) / math.sqrt(D)).to(dev).requires_grad_()
    vstd = (torch.rand(O, M, generator=g) * 0.5 + 0.5).to(dev).requires_grad_()
    ls = torch.full((O, D), ln2, device=dev, requires_grad=True)
    s2 = torch.full((O,), ln2, device=dev, requires_grad=True)
    gcov = torch.randn(O, B, N, N, generator=g).to(dev)
    Linv = torch.stack([ops.kzz_cholesky(Z[o].detach(), ln2, ls[o].detach(), jitter=1e-4).Linv
                        for o in range(O)]).requires_grad_()
    leaves = (X, Z, vstd, ls, s2, Linv)

    def new():
        if O == 1:
            cov = torch.ops.gpk.variational_cov_train(X, Linv[0], Z[0], vstd[0], s2[0], ls[0], 1e-4)[0][None]
        else:
            cov = torch.ops.gpk.variational_cov_train(X, Linv, Z, vstd, s2, ls, 1e-4)[0]
        cov.backward(gcov)

    def parent():
        cov = torch.stack([variational_dense_covariance(X, Z[o], Linv[o], vstd[o], s2[o], ls[o], 1e-4)
                           for o in range(O)])
        cov.backward(gcov)

    fn = new if route == "new" else parent

    def step():
        for t in leaves:
            t.grad = None
        fn()

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
    state_bytes = O * B * M * ((N + 63) // 64 * 64) * 4
    print(json.dumps({"route": route, "shape": shape, "O": O, "B": B, "N": N, "M": M, "D": D,
                      "ms": round(e0.elapsed_time(e1) / reps, 4), "saved_state_bytes": state_bytes,
                      "dX_norm": float(X.grad.norm())}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("ROUTE", "SHAPE"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(*args.child)
        return 0
    lines = []
    for shape in SHAPES:
        ms = {"new": [], "parent": []}
        info = {}
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
        O, B, N, M, D = SHAPES[shape]
        verdict = "new faster" if max(ms["new"]) < min(ms["parent"]) else "NOT faster"
        lines.append(f"{shape} (O={O} B={B} N={N} M={M} D={D}): new {min(ms['new']):.3f}-{max(ms['new']):.3f} ms, "
                     f"parent {min(ms['parent']):.3f}-{max(ms['parent']):.3f} ms, "
                     f"x{min(ms['parent']) / max(ms['new']):.2f} (fastest parent / slowest new): {verdict}; "
                     f"saved state {info['saved_state_bytes'] / 2 ** 20:.1f} MiB")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Sigma of q(f) forward + backward, ms per step (HIP events, 10 steps after 3 warm-up; five "
                    "alternating pairs of fresh processes per shape)\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
