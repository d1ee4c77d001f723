"""Time appending m observations to a cached exact-GP factor against the thing it replaces, over
the same tensors:

  append  ops.exact_append(X, L, z, hyper, Xn, yn): gpk_exact_append_f32 on the cached (L, z) of the
          first N points (the factor itself is computed once, outside the timed window)
  refit   ops.exact_mll(..., want_L=True, want_z=True) on the N + m concatenated points: what
          set_train_data + the next eval call cost before get_fantasy_model existed

Shapes (B, N, m, D): (512, 240, 16, 32), (512, 496, 16, 32), (512, 784, 16, 32), (64, 784, 16, 32).
HIP events after 3 warm-up calls, the mean of 20 calls; every figure comes from a fresh child
process (one route, one shape), five alternating pairs per shape, each child under its own time
limit; the first child that fails ends the run (nothing is started again). The append child also
reports how far its new rows are from the refit's (relative, Frobenius, worst window). The
project's criterion per shape: the slowest append run is faster than the fastest refit run.

  python scripts/time_exact_append.py [--out profiles/exact_append_timing.txt]

Per-kernel split: rocprofv3 --kernel-trace --stats -- python scripts/time_exact_append.py
--child append n800
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"n256": (512, 240, 16, 32), "n512": (512, 496, 16, 32), "n800": (512, 784, 16, 32),
          "n800_b64": (64, 784, 16, 32)}
ROUNDS = 5
CHILD_LIMIT_S = 180


def child(route: str, shape: str) -> None:
    import torch
    sys.path.insert(0, ROOT)
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = torch.device("cuda", 0)
    B, N, m, D = SHAPES[shape]
    ln2 = math.log(2.0)
    g = torch.Generator().manual_seed(0)
    X = (torch.randn(B, N + m, D, generator=g) / math.sqrt(D)).to(dev)
    y = torch.randn(B, N + m, generator=g).to(dev)
    hyper = ops.pack_exact_hyper(ln2, ln2 + 1e-4, 0.3, torch.tensor(ln2), dev)
    Xo, yo = X[:, :N].contiguous(), y[:, :N].contiguous()
    Xn, yn = X[:, N:].contiguous(), y[:, N:].contiguous()
    extra = {}
    if route == "append":
        f = ops.exact_mll(Xo, yo, None, None, None, None, want_L=True, want_z=True, hyper=hyper)
        assert int(f.info.abs().max()) == 0

        def step():
            return ops.exact_append(Xo, f.L, f.z, hyper, Xn, yn)

        L2, z2, info = step()
        r = ops.exact_mll(X, y, None, None, None, None, want_L=True, want_z=True, hyper=hyper)
        assert int(info.abs().max()) == 0 and int(r.info.abs().max()) == 0
        dL = (L2[:, N:] - r.L[:, N:]).flatten(1).norm(dim=1) / r.L[:, N:].flatten(1).norm(dim=1)
        dz = (z2[:, N:] - r.z[:, N:]).norm(dim=1) / r.z[:, N:].norm(dim=1)
        extra = {"new_rows_vs_refit_L": float(dL.max()), "new_rows_vs_refit_z": float(dz.max())}
        del L2, z2, r
    else:
        def step():
            return ops.exact_mll(X, y, None, None, None, None, want_L=True, want_z=True, hyper=hyper)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    reps = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        step()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"route": route, "shape": shape, "B": B, "N": N, "m": m, "D": D,
                      "ms": round(e0.elapsed_time(e1) / reps, 4), **extra}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("ROUTE", "SHAPE"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    if args.child:
        child(*args.child)
        return 0
    raw, lines = [], []
    for shape in args.shapes:
        ms = {"append": [], "refit": []}
        for rnd in range(ROUNDS):
            for route in (("append", "refit") if rnd % 2 == 0 else ("refit", "append")):
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
                raw.append(json.dumps(info))
                print(raw[-1], flush=True)
        B, N, m, D = SHAPES[shape]
        verdict = "append faster" if max(ms["append"]) < min(ms["refit"]) else "NOT faster"
        lines.append(f"{shape} (B={B} N={N} m={m} D={D}): append {min(ms['append']):.3f}-{max(ms['append']):.3f} ms, "
                     f"refit {min(ms['refit']):.3f}-{max(ms['refit']):.3f} ms, "
                     f"x{min(ms['refit']) / max(ms['append']):.2f} (fastest refit / slowest append): {verdict}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Appending m observations to a cached factor (ops.exact_append) against refactoring the "
                    "concatenated data (ops.exact_mll), ms per call (HIP events, 20 calls after 3 warm-up; five "
                    "alternating pairs of fresh processes per shape)\n" + "\n".join(lines) + "\n\nraw\n"
                    + "\n".join(raw) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
