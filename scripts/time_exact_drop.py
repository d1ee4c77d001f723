"""Time dropping the m oldest observations from a cached exact-GP factor against the thing it
replaces, over the same tensors:

  drop    ops.exact_drop(L, z, m): gpk_exact_drop_f32 on the cached (L, z) of the N points (the
          factor itself is computed once, outside the timed window)
  refit   ops.exact_mll(..., want_L=True, want_z=True) on the N - m kept points: what
          set_train_data + the next eval call cost before forget_oldest existed
  slide   drop, then ops.exact_append of m later points: a look-back of constant N moved by m
  reslide ops.exact_mll on the N points [m, N + m): the refit that a slide replaces

Shapes (B, N, m, D): (512, 800, 16, 32), (512, 528, 16, 32), (512, 272, 16, 32), (64, 800, 16, 32);
slide / reslide at (512, 800, 16, 32) only. HIP events after 3 warm-up calls, the mean of 20 calls;
every figure comes from a fresh child process (one route, one shape), five alternating pairs per
shape, each child under its own time limit; the first child that fails ends the run (nothing is
started again). The drop and slide children also report how far their outputs are from the refit's
(relative, Frobenius, worst window). The project's criterion per shape: the slowest new run is
faster than the fastest old run.

  python scripts/time_exact_drop.py [--out profiles/exact_drop_timing.txt]

Per-kernel split: rocprofv3 --kernel-trace --stats -- python scripts/time_exact_drop.py
--child slide n800
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"n800": (512, 800, 16, 32), "n528": (512, 528, 16, 32), "n272": (512, 272, 16, 32),
          "n800_b64": (64, 800, 16, 32)}
PAIRS = [("drop", "refit", s) for s in SHAPES] + [("slide", "reslide", "n800")]
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

    def fit(lo, hi):
        r = ops.exact_mll(X[:, lo:hi].contiguous(), y[:, lo:hi].contiguous(), None, None, None, None, want_L=True,
                          want_z=True, hyper=hyper)
        assert int(r.info.abs().max()) == 0
        return r

    def rel(a, b):
        return float(((a - b).flatten(1).norm(dim=1) / b.flatten(1).norm(dim=1)).max())

    extra = {}
    if route in ("drop", "slide"):
        f = fit(0, N)
        Xk, Xn, yn = X[:, m:N].contiguous(), X[:, N:].contiguous(), y[:, N:].contiguous()

        def step():
            L2, z2 = ops.exact_drop(f.L, f.z, m)
            if route == "drop":
                return L2, z2
            return ops.exact_append(Xk, L2, z2, hyper, Xn, yn)[:2]

        L2, z2 = step()
        r = fit(m, N) if route == "drop" else fit(m, N + m)
        extra = {"vs_refit_L": rel(L2, r.L), "vs_refit_z": rel(z2, r.z)}
        del L2, z2, r
    else:
        Xr = (X[:, m:N] if route == "refit" else X[:, m:]).contiguous()
        yr = (y[:, m:N] if route == "refit" else y[:, m:]).contiguous()

        def step():
            return ops.exact_mll(Xr, yr, None, None, None, None, want_L=True, want_z=True, hyper=hyper)

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
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    if args.child:
        child(*args.child)
        return 0
    raw, lines = [], []
    for new, old, shape in PAIRS:
        if shape not in args.shapes:
            continue
        ms = {new: [], old: []}
        for rnd in range(args.rounds):
            for route in ((new, old) if rnd % 2 == 0 else (old, new)):
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
        verdict = f"{new} faster" if max(ms[new]) < min(ms[old]) else "NOT faster"
        lines.append(f"{shape} (B={B} N={N} m={m} D={D}): {new} {min(ms[new]):.3f}-{max(ms[new]):.3f} ms, "
                     f"{old} {min(ms[old]):.3f}-{max(ms[old]):.3f} ms, "
                     f"x{min(ms[old]) / max(ms[new]):.2f} (fastest {old} / slowest {new}): {verdict}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Dropping the m oldest observations from a cached factor (ops.exact_drop) against refactoring "
                    "the kept data (ops.exact_mll), and a slide (drop + ops.exact_append) against refactoring the "
                    "moved window, ms per call (HIP events, 20 calls after 3 warm-up; alternating pairs of fresh "
                    f"processes, {args.rounds} per shape)\n" + "\n".join(lines) + "\n\nraw\n" + "\n".join(raw) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
