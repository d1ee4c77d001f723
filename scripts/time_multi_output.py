"""Forward and forward + backward times of an O-output DeepGP layer (HIP events, warm-up, the
median of REPS single-step timings), at the reference's sizes b=256, N=192, M=256, D=32 for
O in {1, 4, 8}, plus the unbatched layer (output_dims=None) and the batched factor stage.

    python scripts/time_multi_output.py [--tree DIR] [--reps 50] [--b 256] [--n 192] [--m 256] [--d 32]

--tree DIR imports the package from another checkout (an A/B against the parent commit: run the
two trees alternately in one session and compare the medians against the spread of repeated
runs of one tree). The script uses the public layer API only, so it runs on both. Prints one
JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--b", type=int, default=256)
ap.add_argument("--n", type=int, default=192)
ap.add_argument("--m", type=int, default=256)
ap.add_argument("--d", type=int, default=32)
ap.add_argument("--outputs", type=int, nargs="*", default=[1, 4, 8])
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
from fine_grained_gaussian_process_forcasting_amd import ops, settings  # noqa: E402
from fine_grained_gaussian_process_forcasting_amd.denoising_model.DeepGP import ToyDeepGPHiddenLayer  # noqa: E402

dev = torch.device("cuda", 0)
b, N, M, D = args.b, args.n, args.m, args.d
g = torch.Generator().manual_seed(0)
x = (torch.randn(b, N, D, generator=g) / math.sqrt(D)).to(dev)


def median_ms(fn, reps):
    """Median over reps of one call between its own event pair (the host launch overhead of
    the call's kernels is part of what a training step pays)."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(a.elapsed_time(e))
    return statistics.median(ts)


def layer_times(output_dims):
    layer = ToyDeepGPHiddenLayer(input_dims=D, output_dims=output_dims, seed=0, num_inducing=M,
                                 mean_type="linear").to(dev)
    gm = torch.randn(1, b, N, *(() if output_dims is None else (output_dims,)), generator=g).to(dev)
    vs = layer.variational_strategy

    def clear():   # every step refactors K_ZZ, as training does after an optimizer step
        vs._kzz_cache.clear()
        for c in getattr(vs, "_kzz_caches", []):
            c.clear()

    def fwd():
        clear()
        with torch.no_grad():
            out = layer(x)
            return out.mean, out.variance

    def fwd_bwd():
        clear()
        layer.zero_grad(set_to_none=True)
        out = layer(x)
        ((gm * out.mean).sum() + (gm * out.variance).sum()).backward()

    with settings.num_likelihood_samples(1):
        return {"fwd_ms": round(median_ms(fwd, args.reps), 4), "fwd_bwd_ms": round(median_ms(fwd_bwd, args.reps), 4)}


res = {"tree": os.path.abspath(args.tree), "b": b, "N": N, "M": M, "D": D, "reps": args.reps,
       "single": layer_times(None)}
for no in args.outputs:
    res[f"O{no}"] = layer_times(no)
if hasattr(ops, "kzz_cholesky_batched"):
    # the factor stage alone: O factor workgroups on O CUs, then T x O inverse workgroups
    fac = {}
    for no in (1, 8):
        Z = (torch.randn(no, M, D, generator=g) / math.sqrt(D)).to(dev)
        hyp = torch.full((no, 1 + D), math.log(2.0), device=dev)
        fac[f"O{no}_ms"] = round(median_ms(lambda: ops.kzz_cholesky_batched(Z, hyp, jitter=1e-4), args.reps), 4)
    fac["O8_over_O1"] = round(fac["O8_ms"] / fac["O1_ms"], 3)
    res["factor"] = fac
print(json.dumps(res), flush=True)
