"""A/B proof for the variational path: one library against itself across builds (GPK_LIB selects
the build, as in time_var.py). A move or a change to a shared helper re-canonicalises the callers'
device code; this shows that the plans and every output bit stayed the same.

    python scripts/var_ab.py plans OUT.json      workspace / saved-state sizes on a shape grid (no device)
    python scripts/var_ab.py digest OUT.json     SHA-256 of every output of every TABLE row (GPU)
    python scripts/var_ab.py compare A.json B.json   exit 1 and the differing entries on any difference
"""
import hashlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# Shapes of the digest, derived from the dispatch in csrc/gpk_variational.hip (first match):
#   M <= 64, D <= 32                      register path
#   M > 64                                L^{-1}-in-registers forward; adjoint: saved-state pair with
#                                         `saved`, else adja + adjk if LAdjGeo fits (not <12|16, 64>)
#                                         and M B N 4 < 2^31
#   everything else                       LDS-tiled kernels
# MB = the instantiated block count M is padded to (1 2 3 4 6 8 12 16 x 16 rows); every MB has one M
# that is a multiple of 16 and one that is not. DQ: forward 16 / 32 / 64 for D <= 16 / <= 32 / else,
# adjoint 32 / 64. Chunks are 32 points (128 / 64 / 32 in the tiled kernels for MB <= 4 / <= 8 /
# else): N = 300 is several chunks and a ragged tail in every kernel.
# (Ms, Ds, B, N, big, kernels the row is there to reach; every adjoint row also runs dlinv (paths
#  with a workspace), red and fin, every forward row ell)
TABLE = [
    ((16, 13, 32, 29, 48, 37, 64, 50), (16,), 3, 300, False, "fwd_r<16>  adj_r<32,8,1>"),
    ((16, 13, 32, 29, 48, 37, 64, 50), (17,), 3, 300, False, "fwd_r<32>  adj_r<32,8,1>"),
    ((16, 13), (33,), 3, 300, False, "fwd<1>  adj<1,64>"),
    ((32, 29), (33,), 3, 300, False, "fwd<2>  adj<2,64>"),
    ((48, 37), (33,), 3, 300, False, "fwd<3>  adj<3,64>"),
    ((64, 50), (33,), 3, 300, False, "fwd<4>  adj<4,64>"),
    ((96, 81), (16, 17), 3, 300, False, "fwd_l<6,16|32>  adja_l adjk_l adjs_l kgram_l <6,32>"),
    ((128, 100), (16, 17), 3, 300, False, "fwd_l<8,16|32>  adja_l adjk_l adjs_l kgram_l <8,32>"),
    ((192, 130), (16, 17), 3, 300, False, "fwd_l<12,16|32>  adja_l adjk_l adjs_l kgram_l <12,32>"),
    ((256, 250), (16, 17), 3, 300, False, "fwd_l<16,16|32>  adja_l adjk_l adjs_l kgram_l <16,32>"),
    ((96, 81), (33,), 3, 300, False, "fwd_l<6,64>  adja_l adjk_l adjs_l kgram_l <6,64>"),
    ((128, 100), (33,), 3, 300, False, "fwd_l<8,64>  adja_l adjk_l adjs_l kgram_l <8,64>"),
    ((192, 130), (33,), 3, 300, False, "fwd_l<12,64>  adj<12,64> (no L^-1 plan, no saved state)"),
    ((256, 250), (33,), 3, 300, False, "fwd_l<16,64>  adj<16,64> (no L^-1 plan, no saved state)"),
    # M B N 4 >= 2^31: the tiled adjoint behind the 32-bit buffer offsets of adja / adjk. The dA and
    # K_ZX workspace is 2 M B N 4 bytes = 4.3 GB per row (+ X, dX up to 0.8 GB each); forward with y
    # and the recompute adjoint only, inputs generated on the device. No smaller route: adj_plan takes
    # the L^{-1} path for every M > 64 whose plan fits unless the workspace is that large.
    ((96,), (4,), 8, 700000, True, "adj<6,32>   4.3 GB workspace"),
    ((128,), (4,), 8, 524300, True, "adj<8,32>   4.3 GB workspace"),
    ((192,), (4,), 8, 349530, True, "adj<12,32>  4.3 GB workspace"),
    ((256,), (4,), 8, 262150, True, "adj<16,32>  4.3 GB workspace"),
    ((96,), (33,), 8, 700000, True, "adj<6,64>   4.3 GB workspace"),
    ((128,), (33,), 8, 524300, True, "adj<8,64>   4.3 GB workspace"),
]

GRID_M = (8, 37, 64, 65, 96, 130, 192, 250, 256)
GRID_D = (4, 16, 17, 32, 33, 64)
GRID_BN = ((1, 1), (3, 40), (256, 192), (4096, 4096))


def plans(out):
    from fine_grained_gaussian_process_forcasting_amd import _native
    lib = _native.lib()
    ent = {}
    for M in GRID_M:
        for D in GRID_D:
            for B, N in GRID_BN:
                k = f"B{B} N{N} M{M} D{D}"
                ent[k + "/adjoint_workspace_bytes"] = lib.gpk_variational_adjoint_workspace_bytes(B, N, M, D)
                ent[k + "/saved_bytes"] = lib.gpk_variational_saved_bytes(B, N, M, D)
                ent[k + "/adjoint_saved_workspace_bytes"] = lib.gpk_variational_adjoint_saved_workspace_bytes(B, N, M, D)
                for s in (0, 1):
                    ent[k + f"/adjoint_batched_workspace_bytes O3 saved{s}"] = \
                        lib.gpk_variational_adjoint_batched_workspace_bytes(3, B, N, M, D, s)
    json.dump({"lib": os.environ.get("GPK_LIB", "default"), "entries": ent}, open(out, "w"), indent=0)
    print(f"{len(ent)} plan sizes of {len(ent) // 5} shapes -> {out}")


def digest(out):
    import torch
    from fine_grained_gaussian_process_forcasting_amd import ops
    dev = torch.device("cuda", 0)
    LN2 = math.log(2.0)
    ent, rows = {}, []

    def sha(key, t):
        if t is not None:
            ent[key] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    def inputs(seed, B, N, M, D):
        g = torch.Generator(device=dev).manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, device=dev)   # noqa: E731
        X, y = r(B, N, D) / math.sqrt(D), r(B, N)
        Z, vm = r(M, D) / math.sqrt(D), 1e-3 * r(M)
        vs = 0.5 + 0.5 * torch.rand(M, generator=g, device=dev)
        ls = LN2 * (1.0 + 0.1 * torch.rand(D, generator=g, device=dev))
        hyper = ops.pack_variational_hyper(LN2, LN2 + 1e-4, 1e-4, 0.1, r(D), ls, D, dev)
        kz = ops.kzz_cholesky(Z, None, None, jitter=1e-4, hyper=torch.cat([hyper[:1], ls]).contiguous())
        return X, y, Z, vm, vs, hyper, kz.Linv, r(B, N), r(B, N)

    def adjoint(key, a):
        for n in ("dX", "dLinv", "dZ", "dpar"):
            sha(f"{key}/{n}", getattr(a, n))

    seed = 0
    for Ms, Ds, B, N, big, kernels in TABLE:
        for M in Ms:
            for D in Ds:
                seed += 1
                k = f"B{B} N{N} M{M} D{D}"
                rows.append([k, kernels])
                X, y, Z, vm, vs, hyper, Linv, gm, gv = inputs(seed, B, N, M, D)
                f = ops.variational_forward(X, Z, Linv, vm, vs, y=y, hyper=hyper)
                for n in ("mean", "var", "ell", "flags"):
                    sha(f"{k}/forward/{n}", getattr(f, n))
                adjoint(f"{k}/adjoint", ops.variational_adjoint(X, Z, Linv, vm, vs, hyper, gm, gv))
                if big:
                    del X, f
                    torch.cuda.empty_cache()
                    print(k, kernels, flush=True)
                    continue
                t = ops.variational_forward(X, Z, Linv, vm, vs, hyper=hyper, save=True)
                for n in ("mean", "var", "flags", "saved"):
                    sha(f"{k}/train/{n}", getattr(t, n))
                if t.saved is not None:
                    adjoint(f"{k}/adjoint_saved", ops.variational_adjoint(X, Z, Linv, vm, vs, hyper, gm, gv,
                                                                           saved=t.saved))
                # O = 2 outputs in one launch chain, inputs shared and per output
                o = [inputs(1000 * seed + j, B, N, M, D) for j in (1, 2)]
                st = lambda i: torch.stack([v[i] for v in o])   # noqa: E731
                for name, Xb in (("shared", o[0][0]), ("per_output", st(0))):
                    fb = ops.variational_forward_batched(Xb, st(2), st(6), st(3), st(4), st(5), save=True)
                    for n in ("mean", "var", "flags", "saved"):
                        sha(f"{k}/batched_{name}/{n}", getattr(fb, n))
                    adjoint(f"{k}/batched_{name}/adjoint",
                            ops.variational_adjoint_batched(Xb, st(2), st(6), st(3), st(4), st(5), st(7), st(8)))
                    if fb.saved is not None:
                        adjoint(f"{k}/batched_{name}/adjoint_saved",
                                ops.variational_adjoint_batched(Xb, st(2), st(6), st(3), st(4), st(5), st(7), st(8),
                                                                saved=fb.saved))
                torch.cuda.synchronize()
                print(k, kernels, flush=True)
    json.dump({"lib": os.environ.get("GPK_LIB", "default"), "rows": rows, "entries": ent}, open(out, "w"), indent=0)
    print(f"{len(ent)} output digests of {len(rows)} shapes -> {out}")


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    ea, eb = a["entries"], b["entries"]
    bad = 0
    for k in sorted(set(ea) | set(eb)):
        if ea.get(k) != eb.get(k):
            print("differs:", k, ea.get(k), eb.get(k))
            bad += 1
    for k, kernels in a.get("rows", []):
        print(f"{k:28s} {kernels}")
    print(f"{a['lib']} vs {b['lib']}: {len(ea)} / {len(eb)} entries, "
          + (f"{bad} DIFFERENT" if bad else "identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "plans" and len(sys.argv) == 3:
        plans(sys.argv[2])
    elif mode == "digest" and len(sys.argv) == 3:
        digest(sys.argv[2])
    elif mode == "compare" and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
