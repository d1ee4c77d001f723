"""A/B proof for the exact forward: one library against another across builds (GPK_LIB selects the
build, as in time_exact.py), bit for bit. The sibling of var_ab.py for gpk_exact_kernel; the
comparison is var_ab.compare.

    python scripts/exact_ab.py digest OUT.json [NB,NB,...]   SHA-256 of L, z, MLL, info per shape (GPU)
    python scripts/exact_ab.py compare A.json B.json          exit 1 and the differing entries on any difference

The shapes reach every instantiation of gpk_exact_kernel<NB, W, STAMPS, FULL, OCC> (54 + stamps):
NB = 1..16 (or the NB list given: 8,16 for a GPK_EXACT_DEV build), N = 16 NB (FULL) and 16 NB - 3
(padded), D = 5 (fast prologue, ragged), 32 (fast prologue, DC = 2) and 40 (staged prologue),
B = 3 (one window per CU; 16 waves from NB = 6) and from NB = 6 also B = compute units + 1 (two
windows per CU), each with L and z written and with neither. Window 1 is N copies of one point at
zero noise (the in-kernel jitter ladder). The stamps instantiation (N = 256) goes through
gpk_debug_exact_stamps: its L, z, MLL and info, not the clocks.
"""
import hashlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def digest(out, nbs):
    import torch
    from fine_grained_gaussian_process_forcasting_amd import _native, ops
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ent, rows = {}, []

    def sha(key, t):
        if t is not None:
            ent[key] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    def inputs(B, N, D, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        X = torch.randn(B, N, D, generator=g, device=dev) / math.sqrt(D)
        X[1] = X[1, :1].expand(N, D)
        return X.contiguous(), torch.randn(B, N, generator=g, device=dev)

    for NB in nbs:
        for N in (16 * NB, 16 * NB - 3):
            for D in (5, 32, 40):
                for B in (3, cus + 1) if NB >= 6 else (3,):
                    X, y = inputs(B, N, D, 1000 * NB + D)
                    k = f"NB{NB} N{N} D{D} B{B}"
                    rows.append([k, f"<{NB}, {16 if NB >= 6 and B == 3 else (8 if NB >= 6 else 4)}, false, "
                                    f"{'true' if N == 16 * NB else 'false'}, {1 if NB >= 6 and B == 3 else 2}>"])
                    for on in (True, False):
                        o = ops.exact_mll(X, y, 0.3, 1.0, 0.0, 0.0, want_L=on, want_z=on)
                        for n in ("L", "z", "mll", "info"):
                            sha(f"{k}/{'Lz' if on else 'mll_only'}/{n}", getattr(o, n))
                    torch.cuda.synchronize()
                    print(rows[-1][0], rows[-1][1], flush=True)
    if 16 in nbs:
        B, N, D = 5, 256, 32
        X, y = inputs(B, N, D, 77)
        hyp = ops.pack_exact_hyper(1.0, 0.0, 0.0, 0.3, dev)
        L, mll = torch.empty(B, N, N, device=dev), torch.empty(B, device=dev)
        info = torch.empty(B, dtype=torch.int32, device=dev)
        st = torch.zeros(B, 32 + 16 * 8 * 8, dtype=torch.int64, device=dev)
        z = torch.empty(B, N, device=dev)
        rc = _native.lib().gpk_debug_exact_stamps(X.data_ptr(), y.data_ptr(), hyp.data_ptr(), 1, B, N, D, 1e-6, 3,
                                                  L.data_ptr(), z.data_ptr(), mll.data_ptr(), info.data_ptr(),
                                                  st.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        k = f"stamps N{N} D{D} B{B}"
        rows.append([k, "<16, 8, true, true, 2>"])
        for n, t in (("L", L), ("z", z), ("mll", mll), ("info", info)):
            sha(f"{k}/{n}", t)
        print(*rows[-1], flush=True)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.relpath(os.path.abspath(_native.library_path()), root)   # (no machine paths in the record)
    json.dump({"lib": lib, "rows": rows, "entries": ent}, open(out, "w"), indent=0)
    print(f"{len(ent)} output digests of {len(rows)} shapes -> {out}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "digest" and len(sys.argv) in (3, 4):
        digest(sys.argv[2], [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) == 4 else list(range(1, 17)))
    elif mode == "compare" and len(sys.argv) == 4:
        from var_ab import compare
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
