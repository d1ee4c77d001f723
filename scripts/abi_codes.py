"""Return codes of the C ABI: sweep every int-returning symbol of libgpk.so with argument lists
that are refused (or are an empty-batch no-op) before the device is touched, and compare the codes
with the recorded fixture tests/golden/abi_codes.json.

  python scripts/abi_codes.py                       compare the built library with the fixture
  GPK_LIB=<parent build>/libgpk.so python scripts/abi_codes.py --record tests/golden/abi_codes.json \
      --source <parent>/csrc/gpk_capi.hip           record, and report the codes no list reached

The entry points are handed fake pointers, so this is for a machine without a GPU (it exits at once
on one with a device), and the unmutated base list is never called: every list holds at least one
mutation that the ABI is known to refuse, declared in SPEC below from include/gpk.h and the shim's
ladders. The plan is deterministic (no RNG); its digest is stored with the codes, so the plan and
the fixture cannot drift apart silently (tests/test_abi_codes_host.py).

Per symbol the plan holds
  1. every refused single mutation ("anchor": a required pointer NULL, a pointer that must be
     16-byte aligned misaligned, a count -1 / 0, a size above its limit, a bad float);
  2. every other mutation (an optional pointer NULL, a size on the accepted side of a limit, ...)
     together with the symbol's last unconditionally required pointer NULL, which pins that the
     mutation alone is accepted;
  3. (pointer NULL) x (integer -1 or the first value above its limit), which pins which of two bad
     arguments is reported;
  4. the hand-written lists of SPEC["also"] for checks that need two or three arguments at once.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_codes.json")

LIMITS = (64, 65, 256, 257, 800, 801, 16384, 16385, 65535, 65536)   # both sides of every limit of the shim
INT_VALUES = (-1, 0) + LIMITS
FLOAT_VALUES = (-1.0, math.nan)
NULL, MISALIGNED = "null", "misaligned"   # misaligned: 4-byte but not 16-byte aligned

# ints that count something: -1 is refused by every symbol, 0 is refused or makes the call a no-op
COUNTS = {"B", "N", "M", "D", "O", "Ns", "m", "n", "F", "T", "R"}
# ... but for an empty batch gpk_variational_elbo_grad_f32 zero-fills dm / ds: that touches the device
ZERO_UNSAFE = {("gpk_variational_elbo_grad_f32", "R")}

BASE = {"B": 2, "N": 8, "M": 8, "D": 4, "O": 2, "Ns": 4, "m": 2, "n": 8, "S": 1, "R": 2, "F": 3, "T": 8,
        "n_enc": 4, "pred_len": 2, "target_col": 0, "max_tries": 3, "n_lengthscale": 1, "shared_x": 1,
        "trans": 0, "kind": 0, "slots": 4, "item": 0, "items": 1, "hyp_stride": 0, "ldy": 8, "ldm": 8,
        "ldv": 8, "n_rows": 16, "n0": 4, "n1": 4,
        "jitter": 1e-4, "chol_jitter": 1e-8, "kl_scale": 1.0, "min_var": 1e-6}


def _not01(v):
    return v not in (0, 1)


def _tries(v):
    return v < 0 or v > 12


def _negative(v):
    return not v >= 0   # NaN too


def _spec(req="", cond="", align="", over=None, bad=None, also=(), base=None):
    """req: pointers refused when NULL whatever else the list holds; cond: refused when NULL with
    the base list's other values; align: refused when not 16-byte aligned; over: {int: largest
    accepted value}; bad: {argument: predicate of the refused values} for what COUNTS / over do
    not describe; also: extra lists {argument: value}, each known to be refused; base: base-list
    overrides."""
    return {"req": req.split(), "cond": cond.split(), "align": align.split(), "over": over or {},
            "bad": bad or {}, "also": list(also), "base": base or {}}


_NLS = {"n_lengthscale": lambda v: v not in (1, 4)}            # 1 or D (= 4 in the base list)
_PERWIN = {**_NLS, "hyp_stride": lambda v: v != 0 and v < 4}   # 0 or >= 3 + n_lengthscale
_MD = {"M": 256, "D": 64}
_NO_GRADS = {"gmean": NULL, "gvar": NULL, "gcov": NULL}
_NO_KL = {"kl": NULL, "gkl": NULL}
_TILE_GRID = {"B": 65536, "N": 65536}    # B * T (T + 1) / 2 tiles, T = N / 64, exceed grid x
_B_GRID = {"B": 1 << 29}                 # 4 B (the Cholesky q(u) covariance: 8 B) workgroups exceed grid x
# the saved-state training pair exists for M > 64 only: with M = 256 the saved state is a real
# argument (gpk_variational_saved_bytes(2, 8, 256, 4) > 0), at M <= 64 a non-NULL one is refused
_SAVED_M = {"M": lambda v: v <= 64 or v > 256}


def _exact(req, cond="", align="", over=None, also=(), perwin=False, **kw):
    bad = dict(_PERWIN if perwin else _NLS)
    bad.update(kw.pop("bad", {}))
    return _spec(req, cond, align, over, bad, also, **kw)


def _exact_pair(name, *a, **kw):
    return {f"gpk_exact_{name}_f32": _exact(*a, **kw), f"gpk_exact_{name}_perwin_f32": _exact(*a, perwin=True, **kw)}


SPEC = {}
SPEC.update(_exact_pair("mll", "X y hyp mll info", over={"N": 800},
                        bad={"jitter": _negative, "max_tries": _tries},
                        also=[{"N": 257, "L": NULL}, {"N": 257, "D": 65}]))
SPEC.update(_exact_pair("mll_grad", "X L z hyp gout dhyp", cond="workspace", over={"N": 800, "D": 64}))
SPEC.update(_exact_pair("posterior", "X L z hyp Xs mean var", over={"N": 800, "D": 64}))
SPEC.update(_exact_pair("posterior_cov", "X L z hyp Xs workspace mean var cov", align="workspace",
                        over={"N": 800, "D": 64}, also=[{"N": 257, "B": 65536}]))
SPEC.update(_exact_pair("posterior_grad", "X L z hyp Xs state workspace dhyp", align="state workspace",
                        over={"N": 256, "Ns": 256, "D": 64}, also=[_NO_GRADS]))
# N + m <= 800 with the base list's m = 2
SPEC.update(_exact_pair("append", "X L z hyp Xn yn Lout zout info", cond="workspace", align="workspace",
                        over={"N": 798, "m": 256, "D": 64}, bad={"jitter": _negative},
                        also=[{"N": 257, "B": 65536}]))
SPEC["gpk_exact_drop_f32"] = _spec("L z Lout zout", over={"N": 800, "m": 7})   # m < N = 8
SPEC["gpk_kzz_chol_f64"] = _spec("Z hyp L Linv info", over=_MD, bad={"max_tries": _tries})
SPEC["gpk_kzz_backward_f64"] = _spec("dLinv L Linv Z hyp workspace dZ dhyp", over=_MD)
SPEC["gpk_gauss_ell_f32"] = _spec("y mean var noise ell")
SPEC["gpk_gauss_ell_grad_f32"] = _spec("y mean var noise gell")
SPEC["gpk_meanfield_kl_f32"] = _spec("m s", cond="dm ds", also=[_NO_KL])
_LD = {k: (lambda v: v < 8) for k in ("ldy", "ldm", "ldv")}   # a row stride below N
SPEC["gpk_variational_elbo_f32"] = _spec("y mean var noise m s elbo", bad=_LD)
SPEC["gpk_variational_elbo_grad_f32"] = _spec("y mean var noise m s dm ds", cond="gelbo dmean dvar dnoise_part",
                                              bad=_LD)
SPEC["gpk_record_check"] = _spec("counter", cond="info in0 in1 ring sticky",
                                 bad={"kind": lambda v: v < 0 or v > 2, "slots": lambda v: v < 1,
                                      "item": lambda v: v != 0, "items": lambda v: v < 1})
SPEC["gpk_variational_f32"] = _spec("X Z Linv vmean vstd hyp mean var", cond="y", over=_MD)
SPEC["gpk_variational_train_f32"] = _spec("X Z Linv vmean vstd hyp mean var", cond="y saved", over=_MD,
                                          base={"M": 256})
SPEC["gpk_variational_batched_f32"] = _spec("X Z Linv vmean vstd hyp mean var", over={"D": 64, "O": 65535},
                                            bad=_SAVED_M, base={"M": 256})
SPEC["gpk_variational_adjoint_f32"] = _spec("X Z Linv vmean vstd hyp gmean gvar workspace dX dLinv dZ dpar",
                                            over=_MD)
SPEC["gpk_variational_adjoint_saved_f32"] = _spec(
    "X Z Linv vmean vstd hyp gmean gvar saved workspace dX dLinv dZ dpar", over={"D": 64}, bad=_SAVED_M,
    base={"M": 256})
SPEC["gpk_variational_adjoint_batched_f32"] = _spec(
    "X Z Linv vmean vstd hyp gmean gvar workspace dX dLinv dZ dpar", over={"D": 64, "O": 65535}, bad=_SAVED_M,
    base={"M": 256})
SPEC["gpk_variational_cov_f32"] = _spec("X Z Linv vstd hyp workspace cov", align="workspace", over=_MD,
                                        also=[_TILE_GRID])
SPEC["gpk_variational_cov_grad_f32"] = _spec("X Z Linv vstd hyp state gcov workspace dX dLinv dZ dpar",
                                             align="state workspace", over={"N": 256, **_MD}, also=[_B_GRID])
SPEC["gpk_variational_chol_f32"] = _spec("X Z Linv vmean vchol hyp mean var", align="saved", over=_MD)
SPEC["gpk_variational_chol_adjoint_f32"] = _spec(
    "X Z Linv vmean vchol hyp gmean gvar saved workspace dX dLinv dZ dpar dchol", align="saved workspace",
    over={"N": 256, **_MD}, also=[_B_GRID])
SPEC["gpk_variational_chol_cov_f32"] = _spec("X Z Linv vchol hyp workspace cov", align="workspace", over=_MD,
                                             also=[_TILE_GRID])
SPEC["gpk_variational_chol_cov_grad_f32"] = _spec(
    "X Z Linv vchol hyp state gcov workspace dX dLinv dZ dpar dchol", align="state workspace",
    over={"N": 256, **_MD}, also=[_B_GRID])
SPEC["gpk_cholesky_kl_f32"] = _spec("m chol", cond="dm dchol", over={"M": 16384}, also=[_NO_KL])
for _single, _name in (("gpk_kzz_chol_f64", "gpk_kzz_chol_f64_batched"),
                       ("gpk_kzz_backward_f64", "gpk_kzz_backward_f64_batched"),
                       ("gpk_variational_cov_f32", "gpk_variational_cov_batched_f32"),
                       ("gpk_variational_cov_grad_f32", "gpk_variational_cov_grad_batched_f32"),
                       ("gpk_variational_chol_f32", "gpk_variational_chol_batched_f32"),
                       ("gpk_variational_chol_adjoint_f32", "gpk_variational_chol_adjoint_batched_f32"),
                       ("gpk_variational_chol_cov_f32", "gpk_variational_chol_cov_batched_f32"),
                       ("gpk_variational_chol_cov_grad_f32", "gpk_variational_chol_cov_grad_batched_f32"),
                       ("gpk_cholesky_kl_f32", "gpk_cholesky_kl_batched_f32")):
    SPEC[_name] = {**SPEC[_single], "over": {**SPEC[_single]["over"], "O": 65535}}   # plus O in 1 .. 65535
SPEC["gpk_mvn_root_f32"] = _spec("cov info", cond="mean eps samples", over={"n": 256},
                                 bad={"jitter": _negative, "S": lambda v: v < 0})
SPEC["gpk_mvn_root_grad_f32"] = _spec("R dcov", cond="gsamples eps workspace", align="workspace", over={"n": 256},
                                      bad={"S": lambda v: v < 0})
SPEC["gpk_tri_solve_f32"] = _spec("R d w", over={"n": 256}, bad={"trans": _not01})
SPEC["gpk_mvn_root_refine_f32"] = _spec("cov R Rout", cond="workspace", align="workspace", over={"n": 256},
                                        bad={"jitter": _negative})
SPEC["gpk_window_gather_f32"] = _spec(
    "table", cond="rows enc dec y",
    bad={"n_rows": lambda v: v < 0, "n_enc": lambda v: v < 0 or v > 8, "pred_len": lambda v: v < 0 or v > 4,
         "target_col": lambda v: v < 0 or v > 2})


def prototypes():
    """{symbol: (return type, [(type, name), ...])} of include/gpk.h, types normalised to 'ptr',
    'int', 'long long', 'float', 'double', 'size_t' ('const char*' for the one string return)."""
    src = open(os.path.join(ROOT, "include", "gpk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t|const char\*)\s+(gpk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        plist = []
        for a in (x.strip() for x in args.split(",")):
            if a == "void" or not a:
                continue
            m = re.fullmatch(r"(.*?)(\w+)", a, flags=re.S)
            typ = " ".join(m.group(1).replace("const", " ").split())
            plist.append(("ptr" if "*" in typ else typ, m.group(2)))
        out[name] = (ret, plist)
    return out


def _is_anchor(sym, spec, kind, name, v):
    if kind == "ptr":
        return (v == NULL and name in spec["req"] + spec["cond"]) or (v == MISALIGNED and name in spec["align"])
    if name in spec["bad"]:
        return bool(spec["bad"][name](v))
    if kind in ("float", "double"):
        return False
    if name in spec["over"] and v > spec["over"][name]:
        return True
    return name in COUNTS and (v == -1 or (v == 0 and (sym, name) not in ZERO_UNSAFE))


def plan():
    """{symbol: [list, ...]}, a list = {argument index: value} applied to the symbol's base list."""
    from fine_grained_gaussian_process_forcasting_amd import _native
    protos = prototypes()
    out = {}
    for sym, (res, argtypes) in _native.SIGNATURES.items():
        if res is not ctypes.c_int or not argtypes:
            continue
        spec, params = SPEC[sym], protos[sym][1]
        index = {name: i for i, (_, name) in enumerate(params)}
        for name in spec["req"] + spec["cond"] + spec["align"] + list(spec["over"]) + list(spec["bad"]):
            assert name in index, (sym, name)
        muts = []
        for i, (kind, name) in enumerate(params):
            if name == "stream":
                continue
            values = ((NULL, MISALIGNED) if kind == "ptr" else
                      FLOAT_VALUES if kind in ("float", "double") else INT_VALUES)
            muts += [(i, kind, name, v) for v in values]
        anchors = [m for m in muts if _is_anchor(sym, spec, *m[1:])]
        tail = index[spec["req"][-1]]
        lists = [{i: v} for i, _, _, v in anchors]
        lists += [{i: v, tail: NULL} for i, kind, name, v in muts
                  if not _is_anchor(sym, spec, kind, name, v) and i != tail]
        nulls = [m for m in anchors if m[3] == NULL]
        for i, kind, name, v in anchors:
            if kind not in ("int", "long long"):
                continue
            above = [x for x in LIMITS if name in spec["over"] and x > spec["over"][name]]
            if v == -1 or (above and v == above[0]):
                lists += [{p: NULL, i: v} for p, _, _, _ in nulls]
        lists += [{index[k]: v for k, v in extra.items()} for extra in spec["also"]]
        out[sym] = lists
    return out


def base_list(sym, params):
    """A list the symbol would accept: distinct, far-apart 16-byte-aligned fake pointers (the
    overlap checks of gpk_exact_drop_f32 pass) and small in-range sizes."""
    over = SPEC[sym]["base"]
    return [(i + 1) << 36 if kind == "ptr" else over.get(name, BASE[name]) for i, (kind, name) in enumerate(params)]


def digest(p) -> str:
    """Of the plan and the base lists: what a fixture's codes are the answers to."""
    protos = prototypes()
    doc = [[sym, base_list(sym, protos[sym][1]), [sorted((i, repr(v)) for i, v in m.items()) for m in lists]]
           for sym, lists in sorted(p.items())]
    return hashlib.sha256(json.dumps(doc).encode()).hexdigest()


def describe(sym, mut) -> str:
    params = prototypes()[sym][1]
    return ", ".join(f"{params[i][1]} = {v}" for i, v in sorted(mut.items()))


def replay(lib, p):
    """{symbol: [code, ...]} of the plan's lists. `lib`: _native.lib() (argtypes bound)."""
    protos = prototypes()
    out = {}
    for sym, lists in p.items():
        fn, base = getattr(lib, sym), base_list(sym, protos[sym][1])
        codes = []
        for mut in lists:
            args = list(base)
            for i, v in mut.items():
                args[i] = None if v == NULL else base[i] + 4 if v == MISALIGNED else v
            codes.append(fn(*args))
        out[sym] = codes
    return out


def unreached(sources, codes):
    """{symbol: [code, ...]}: the `return -k` of each symbol's body in `sources` (the C ABI units
    of the build that was recorded) that no list reached."""
    text = "\n".join(open(s).read() for s in sources)
    out = {}
    for sym, got in codes.items():
        m = re.search(r"^int " + sym + r"\([^)]*\)\s*\{", text, flags=re.M)
        if m is None:
            out[sym] = ["body not found"]
            continue
        depth, k = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[k], 0)
            k += 1
        want = {-int(x) for x in re.findall(r"return -(\d+)", text[m.end():k])}
        missing = sorted(want - set(got), reverse=True)
        if missing:
            out[sym] = missing
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", metavar="PATH", help="write the codes of the library named by GPK_LIB")
    ap.add_argument("--source", action="append", default=[], metavar="FILE",
                    help="with --record: the recorded build's C ABI sources, for the codes-not-reached report")
    ap.add_argument("--fixture", default=FIXTURE)
    args = ap.parse_args()
    import torch
    if torch.cuda.is_available():
        sys.exit("abi_codes.py hands fake pointers to the entry points: run it on a machine without a GPU")
    sys.path.insert(0, ROOT)
    from fine_grained_gaussian_process_forcasting_amd import _native
    p = plan()
    codes = replay(_native.lib(), p)
    positive = [(s, describe(s, m), c) for s in p for m, c in zip(p[s], codes[s]) if c > 0]
    if positive:
        print("lists that reached the device (the plan must not hold them):", *positive, sep="\n  ")
        return 2
    n = sum(len(v) for v in codes.values())
    if args.record:
        with open(args.record, "w") as f:
            json.dump({"library": "recorded from a build of the parent commit", "digest": digest(p), "codes": codes},
                      f, separators=(",", ":"))
            f.write("\n")
        print(f"recorded {n} codes of {len(codes)} symbols from {_native.library_path()}")
        if args.source:
            missing = unreached(args.source, codes)
            print("codes not reached:", "none" if not missing else "")
            for sym, c in missing.items():
                print(f"  {sym}: {c}")
        return 0
    fixture = json.load(open(args.fixture))
    if fixture["digest"] != digest(p):
        print("the plan's digest differs from the fixture's: re-record the fixture from the parent commit")
        return 1
    bad = 0
    for sym, lists in p.items():
        for mut, want, got in zip(lists, fixture["codes"][sym], codes[sym]):
            if want != got:
                bad += 1
                print(f"{sym}({describe(sym, mut)}): fixture {want}, {_native.library_path()} {got}")
    print(f"{n} codes of {len(codes)} symbols, {bad} differ from {os.path.relpath(args.fixture, ROOT)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
