"""CPU: the return codes of the C ABI are the ones recorded in tests/golden/abi_codes.json (from a
build of the commit before the shim's one-body-per-family refactor; scripts/abi_codes.py has the
plan of refused argument lists and re-records it), and _native.SIGNATURES mirrors include/gpk.h."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_script():
    spec = importlib.util.spec_from_file_location("abi_codes", os.path.join(ROOT, "scripts", "abi_codes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


abi_codes = _load_script()
# the sweep hands fake pointers to the entry points: never where a device could be reached
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="fake-pointer sweep: for a machine without a GPU")


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(abi_codes.FIXTURE))


@pytest.fixture(scope="module")
def plan():
    return abi_codes.plan()


def test_plan_digest_matches_fixture(fixture, plan):
    """The fixture's codes answer exactly this plan: a changed plan needs a re-recorded fixture."""
    assert abi_codes.digest(plan) == fixture["digest"]
    assert set(plan) == set(fixture["codes"])
    for sym, lists in plan.items():
        assert len(lists) == len(fixture["codes"][sym]), sym
        assert all(c <= 0 for c in fixture["codes"][sym]), sym   # refused, or an empty-batch no-op


def test_plan_covers_every_int_symbol(plan):
    from fine_grained_gaussian_process_forcasting_amd import _native
    want = {n for n, (res, args) in _native.SIGNATURES.items() if res is ctypes.c_int and args}
    assert set(plan) == want
    assert all(len(v) > 0 for v in plan.values())


@no_gpu
def test_return_codes_match_fixture(fixture, plan):
    from fine_grained_gaussian_process_forcasting_amd import _native
    codes = abi_codes.replay(_native.lib(), plan)
    bad = [f"{sym}({abi_codes.describe(sym, mut)}): fixture {want}, library {got}"
           for sym, lists in plan.items()
           for mut, want, got in zip(lists, fixture["codes"][sym], codes[sym]) if want != got]
    assert not bad, f"{len(bad)} return codes differ from the fixture:\n" + "\n".join(bad[:40])


_CTYPES = {"ptr": ctypes.c_void_p, "int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}


def test_signatures_mirror_header():
    """Return type and, per argument, the class (any pointer -> c_void_p) of every prototype of
    include/gpk.h against _native.SIGNATURES."""
    from fine_grained_gaussian_process_forcasting_amd import _native
    protos = abi_codes.prototypes()
    assert set(protos) == set(_native.SIGNATURES)
    for name, (ret, params) in protos.items():
        res, args = _native.SIGNATURES[name]
        assert res is _CTYPES[ret], f"{name}: returns {ret}, bound as {res}"
        assert len(args) == len(params), f"{name}: {len(params)} arguments in gpk.h, {len(args)} bound"
        for i, ((kind, pname), bound) in enumerate(zip(params, args), 1):
            assert bound is _CTYPES[kind], f"{name}: argument {i} ({pname}) is {kind}, bound as {bound}"
