"""CPU: the C ABI of sdm_get_dispatch_counts -- declared in the header beside the other instrumentation, exported, bound with
the header's types, mirrored by Engine.dispatch_counts, refusing NULL arguments without a GPU -- and sdm_stats left as it
was: the counters of the sliced launches are host-side integers of the context, not fields of that struct."""
import ctypes
import inspect
import os
import re

from test_extract_abi import ROOT
from test_vmap_obs_abi import _layout
from test_vmap_recarve_abi import _binding

STATS = ("searches", "candidates", "gate_pass", "hypotheses", "fused", "mask_waves", "mask_steps", "mask_row_mismatch",
         "open_pixels", "table_stagings")


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    m = re.search(r"int\s+sdm_get_dispatch_counts\s*\(([^;]*)\)\s*;", text)
    assert m
    kinds = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert kinds == ["sdm_ctx *ctx", "long long out[3]", "int reset"], kinds
    assert text.index("int sdm_get_stats") < text.index("int sdm_get_dispatch_counts") < text.index("int sdm_enable_timing")
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    at = flat.rindex("/*", 0, flat.index("int sdm_get_dispatch_counts"))
    note = flat[at:flat.index("*/", at)]
    for phrase in ("SDM_MAX_DISPATCH_LOG2 in [8, 31]", "read by sdm_create", "counted on the host", "sdm_stats does not move",
                   "out[0] = groups", "out[1] = dispatches", "out[2] = groups that took more than one dispatch"):
        assert phrase in note, phrase


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    want = [C.c_void_p, C.POINTER(C.c_longlong), C.c_int]
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_get_dispatch_counts")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_get_dispatch_counts"]
    assert sym[1] is ctypes.c_int and sym[2] == want
    fn = pkg.load_library().sdm_get_dispatch_counts
    assert list(fn.argtypes) == want and fn.restype is ctypes.c_int
    sig = inspect.signature(pkg.Engine.dispatch_counts)
    assert list(sig.parameters)[1:] == ["reset"] and sig.parameters["reset"].default is False


def test_stats_struct_keeps_its_layout(pkg, tmp_path):
    b = _binding(pkg)
    assert tuple(f for f, _ in b.Stats._fields_) == STATS
    got = _layout(tmp_path, "sdm_stats", STATS)
    assert got["size"] == [ctypes.sizeof(b.Stats)] == [8 * len(STATS)]
    for f in STATS:
        fd = getattr(b.Stats, f)
        assert got[f] == [fd.offset, fd.size], f


def test_null_arguments_are_einval(pkg):
    lib = pkg.load_library()
    out = (ctypes.c_longlong * 3)(7, 7, 7)
    assert lib.sdm_get_dispatch_counts(None, out, 0) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert list(out) == [7, 7, 7]
    assert lib.sdm_get_dispatch_counts(None, None, 1) == 1
