"""CPU: the C ABI of sdm_vmap_recarve and its struct -- declared in the header, exported, laid out in ctypes as the C
compiler lays out include/sdm_c.h, refusing NULL arguments without a GPU, and leaving every earlier struct as it was."""
import ctypes
import inspect
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_obs_abi import _layout
from test_vmap_retire_abi import SIZES as RETIRE_SIZES, STRUCTS as RETIRE_STRUCTS, UNCHANGED as EARLIER

STRUCTS = {
    "sdm_vmap_recarve_args": ("VmapRecarveArgs", ("end_margin", "max_steps", "reset", "first", "count", "pairs_total", "pairs_unposed",
                                                  "rays_total", "rays_skipped", "cells_visited", "cells_hit", "ends_hit")),
}
FUNCTIONS = {
    "sdm_vmap_recarve": ["sdm_ctx", "int", "const int", "const float", "sdm_vmap_recarve_args"],
}
SIZES = {"sdm_vmap_recarve_args": 88}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (RETIRE_STRUCTS[c][0], RETIRE_SIZES[c]) for c in RETIRE_STRUCTS})


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def test_header_declares_struct_and_function():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    for name in STRUCTS:
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    for name, want in FUNCTIONS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        kinds = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0].strip() for a in args.split(",")]
        assert kinds == want, (name, kinds)
    assert text.index("int sdm_vmap_retire") < text.index("int sdm_vmap_recarve") < text.index("int sdm_extract_bound")
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    # the three limits that postponed the call now point at it
    for limit in ("counters go stale with sdm_set_pose", "carried evidence belongs to rays walked under the old poses",
                  "carried counters still contain the rays of retired keyframes"):
        at = flat.index(limit)
        assert "sdm_vmap_recarve" in flat[at:flat.index("*/", at)], limit
    assert "rebuilding evidence from the log's pairs is not part of this" not in flat
    for phrase in ("adds 1 to pairs_unposed and nothing else", "P is the xyz of record e as it stands now", "no FMA",
                   "A non-finite pose is not an error", "whatever end_margin", "also when the range or the table is empty",
                   "No log (E == 0) is not an error", "a pure function of (records, log, table)", "additive over any split",
                   "ends_hit == rays_total - rays_skipped", "a tag listed twice", "first + count > E", "On a refusal the outs are 0",
                   "everything is allocated before anything is written", "one ray per distinct (entry, tag)", "WINNING point",
                   "one rank only", "recarving a range twice without reset counts twice"):
        assert phrase in flat, phrase


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    want = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(b.VmapRecarveArgs)]
    raw = ctypes.CDLL(pkg.lib_path())
    assert hasattr(raw, "sdm_vmap_recarve")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_vmap_recarve"]
    assert sym[1] is ctypes.c_int and sym[2] == want
    fn = pkg.load_library().sdm_vmap_recarve
    assert list(fn.argtypes) == want and fn.restype is ctypes.c_int
    assert b.VMAP_RECARVE_OUTS == tuple(f for f, _ in b.VmapRecarveArgs._fields_[5:])
    sig = inspect.signature(pkg.Engine.vmap_recarve)
    assert list(sig.parameters)[1:] == ["tags", "Tcw", "end_margin", "max_steps", "reset", "first", "count"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [1, 4096, True, 0, None]


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_header(pkg, tmp_path, cname):
    b = _binding(pkg)
    pyname, fields = STRUCTS[cname]
    st = getattr(b, pyname)
    got = _layout(tmp_path, cname, fields)
    assert got["size"] == [ctypes.sizeof(st)] == [SIZES[cname]]
    assert [f[0] for f in st._fields_] == list(fields)
    for f in fields:
        fd = getattr(st, f)
        assert got[f] == [fd.offset, fd.size], f


@pytest.mark.parametrize("cname", sorted(UNCHANGED))
def test_existing_structs_keep_their_layout(pkg, tmp_path, cname):
    b = _binding(pkg)
    pyname, size = UNCHANGED[cname]
    st = getattr(b, pyname)
    fields = [f[0] for f in st._fields_]
    got = _layout(tmp_path, cname, fields)
    assert got["size"] == [size] == [ctypes.sizeof(st)]
    for f in fields:
        fd = getattr(st, f)
        assert got[f] == [fd.offset, fd.size], f
    # the recarve exists beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_recarve")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    rc = b.VmapRecarveArgs()
    rc.end_margin, rc.max_steps, rc.reset, rc.count = 1, 4096, 1, -1
    for f in b.VMAP_RECARVE_OUTS:
        setattr(rc, f, 7)
    assert lib.sdm_vmap_recarve(None, 0, None, None, ctypes.byref(rc)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(rc, f) for f in b.VMAP_RECARVE_OUTS] == [0] * 7  # the outs of a refusal
    assert (rc.end_margin, rc.max_steps, rc.reset, rc.first, rc.count) == (1, 4096, 1, 0, -1)  # the ins stay
    assert lib.sdm_vmap_recarve(None, 0, None, None, None) == 1
    tags = (ctypes.c_int * 1)(3)
    assert lib.sdm_vmap_recarve(None, 1, tags, None, ctypes.byref(rc)) == 1
