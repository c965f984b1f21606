"""CPU: the C ABI of sdm_vmap_retire and its struct -- declared in the header, exported, laid out in ctypes as the C
compiler lays out include/sdm_c.h, refusing NULL arguments without a GPU, and leaving every earlier struct as it was."""
import ctypes
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_obs_abi import _layout
from test_vmap_repose_abi import SIZES as REPOSE_SIZES, STRUCTS as REPOSE_STRUCTS, UNCHANGED as EARLIER

STRUCTS = {
    "sdm_vmap_retire_delta": ("VmapRetireDelta", ("mode", "carry", "on_device", "remap", "remap_capacity", "dropped_ids",
                                                  "dropped_published", "dropped_capacity", "removed_entry", "removed_tag",
                                                  "removed_capacity", "examined", "dropped", "dropped_were_published", "orphaned",
                                                  "voxels", "observations_before", "observations", "removed", "published_total")),
}
FUNCTIONS = {
    "sdm_vmap_retire": ["sdm_ctx", "int", "const int", "int", "sdm_vmap_retire_delta"],
}
SIZES = {"sdm_vmap_retire_delta": 152}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (REPOSE_STRUCTS[c][0], REPOSE_SIZES[c]) for c in REPOSE_STRUCTS})


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def test_header_declares_struct_constants_and_function():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    for name in STRUCTS:
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    assert re.search(r"#define\s+SDM_VMAP_RETIRE_WINNER\s+0\b", text) and re.search(r"#define\s+SDM_VMAP_RETIRE_UNOBSERVED\s+1\b", text)
    for name, want in FUNCTIONS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        kinds = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0].strip() for a in args.split(",")]
        assert kinds == want, (name, kinds)
    assert text.index("int sdm_vmap_repose") < text.index("int sdm_vmap_retire") < text.index("int sdm_extract_bound")
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    # each of the four "cannot be removed" limits now points at the call
    assert len(re.findall(r"sdm_vmap_retire[ ,(]+below", flat)) == 4
    for limit in ("a keyframe's contribution cannot be removed by these calls", "a keyframe's contribution cannot be removed from the counters",
                  "an observation cannot be removed", "a record cannot be removed by an import"):
        at = flat.index(limit)
        assert "sdm_vmap_retire" in flat[at:flat.index("*/", at)], limit
    for phrase in ("retired iff tag is in R", "integrate, then observe", "rank of i among the survivors", "0xFFFFFFFF for a dropped entry",
                   "the multiplicity is NOT reduced", "del point", "del observation", "commit == 0", "n_tags == 0",
                   "No memory of R", "a tag listed twice", "all counts are filled, no array is written",
                   "everything is allocated before anything is written", "one second set of records",
                   "carried counters still contain the rays of retired keyframes", "one rank only per map"):
        assert phrase in flat, phrase


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    want = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(b.VmapRetireDelta)]
    raw = ctypes.CDLL(pkg.lib_path())
    assert hasattr(raw, "sdm_vmap_retire")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_vmap_retire"]
    assert sym[1] is ctypes.c_int and sym[2] == want
    fn = pkg.load_library().sdm_vmap_retire
    assert list(fn.argtypes) == want and fn.restype is ctypes.c_int
    assert b.VMAP_RETIRE_OUTS == tuple(f for f, _ in b.VmapRetireDelta._fields_[11:])
    assert set(b.VMAP_RETIRE_LISTS) <= set(f for f, _ in b.VmapRetireDelta._fields_[:11])
    assert b.VMAP_RETIRE_MODES == {"winner": 0, "unobserved": 1}
    assert callable(pkg.Engine.vmap_retire)


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
    # the retire exists beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_retire")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    d = b.VmapRetireDelta()
    for f in b.VMAP_RETIRE_OUTS:
        setattr(d, f, 7)
    assert lib.sdm_vmap_retire(None, 0, None, 1, ctypes.byref(d)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(d, f) for f in b.VMAP_RETIRE_OUTS] == [0] * 9  # the outs of a refusal
    assert lib.sdm_vmap_retire(None, 0, None, 1, None) == 1
    tags = (ctypes.c_int * 1)(3)
    assert lib.sdm_vmap_retire(None, 1, tags, 0, ctypes.byref(d)) == 1
