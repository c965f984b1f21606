"""CPU: the C ABI of sdm_vmap_repose and its struct -- declared in the header, exported, laid out in ctypes as the C
compiler lays out include/sdm_c.h, refusing NULL arguments without a GPU, and leaving every earlier struct as it was."""
import ctypes
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_import_abi import SIZES as IMPORT_SIZES, STRUCTS as IMPORT_STRUCTS, UNCHANGED as EARLIER
from test_vmap_obs_abi import _layout

STRUCTS = {
    "sdm_vmap_repose_delta": ("VmapReposeDelta", ("remap", "remap_capacity", "on_device", "carry", "examined", "reposed", "moved",
                                                  "dropped", "merged", "voxels", "observations_before", "observations")),
}
FUNCTIONS = {
    "sdm_vmap_repose": ["sdm_ctx", "int", "const int", "const float", "const float", "sdm_vmap_repose_delta"],
}
SIZES = {"sdm_vmap_repose_delta": 88}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (IMPORT_STRUCTS[c][0], IMPORT_SIZES[c]) for c in IMPORT_STRUCTS})


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
    assert text.index("int sdm_vmap_import_observations") < text.index("int sdm_vmap_repose") < text.index("int sdm_extract_bound")
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    # each of the four "stale with sdm_set_pose" limits now ends in a pointer to the call
    assert len(re.findall(r"sdm_vmap_repose \(below\)", flat)) == 4
    for limit in ("stored xyz go stale after sdm_set_pose", "counters go stale with sdm_set_pose", "lists go stale with sdm_set_pose",
                  "flags go stale with sdm_set_pose"):
        at = flat.index(limit)
        assert "sdm_vmap_repose (below)" in flat[at:flat.index("*/", at)], limit
    for phrase in ("keeps its xyz bits", "OLD epoch", "0xFFFFFFFF for a dropped one", "entry_map = remap", "64-bit sums",
                   "n_poses == 0", "a tag listed twice", "everything is allocated before anything is written",
                   "one second set of records", "only each voxel's winning point is re-placed",
                   "not one repose with the union table", "one rank only per map"):
        assert phrase in flat, phrase


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    want = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(b.VmapReposeDelta)]
    raw = ctypes.CDLL(pkg.lib_path())
    assert hasattr(raw, "sdm_vmap_repose")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_vmap_repose"]
    assert sym[1] is ctypes.c_int and sym[2] == want
    fn = pkg.load_library().sdm_vmap_repose
    assert list(fn.argtypes) == want and fn.restype is ctypes.c_int
    assert b.VMAP_REPOSE_OUTS == tuple(f for f, _ in b.VmapReposeDelta._fields_[4:])
    assert callable(pkg.Engine.vmap_repose)


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
    # the repose exists beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_repose")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    d = b.VmapReposeDelta()
    for f in b.VMAP_REPOSE_OUTS:
        setattr(d, f, 7)
    assert lib.sdm_vmap_repose(None, 0, None, None, None, ctypes.byref(d)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(d, f) for f in b.VMAP_REPOSE_OUTS] == [0] * 8  # the outs of a refusal
    assert lib.sdm_vmap_repose(None, 0, None, None, None, None) == 1
    tags = (ctypes.c_int * 1)(3)
    assert lib.sdm_vmap_repose(None, 1, tags, None, None, ctypes.byref(d)) == 1
