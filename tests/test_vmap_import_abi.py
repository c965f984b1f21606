"""CPU: the C ABI of the voxel map's imports (sdm_vmap_import, sdm_vmap_import_observations and their two structs) --
declared in the header, exported, laid out in ctypes as the C compiler lays out include/sdm_c.h, refusing NULL arguments
without a GPU, and leaving every earlier struct as it was."""
import ctypes
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_class_abi import SIZES as CLASS_SIZES, STRUCTS as CLASS_STRUCTS, UNCHANGED as EARLIER
from test_vmap_obs_abi import _layout

STRUCTS = {
    "sdm_vmap_import_delta": ("VmapImportDelta", ("dst_ids", "updated_ids", "updated_capacity", "on_device", "total", "dropped",
                                                  "first_created", "created", "updated")),
    "sdm_vmap_obs_import": ("VmapObsImport", ("entry", "tag", "entry_map", "map_count", "on_device", "total", "rejected",
                                              "first_created", "created")),
}
FUNCTIONS = {
    "sdm_vmap_import": ["sdm_ctx", "const sdm_point_buffers", "const sdm_vmap_fields", "long long", "sdm_vmap_import_delta"],
    "sdm_vmap_import_observations": ["sdm_ctx", "long long", "sdm_vmap_obs_import"],
}
SIZES = {"sdm_vmap_import_delta": 72, "sdm_vmap_obs_import": 72}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (CLASS_STRUCTS[c][0], CLASS_SIZES[c]) for c in CLASS_STRUCTS})


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def _argtypes(b):
    C = ctypes
    ctx = C.c_void_p
    return {
        "sdm_vmap_import": [ctx, C.POINTER(b.PointBuffers), C.POINTER(b.VmapFields), C.c_longlong, C.POINTER(b.VmapImportDelta)],
        "sdm_vmap_import_observations": [ctx, C.c_longlong, C.POINTER(b.VmapObsImport)],
    }


def test_header_declares_structs_and_functions():
    text = open(os.path.join(ROOT, "include", "sdm_c.h")).read()
    for name in STRUCTS:
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    for name, want in FUNCTIONS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        kinds = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0].strip() for a in args.split(",")]
        assert kinds == want, (name, kinds)
    assert text.index("int sdm_vmap_fetch_published") < text.index("int sdm_vmap_import")
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    # the four limits name the import now, and the new block says what does not travel
    assert len(re.findall(r"one rank only[^.]*?sdm_vmap_import", flat)) == 4
    for phrase in ("I1:", "I2:", "I3:", "STRICTLY", "min(2^32 - 1, multiplicity + m_r)", "0xFFFFFFFF", "do not travel",
                   "28 B", "no refusal depends on device data"):
        assert phrase in flat, phrase


def test_symbols_exported_and_argtypes(pkg):
    b = _binding(pkg)
    raw = ctypes.CDLL(pkg.lib_path())
    syms = {s[0]: s for s in b.SYMBOLS}
    lib = pkg.load_library()
    for name, want in _argtypes(b).items():
        assert hasattr(raw, name), name
        assert syms[name][1] is ctypes.c_int and syms[name][2] == want, name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want and fn.restype is ctypes.c_int, name
    assert b.VMAP_IMPORT_OUTS == tuple(f for f, _ in b.VmapImportDelta._fields_[4:])
    assert b.VMAP_OBS_IMPORT_OUTS == tuple(f for f, _ in b.VmapObsImport._fields_[5:])
    for f in ("vmap_import", "vmap_import_observations"):
        assert callable(getattr(pkg.Engine, f)), f
    shard = sys.modules.get(pkg.__name__ + ".shard") or __import__(pkg.__name__ + ".shard", fromlist=["x"])
    assert callable(shard.vmap_allgather_merge)


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
    # the imports exist beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_import")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    pb, vf, d, io = b.PointBuffers(), b.VmapFields(), b.VmapImportDelta(), b.VmapObsImport()
    d.total = d.dropped = d.first_created = d.created = d.updated = 7
    assert lib.sdm_vmap_import(None, ctypes.byref(pb), ctypes.byref(vf), 0, ctypes.byref(d)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(d, f) for f in b.VMAP_IMPORT_OUTS] == [0] * 5  # the outs of a refusal
    assert lib.sdm_vmap_import(None, None, None, 0, ctypes.byref(d)) == 1
    assert lib.sdm_vmap_import(None, ctypes.byref(pb), None, 0, None) == 1
    io.total = io.rejected = io.first_created = io.created = 7
    assert lib.sdm_vmap_import_observations(None, 0, ctypes.byref(io)) == 1
    assert [getattr(io, f) for f in b.VMAP_OBS_IMPORT_OUTS] == [0] * 4
    assert lib.sdm_vmap_import_observations(None, 0, None) == 1
