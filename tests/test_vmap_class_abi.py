"""CPU: the C ABI of the voxel map's classification (sdm_vmap_classify, sdm_vmap_get_class_info, sdm_vmap_fetch_published and
their four structs) -- declared in the header, exported, laid out in ctypes as the C compiler lays out include/sdm_c.h,
refusing bad arguments without a GPU, and leaving every earlier struct as it was."""
import ctypes
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_obs_abi import UNCHANGED as EARLIER, _layout

STRUCTS = {
    "sdm_vmap_rule": ("VmapRule", ("min_multiplicity", "min_cameras", "min_ends", "ratio_num", "ratio_den", "max_sigma",
                                   "min_neighbours")),
    "sdm_vmap_class_delta": ("VmapClassDelta", ("accepted_ids", "retracted_ids", "accepted_capacity", "retracted_capacity",
                                                "on_device", "examined", "accepted", "retracted", "published_total")),
    "sdm_vmap_class_info": ("VmapClassInfo", ("published", "calls")),
    "sdm_vmap_published": ("VmapPublished", ("published", "capacity", "on_device")),
}
FUNCTIONS = {
    "sdm_vmap_classify": ["sdm_ctx", "const sdm_vmap_rule", "int", "sdm_vmap_class_delta"],
    "sdm_vmap_get_class_info": ["sdm_ctx", "sdm_vmap_class_info"],
    "sdm_vmap_fetch_published": ["sdm_ctx", "const unsigned", "long long", "long long", "sdm_vmap_published"],
}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, sdm_vmap_observe_delta=("VmapObserveDelta", 40), sdm_vmap_observations=("VmapObservations", 32),
                 sdm_vmap_cameras=("VmapCameras", 48), sdm_vmap_obs_info=("VmapObsInfo", 32))
SIZES = {"sdm_vmap_rule": 32, "sdm_vmap_class_delta": 72, "sdm_vmap_class_info": 16, "sdm_vmap_published": 24}


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def _argtypes(b):
    C = ctypes
    ctx = C.c_void_p
    return {
        "sdm_vmap_classify": [ctx, C.POINTER(b.VmapRule), C.c_int, C.POINTER(b.VmapClassDelta)],
        "sdm_vmap_get_class_info": [ctx, C.POINTER(b.VmapClassInfo)],
        "sdm_vmap_fetch_published": [ctx, C.c_void_p, C.c_longlong, C.c_longlong, C.POINTER(b.VmapPublished)],
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
    assert text.index("int sdm_vmap_fetch_cameras") < text.index("int sdm_vmap_classify")
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    # the earlier limits stay true: classification labels entries, it removes nothing
    for phrase in ("an observation cannot be removed", "never shrink", "camera lists on the persistent map remain later work"):
        assert phrase in flat, phrase
    for phrase in ("no hysteresis", "O(M) per call", "latency-bound", "stale with sdm_set_pose", "one rank only",
                   "1 B per record of capacity", "128 bits", "C1:", "C2:", "C3:", "C4:", "C5:"):
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
    assert tuple(b.VMAP_RULE_DEFAULTS) == tuple(f for f, _ in b.VmapRule._fields_)
    assert b.VMAP_CLASS_OUTS == tuple(f for f, _ in b.VmapClassDelta._fields_[5:])
    for f in ("vmap_classify", "vmap_class_info", "vmap_fetch_published"):
        assert callable(getattr(pkg.Engine, f)), f


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
    # the classification calls exist beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_classify")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    rule, d, info, vp = b.VmapRule(), b.VmapClassDelta(), b.VmapClassInfo(), b.VmapPublished()
    rule.ratio_den = 1
    d.examined = d.accepted = d.retracted = d.published_total = 7
    assert lib.sdm_vmap_classify(None, ctypes.byref(rule), 1, ctypes.byref(d)) == 1
    assert [getattr(d, f) for f in b.VMAP_CLASS_OUTS] == [0] * 4  # the outs of a refusal
    assert lib.sdm_vmap_classify(None, None, 1, ctypes.byref(d)) == 1
    assert lib.sdm_vmap_classify(None, ctypes.byref(rule), 0, None) == 1
    assert lib.sdm_vmap_get_class_info(None, ctypes.byref(info)) == 1
    assert lib.sdm_vmap_get_class_info(None, None) == 1
    assert lib.sdm_vmap_fetch_published(None, None, 0, 0, ctypes.byref(vp)) == 1
    assert lib.sdm_vmap_fetch_published(None, None, 0, 0, None) == 1
