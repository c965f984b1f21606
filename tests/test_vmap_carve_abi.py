"""CPU: the C ABI of the voxel map's free-space evidence (sdm_vmap_carve, sdm_vmap_fetch_evidence, sdm_vmap_carve_args /
sdm_vmap_evidence) -- declared in the header, exported, laid out in ctypes as the C compiler lays out include/sdm_c.h, and
refusing bad arguments without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from test_extract_abi import ROOT, _c_compiler

STRUCTS = {
    "sdm_vmap_carve_args": ("VmapCarveArgs", ("end_margin", "max_steps", "plain_total", "rays_total", "rays_skipped",
                                              "cells_visited", "cells_hit", "ends_hit")),
    "sdm_vmap_evidence": ("VmapEvidence", ("crossings", "ends", "capacity", "on_device")),
}
FUNCTIONS = {
    "sdm_vmap_carve": ["sdm_ctx", "int", "const int", "int", "const int", "int", "double", "double", "sdm_vmap_carve_args"],
    "sdm_vmap_fetch_evidence": ["sdm_ctx", "const unsigned", "long long", "long long", "sdm_vmap_evidence"],
}


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def _argtypes(b):
    C = ctypes
    ip, ctx = C.POINTER(C.c_int), C.c_void_p
    return {
        "sdm_vmap_carve": [ctx, C.c_int, ip, C.c_int, ip, C.c_int, C.c_double, C.c_double, C.POINTER(b.VmapCarveArgs)],
        "sdm_vmap_fetch_evidence": [ctx, C.c_void_p, C.c_longlong, C.c_longlong, C.POINTER(b.VmapEvidence)],
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
    # the limits speak of what exists now
    assert "no camera lists or free-space evidence" not in text
    assert re.search(r"camera lists on\s+\*?\s*the persistent map remain later work", text)


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
    assert b.VMAP_EVIDENCE_FIELDS == ("crossings", "ends")
    assert b.VMAP_CARVE_OUTS == tuple(f for f, _ in b.VmapCarveArgs._fields_[2:])


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_header(pkg, tmp_path, cname):
    b = _binding(pkg)
    pyname, fields = STRUCTS[cname]
    st = getattr(b, pyname)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdm_c.h"\nint main(void) {\n'
                   '  printf("size %%zu\\n", sizeof(%s));\n' % cname +
                   "".join('  printf("%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));\n' % (f, cname, f, cname, f)
                           for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_c_compiler(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines if ln.strip()}
    assert got["size"] == [ctypes.sizeof(st)]
    assert [f[0] for f in st._fields_] == list(fields)
    for f in fields:
        fd = getattr(st, f)
        assert got[f] == [fd.offset, fd.size], f


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    cv, ev = b.VmapCarveArgs(), b.VmapEvidence()
    cv.end_margin, cv.max_steps = 1, 4096
    cv.rays_total = cv.cells_hit = 7
    slots = (ctypes.c_int * 1)(0)
    assert lib.sdm_vmap_carve(None, 1, slots, 0, None, 1, 0.01, 1e-6, ctypes.byref(cv)) == 1
    assert (cv.rays_total, cv.cells_hit) == (0, 0) and (cv.end_margin, cv.max_steps) == (1, 4096)  # the outs of a refusal
    assert lib.sdm_vmap_carve(None, 1, slots, 1, slots, 1, 0.01, 1e-6, None) == 1
    assert lib.sdm_vmap_fetch_evidence(None, None, 0, 0, ctypes.byref(ev)) == 1
    assert lib.sdm_vmap_fetch_evidence(None, None, 0, 0, None) == 1
