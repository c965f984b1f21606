"""CPU: the C ABI of the persistent voxel map (sdm_vmap_*, sdm_vmap_info / _delta / _fields) -- declared in the header,
exported, laid out in ctypes as the C compiler lays out include/sdm_c.h, and refusing bad arguments without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from test_extract_abi import ROOT, _c_compiler

STRUCTS = {
    "sdm_vmap_info": ("VmapInfo", ("voxels", "points", "dropped", "calls", "table_slots", "rehashes", "voxel_size")),
    "sdm_vmap_delta": ("VmapDelta", ("updated_ids", "updated_capacity", "on_device", "plain_total", "dropped", "first_created",
                                     "created", "updated")),
    "sdm_vmap_fields": ("VmapFields", ("tag", "multiplicity", "epoch")),
}
FUNCTIONS = {
    "sdm_vmap_open": ["sdm_ctx", "float", "long long"],
    "sdm_vmap_clear": ["sdm_ctx"],
    "sdm_vmap_close": ["sdm_ctx"],
    "sdm_vmap_get_info": ["sdm_ctx", "sdm_vmap_info"],
    "sdm_vmap_integrate": ["sdm_ctx", "int", "const int", "const int", "int", "double", "double", "sdm_vmap_delta"],
    "sdm_vmap_fetch": ["sdm_ctx", "const unsigned", "long long", "long long", "sdm_point_buffers", "sdm_vmap_fields"],
}


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def _argtypes(b):
    C = ctypes
    ip, ctx = C.POINTER(C.c_int), C.c_void_p
    return {
        "sdm_vmap_open": [ctx, C.c_float, C.c_longlong],
        "sdm_vmap_clear": [ctx],
        "sdm_vmap_close": [ctx],
        "sdm_vmap_get_info": [ctx, C.POINTER(b.VmapInfo)],
        "sdm_vmap_integrate": [ctx, C.c_int, ip, ip, C.c_int, C.c_double, C.c_double, C.POINTER(b.VmapDelta)],
        "sdm_vmap_fetch": [ctx, C.c_void_p, C.c_longlong, C.c_longlong, C.POINTER(b.PointBuffers), C.POINTER(b.VmapFields)],
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


def test_null_ctx_is_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    info, delta, pb, vf = b.VmapInfo(), b.VmapDelta(), b.PointBuffers(), b.VmapFields()
    slots = (ctypes.c_int * 1)(0)
    assert lib.sdm_vmap_open(None, 0.02, 0) == 1
    assert lib.sdm_vmap_clear(None) == 1
    assert lib.sdm_vmap_close(None) == 1
    assert lib.sdm_vmap_get_info(None, ctypes.byref(info)) == 1
    assert lib.sdm_vmap_integrate(None, 1, slots, None, 1, 0.01, 1e-6, ctypes.byref(delta)) == 1
    assert lib.sdm_vmap_integrate(None, 1, slots, slots, 1, 0.01, 1e-6, None) == 1
    assert lib.sdm_vmap_fetch(None, None, 0, 0, ctypes.byref(pb), ctypes.byref(vf)) == 1
    assert lib.sdm_vmap_fetch(None, None, 0, 0, None, None) == 1
