"""CPU: the C ABI of the point-cloud extraction (sdm_extract_points, sdm_point_buffers) -- exported, laid out in ctypes as
the C compiler lays out include/sdm_c.h, and refusing a null context without a GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("xyz", "pixel", "rho_sigma", "intensity", "capacity", "on_device")


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def _c_compiler():
    for cc in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang"):
        p = shutil.which(cc)
        if p:
            return p
    pytest.fail("no C compiler to lay out include/sdm_c.h with")


def test_symbol_exported(pkg):
    b = _binding(pkg)
    raw = ctypes.CDLL(pkg.lib_path())
    assert hasattr(raw, "sdm_extract_points")
    assert "sdm_extract_points" in {s[0] for s in b.SYMBOLS}


def test_point_buffers_layout_matches_header(pkg, tmp_path):
    b = _binding(pkg)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdm_c.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sdm_point_buffers));\n' +
                   "".join('  printf("%s %%zu %%zu\\n", offsetof(sdm_point_buffers, %s), sizeof(((sdm_point_buffers*)0)->%s));\n'
                           % (f, f, f) for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_c_compiler(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines if ln.strip()}
    assert got["size"] == [ctypes.sizeof(b.PointBuffers)]
    for f in FIELDS:
        fd = getattr(b.PointBuffers, f)
        assert got[f] == [fd.offset, fd.size], f


def test_null_context_is_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    pb = b.PointBuffers()
    pb.capacity = 0
    offs = (ctypes.c_longlong * 2)()
    slots = (ctypes.c_int * 1)(0)
    assert lib.sdm_extract_points(None, 1, slots, 1, 0.01, 1e-6, ctypes.byref(pb), offs) == 1  # SDM_EINVAL
    assert lib.sdm_extract_points(None, 1, slots, 1, 0.01, 1e-6, None, None) == 1
