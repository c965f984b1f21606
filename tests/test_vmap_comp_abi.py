"""CPU: the C ABI of sdm_vmap_components and its struct -- declared in the header, exported, laid out in ctypes as the C
compiler lays out include/sdm_c.h, refusing NULL arguments without a GPU, and leaving every earlier struct as it was."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_cast_abi import SIZES as CAST_SIZES, STRUCTS as CAST_STRUCTS, UNCHANGED as EARLIER
from test_vmap_obs_abi import _c_compiler, _layout

STRUCTS = {
    "sdm_vmap_comp_args": ("VmapCompArgs", ("connectivity", "min_multiplicity", "require_published", "min_size", "on_device",
                                            "capacity", "small_capacity", "label", "size", "small_ids", "entries", "members",
                                            "components", "largest", "small", "small_components")),
}
FUNCTIONS = {"sdm_vmap_components": ["sdm_ctx", "sdm_vmap_comp_args"]}
SIZES = {"sdm_vmap_comp_args": 112}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (CAST_STRUCTS[c][0], CAST_SIZES[c]) for c in CAST_STRUCTS})
INS = ("connectivity", "min_multiplicity", "require_published", "min_size", "on_device", "capacity", "small_capacity")


def _binding(pkg):
    pkg.load_library()
    return sys.modules[pkg.__name__ + ".binding"]


def _own_layout(tmp_path, cname, fields):
    """_layout for a struct with a field called `size`: {"sizeof": [bytes], field: [offset, bytes]}"""
    src = tmp_path / "own_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdm_c.h"\nint main(void) {\n'
                   '  printf("sizeof %%zu\\n", sizeof(%s));\n' % cname +
                   "".join('  printf("%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));\n' % (f, cname, f, cname, f)
                           for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "own_layout"
    subprocess.check_call([_c_compiler(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in lines if ln.strip()}


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
    assert text.index("int sdm_vmap_render") < text.index("int sdm_vmap_components") < text.index("int sdm_extract_bound")
    assert re.search(r"#define SDM_VMAP_NO_COMPONENT 0xFFFFFFFFu\b", text)
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("entry id is a MEMBER iff multiplicity[id] >= min_multiplicity", "if no classify has run every flag reads 0",
                   "floorf(xyz_k * inv) of its record, as sdm_vmap_classify forms it", "d in {-1, 0, 1}^3, d != 0",
                   "1, 2, 3 for connectivity = 6, 18, 26", "outside [-2^20, 2^20) holds nothing",
                   "the range test comes before the key is formed", "the transitive closure of \"both members, cells adjacent\"",
                   "label[id] = the smallest id of its component", "size[id] = the number of members of its component",
                   "A non-member gets label SDM_VMAP_NO_COMPONENT and size 0", "Ids stay below 2^30",
                   "fewer than min_size members", "min_size == 0 lists nothing", "largest = the size of the largest component (0 without members)",
                   "all three NULL is valid and gives the totals only", "M == 0 is valid and queues nothing",
                   "the six totals are filled and no destination is written", "The caller sizes the array and calls again",
                   "whatever the table layout", "before anything is queued", "connectivity not 6, 18 or 26",
                   "require_published not 0 or 1", "a negative capacity", "capacity < M with label or size given",
                   "a misaligned device pointer", "raised before any launch", "O(M) per call and not incremental",
                   "voxel-level -- the winning point's cell", "goes stale with sdm_set_pose", "there is no hysteresis",
                   "the flags are not touched", "one rank only"):
        assert phrase in flat, phrase


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    types = [C.c_void_p, C.POINTER(b.VmapCompArgs)]
    raw = ctypes.CDLL(pkg.lib_path())
    lib = pkg.load_library()
    assert hasattr(raw, "sdm_vmap_components")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_vmap_components"]
    assert sym[1] is ctypes.c_int and sym[2] == types
    fn = lib.sdm_vmap_components
    assert list(fn.argtypes) == types and fn.restype is ctypes.c_int
    assert b.VMAP_COMP_OUTS == tuple(f for f, _ in b.VmapCompArgs._fields_[10:])
    assert b.VMAP_NO_COMPONENT == 0xFFFFFFFF
    sig = inspect.signature(pkg.Engine.vmap_components)
    assert list(sig.parameters)[1:] == ["connectivity", "min_multiplicity", "require_published", "min_size", "labels", "sizes",
                                        "small_ids"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [26, 0, False, 0, True, True, True]


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_header(pkg, tmp_path, cname):
    b = _binding(pkg)
    pyname, fields = STRUCTS[cname]
    st = getattr(b, pyname)
    got = _own_layout(tmp_path, cname, fields)
    assert got["sizeof"] == [ctypes.sizeof(st)] == [SIZES[cname]]
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
    # the components call exists beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_components")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    a = b.VmapCompArgs()
    ins = (26, 3, 1, 8, 0, 5, 6)
    for f, v in zip(INS, ins):
        setattr(a, f, v)
    for f in b.VMAP_COMP_OUTS:
        setattr(a, f, 7)
    assert lib.sdm_vmap_components(None, ctypes.byref(a)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(a, f) for f in b.VMAP_COMP_OUTS] == [0] * 6   # the outs of a refusal
    assert tuple(getattr(a, f) for f in INS) == ins
    assert (a.label, a.size, a.small_ids) == (None, None, None)
    assert lib.sdm_vmap_components(None, None) == 1
