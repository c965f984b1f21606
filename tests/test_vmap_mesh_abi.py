"""CPU: the C ABI of sdm_vmap_mesh and its struct -- declared in the header at its place, exported, laid out in ctypes as the C
compiler lays out include/sdm_c.h, its normative phrases in the header, refusing NULL arguments without a GPU, and leaving
every earlier struct as it was."""
import ctypes
import inspect
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_comp_abi import _own_layout
from test_vmap_normals_abi import SIZES as NORMAL_SIZES, STRUCTS as NORMAL_STRUCTS, UNCHANGED as EARLIER
from test_vmap_obs_abi import _layout

STRUCTS = {
    "sdm_vmap_mesh_args": ("VmapMeshArgs", ("min_multiplicity", "require_published", "on_device", "first", "count", "capacity",
                                            "tri_capacity", "used_capacity", "normal", "tri", "owner_tris", "vertex_used",
                                            "entries", "members", "owners", "quads", "singles", "triangles", "vertices")),
}
FUNCTIONS = {"sdm_vmap_mesh": ["sdm_ctx", "sdm_vmap_mesh_args"]}
SIZES = {"sdm_vmap_mesh_args": 144}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (NORMAL_STRUCTS[c][0], NORMAL_SIZES[c]) for c in NORMAL_STRUCTS})
INS = ("min_multiplicity", "require_published", "on_device", "first", "count", "capacity", "tri_capacity", "used_capacity")
PHRASES = (
    "every output is an integer decided by comparisons and bitwise reproducible",
    "entry id is a MEMBER iff multiplicity[id] >= min_multiplicity", "if no classify has run every flag reads 0",
    "the member test of sdm_vmap_components, word for word",
    "c = floorf(P_k * inv) of its record point P, as sdm_vmap_components forms it", "outside [-2^20, 2^20) holds nothing",
    "the range test comes before the key is formed", "\"the member of a cell\" is the cell's entry if it exists and is a member",
    "normal[(id - first)*3 + 0..2] is caller-supplied binary32", "It is only compared, never used in arithmetic",
    "a = 0; if (fabsf(n_1) > fabsf(n_a)) a = 1; if (fabsf(n_2) > fabsf(n_a)) a = 2",
    "ties go to the lower index and a NaN never wins", "a denormal component is > 0", "u = (a+1) mod 3 and v = (a+2) mod 3",
    "is an OWNER iff it is a member, fabsf(n_a) > 0", "an all-zero or NaN-at-a normal owns nothing",
    "the cell c - e_a holds no member: it is the bottom of its run along a", "t = cell(j) + e_ax",
    "for da in the order 0, -1, +1", "if the cell t + da*e_a holds a member k, then at most twice",
    "if the cell below it along -e_a holds a member, take that one and move down", "No hit gives NONE",
    "Nu = step(id, u); Nv = step(id, v); C = step(Nu, v) if Nu exists", "if C is NONE and Nv exists, C = step(Nv, u)",
    "The four lie in four distinct columns, so they are distinct ids", "all three exist: (id,Nu,C), (id,C,Nv), a QUAD",
    "only Nu and Nv: (id,Nu,Nv)", "only Nu and C: (id,Nu,C)", "only Nv and C: (id,C,Nv)",
    "If n_a < 0 the second and third index of each triangle are swapped",
    "the triangles of the owners in ascending id, an owner's first triangle before its second",
    "owner_tris[id - first] in {0, 1, 2}", "1 iff j is a corner of a triangle of this call, else 0",
    "entries = the size of the range", "triangles = 2*quads + singles", "counted even when that pointer is NULL",
    "count == -1: to M", "A sub-range returns exactly the whole call's triangles whose owner lies in it, in order",
    "An empty range queues nothing", "capacity >= the size of the range", "used_capacity >= M bytes",
    "triangles > tri_capacity with tri != NULL is SDM_EINVAL", "the seven totals are filled and no destination is written",
    "the writing launch is queued only if the call is not refused", "all three NULL is valid and returns the totals only",
    "State: the call changes nothing in the map or the engine", "whatever the table layout and the slicing",
    "before anything is queued; the seven totals are then 0", "require_published not 0 or 1",
    "first < 0, count < -1, or first + count > M", "a NULL normal with a range that is not empty",
    "a negative capacity, tri_capacity or used_capacity", "capacity below the range", "used_capacity < M with vertex_used given",
    "a misaligned device pointer", "raised before any launch", "at most 21 read-only probes (1 + 4 x (3 + 2))",
    "Two host waits: the totals (56 B), then the end", "the mesh is voxel-level, at each voxel's winning point",
    "the vertices are the run bottoms only", "a missing owner corner loses that cell's triangle",
    "there are seams where the dominant axis changes", "the mesh is not watertight", "is the bad case",
    "O(range) per call, not incremental", "goes stale with sdm_set_pose", "one rank only")


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
    assert text.index("int sdm_vmap_normals") < text.index("int sdm_vmap_mesh") < text.index("int sdm_extract_bound")
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in PHRASES:
        assert phrase in flat, phrase


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    types = [C.c_void_p, C.POINTER(b.VmapMeshArgs)]
    raw = ctypes.CDLL(pkg.lib_path())
    lib = pkg.load_library()
    assert hasattr(raw, "sdm_vmap_mesh")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_vmap_mesh"]
    assert sym[1] is ctypes.c_int and sym[2] == types
    names = [s[0] for s in b.SYMBOLS]
    assert names.index("sdm_vmap_normals") + 1 == names.index("sdm_vmap_mesh") == names.index("sdm_extract_bound") - 1
    fn = lib.sdm_vmap_mesh
    assert list(fn.argtypes) == types and fn.restype is ctypes.c_int
    assert b.VMAP_MESH_OUTS == tuple(f for f, _ in b.VmapMeshArgs._fields_[12:])
    assert tuple(b.VMAP_MESH_FIELDS) == ("tri", "owner_tris", "vertex_used")
    sig = inspect.signature(pkg.Engine.vmap_mesh)
    assert list(sig.parameters)[1:] == ["normal", "min_multiplicity", "require_published", "first", "count", "tri", "owner_tris",
                                        "vertex_used", "tri_capacity"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [0, False, 0, None, True, True, True, None]


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
    if cname == "sdm_vmap_comp_args":   # (it has a field called `size`: test_vmap_comp_abi's own layout program)
        got = _own_layout(tmp_path, cname, fields)
        assert got["sizeof"] == [size] == [ctypes.sizeof(st)] == [112]
    else:
        got = _layout(tmp_path, cname, fields)
        assert got["size"] == [size] == [ctypes.sizeof(st)]
    for f in fields:
        fd = getattr(st, f)
        assert got[f] == [fd.offset, fd.size], f
    # the mesh call exists beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_mesh")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    a = b.VmapMeshArgs()
    ins = (3, 1, 0, 4, -1, 6, 7, 8)
    for f, v in zip(INS, ins):
        setattr(a, f, v)
    for f in b.VMAP_MESH_OUTS:
        setattr(a, f, 7)
    assert lib.sdm_vmap_mesh(None, ctypes.byref(a)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(a, f) for f in b.VMAP_MESH_OUTS] == [0] * 7   # the outs of a refusal
    assert tuple(getattr(a, f) for f in INS) == ins
    assert (a.normal, a.tri, a.owner_tris, a.vertex_used) == (None, None, None, None)
    assert lib.sdm_vmap_mesh(None, None) == 1
