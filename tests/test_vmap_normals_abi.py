"""CPU: the C ABI of sdm_vmap_normals and its struct -- declared in the header at its place, exported, laid out in ctypes as the
C compiler lays out include/sdm_c.h, its normative phrases in the header, refusing NULL arguments without a GPU, and leaving
every earlier struct as it was."""
import ctypes
import inspect
import os
import re
import sys

import pytest

from test_extract_abi import ROOT
from test_vmap_comp_abi import SIZES as COMP_SIZES, STRUCTS as COMP_STRUCTS, UNCHANGED as EARLIER, _own_layout
from test_vmap_obs_abi import _layout

STRUCTS = {
    "sdm_vmap_normal_args": ("VmapNormalArgs", ("radius", "min_points", "min_multiplicity", "require_published", "on_device",
                                                "first", "count", "capacity", "normal", "variation", "points", "entries",
                                                "members", "estimated", "oriented")),
}
FUNCTIONS = {"sdm_vmap_normals": ["sdm_ctx", "int", "const int", "const float", "sdm_vmap_normal_args"]}
SIZES = {"sdm_vmap_normal_args": 104}
# sizeof of the structs that existed before, on the LP64 targets the library is built for
UNCHANGED = dict(EARLIER, **{c: (COMP_STRUCTS[c][0], COMP_SIZES[c]) for c in COMP_STRUCTS})
INS = ("radius", "min_points", "min_multiplicity", "require_published", "on_device", "first", "count", "capacity")


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
    assert text.index("int sdm_vmap_components") < text.index("int sdm_vmap_normals") < text.index("int sdm_extract_bound")
    assert "no sub-voxel intersection, no normals" in text   # the ray queries' own limit stays true of them
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("IEEE binary32: no fused multiply-add, the plain correctly rounded division and sqrtf, denormals kept",
                   "entry id is a MEMBER iff multiplicity[id] >= min_multiplicity", "if no classify has run every flag reads 0",
                   "c = floorf(P_k * inv) of its record point P, as sdm_vmap_components forms it",
                   "d in {-r..r}^3, r = radius, in lexicographic order, dx slowest and dz fastest",
                   "(0,0,0) is included and gives the entry itself", "outside [-2^20, 2^20) holds nothing",
                   "the range test comes before the key is formed", "is a sample iff it exists and is a member",
                   "q_a = (xyz_j[a] - P[a]) * inv: one subtract, then one multiply",
                   "all sums start at +0 and accumulate in visiting order", "m_ab = m_ab + q_a*q_b for (a,b) = (0,0),(0,1),(0,2),(1,1),(1,2),(2,2)",
                   "k for a member and 0 for a non-member", "if k < min_points the entry is not estimated",
                   "kf = (float)k; mu_a = s_a / kf; C_ab = m_ab / kf - mu_a*mu_b", "exactly 6 sweeps",
                   "(p,q) = (0,1), (0,2), (1,2) in that order", "If A_pq == 0 (-0 too) the pair does nothing",
                   "theta = (A_qq - A_pp) / (2*A_pq)", "t = copysignf(1, theta) / (fabsf(theta) + sqrtf(theta*theta + 1))",
                   "c = 1 / sqrtf(t*t + 1); s = t*c; h = t*A_pq", "A_pp = A_pp - h; A_qq = A_qq + h; A_pq = +0",
                   "A_rp = c*x - s*y, A_rq = s*x + c*y", "V_ip = c*x - s*y, V_iq = s*x + c*y", "gives t = +-0",
                   "this is no special case in code", "ties go to the lower index", "sum = (lambda_0 + lambda_1) + lambda_2",
                   "if !(sum > 0) the entry is not estimated", "column m of V, not renormalised",
                   "variation = (lambda_m < 0 ? +0.0f : lambda_m) / sum", "the pose table is sdm_vmap_recarve's",
                   "n_poses == 0 is valid", "dot = (n_0*d_0 + n_1*d_1) + n_2*d_2", "if dot < 0 every component is negated",
                   "A NaN dot does not flip, and the entry still counts as oriented", "keeps the sign the rotations left",
                   "normal = (+0,+0,+0) and variation = -1.0f", "outputs are indexed by id - first",
                   "all three NULL is valid and returns the totals only", "An empty range queues nothing",
                   "entries = the size of the range", "State: the call changes nothing", "whatever the table layout and the slicing",
                   "before anything is queued", "radius not 1 or 2", "min_points outside 3 .. (2*radius+1)^3",
                   "require_published not 0 or 1", "first < 0, count < -1, or first + count > M", "a negative capacity",
                   "capacity below the range with any destination given", "a misaligned device pointer", "negative n_poses",
                   "NULL tags or Tcw with n_poses > 0", "a tag outside [0, 2^31)", "a tag listed twice", "raised before any launch",
                   "O(range x (2r+1)^3) probes per call, not incremental", "built on each voxel's winning point only",
                   "goes stale with sdm_set_pose as the records do", "oriented by the winner's camera alone", "one rank only"):
        assert phrase in flat, phrase


def test_symbol_exported_and_argtypes(pkg):
    b = _binding(pkg)
    C = ctypes
    types = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(b.VmapNormalArgs)]
    raw = ctypes.CDLL(pkg.lib_path())
    lib = pkg.load_library()
    assert hasattr(raw, "sdm_vmap_normals")
    sym = {s[0]: s for s in b.SYMBOLS}["sdm_vmap_normals"]
    assert sym[1] is ctypes.c_int and sym[2] == types
    fn = lib.sdm_vmap_normals
    assert list(fn.argtypes) == types and fn.restype is ctypes.c_int
    assert b.VMAP_NORMAL_OUTS == tuple(f for f, _ in b.VmapNormalArgs._fields_[11:])
    sig = inspect.signature(pkg.Engine.vmap_normals)
    assert list(sig.parameters)[1:] == ["tags", "Tcw", "radius", "min_points", "min_multiplicity", "require_published", "first",
                                        "count", "normals", "variations", "counts"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, None, 1, 3, 0, False, 0, None, True, True, True]


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
    # the normals call exists beside them
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_vmap_normals")


def test_null_arguments_are_einval(pkg):
    b = _binding(pkg)
    lib = pkg.load_library()
    a = b.VmapNormalArgs()
    ins = (2, 5, 3, 1, 0, 4, -1, 6)
    for f, v in zip(INS, ins):
        setattr(a, f, v)
    for f in b.VMAP_NORMAL_OUTS:
        setattr(a, f, 7)
    assert lib.sdm_vmap_normals(None, 0, None, None, ctypes.byref(a)) == 1
    assert b"null argument" in lib.sdm_last_error()
    assert [getattr(a, f) for f in b.VMAP_NORMAL_OUTS] == [0] * 4   # the outs of a refusal
    assert tuple(getattr(a, f) for f in INS) == ins
    assert (a.normal, a.variation, a.points) == (None, None, None)
    assert lib.sdm_vmap_normals(None, 0, None, None, None) == 1
