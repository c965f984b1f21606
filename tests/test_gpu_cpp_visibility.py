"""GPU: ProbabilityMapping::AppendTranscriptEntryWithVisibility -- the transcript entry in the visibility-list form
(SFMTranscriptInterface_ORBSLAM.cpp:274-284) -- against the Python writer fed Engine.extract_points_support on an engine
driven through the class's call order (PM.cc:137-315: a reconstruction per keyframe, each followed by the in-place
inter-keyframe check of every keyframe whose neighbours are all reconstructed)."""
import subprocess
import sys

import numpy as np
import pytest

from common import Sequence
from test_gpu_cpp_class import build_driver, write_blob

pytestmark = pytest.mark.gpu


def visibility_entry(T, xyz, support, cam, nbr_cams):
    """the text of one entry: numbers through operator<<(double), i.e. %g"""
    T = np.asarray(T, np.float32)
    Ow = [-np.float32((np.float32(T[0, i] * T[0, 3]) + np.float32(T[1, i] * T[1, 3])) + np.float32(T[2, i] * T[2, 3]))
          for i in range(3)]
    lines = ["new cam: [%s; %s; %s] {" % tuple("%g" % float(v) for v in Ow)]
    for p, w in zip(xyz, support):
        seen = [cam] + [c for j, c in enumerate(nbr_cams) if (int(w) >> j) & 1]
        lines.append("new point: [%s; %s; %s], %s" % (tuple("%g" % float(v) for v in p) + (", ".join(str(c) for c in seen),)))
    lines.append("}")
    return lines


def test_visibility_entries_match_the_engine(pkg, oracle, gpu_ok, tmp_path):
    exe = build_driver(pkg, "test_pm_visibility")
    n_kf, n, W, H, max_sigma = 8, 7, 160, 120, 0.25
    seq = Sequence(pkg, oracle, W, H, n_kf, 0x5EED0E07)
    rng = np.random.default_rng(2)
    depths = [(1.0 + 0.1 * rng.standard_normal(200)).astype(np.float32) for _ in range(n_kf)]
    blob, tr, ret = tmp_path / "in.bin", tmp_path / "transcript.txt", tmp_path / "returns.txt"
    write_blob(blob, seq, n_kf, n, depths)
    r = subprocess.run([exe, str(blob), str(tr), str(ret)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    returns = [[int(v) for v in line.split()] for line in open(ret)]
    # a neighbour without a depth map, then vectors of different sizes: -1, a message, nothing written
    assert returns[0] == [-1, 0] and returns[1] == [-1, 0]
    assert "AppendTranscriptEntryWithVisibility: neighbour 0 has no depth map" in r.stderr
    assert "AppendTranscriptEntryWithVisibility: 7 neighbours, 6 camera indices" in r.stderr

    # the same call order on an engine: slot = keyframe index
    binding = sys.modules[pkg.__name__ + ".binding"]
    nbrs = {k: seq.scene.neighbours(k, n_kf, n_kf - 1)[:n] for k in range(n_kf)}
    eng = pkg.Engine(W, H, n_kf, max_neighbours=n)
    for k in range(n_kf):
        eng.upload_image(k, seq.im[k], seq.K, seq.Tcw[k])
    semi, inter = [False] * n_kf, [False] * n_kf
    for k in range(n_kf):
        mn, mx = binding.stereo_search_constraints(depths[k])
        eng.recon([k], [nbrs[k]], float(mn), float(mx))
        semi[k] = True
        for i in range(n_kf):  # PM.cc:262-315
            if inter[i] or not semi[i] or not all(semi[j] for j in nbrs[i]):
                continue
            eng.inter_check([i], [nbrs[i]], commit=True)
            eng.pointset([i], source=0)
            inter[i] = True
    assert all(inter)
    want, counts, lists = [], [], set()
    for k in range(n_kf):
        got = eng.extract_points_support([k], [nbrs[k]], source=0, max_sigma=max_sigma, fields=("xyz",))
        want += visibility_entry(seq.Tcw[k], got["xyz"], got["support"], 100 + k, [100 + j for j in nbrs[k]])
        counts.append(len(got["support"]))
        lists |= set(int(w) for w in got["support"])
    eng.close()
    assert returns[2:] == [[c, 1] for c in counts]
    text = open(tr).read().split("\n")
    assert text[-1] == ""
    assert text[:-1] == want
    assert sum(counts) > 50 and len(lists) > 1  # points were emitted, and not all with the same list
