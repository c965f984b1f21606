"""The C++ class with sdm::Options::device_priors on and off (tests/cpp/test_pm_priors.cc): the search priors derived on
the device from the keyframes' ORB observations give the same maps and point cloud as the host helpers, and a keyframe
whose observations the engine refuses (a map point at two keypoints) falls back to the host helpers."""
import os
import subprocess

import numpy as np
import pytest

from common import Sequence, assert_bit_equal
from test_gpu_cpp_class import build_driver

pytestmark = pytest.mark.gpu


def write_blob(path, seq, n, obs):
    with open(path, "wb") as f:
        np.array([seq.W, seq.H, seq.n_kf, n], np.int32).tofile(f)
        for k in range(seq.n_kf):
            seq.im[k].tofile(f)
            seq.K.astype(np.float32).tofile(f)
            seq.Tcw[k].astype(np.float32).tofile(f)
            cov = np.array(seq.scene.neighbours(k, seq.n_kf, seq.n_kf - 1), np.int32)
            ids, ang, dep = obs[k]
            for a, dt in ((cov, np.int32), (dep, np.float32), (ids, np.int32), (ang, np.float32)):
                np.array([len(a)], np.int32).tofile(f)
                np.ascontiguousarray(a, dt).tofile(f)


def run(exe, tmp_path, blob, on, mode):
    out = tmp_path / ("out_%d_%s.bin" % (on, mode))
    obj = tmp_path / ("cloud_%d_%s.obj" % (on, mode))
    r = subprocess.run([exe, str(blob), str(out), str(obj), str(on), mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(out, np.uint8), obj.read_bytes(), r.stderr


@pytest.mark.parametrize("mode,dup", [("recon", True), ("block", False), ("block", True)])
def test_cpp_device_priors_match_host_helpers(pkg, oracle, gpu_ok, tmp_path, mode, dup):
    """dup: the last keyframe holds one map point at two keypoints.  The engine refuses its observations, so every call
    that reads it (SemiDenseRecon of keyframes 11..15, the whole block) falls back to the host helpers; SemiDenseRecon of
    keyframes 0..10 still derives its priors on the device"""
    exe = build_driver(pkg, "test_pm_priors")
    n_kf, n = 16, 7
    seq = Sequence(pkg, oracle, 160, 120, n_kf, 0x5EED0104, disparity_px=3.0, strip=True, roll_deg=5.0)
    obs = [seq.scene.observations(k, 1500, 11) for k in range(n_kf)]
    if dup:
        ids, ang, dep = obs[-1]
        ids = ids.copy()
        pos = np.nonzero(ids >= 0)[0]
        ids[pos[1]] = ids[pos[0]]
        obs[-1] = (ids, ang, dep)
    blob = tmp_path / "in.bin"
    write_blob(blob, seq, n, obs)
    off, obj_off, _ = run(exe, tmp_path, blob, 0, mode)
    on, obj_on, _ = run(exe, tmp_path, blob, 1, mode)
    W, H = seq.W, seq.H
    per = 8 + 4 * (5 * W * H)
    assert len(on) == len(off) == n_kf * per + 8
    for k in range(n_kf):
        a = on[k * per:(k + 1) * per]
        b = off[k * per:(k + 1) * per]
        assert np.array_equal(a[:8], b[:8]), "flags kf %d" % k
        assert_bit_equal(a[8:].view(np.float32), b[8:].view(np.float32), "maps kf %d (%s)" % (k, mode))
    assert on[-8:].view(np.int64)[0] == off[-8:].view(np.int64)[0]  # obj vertices (none pass sigma <= 0.01 here)
    assert obj_on == obj_off
    assert on[:8].view(np.int32)[0] == 1, "keyframe 0 is reconstructed"
    assert (on[8:8 + 4 * W * H].view(np.float32) > 0).mean() > 0.05, "keyframe 0 has a depth map"
