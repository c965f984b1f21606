"""CPU: the call sequences of tests/test_gpu_cloudfuzz.py run against the model alone (tests/cloud_model.py; the oracle and
the NumPy mirrors are CPU code).  What is asserted are conditions on the sequences -- every op kind occurs, both walks and
the states between them are extracted, the refusals are there but few, a model that always walks the lists would be
noticed, the persistent map is created, updated, carved, cleared and reopened -- so that a later edit of the generator
cannot hollow the GPU test out.  The GPU test asserts the same counters at the end of each of its sequences."""
import numpy as np
import pytest

import cloud_model as cm
from common import Sequence

@pytest.fixture(scope="module")
def sequences(pkg, oracle):
    """seed -> the World after its whole sequence, run once per module"""
    done = {}

    def run(seed):
        if seed in done:
            return done[seed]
        seq = Sequence(pkg, oracle, cm.W, cm.H, cm.N_KF, cm.SEED0 + seed)
        try:
            w = cm.World(oracle, seq)
            log = []
            for step, (op, a) in enumerate(cm.generate(seed, w)):
                log.append("%3d %s" % (step, cm.describe(op, a)))
                try:
                    w.apply(op, a)
                except Exception:
                    print("\n".join(log[-10:]))
                    raise
        finally:
            oracle.params.lambdaG = 8.0
        print("seed %d: %r\n  ops %r" % (seed, w.cov, w.count))
        done[seed] = w
        return w
    return run


@pytest.mark.parametrize("seed", cm.seeds())
def test_sequences_cover_the_seam(sequences, seed):
    cm.check_coverage(sequences(seed), seed)


def test_one_map_outgrows_its_first_table(sequences):
    """in at least one seed of the set the map exceeds 512 voxels: the table leaves its initial 1024 slots and the counters
    survive a rehash"""
    most = {seed: sequences(seed).cov["max_voxels"] for seed in cm.seeds()}
    assert max(most.values()) > 512, most


def test_plain_cloud_is_the_host_filter():
    """the model's plain cloud on hand-made planes: raster order, the slot order of the call, the listed-only variant"""
    class M:
        pass
    m = M()
    rng = np.random.default_rng(0)
    h, w = 12, 16
    m.rho = {k: np.where(rng.random((h, w)) < 0.5, rng.uniform(0.1, 2, (h, w)), 0).astype(np.float32) for k in range(2)}
    m.chk = {k: np.where(rng.random((h, w)) < 0.5, m.rho[k], 0).astype(np.float32) for k in range(2)}
    m.sig = {k: np.where(m.rho[k] > 0, rng.uniform(0, 0.4, (h, w)), 0).astype(np.float32) for k in range(2)}
    m.xyz = {k: rng.normal(size=(h, 3 * w)).astype(np.float32) for k in range(2)}
    m.im = {k: rng.integers(0, 256, (h, w)).astype(np.uint8) for k in range(2)}
    m.der = {k: (rng.uniform(0, 20, (h, w)).astype(np.float32),) for k in range(2)}
    for src in (0, 1):
        offs, pix, rs, xyz, inten = cm.plain(m, [1, 0], src, 0.3, 1e-6)
        pos = 0
        for i, k in enumerate([1, 0]):
            rho = (m.chk if src else m.rho)[k]
            keep = (rho > 1e-6) & ~(m.sig[k].astype(np.float64) > 0.3)
            ys, xs = np.nonzero(keep)
            n = len(ys)
            assert offs[i] == pos and offs[i + 1] == pos + n and n > 0
            np.testing.assert_array_equal(pix[pos:pos + n], (ys << 16) | xs)
            np.testing.assert_array_equal(rs[pos:pos + n, 0], rho[ys, xs])
            np.testing.assert_array_equal(rs[pos:pos + n, 1], m.sig[k][ys, xs])
            np.testing.assert_array_equal(xyz[pos:pos + n], m.xyz[k].reshape(h, w, 3)[ys, xs])
            np.testing.assert_array_equal(inten[pos:pos + n], m.im[k][ys, xs])
            pos += n
        wrong = cm.plain(m, [1, 0], src, 0.3, 1e-6, listed_only=8.0)
        assert 0 < wrong[0][-1] < offs[-1] and set(wrong[1].tolist()) <= set(pix.tolist())
        codes = wrong[1].astype(np.int64)
        assert ((codes >> 16) >= 2).all() and ((codes >> 16) < h - 2).all() and ((codes & 0xffff) >= 2).all()
        everything = cm.plain(m, [0], src, 0.3, -1.0)
        assert everything[0][-1] == int((~(m.sig[0].astype(np.float64) > 0.3)).sum())  # the zeros are points
