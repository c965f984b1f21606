"""CPU: the call sequences of tests/test_gpu_mapfuzz.py run against the model alone (tests/map_model.py; the oracle and the
NumPy restatements are CPU code).  What is asserted are conditions on the sequences -- every op kind and every refusal
occurs, the map is re-placed, retired from and re-carved with the outcomes that matter (entries moved, merged, dropped,
orphaned; pairs removed), the rebuilt table and set grow again, flags are carried, and a model that is wrong in one of five
deliberate ways would be noticed -- so that a later edit of the generator cannot hollow the GPU test out.  The GPU test
asserts the same counters at the end of each of its sequences."""
import pytest

import cloud_model as cm
import map_model as mm
from common import Sequence

DEFAULT_SEEDS = range(1, 9)


def digest(w):
    """the whole state of the model's map, as bytes"""
    mp = w.map
    if mp is None:
        return None
    return (mp.voxel, mp.vm.info(), mp.ol.info(), mp.cl.info(), {f: v.tobytes() for f, v in mp.vm.rec.items()},
            mp.vm.keys.tobytes(), mp.vm.ids.tobytes(), mp.ol.entry.tobytes(), mp.ol.tag.tobytes(), mp.ol.pairs.tobytes(),
            {f: v.tobytes() for f, v in mp.ev.items()}, mp.cl.published.tobytes())


def run_model(pkg, oracle, seed, steps=mm.STEPS):
    """the MapWorld after the seed's whole sequence"""
    seq = Sequence(pkg, oracle, cm.W, cm.H, cm.N_KF, cm.SEED0 + seed)
    try:
        w = mm.MapWorld(oracle, seq)
        log = []
        for step, (op, a) in enumerate(mm.generate(seed, w, steps)):
            log.append("%3d %s" % (step, mm.describe(op, a)))
            try:
                refused = op in mm.MAP_OPS and w.refusal(op, a) is not None
                before = digest(w) if refused else None
                res = w.apply(op, a)
                if refused:  # a refused call leaves the model untouched
                    assert res["refused"] and digest(w) == before, log[-1]
            except Exception:
                print("\n".join(log[-10:]))
                raise
    finally:
        oracle.params.lambdaG = 8.0
    return w


@pytest.fixture(scope="module")
def sequences(pkg, oracle):
    """seed -> the MapWorld after its whole sequence, run once per module"""
    done = {}

    def run(seed):
        if seed not in done:
            done[seed] = w = run_model(pkg, oracle, seed)
            print("seed %d: %r\n  histories %r\n  max_voxels %d sensitive_calls %d\n  ops %r" %
                  (seed, w.mcov, {h: w.cov["hist_" + h] for h in cm.HISTORIES}, w.cov["max_voxels"],
                   w.cov["sensitive_calls"], w.count))
        return done[seed]
    return run


@pytest.mark.parametrize("seed", cm.seeds())
def test_sequences_cover_the_life_cycle(sequences, seed):
    mm.check_coverage(sequences(seed), seed)


def test_one_map_outgrows_its_first_table(sequences):
    """in at least one default seed the map exceeds 512 entries: the table leaves its initial 1024 slots"""
    most = {seed: sequences(seed).cov["max_voxels"] for seed in DEFAULT_SEEDS}
    assert max(most.values()) > 512, most


def test_one_observation_set_outgrows_its_first_table(sequences):
    """in at least one default seed the log exceeds 512 pairs: the observation set leaves its initial 1024 slots"""
    most = {seed: sequences(seed).mcov["max_pairs"] for seed in DEFAULT_SEEDS}
    assert max(most.values()) > 512, most


def test_online_recipe_on_the_model(pkg, oracle):
    """the fixed sequence tests/test_gpu_mapfuzz.py also runs: on the model it re-places, retires, re-carves and imports
    with the outcomes the recipe is about"""
    seq = Sequence(pkg, oracle, cm.W, cm.H, cm.N_KF, cm.SEED0 + 1)
    try:
        w = mm.MapWorld(oracle, seq)
        seen = {}
        for op, a in mm.online_recipe(w):
            res = w.apply(op, a)
            assert not res["refused"], op
            seen.setdefault(op, []).append(res)
    finally:
        oracle.params.lambdaG = 8.0
    repose, retire = seen["vmap_repose"][0]["delta"], seen["vmap_retire"][0]["delta"]
    print(repose, retire, seen["vmap_recarve"][0]["totals"], [r["delta"] for r in seen["vmap_classify"]])
    assert repose["moved"] > 0 and repose["merged"] > 0 and repose["observations"] < repose["observations_before"]
    assert retire["removed"] > 0 and retire["orphaned"] > 0  # (every voxel of keyframe 2 was seen by a neighbour too)
    assert w.cov["max_voxels"] > 512  # the import takes the table past its first 1024 slots
    assert seen["vmap_recarve"][0]["totals"]["ends_hit"] > 0 and w.mcov["recarve_chain"] == 1
    assert seen["vmap_import"][0]["delta"]["created"] > 0 and seen["vmap_import_observations"][0]["delta"]["created"] > 0
    assert seen["vmap_classify"][-1]["delta"]["published_total"] > 0


def test_the_model_imports_no_torch_and_holds_no_engine():
    src = open(mm.__file__).read()
    assert "import torch" not in src.split('"""', 2)[2] and "eng." not in src and "Engine" not in src
