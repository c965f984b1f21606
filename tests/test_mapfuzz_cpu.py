"""CPU: the call sequences of tests/test_gpu_mapfuzz.py run against the model alone (tests/map_model.py; the oracle and the
NumPy restatements are CPU code).  What is asserted are conditions on the sequences -- every op kind and every refusal
occurs, the map is re-placed, retired from and re-carved with the outcomes that matter (entries moved, merged, dropped,
orphaned; pairs removed), the rebuilt table and set grow again, flags are carried, and a model that is wrong in one of five
deliberate ways would be noticed -- so that a later edit of the generator cannot hollow the GPU test out.  The GPU test
asserts the same counters at the end of each of its sequences.

The five read-only queries ride along in a stream of their own (map_model.QueryStream).  Asserted here: the conditions on
that stream per seed (map_model.check_query_coverage: every kind and refusal, the events a query follows, the contents of
the answers, and that an answer from the state before the last change or without the flags would differ); that a query
changes nothing in the model; and that with the queries filtered out every default seed's sequence is, call by call and in
its final state, the one generated without them."""
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


def run_model(pkg, oracle, seed, steps=mm.STEPS, queries=True):
    """the MapWorld after the seed's whole sequence; w.trace: (op, its description) of every call of the main stream"""
    seq = Sequence(pkg, oracle, cm.W, cm.H, cm.N_KF, cm.SEED0 + seed)
    try:
        w = mm.MapWorld(oracle, seq)
        w.trace = []
        log = []
        for step, (op, a) in enumerate(mm.generate(seed, w, steps, queries)):
            log.append("%3d %s" % (step, mm.describe(op, a)))
            if op not in mm.QUERY_OPS:
                w.trace.append((op, log[-1][4:]))
            try:
                query = op in mm.QUERY_OPS
                refused = op in mm.MAP_OPS + mm.QUERY_OPS and w.refusal(op, a) is not None
                before = digest(w) if refused or query else None
                main = (dict(w.count), dict(w.cov), dict(w.mcov), w.last) if query else None
                res = w.apply(op, a)
                if refused:  # a refused call leaves the model untouched
                    assert res["refused"] and digest(w) == before, log[-1]
                if query:  # a query changes nothing in the model, and nothing the main stream draws from
                    assert bool(res["refused"]) == refused and digest(w) == before, log[-1]
                    assert main == (w.count, w.cov, w.mcov, w.last), log[-1]
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


@pytest.mark.parametrize("seed", cm.seeds())
def test_query_streams_cover_the_queries(sequences, seed):
    """the five read-only queries in the life cycle: every kind and every refusal, behind a repose, a committing retire and a
    committing classify, with require_published before and after the flags exist, with the contents that matter, and a
    query answered from the state before the last change or without the flags would be noticed"""
    w = sequences(seed)
    print("seed %d queries: %r" % (seed, w.qcov))
    mm.check_query_coverage(w, seed)


@pytest.mark.parametrize("seed", DEFAULT_SEEDS)
def test_queries_leave_the_main_stream_as_it_is(pkg, oracle, sequences, seed):
    """with the queries filtered out the sequence is, call by call, the one generated without them, and it ends in the
    same state: the tuned sequences and what tests/test_gpu_slices.py asserts per seed are as they were"""
    w = sequences(seed)
    bare = run_model(pkg, oracle, seed, queries=False)
    assert bare.qcov["calls"] == 0 and w.qcov["calls"] > 0
    assert len(w.trace) == len(bare.trace) == mm.STEPS
    for i, (a, b) in enumerate(zip(w.trace, bare.trace)):
        assert a == b, (seed, i, a, b)
    assert digest(w) == digest(bare) and (w.count, w.cov, w.mcov) == (bare.count, bare.cov, bare.mcov)


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
    # the consumer's step: the map falls into several components, normals are estimated and turned towards their cameras,
    # the mesh made from them has triangles, rays of the occlusion test and of the view are stopped
    q = {op: seen[op][0]["totals"] for op in mm.QUERY_OPS}
    print(q)
    assert q["vmap_components"]["components"] > 1 and q["vmap_components"]["small"] > 0
    assert q["vmap_normals"]["estimated"] > 0 and q["vmap_normals"]["oriented"] > 0
    assert q["vmap_mesh"]["triangles"] > 0 and q["vmap_mesh"]["quads"] > 0
    assert q["vmap_cast_segments"]["rays_total"] > 512 and q["vmap_cast_segments"]["rays_hit"] > 0
    assert 0 < q["vmap_render"]["rays_hit"] < q["vmap_render"]["rays_total"] == 33 * 17


def test_the_model_imports_no_torch_and_holds_no_engine():
    src = open(mm.__file__).read()
    assert "import torch" not in src.split('"""', 2)[2] and "eng." not in src and "Engine" not in src
