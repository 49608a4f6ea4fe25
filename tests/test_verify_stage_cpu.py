"""The rank / gather / scatter stage of match-and-verify, on a machine with no GPU: the designed scenes of tests/verify_ref.py yield
exactly the kept sets they state under oracle.matcher_np.match_snn, and the restatement they are compared with on the GPU
(tests/test_gpu_verify_stage.py) has power: a wrong row order, a dropped row or a neighbour's seed changes what it computes by more than
the GPU tests tolerate."""
import numpy as np
import pytest

from oracle import matcher_np as mo
from tests import verify_ref as vr


def _stated(sc, mutual):
    q = sc["kept"][mutual]
    return q, sc["train_of"][q]


def _check_kept(sc):
    """match_snn on the scene = the stated kept set and train rows, with and without mutual, and the stated distances"""
    for mutual in (False, True):
        q, t = vr.tentatives(sc["d1"], sc["d2"], sc["ratio"], mutual, sc["norm"])
        wq, wt = _stated(sc, mutual)
        assert np.array_equal(q, wq) and np.array_equal(t, wt), (mutual, sc["norm"])
    if sc["n1"] and sc["n2"] >= 2:
        _, dist = mo.knn2(sc["d1"], sc["d2"], "l2" if sc["norm"] == "l2_u8" else sc["norm"])
        kept = np.zeros(sc["n1"], bool); kept[sc["kept"][False]] = True
        assert (dist[kept, 0] == 0).all() and (dist[kept, 1] >= (8 if sc["norm"] == "hamming" else 4)).all()
        d = dist[~kept]                                                 # the dropped queries: 0 | 0, 1 | 1 or (ratio 0.5) 1 | 2, as integers
        assert (((d[:, 0] == d[:, 1]) & (d[:, 0] <= 1)) | ((d[:, 0] == 1) & (d[:, 1] == 2) & (sc["ratio"] <= 0.5))).all()


@pytest.mark.parametrize("sel,n", vr.RANK_CASES)
def test_rank_scenes_keep_what_they_state(sel, n):
    want = vr.RANK_SELECTORS[sel][0](n)
    assert len(want) >= 8 and want.max() < n
    for model in ("F", "H"):
        sc = vr.rank_scene(model, sel, n)
        assert np.array_equal(sc["kept"][False], want) and sc["n1"] == n and sc["d1"].shape == (n, vr.DIM)
        _check_kept(sc)
    for norm in vr.NORMS:                                               # the scene under the other norms: the same decisions
        _check_kept(vr.designed_pair("F", n, want, norm=norm, seed=1))


def test_rank_cases_cover_the_issue():
    cases = set(vr.RANK_CASES)
    assert {n for _, n in cases} == {64, 65, 256, 257, 512, 513, 600} and {s for s, _ in cases} == set(vr.RANK_SELECTORS)
    assert list(vr.RANK_SELECTORS["wave"][0](256)) == list(range(60, 68)) and list(vr.RANK_SELECTORS["sweep"][0](512)) == list(range(252, 260))
    k = vr.RANK_SELECTORS["sweep2"][0](600)
    assert len(k) == 8 and k.min() >= 512
    for n in (512, 513, 600):
        k = vr.RANK_SELECTORS["per_wave"][0](n)
        assert list(k // 64) == list(range((n + 63) // 64))
    assert {vr.NORMS[i % 3] for i in range(len(vr.RANK_CASES))} == set(vr.NORMS)


@pytest.mark.parametrize("model", ["F", "H"])
@pytest.mark.parametrize("norm", vr.NORMS)
def test_count_scenes_keep_what_they_state(model, norm):
    need = vr.MIN_PTS[model]
    seen = set()
    for core, nd in vr.COUNT_CASES[model]:
        sc = vr.count_scene(model, core, nd, norm)
        assert len(sc["kept"][True]) == core and len(sc["kept"][False]) == core + nd and sc["n1"] == 300
        assert sc["kept"][True][-1] >= 256 and sc["kept"][True][0] < 256     # the last tentative lies in the second sweep
        _check_kept(sc)
        seen |= {(core + nd >= need, core >= need)}
    assert {core + nd for core, nd in vr.COUNT_CASES[model] if nd == 0} == {need - 1, need, need + 1}
    assert (True, False) in seen                                       # eligible without mutual, short with it


@pytest.mark.parametrize("name", list(vr.ARRANGEMENTS))
def test_batch_scenes_keep_what_they_state(name):
    assert len(vr.ARRANGEMENTS[name]) == vr.BATCH_K and len(set(vr.batch_seeds(name))) == vr.BATCH_K
    for model in ("F", "H"):
        elig = []
        for kind, sc in zip(vr.ARRANGEMENTS[name], vr.batch_scene(model, name)):
            _check_kept(sc)
            elig.append(len(sc["kept"][False]) >= vr.MIN_PTS[model])
            assert elig[-1] == (kind == "E")
            assert (sc["n1"] == 0) == (kind == "Q") and sc["n2"] == {"T": 0, "O": 1}.get(kind, sc["n2"])
            assert kind != "S" or 0 < len(sc["kept"][False]) < vr.MIN_PTS[model]
        assert sum(elig) == {"all_short": 0, "all_eligible": 12, "short_first": 6, "short_last": 6, "around_one": 1}[name]
    seeds = [s for n in vr.ARRANGEMENTS for s in vr.batch_seeds(n)]
    assert len(set(seeds)) == len(seeds)


@pytest.mark.parametrize("ratio,kinds", vr.EDGE_CASES)
@pytest.mark.parametrize("norm", vr.NORMS)
def test_edge_scenes_keep_what_they_state(ratio, kinds, norm):
    sc = vr.edge_scene("F", ratio, kinds, norm)
    _check_kept(sc)
    assert len(sc["kept"][False]) == len(sc["kept"][True]) + 2
    if "edge" in kinds:                                                 # the same rows at a ratio just above the edge: the edge queries pass
        q, _ = vr.tentatives(sc["d1"], sc["d2"], float(np.nextafter(np.float32(0.5), np.float32(1))), False, norm)
        assert len(q) > len(sc["kept"][False])


def test_builder_refuses_the_edge_kind_above_its_ratio():
    with pytest.raises(AssertionError):
        vr.designed_pair("F", 20, [1, 2], ratio=0.9, kinds=("edge",))


# ---- the expectation has power ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["F", "H"])
@pytest.mark.parametrize("sel,n", vr.RANK_CASES)
def test_rank_cases_notice_order_row_and_seed_defects(oracle_port, model, sel, n):
    sc = vr.rank_scene(model, sel, n); seed = vr.rank_seed(model, sel, n)
    base = vr.scene_ref(oracle_port, sc, seed)
    assert base["cnt"] == len(sc["kept"][False]) and base["counters"][0] > 0 and base["inlier"].any()
    assert vr.disagreements(vr.scene_ref(oracle_port, sc, seed), base) == []      # the restatement repeats itself
    muts = vr.ORDER_MUTATIONS + (("swap256",) if vr.crosses_256(sel, n) else ())
    for mut in muts:
        got = vr.mutated(oracle_port, model, sc, seed, mut, other_seed=seed + 1)
        assert vr.disagreements(got, base), (mut, base["counters"], got["counters"])


@pytest.mark.parametrize("model", ["F", "H"])
@pytest.mark.parametrize("name", [n for n in vr.ARRANGEMENTS if n != "all_short"])
def test_batch_pairs_notice_the_neighbours_seed(oracle_port, model, name):
    seeds = vr.batch_seeds(name)
    for p, sc in enumerate(vr.batch_scene(model, name)):
        if len(sc["kept"][False]) < vr.MIN_PTS[model]:
            continue
        base = vr.scene_ref(oracle_port, sc, seeds[p])
        for nb in (q for q in (p - 1, p + 1) if 0 <= q < vr.BATCH_K):
            got = vr.mutated(oracle_port, model, sc, seeds[p], "seed", other_seed=seeds[nb])
            assert vr.disagreements(got, base), (p, nb)


def test_pairs_restatement_is_the_batch_restatement_on_the_expansion(oracle_port):
    """one query image against three train images, listed last first: the list form of the restatement is the pair form entry by entry"""
    scs = [vr.designed_pair("F", 65, np.arange(0, 65, 3), seed=900)]
    d1 = scs[0]["d1"]; k1 = scs[0]["k1"]
    # the three train images answer the SAME queries: rebuild them from scene 0's codes, each under its own shuffle
    rng = np.random.default_rng(3)
    perms = [rng.permutation(scs[0]["n2"]) for _ in range(3)]
    d2 = np.concatenate([scs[0]["d2"][p] for p in perms]); k2 = np.concatenate([scs[0]["k2"][p] for p in perms])
    c2 = [scs[0]["n2"]] * 3
    pairs = [(0, 2), (0, 1), (0, 0)]; seeds = [5, 6, 7]
    got = vr.pairs_ref(oracle_port, "F", k1, d1, [65], k2, d2, c2, pairs, seeds)
    for e, (i, j) in enumerate(pairs):
        want = vr.pair_ref(oracle_port, "F", k1, scs[0]["k2"][perms[j]], d1, scs[0]["d2"][perms[j]], seeds[e])
        assert vr.disagreements(got[e], want) == []
        assert np.array_equal(np.flatnonzero(got[e]["match"] >= 0), scs[0]["kept"][False])
        assert np.array_equal(perms[j][got[e]["match"][scs[0]["kept"][False]]], scs[0]["train_of"][scs[0]["kept"][False]])
