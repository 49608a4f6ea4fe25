"""GPU: the rank / gather / scatter stage that every match_and_verify_* entry point shares (mt_filter_rank_kernel, the compaction of the
eligible pairs in mv_estimate, mt_gather_kernel, mt_scatter_kernel), on the designed scenes of tests/verify_ref.py: the kept queries lie
where the caller states, at the edges of the 64-lane ballot, the four-wave prefix and the 256-row sweep, the tentative counts sit at the
eligibility thresholds, and short, empty and eligible pairs are mixed in every order.  Every result is compared with the CPU restatement of
the whole pipeline: match, inlier, tentative count and the counters bit for bit, the model to 1e-9 relative Frobenius
(verify_ref.disagreements).  tests/test_verify_stage_cpu.py shows that this expectation notices a wrong row order, a dropped row and a
neighbour's seed."""
import ctypes as C
import functools

import numpy as np
import pytest

import pydegensac_amd as pd
from pydegensac_amd import _lib, matcher, tensor_api
from tests import verify_ref as vr

pytestmark = pytest.mark.gpu

CTR = [0, 1, 3]                                                         # samples, lo_runs, I of a stats row


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _split(res, offsets):
    """the device tuple (model, match, inlier, stats, cnt, ...) -> one dict per pair, as verify_ref.result builds them"""
    M, match, inl, st = (x.cpu().numpy() for x in res[:4]); cnt = res[4]
    out = []
    for p in range(len(cnt)):
        rows = slice(int(offsets[p]), int(offsets[p + 1]))
        out.append(dict(model=M[p], match=match[rows], inlier=inl[rows], cnt=int(cnt[p]), counters=tuple(int(c) for c in st[p, CTR]), stats=st[p]))
    return out


def _run(scs, seeds, mutual=False, kpts=False, **kw):
    """match_and_verify_batch_tensors on designed pairs of one model, norm and ratio"""
    sc0 = scs[0]; k1, k2 = ("k4_1", "k4_2") if kpts else ("k1", "k2")
    c1 = [s["n1"] for s in scs]; c2 = [s["n2"] for s in scs]
    res = tensor_api.match_and_verify_batch_tensors(_t(np.concatenate([s[k1] for s in scs])), _t(np.concatenate([s[k2] for s in scs])),
                                                    _t(np.concatenate([s["d1"] for s in scs])), _t(np.concatenate([s["d2"] for s in scs])), c1, c2,
                                                    model=sc0["model"], ratio=sc0["ratio"], mutual=mutual, seeds=seeds, norm=sc0["norm"],
                                                    **vr.BUDGET[sc0["model"]], **kw)
    return _split(res, np.r_[0, np.cumsum(c1)]), res


def _agree(got, want, sc, mutual, tag=None):
    bad = vr.disagreements(got, want)
    assert not bad, (tag, bad, got["cnt"], want["cnt"], got["counters"], want["counters"])
    kept = sc["kept"][mutual]                                           # ... and the restatement's tentatives are the stated ones
    assert want["cnt"] == len(kept) and np.array_equal(np.flatnonzero(want["match"] >= 0), kept)
    if want["cnt"] < vr.MIN_PTS[sc["model"]]:                           # a short pair: zero model, zero stats row, no inliers
        assert not got["model"].any() and not got["stats"].any() and not got["inlier"].any(), tag
    else:
        assert got["counters"][0] > 0, tag                             # estimated (four rows may still yield no model: then both agree on zeros)


@functools.lru_cache(maxsize=None)
def _ref(port, key, seed, mutual=False):
    """the restatement of a cached scene of verify_ref, computed once per process"""
    kind, args = key[0], key[1:]
    sc = {"rank": vr.rank_scene, "count": vr.count_scene, "edge": vr.edge_scene}[kind](*args)
    return vr.scene_ref(port, sc, seed, mutual)


# ---- rank positions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel,n", vr.RANK_CASES)
def test_rank_positions_fundamental(oracle_port, sel, n):
    sc = vr.rank_scene("F", sel, n); seed = vr.rank_seed("F", sel, n)
    (got,), _ = _run([sc], [seed])
    _agree(got, _ref(oracle_port, ("rank", "F", sel, n), seed), sc, False)


@pytest.mark.parametrize("sel,n", vr.RANK_CASES)
def test_rank_positions_homography_rows_and_keypoints(oracle_port, sel, n):
    sc = vr.rank_scene("H", sel, n); seed = vr.rank_seed("H", sel, n)
    want = _ref(oracle_port, ("rank", "H", sel, n), seed)
    for kpts in (False, True):                                          # float64 [n, 6] rows, float32 [n, 4] keypoints
        (got,), _ = _run([sc], [seed], kpts=kpts)
        _agree(got, want, sc, False, kpts)


# ---- count threshold ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model,core,dups", [(m, c, d) for m in ("F", "H") for c, d in vr.COUNT_CASES[m]])
def test_count_threshold(oracle_port, model, core, dups, mutual):
    norm = vr.NORMS[(core + dups) % 3]
    sc = vr.count_scene(model, core, dups, norm); seed = 100 + core
    (got,), _ = _run([sc], [seed], mutual=mutual)
    _agree(got, _ref(oracle_port, ("count", model, core, dups, norm), seed, mutual), sc, mutual)
    assert got["cnt"] == core + (0 if mutual else dups)
    assert (got["counters"][0] > 0) == (got["cnt"] >= vr.MIN_PTS[model])


# ---- batch composition --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vr.ARRANGEMENTS))
@pytest.mark.parametrize("model", ["F", "H"])
def test_batch_composition(oracle_port, model, name):
    scs = vr.batch_scene(model, name); seeds = vr.batch_seeds(name)
    want = [vr.scene_ref(oracle_port, sc, seeds[p]) for p, sc in enumerate(scs)]
    got, _ = _run(scs, seeds)
    for p, sc in enumerate(scs):
        _agree(got[p], want[p], sc, False, p)
        (alone,), _ = _run([sc], [seeds[p]])
        _agree(alone, want[p], sc, False, (p, "alone"))
    n_elig = sum(w["cnt"] >= vr.MIN_PTS[model] for w in want)
    assert n_elig == vr.ARRANGEMENTS[name].count("E") and sum(g["counters"][0] > 0 for g in got) == n_elig


# ---- decision edges inside the batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("norm", vr.NORMS)
@pytest.mark.parametrize("ratio,kinds", vr.EDGE_CASES)
@pytest.mark.parametrize("model", ["F", "H"])
def test_decision_edges(oracle_port, model, ratio, kinds, norm, mutual):
    sc = vr.edge_scene(model, ratio, kinds, norm); seed = 17
    (got,), _ = _run([sc], [seed], mutual=mutual)
    _agree(got, _ref(oracle_port, ("edge", model, ratio, kinds, norm), seed, mutual), sc, mutual)
    assert got["cnt"] == len(sc["kept"][mutual]) >= vr.MIN_PTS[model]


# ---- the same rows through every entry point that reaches mv_estimate ------------------------------------------------------------------
def _entry_scenes(model):
    return [vr.designed_pair(model, 129, np.arange(0, 129, 2), seed=700), vr.designed_pair(model, 40, [2, 11, 30], seed=701),
            vr.designed_pair(model, 70, np.arange(60, 70), seed=702), vr.designed_pair(model, 0, [], seed=703)]


ENTRY_SEEDS = [41, 4000000000, 43, 44]


@pytest.mark.parametrize("model", ["F", "H"])
def test_batch_tensors_plain_and_guided(oracle_port, model):
    import torch
    scs = _entry_scenes(model)
    got, res = _run(scs, ENTRY_SEEDS)
    for p, sc in enumerate(scs):
        _agree(got[p], vr.scene_ref(oracle_port, sc, ENTRY_SEEDS[p]), sc, False, p)
    _, gres = _run(scs, ENTRY_SEEDS, guided=True)
    assert len(gres) == 6 and gres[5].shape == res[1].shape
    det = [c for c in range(16) if c not in (12, 13)]                   # every stats column but the two device clock readings
    assert torch.equal(gres[0], res[0]) and torch.equal(gres[1], res[1]) and torch.equal(gres[2], res[2])
    assert torch.equal(gres[3][:, det], res[3][:, det]) and np.array_equal(gres[4], res[4])


@pytest.mark.parametrize("model", ["F", "H"])
def test_numpy_entry(oracle_port, model):
    scs = _entry_scenes(model)
    M, match, inl = matcher.match_and_verify_batch([s["k1"] for s in scs], [s["k2"] for s in scs], [s["d1"] for s in scs], [s["d2"] for s in scs],
                                                   model=model, seeds=ENTRY_SEEDS, **vr.BUDGET[model])
    st = pd.last_stats()
    for p, sc in enumerate(scs):
        got = dict(model=M[p], match=match[p], inlier=inl[p], cnt=st[p]["tentatives"], counters=(st[p]["samples"], st[p]["lo_runs"], st[p]["I"]),
                   stats=np.array([st[p]["samples"], st[p]["lo_runs"], st[p]["I"]]))
        _agree(got, vr.scene_ref(oracle_port, sc, ENTRY_SEEDS[p]), sc, False, p)


def _store_scene(model):
    """store 1: a junk image of 10 rows, then one query image; store 2: three train images, each the query image's train set under its own
    shuffle.  The list runs the query image against the three, last image first: entry 0's output rows start at 0, its query rows at 10."""
    sc = vr.designed_pair(model, 129, np.arange(1, 129, 2), seed=710)
    junk = vr.designed_pair(model, 10, [0, 5], seed=711)
    rng = np.random.default_rng(712)
    perms = [rng.permutation(sc["n2"]) for _ in range(3)]
    st1 = {k: np.concatenate([junk[k], sc[k]]) for k in ("k1", "d1")}
    st2 = {k: np.concatenate([sc[k][p] for p in perms]) for k in ("k2", "d2")}
    return sc, perms, st1, [10, 129], st2, [sc["n2"]] * 3, [(1, 2), (1, 1), (1, 0)], [51, 52, 53]


@pytest.mark.parametrize("fginn", [False, True])
@pytest.mark.parametrize("model", ["F", "H"])
def test_pair_list_entries(oracle_port, model, fginn):
    sc, perms, st1, c1, st2, c2, pairs, seeds = _store_scene(model)
    want = vr.pairs_ref(oracle_port, model, st1["k1"], st1["d1"], c1, st2["k2"], st2["d2"], c2, pairs, seeds)
    args = (_t(st1["k1"]), _t(st2["k2"]), _t(st1["d1"]), _t(st2["d2"]), c1, c2, pairs)
    kw = dict(model=model, seeds=seeds, **vr.BUDGET[model])
    if fginn:                                                           # radius 0: every row is far enough, the plain second neighbour
        res = tensor_api.match_and_verify_fginn_pairs_tensors(*args, 0.0, **kw)
    else:
        res = tensor_api.match_and_verify_pairs_tensors(*args, **kw)
    assert list(res[5]) == [0, 129, 258, 387]
    got = _split(res, res[5])
    kept = sc["kept"][False]
    for e, (_, j) in enumerate(pairs):
        bad = vr.disagreements(got[e], want[e])
        assert not bad, (e, bad, got[e]["counters"], want[e]["counters"])
        assert np.array_equal(np.flatnonzero(got[e]["match"] >= 0), kept) and np.array_equal(perms[j][got[e]["match"][kept]], sc["train_of"][kept])
        assert got[e]["counters"][0] > 0


def test_c_entry_whose_first_offsets_are_above_zero(oracle_port):
    """mi_degensac_match_verify_batch_dev on offsets that start at 5 and 12, with the mutual check: the rows in front are never read, the
    output rows outside the batch never written"""
    import torch
    scs = _entry_scenes("F"); K = len(scs); dev = _dev()
    sc_m = vr.designed_pair("F", 70, np.arange(50, 70, 2), dups=[(61, 60)], seed=702)
    scs[2] = sc_m
    want = [vr.scene_ref(oracle_port, sc, ENTRY_SEEDS[p], True) for p, sc in enumerate(scs)]
    rng = np.random.default_rng(43)
    def framed(key, front, back):
        x = np.concatenate([s[key] for s in scs])
        junk = lambda n: rng.integers(0, 5, (n,) + x.shape[1:]).astype(x.dtype)
        return _t(np.concatenate([junk(front), x, junk(back)]))
    a, k1 = framed("d1", 5, 3), framed("k1", 5, 3); b, k2 = framed("d2", 12, 2), framed("k2", 12, 2)
    o1 = np.r_[0, np.cumsum([s["n1"] for s in scs])].astype(np.int64) + 5; o2 = np.r_[0, np.cumsum([s["n2"] for s in scs])].astype(np.int64) + 12
    n = a.shape[0]
    M = torch.zeros((K, 9), dtype=torch.float64, device=dev); st = torch.zeros((K, 16), dtype=torch.int32, device=dev)
    match = torch.full((n,), -7, dtype=torch.int32, device=dev); inl = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_seeds = _t(np.asarray(ENTRY_SEEDS, np.uint32).view(np.int32)); cnt = np.zeros(K, np.int32)
    mp = _lib.MatchParams(0, vr.DIM, 0.9, True); prm = matcher.estimator_params("F", **vr.BUDGET["F"])
    lp = C.POINTER(C.c_int64)
    rc = _lib.lib().mi_degensac_match_verify_batch_dev(0, C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), o2.ctypes.data_as(lp),
                                                       k1.data_ptr(), k2.data_ptr(), 2, K, C.byref(prm), d_seeds.data_ptr(), 0,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream), M.data_ptr(), match.data_ptr(),
                                                       inl.data_ptr(), st.data_ptr(), cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, _lib.lib().mi_degensac_last_error()
    torch.cuda.synchronize()
    own = slice(int(o1[0]), int(o1[-1]))
    got = _split((M.view(K, 3, 3), match[own], inl[own].to(torch.bool), st, cnt), o1 - 5)
    for p, sc in enumerate(scs):
        _agree(got[p], want[p], sc, True, p)
    assert (match[:own.start] == -7).all() and (match[own.stop:] == -7).all() and (inl[:own.start] == 7).all() and (inl[own.stop:] == 7).all()
    assert got[2]["cnt"] == 10 and len(sc_m["kept"][False]) == 11       # the duplicated query fell to the mutual check
