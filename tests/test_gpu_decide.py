"""GPU: the decision rule (NN, MNN, SMNN, max_dist) through the dense, batched, pair-list, F+H and guided calls.  Equality only.  Every
decision is checked against the restatement of tests/decide_ref.py applied to the 2-NN outputs of the existing knn_match_* calls (forward,
and sides swapped) and against the kept set the scene states; the estimator half of the pipeline calls against the CPU restatement of
tests/verify_ref.py on the restatement's tentatives (masks and counters bit for bit, models to 1e-9)."""
import numpy as np
import pytest

from pydegensac_amd import matcher, tensor_api
from tests import decide_ref as dr
from tests import verify_ref as vr

pytestmark = pytest.mark.gpu
CTR = [0, 1, 3]
STABLE = list(range(12)) + [14, 15]                                     # a stats row but for its two tick counters


def _same(a, b, stats=(3,)):
    """two device result tuples bit for bit; the stats rows (positions `stats`) but for the tick counters, which are timings"""
    for i, (x, y) in enumerate(zip(a, b)):
        x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x); y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
        if i in stats:
            x, y = x[:, STABLE], y[:, STABLE]
        if not np.array_equal(x, y):
            return False
    return True


NEXT_BELOW_1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
F_ANY = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])     # with a huge px_th every row passes the gate


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _knn_both(d1, d2, c1, c2, norm):
    """the existing batched 2-NN, forward and with the sides swapped, as numpy"""
    a, b = _t(d1), _t(d2)
    idx, dist = tensor_api.knn_match_batch_tensors(a, b, c1, c2, norm)
    back, bdist = tensor_api.knn_match_batch_tensors(b, a, c2, c1, norm)
    return [x.cpu().numpy() for x in (idx, dist, back, bdist)]


def _restated(d1, d2, c1, c2, norm, ratio, mutual, max_dist, guided=False):
    """match [N1] of the restatement on the device's own 2-NN outputs, pair by pair"""
    idx, dist, back, bdist = _knn_both(d1, d2, c1, c2, norm)
    flags, r, mu, md = dr.rule_flags(ratio, mutual, max_dist)
    o1 = np.r_[0, np.cumsum(c1)]; o2 = np.r_[0, np.cumsum(c2)]
    out = np.full(len(d1), -1, np.int32)
    for p in range(len(c1)):
        s1 = slice(o1[p], o1[p + 1]); s2 = slice(o2[p], o2[p + 1])
        keep = (dr.decide_guided if guided else dr.decide)(idx[s1], dist[s1], r, back[s2] if mu else None, bdist[s2], flags, md)
        out[s1] = np.where(keep, idx[s1, 0], -1)
    return out


def _stated(sc, key):
    m = np.full(sc["n1"], -1, np.int32); q = np.asarray(dr.KEPT[key], np.int64); m[q] = sc["train_of"][q]
    return m


def _kp(n, seed=0):
    return np.random.default_rng(seed).uniform(0, 500, (n, 2))


# ---- the dense calls ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", vr.NORMS)
def test_dense_calls_on_the_designed_scene(norm):
    import torch
    sc = dr.scene(norm)
    a, b = _t(sc["d1"]), _t(sc["d2"])
    idx, dist = tensor_api.knn_match_tensors(a, b, norm); back, bdist = tensor_api.knn_match_tensors(b, a, norm)
    side = torch.cuda.Stream()
    for key in dr.KEPT:
        ratio, mutual, md = key; want = _stated(sc, key)
        assert np.array_equal(_restated(sc["d1"], sc["d2"], [sc["n1"]], [sc["n2"]], norm, *key), want), key
        keep = tensor_api.match_decide_tensors(idx, dist, ratio, back if mutual else None, bdist if mutual else None, md, mutual == "ratio")
        assert np.array_equal(np.flatnonzero(keep.cpu().numpy()), dr.KEPT[key]), key
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                   # a second stream
            q, t, d = tensor_api.match_snn_tensors(a, b, ratio, mutual, norm, max_dist=md)
        side.synchronize()
        assert np.array_equal(q.cpu().numpy(), dr.KEPT[key]) and np.array_equal(t.cpu().numpy(), sc["train_of"][dr.KEPT[key]]), key
        qn, tn, dn = matcher.match_snn(sc["d1"], sc["d2"], ratio, mutual, norm, max_dist=md)     # the numpy entry point
        assert np.array_equal(qn, dr.KEPT[key]) and np.array_equal(tn, sc["train_of"][qn]) and np.array_equal(dn, d.cpu().numpy()), key
    for f, key in ((matcher.match_nn, (None, False, None)), (matcher.match_mnn, (None, True, None))):
        assert list(f(sc["d1"], sc["d2"], norm=norm)[0]) == dr.KEPT[key]
    assert list(matcher.match_mnn(sc["d1"], sc["d2"], 1.0, norm)[0]) == dr.KEPT[(None, True, 1.0)]
    assert list(matcher.match_mnn(sc["d1"], sc["d2"], NEXT_BELOW_1, norm)[0]) == dr.KEPT[(None, True, NEXT_BELOW_1)]
    assert list(matcher.match_smnn(sc["d1"], sc["d2"], dr.RATIO, norm=norm)[0]) == dr.KEPT[(dr.RATIO, "ratio", None)]
    assert list(matcher.match_smnn(sc["d1"], sc["d2"], 0.6, norm=norm)[0]) == dr.KEPT[(0.6, "ratio", None)]


def test_decide_0_and_a_max_dist_above_every_d0_are_the_existing_dense_call():
    sc = dr.scene("l2"); a, b = _t(sc["d1"]), _t(sc["d2"])
    idx, dist = tensor_api.knn_match_tensors(a, b); back, bdist = tensor_api.knn_match_tensors(b, a)
    for bk in (None, back):
        old = tensor_api.match_filter_tensors(idx, dist, dr.RATIO, bk).cpu().numpy()
        for md in (None, 2.0, 1e30):
            new = tensor_api.match_decide_tensors(idx, dist, dr.RATIO, bk, None, md).cpu().numpy()
            assert np.array_equal(old, new)
    q0 = matcher.match_snn(sc["d1"], sc["d2"], dr.RATIO, True)
    q1 = matcher.match_snn(sc["d1"], sc["d2"], dr.RATIO, True, max_dist=2.0)
    assert all(np.array_equal(x, y) for x, y in zip(q0, q1))


def test_no_ratio_needs_slot_0_only():
    one = vr.designed_pair("F", 9, [], train="one")
    for n2 in (0, 1, 2):
        d2 = np.concatenate([one["d2"], one["d1"][3:4]])[:n2]
        q, t, _ = matcher.match_nn(one["d1"], d2)
        qr, tr = dr.tentatives(one["d1"], d2, None, False, None)
        assert np.array_equal(q, qr) and np.array_equal(t, tr) and list(q) == ([] if n2 == 0 else list(range(9)))       # a single train row matches
        assert n2 != 1 or not t.any()
        qs = matcher.match_snn(one["d1"], d2, 0.9)[0]
        assert np.array_equal(qs, dr.tentatives(one["d1"], d2, 0.9, False, None)[0]) and (n2 == 2 or len(qs) == 0)
    bad = np.full((1, 16), np.nan, np.float32)                             # a non-finite train row is no neighbour: slot 0 stays empty
    assert len(matcher.match_nn(one["d1"], bad)[0]) == 0 and len(matcher.match_mnn(one["d1"], bad)[0]) == 0
    q, t, _ = matcher.match_nn(one["d1"], np.concatenate([bad, one["d2"]]))
    assert list(q) == list(range(9)) and list(t) == [1] * 9


# ---- the batched and pair-list pipeline ---------------------------------------------------------------------------------------------------
def _split(res, offsets):
    M, match, inl, st = (x.cpu().numpy() for x in res[:4]); cnt = res[4]
    return [dict(model=M[p], match=match[offsets[p]:offsets[p + 1]], inlier=inl[offsets[p]:offsets[p + 1]], cnt=int(cnt[p]),
                 counters=tuple(int(c) for c in st[p, CTR]), stats=st[p]) for p in range(len(cnt))]


def _batch(scs, seeds, **kw):
    sc0 = scs[0]; c1 = [s["n1"] for s in scs]; c2 = [s["n2"] for s in scs]
    args = [_t(np.concatenate([s[k] for s in scs])) for k in ("k1", "k2", "d1", "d2")]
    res = tensor_api.match_and_verify_batch_tensors(*args, c1, c2, model=sc0["model"], seeds=seeds, norm=sc0["norm"], **vr.BUDGET[sc0["model"]], **kw)
    return _split(res, np.r_[0, np.cumsum(c1)]), res


def _check_pair(port, got, sc, seed, ratio, mutual, md, tag):
    want = dr.pair_ref(port, sc["model"], sc["k1"], sc["k2"], sc["d1"], sc["d2"], seed, ratio, mutual, md, sc["norm"])
    bad = vr.disagreements(got, want)
    assert not bad, (tag, bad, got["cnt"], want["cnt"], got["counters"], want["counters"])
    dev = _restated(sc["d1"], sc["d2"], [sc["n1"]], [sc["n2"]], sc["norm"], ratio, mutual, md)
    assert np.array_equal(got["match"], dev), tag
    return want


@pytest.mark.parametrize("model,n", [("F", 7), ("F", 8), ("F", 9), ("H", 3), ("H", 4), ("H", 5)])
def test_tentative_counts_from_a_single_train_row(oracle_port, model, n):
    """n queries against ONE train row: the ratio test keeps nothing, NO_RATIO keeps all n, at the eligibility thresholds"""
    sc = vr.designed_pair(model, n, [], train="one", seed=n)
    (got,), _ = _batch([sc], [70 + n], ratio=None)
    want = _check_pair(oracle_port, got, sc, 70 + n, None, False, None, n)
    assert got["cnt"] == n and list(got["match"]) == [0] * n
    assert (got["counters"][0] > 0) == (n >= vr.MIN_PTS[model]) and want["cnt"] == n
    (old,), _ = _batch([sc], [70 + n], ratio=0.9)
    assert old["cnt"] == 0 and not old["stats"].any()


ROW_CASES = [(0, []), (1, [0]), (63, list(range(55, 63))), (64, [0, 1, 2, 3, 60, 61, 62, 63]), (65, [0, 1, 62, 63, 64, 30, 31, 32]),
             (255, [0, 63, 64, 127, 128, 191, 192, 254]), (256, [0, 1, 2, 3, 252, 253, 254, 255]), (257, [0, 63, 64, 255, 256, 100, 101, 102]),
             (600, [0, 255, 256, 257, 511, 512, 513, 599])]


@pytest.mark.parametrize("n,kept", ROW_CASES, ids=[str(n) for n, _ in ROW_CASES])
def test_row_counts_around_the_sweep(oracle_port, n, kept):
    """kept rows at the ballot, wave and sweep edges of mt_filter_rank_kernel; ratio 0.9 with max_dist = 0 keeps the exact copies, i.e. the
    stated rows, and MNN keeps them too (plus what the dropped kinds add, from the restatement)"""
    kept = sorted(kept)
    sc = vr.designed_pair("F", n, kept, norm=vr.NORMS[n % 3], seed=n)
    (got,), res = _batch([sc], [n + 5], ratio=0.9, max_dist=0.0)
    _check_pair(oracle_port, got, sc, n + 5, 0.9, False, 0.0, n)
    assert list(np.flatnonzero(got["match"] >= 0)) == kept and np.array_equal(got["match"][kept], sc["train_of"][kept])
    (old,), res0 = _batch([sc], [n + 5], ratio=0.9)                     # max_dist at every d0 (= 0): bit for bit the existing call
    assert _same(res[:5], res0[:5])
    (mnn,), _ = _batch([sc], [n + 5], ratio=None, mutual=True)
    _check_pair(oracle_port, mnn, sc, n + 5, None, True, None, (n, "mnn"))
    assert set(kept) <= set(np.flatnonzero(mnn["match"] >= 0))


@pytest.mark.parametrize("name", list(vr.ARRANGEMENTS))
def test_pair_arrangements(oracle_port, name):
    scs = vr.batch_scene("F", name); seeds = vr.batch_seeds(name)
    got, res = _batch(scs, seeds, ratio=None, mutual=True, max_dist=0.0)      # MNN at distance 0: the exact copies
    for p, sc in enumerate(scs):
        _check_pair(oracle_port, got[p], sc, seeds[p], None, True, 0.0, (name, p))
        assert set(sc["kept"][True]) <= set(np.flatnonzero(got[p]["match"] >= 0))
    _, old = _batch(scs, seeds, ratio=0.9)
    _, same = _batch(scs, seeds, ratio=0.9, max_dist=1e30)
    assert _same(old[:5], same[:5])


# ---- pair lists over stores, the FGINN list, F+H, guided ---------------------------------------------------------------------------------
LIST = [(3, 3), (0, 1), (1, 0), (2, 2), (0, 0), (3, 0)]                  # the last image first, self-indexed pairs, both orders


def _stores(norm):
    scs = [dr.scene(norm, seed=s) for s in range(4)]
    D1 = np.concatenate([s["d1"] for s in scs]); D2 = np.concatenate([s["d2"] for s in scs])
    c1 = [s["n1"] for s in scs]; c2 = [s["n2"] for s in scs]
    return scs, D1, D2, c1, c2, _kp(len(D1), 1), _kp(len(D2), 2)


@pytest.mark.parametrize("norm", vr.NORMS)
@pytest.mark.parametrize("key", [(dr.RATIO, "ratio", None), (None, True, 1.0), (None, True, NEXT_BELOW_1), (dr.RATIO, False, 1.0), (None, False, None)],
                         ids=repr)
def test_pair_lists_on_two_stores(norm, key):
    scs, D1, D2, c1, c2, K1, K2 = _stores(norm)
    ratio, mutual, md = key
    want = np.concatenate([_stated(scs[j], key) for _, j in LIST])        # the queries' codes are the same in every image: image j's rows decide
    from tests import pairs_ref
    (e1,), (e2,), ec1, ec2, po = pairs_ref.expand((D1,), c1, (D2,), c2, LIST)
    assert np.array_equal(_restated(e1, e2, ec1, ec2, norm, *key), want)
    kw = dict(ratio=ratio, mutual=mutual, max_dist=md, norm=norm)
    r = tensor_api.match_and_verify_pairs_tensors(_t(K1), _t(K2), _t(D1), _t(D2), c1, c2, LIST, **kw)
    assert np.array_equal(r[1].cpu().numpy(), want) and list(r[4]) == [len(dr.KEPT[key])] * len(LIST) and np.array_equal(r[5], po)
    fh = tensor_api.match_and_verify_fh_pairs_tensors(_t(K1), _t(K2), _t(D1), _t(D2), c1, c2, LIST, **kw)
    assert np.array_equal(fh[2].cpu().numpy(), want) and np.array_equal(fh[7].cpu().numpy()[:, 0], r[4])
    Ms = _t(np.tile(F_ANY, (len(LIST), 1, 1)))
    g = tensor_api.guided_match_pairs_tensors(_t(K1), _t(K2), _t(D1), _t(D2), c1, c2, LIST, Ms, px_th=1e9, **kw)
    assert np.array_equal(g[0].cpu().numpy(), _restated(e1, e2, ec1, ec2, norm, *key, guided=True))
    assert np.array_equal(g[0].cpu().numpy(), want)                       # every train row here has two query rows: both forms agree
    if mutual != "ratio" and ratio is not None:                          # FGINN goes with max_dist only; radius 0 is the plain second neighbour
        f = tensor_api.match_and_verify_fginn_pairs_tensors(_t(K1), _t(K2), _t(D1), _t(D2), c1, c2, LIST, 0.0, **kw)
        assert np.array_equal(f[1].cpu().numpy(), want)
        gf = tensor_api.guided_match_pairs_tensors(_t(K1), _t(K2), _t(D1), _t(D2), c1, c2, LIST, Ms, px_th=1e9, fginn_th=0.0, **kw)
        assert np.array_equal(gf[0].cpu().numpy(), want)
    M, ml, il = matcher.match_and_verify_pairs([K1[s:s + 10] for s in range(0, 40, 10)], [D1[s:s + 10] for s in range(0, 40, 10)], LIST,
                                               kps2_list=np.split(K2, np.cumsum(c2)[:-1]), desc2_list=np.split(D2, np.cumsum(c2)[:-1]), **kw)
    assert np.array_equal(np.concatenate(ml), want)                       # the numpy entry point


def test_self_pairs_in_one_store():
    """a collection against itself: the list holds (i, i); every query's nearest row is itself at distance 0, so MNN keeps the lower of two
    equal rows and max_dist = 0 changes nothing"""
    scs, D1, _, c1, _, K1, _ = _stores("l2")
    lst = [(2, 2), (0, 1), (1, 0)]
    from tests import pairs_ref
    (e1,), (e2,), ec1, ec2, _ = pairs_ref.expand((D1,), c1, (D1,), c1, lst)
    d = _t(D1); k = _t(K1)
    for key in ((None, True, None), (None, True, 0.0), (0.9, "ratio", None)):
        r = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, c1, c1, lst, ratio=key[0], mutual=key[1], max_dist=key[2])
        assert np.array_equal(r[1].cpu().numpy(), _restated(e1, e2, ec1, ec2, "l2", *key)), key
    # the self pair (2, 2) under SMNN: every row is its own neighbour at 0, and the equal rows 8 | 9 fail d0 < r d1 in both directions
    assert np.array_equal(r[1].cpu().numpy()[:10] >= 0, np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 0], bool))      # SMNN: the tie 8 | 9 fails bd0 < r bd1


def test_back_ratio_with_a_single_query_row_unguided_dropped_guided_kept():
    sc = dr.scene("l2")
    d1 = sc["d1"][:1]; d2 = sc["d2"]; k1 = _kp(1); k2 = _kp(sc["n2"], 3)
    args = (_t(k1), _t(k2), _t(d1), _t(d2), [1], [sc["n2"]])
    r = tensor_api.match_and_verify_batch_tensors(*args, ratio=0.9, mutual="ratio")
    assert r[1].cpu().numpy()[0] == -1 and _restated(d1, d2, [1], [sc["n2"]], "l2", 0.9, "ratio", None)[0] == -1
    assert tensor_api.match_and_verify_batch_tensors(*args, ratio=0.9, mutual=True)[1].cpu().numpy()[0] == sc["train_of"][0]
    g = tensor_api.guided_match_batch_tensors(*args, _t(F_ANY[None]), px_th=1e9, ratio=0.9, mutual="ratio")
    assert g[0].cpu().numpy()[0] == sc["train_of"][0] == _restated(d1, d2, [1], [sc["n2"]], "l2", 0.9, "ratio", None, guided=True)[0]
    q, t, _ = matcher.guided_match(k1, k2, d1, d2, F_ANY, px_th=1e9, ratio=0.9, mutual="ratio")
    assert list(q) == [0] and list(t) == [sc["train_of"][0]]
    assert len(matcher.match_smnn(d1, d2, 0.9)[0]) == 0 and list(matcher.match_mnn(d1, d2)[0]) == [0]


@pytest.mark.parametrize("model", ["F", "H"])
def test_the_estimator_half_under_a_rule_and_unchanged_outputs_of_fh_and_guided(oracle_port, model):
    sc = vr.rank_scene(model, "every2", 65); seed = vr.rank_seed(model, "every2", 65)
    for key in ((0.9, "ratio", None), (0.9, True, 0.0)):
        (got,), _ = _batch([sc], [seed], ratio=key[0], mutual=key[1], max_dist=key[2])
        want = _check_pair(oracle_port, got, sc, seed, *key, key)
        assert want["cnt"] >= vr.MIN_PTS[model] and got["counters"][0] > 0
    args = [_t(sc[k]) for k in ("k1", "k2", "d1", "d2")] + [[sc["n1"]], [sc["n2"]]]
    a = tensor_api.match_and_verify_fh_batch_tensors(*args, ratio=0.9, mutual=True, norm=sc["norm"], seeds=[seed])
    b = tensor_api.match_and_verify_fh_batch_tensors(*args, ratio=0.9, mutual=True, norm=sc["norm"], seeds=[seed], max_dist=1e30)
    assert _same(a[:9], b[:9], stats=(5, 6))
    Ms = _t(F_ANY[None])
    ga = tensor_api.guided_match_batch_tensors(*args, Ms, px_th=1e9, norm=sc["norm"], mutual=True, driver_form=True, model=model)
    gb = tensor_api.guided_match_batch_tensors(*args, Ms, px_th=1e9, norm=sc["norm"], mutual=True, driver_form=True, model=model, max_dist=1e30)
    assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(ga, gb))
