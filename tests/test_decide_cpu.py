"""The decision rule (include/mi_degensac.h MI_DEGENSAC_DECIDE_*: NN, MNN, SMNN and max_dist) without a device: every refusal of the rule
through each family of C entry points, with its message and before a device is looked for (no device exists where these tests run, so a
refusal that needed one would come back as ENODEV); the struct sizes that mean today's rule; the Python keywords and their ValueErrors;
the restatement of tests/decide_ref.py against oracle.matcher_np.match_snn at decide = 0; the stated kept sets of the designed scene under
every rule and norm; and three broken restatements, each rejected by a scene."""
import ctypes as C

import numpy as np
import pytest

from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher, tensor_api
from tests import decide_ref as dr
from tests import verify_ref as vr

EINVAL, ENODEV = -1, -2
NO_RATIO, BACK_RATIO, MAX_DIST = _lib.DECIDE_NO_RATIO, _lib.DECIDE_BACK_RATIO, _lib.DECIDE_MAX_DIST


def _mp(decide=0, max_dist=0.0, ratio=0.9, mutual=False, fginn_th=None, norm=0, dim=8):
    return _lib.MatchParamsEx(norm, dim, ratio, mutual, fginn_th, decide, max_dist)


# ---- every entry point that reads mp->ratio, on the same arguments ----------------------------------------------------------------------
def _abi(mp, ptrs=False, n_pairs=None):
    """{entry point: (rc, message)}.  ptrs=False: every data pointer is NULL, so a call whose rule is accepted ends at the NULL check and
    nothing is ever read; n_pairs=0: an accepted call returns 0."""
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    o1 = np.array([0, 4, 10], np.int64); o2 = np.array([0, 3, 7], np.int64); pr = np.array([[0, 1], [1, 0]], np.int32)
    K = 2 if n_pairs is None else n_pairs
    buf = np.zeros(64); a = buf.ctypes.data if ptrs else None
    t = lambda ty: C.cast(a, C.POINTER(ty)) if a is not None else None                                              # noqa: E731
    prm_f = matcher.estimator_params("F"); prm_h = matcher.estimator_params("H"); gp = _lib.GuideParams(0, 0, 0.5)
    O = (o1.ctypes.data_as(lp), o2.ctypes.data_as(lp)); S = (o1.ctypes.data_as(lp), 2, o2.ctypes.data_as(lp), 2); P = pr.ctypes.data_as(ip)
    dd, uu, ii, bb, ff = t(C.c_double), t(C.c_uint32), t(C.c_int32), t(C.c_uint8), t(C.c_float)
    m = C.byref(mp); out = {}

    def run(name, err, *args):
        rc = getattr(L, name)(*args)
        out[name] = (rc, getattr(L, err)())
    E, M = "mi_degensac_last_error", "mi_degensac_match_last_error"
    run("mi_degensac_match_verify_batch_dev", E, 0, m, a, a, *O, a, a, 2, K, C.byref(prm_f), a, 0, None, a, a, a, None, None)
    run("mi_degensac_match_verify_batch", E, 0, m, a, a, *O, dd, dd, 2, K, C.byref(prm_f), uu, 0, dd, ii, bb, None, None)
    for fg in ("", "fginn_"):
        run(f"mi_degensac_match_verify_{fg}pairs_dev", E, 0, m, a, a, *S, a, a, 2, P, K, C.byref(prm_f), a, 0, None, a, a, a, None, None)
        run(f"mi_degensac_match_verify_{fg}pairs", E, 0, m, a, a, *S, dd, dd, 2, P, K, C.byref(prm_f), uu, 0, dd, ii, bb, None, None)
    f2 = (C.byref(prm_f), C.byref(prm_h))
    run("mi_degensac_match_verify_fh_batch_dev", E, m, a, a, *O, a, a, 2, K, *f2, a, 0, None, a, a, a, a, a, None, None, a, None)
    run("mi_degensac_match_verify_fh_batch", E, m, a, a, *O, dd, dd, 2, K, *f2, uu, 0, dd, dd, ii, bb, bb, None, None, ii, None)
    run("mi_degensac_match_verify_fh_pairs_dev", E, m, a, a, *S, a, a, 2, P, K, *f2, a, 0, None, a, a, a, a, a, None, None, a, None)
    run("mi_degensac_match_verify_fh_pairs", E, m, a, a, *S, dd, dd, 2, P, K, *f2, uu, 0, dd, dd, ii, bb, bb, None, None, ii, None)
    for fg in ("", "fginn_"):
        run(f"mi_degensac_match_guided_{fg}batch_dev", M, m, a, a, *O, a, a, 2, K, a, C.byref(gp), 0, None, a, a, a, None, None)
        run(f"mi_degensac_match_guided_{fg}batch", M, m, a, a, *O, dd, dd, 2, K, dd, C.byref(gp), 0, ii, ff, ii, None)
        run(f"mi_degensac_match_guided_{fg}pairs_dev", M, m, a, a, *S, P, K, a, a, 2, a, C.byref(gp), 0, None, a, a, a, None, None)
        run(f"mi_degensac_match_guided_{fg}pairs", M, m, a, a, *S, P, K, dd, dd, 2, dd, C.byref(gp), 0, ii, ff, ii, None)
    if n_pairs is None:                         # the dense siblings have no pair count: rows, and NULL data
        run("mi_degensac_match_decide_dev", M, m, a, a, 5, a, a, 0, None, a)
        run("mi_degensac_match_ex", M, m, a, 5, a, 5, 0, ii, ff, bb)
    return out


FGINN_ENTRIES = lambda name: "fginn" in name or "_fh_" in name or name.endswith("verify_batch_dev") or name.endswith("verify_batch")   # noqa: E731


def _refused(res, word, only=None):
    hit = 0
    for name, (rc, msg) in res.items():
        if only is not None and not only(name):
            continue
        assert rc == EINVAL and word in msg, (name, rc, msg)
        hit += 1
    assert hit


def _accepted(mp):
    """the rule is taken: with NULL data every call ends at its NULL / bad-argument check (mi_degensac_match_verify_batch_dev asks for the
    device first: ENODEV where there is none), with no pairs it returns 0"""
    for name, (rc, msg) in _abi(mp).items():
        assert (rc == EINVAL and (b"NULL" in msg or b"bad argument" in msg)) or (rc == ENODEV and b"no HIP device" in msg), (name, rc, msg)
    assert all(rc == 0 for rc, _ in _abi(mp, n_pairs=0).values())


def test_the_symbols_and_the_layout():
    assert hasattr(_lib.lib(), "mi_degensac_match_decide_dev") and hasattr(_lib.lib(), "mi_degensac_match_ex")
    assert C.sizeof(_lib.MatchParamsEx) == 40 and _lib.MatchParamsEx.decide.offset == 32 and _lib.MatchParamsEx.max_dist.offset == 36
    assert C.sizeof(_lib.MatchParams) == 32                              # the first layouts stay what they were
    assert _mp().struct_size == 40 and isinstance(_mp(), _lib.MatchParams)


@pytest.mark.parametrize("decide", [8, 16, -1, 1 << 30, 8 | NO_RATIO])
def test_abi_refuses_an_unknown_bit(decide):
    _refused(_abi(_mp(decide, mutual=True)), b"unknown bit")
    _refused(_abi(_mp(decide, mutual=True), n_pairs=0), b"unknown bit")


def test_abi_refuses_no_ratio_with_back_ratio():
    _refused(_abi(_mp(NO_RATIO | BACK_RATIO, mutual=True)), b"exclude")
    _refused(_abi(_mp(NO_RATIO | BACK_RATIO | MAX_DIST, 1.0, mutual=True), n_pairs=0), b"exclude")


def test_abi_refuses_back_ratio_without_mutual():
    _refused(_abi(_mp(BACK_RATIO, mutual=False)), b"mutual")
    _refused(_abi(_mp(BACK_RATIO | MAX_DIST, 1.0, mutual=False), n_pairs=0), b"mutual")
    _accepted(_mp(BACK_RATIO, mutual=True))


@pytest.mark.parametrize("decide", [NO_RATIO, BACK_RATIO, NO_RATIO | MAX_DIST])
def test_abi_refuses_no_ratio_and_back_ratio_with_an_honoured_fginn(decide):
    mp = _mp(decide, 1.0, mutual=True, fginn_th=5.0)
    res = _abi(mp)
    _refused(res, b"second_nn", FGINN_ENTRIES)                          # where second_nn = 1 is honoured the rule refuses it
    _refused({k: v for k, v in res.items() if k.endswith("match_ex")}, b"second_nn")
    for name, (rc, msg) in res.items():                                  # the plain guided calls and decide_dev do not read second_nn
        if "guided_b" in name or "guided_p" in name or name.endswith("decide_dev"):
            assert rc == EINVAL and b"NULL" in msg, (name, msg)
    _refused(_abi(mp, n_pairs=0), b"second_nn", FGINN_ENTRIES)


def test_abi_max_dist_goes_with_fginn():
    mp = _mp(MAX_DIST, 3.0, fginn_th=5.0)
    for name, (rc, msg) in _abi(mp).items():
        if FGINN_ENTRIES(name) or "guided" in name:
            assert (rc == EINVAL and b"NULL" in msg) or rc == ENODEV, (name, msg)


@pytest.mark.parametrize("md", [-1.0, -1e-30, float("nan"), float("inf"), -float("inf")])
def test_abi_refuses_a_bad_max_dist_only_with_its_bit(md):
    _refused(_abi(_mp(MAX_DIST, md)), b"max_dist")
    _refused(_abi(_mp(MAX_DIST | NO_RATIO, md), n_pairs=0), b"max_dist")
    _accepted(_mp(0, md)); _accepted(_mp(NO_RATIO, md))                  # not read without the bit


def test_abi_ratio_is_not_read_under_no_ratio_and_still_checked_without():
    for r in (0.0, -1.0, float("nan"), float("inf")):
        _accepted(_mp(NO_RATIO, ratio=r)); _accepted(_mp(NO_RATIO | MAX_DIST, 2.0, ratio=r, mutual=True))
        _refused(_abi(_mp(MAX_DIST, 2.0, ratio=r)), b"ratio")
        _refused(_abi(_mp(BACK_RATIO, ratio=r, mutual=True)), b"ratio")


@pytest.mark.parametrize("size", [0, 24, 32, 36, -1, -40])
def test_abi_a_struct_size_that_does_not_cover_the_rule_is_todays_rule_whatever_the_bytes_hold(size):
    for decide, md in ((NO_RATIO | BACK_RATIO, float("nan")), (-1, -5.0), (BACK_RATIO, 0.0)):
        mp = _mp(decide, md, mutual=False); mp.struct_size = size
        _accepted(mp)
    mp = _mp(NO_RATIO, ratio=0.0); mp.struct_size = size                 # ... so the ratio is read, and refused
    _refused(_abi(mp), b"ratio")


def test_abi_a_zeroed_struct_of_the_new_size_is_todays_rule():
    mp = _lib.MatchParamsEx.from_buffer_copy(bytes(40))
    mp.dim = 8; mp.ratio = 0.9; mp.struct_size = 40
    assert mp.decide == 0 and mp.max_dist == 0.0
    _accepted(mp)
    mp.ratio = 0.0
    _refused(_abi(mp), b"ratio")


def test_abi_the_dense_siblings_check_their_own_arguments():
    L = _lib.lib(); mp = _mp(BACK_RATIO, mutual=True); buf = np.zeros(64); a = buf.ctypes.data
    assert L.mi_degensac_match_decide_dev(None, a, a, 5, a, a, 0, None, a) == EINVAL and b"NULL" in L.mi_degensac_match_last_error()
    assert L.mi_degensac_match_decide_dev(C.byref(mp), a, a, -1, a, a, 0, None, a) == EINVAL
    assert L.mi_degensac_match_decide_dev(C.byref(mp), a, a, 5, None, a, 0, None, a) == EINVAL and b"d_back_idx" in L.mi_degensac_match_last_error()
    assert L.mi_degensac_match_decide_dev(C.byref(mp), a, a, 5, a, None, 0, None, a) == EINVAL and b"d_back_dist" in L.mi_degensac_match_last_error()
    assert L.mi_degensac_match_ex(None, None, 5, None, 5, 0, None, None, None) == EINVAL
    for norm, dim in ((2, 8), (1, 6), (4, 260), (0, 0)):
        assert L.mi_degensac_match_ex(C.byref(_mp(NO_RATIO, norm=norm, dim=dim)), None, 5, None, 5, 0, None, None, None) == EINVAL


# ---- the Python keywords ----------------------------------------------------------------------------------------------------------------
def test_check_rule_builds_the_flags():
    R = matcher.check_rule
    assert R(0.9) == (0.9, False, 0, 0.0) and R(0.9, True) == (0.9, True, 0, 0.0)
    assert R(None).decide == NO_RATIO and R(None, True, 2).decide == NO_RATIO | MAX_DIST and R(None, True, 2).max_dist == 2.0
    assert R(0.8, "ratio") == (0.8, True, BACK_RATIO, 0.0)
    assert R(0.8, False, 0, fginn=True).decide == MAX_DIST
    assert isinstance(_lib.match_params(0, 8, R(0.9, True)), _lib.MatchParams) and not isinstance(_lib.match_params(0, 8, R(0.9, True)), _lib.MatchParamsEx)
    mp = _lib.match_params(0, 8, R(None, True, 1.5), None)
    assert isinstance(mp, _lib.MatchParamsEx) and (mp.decide, mp.max_dist, mp.mutual, mp.struct_size) == (NO_RATIO | MAX_DIST, 1.5, 1, 40)


@pytest.mark.parametrize("kw,word", [(dict(ratio=0.0), "ratio"), (dict(ratio=float("nan")), "ratio"), (dict(ratio="x"), "ratio"),
                                     (dict(mutual="both"), "mutual"), (dict(ratio=None, mutual="ratio"), "ratio"),
                                     (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("inf")), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
                                     (dict(max_dist="far"), "max_dist"), (dict(max_dist=1e39), "max_dist"),
                                     (dict(ratio=None, fginn=True), "FGINN"), (dict(mutual="ratio", fginn=True), "FGINN")], ids=repr)
def test_check_rule_refuses(kw, word):
    with pytest.raises(ValueError, match=word):
        matcher.check_rule(**{"ratio": 0.9, **kw})


BAD = [dict(max_dist=-1.0), dict(mutual="both"), dict(ratio=None, mutual="ratio"), dict(max_dist=float("nan"))]


@pytest.mark.parametrize("kw", BAD, ids=repr)
def test_every_call_takes_the_keywords_and_refuses_bad_values_before_anything_else(kw):
    d = np.zeros((6, 8), np.float32); k = np.zeros((6, 2)); pairs = [(0, 1)]; M = np.zeros((1, 3, 3))
    calls = [lambda: matcher.match_snn(d, d, **{"ratio": 0.9, **kw}),
             lambda: matcher.tentative_points(k, k, d, d, **{"ratio": 0.9, **kw}),
             lambda: matcher.match_fginn(d, d, k, **{"ratio": 0.9, **kw}),
             lambda: matcher.guided_match_batch([k], [k], [d], [d], M, **kw), lambda: matcher.guided_match(k, k, d, d, M[0], **kw),
             lambda: matcher.match_and_verify_batch([k], [k], [d], [d], **kw), lambda: matcher.match_and_verify_pairs([k, k], [d, d], pairs, **kw),
             lambda: matcher.match_and_verify_fginn_pairs([k, k], [d, d], pairs, 5.0, **kw),
             lambda: matcher.match_and_verify_fh_batch([k], [k], [d], [d], **kw), lambda: matcher.match_and_verify_fh_pairs([k, k], [d, d], pairs, **kw),
             lambda: matcher.guided_match_pairs([k, k], [d, d], pairs, M, **kw),
             lambda: tensor_api.match_snn_tensors(None, None, **{"ratio": 0.9, **kw}),
             lambda: tensor_api.guided_match_batch_tensors(None, None, None, None, [6], [6], None, **kw),
             lambda: tensor_api.match_and_verify_batch_tensors(None, None, None, None, [6], [6], **kw),
             lambda: tensor_api.match_and_verify_pairs_tensors(None, None, None, None, [6], [6], pairs, **kw),
             lambda: tensor_api.match_and_verify_fginn_pairs_tensors(None, None, None, None, [6], [6], pairs, 5.0, **kw),
             lambda: tensor_api.match_and_verify_fh_batch_tensors(None, None, None, None, [6], [6], **kw),
             lambda: tensor_api.match_and_verify_fh_pairs_tensors(None, None, None, None, [6], [6], pairs, **kw),
             lambda: tensor_api.guided_match_pairs_tensors(None, None, None, None, [6], [6], pairs, None, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="ratio|mutual|max_dist"):
            call()


def test_fginn_calls_refuse_the_rules_that_have_no_second_neighbour():
    d = np.zeros((6, 8), np.float32); k = np.zeros((6, 2)); M = np.zeros((1, 3, 3))
    for kw in (dict(ratio=None), dict(mutual="ratio")):
        for call in (lambda: matcher.match_fginn(d, d, k, **{"ratio": 0.9, **kw}), lambda: matcher.match_and_verify_batch([k], [k], [d], [d], fginn_th=5.0, **kw),
                     lambda: matcher.match_and_verify_fginn_pairs([k, k], [d, d], [(0, 1)], 5.0, **kw),
                     lambda: matcher.guided_match_batch([k], [k], [d], [d], M, fginn_th=5.0, **kw),
                     lambda: matcher.match_and_verify_batch([k], [k], [d], [d], guided=True, guided_fginn_th=5.0, **kw),
                     lambda: tensor_api.match_and_verify_fh_batch_tensors(None, None, None, None, [6], [6], fginn_th=5.0, **kw)):
            with pytest.raises(ValueError, match="FGINN"):
                call()


def test_match_decide_tensors_checks_its_arguments():
    for kw in (dict(back_ratio=True), dict(back_ratio=True, back=object())):
        with pytest.raises(ValueError, match="back_dist"):
            tensor_api.match_decide_tensors(None, None, **kw)
    with pytest.raises(ValueError, match="max_dist"):
        tensor_api.match_decide_tensors(None, None, max_dist=-2.0)
    with pytest.raises(ValueError, match="ratio"):
        tensor_api.match_decide_tensors(None, None, ratio=0.0)


def test_match_nn_mnn_smnn_check_their_arguments():
    d = np.zeros((6, 8), np.float32)
    for f in (matcher.match_nn, matcher.match_mnn, matcher.match_smnn):
        with pytest.raises(ValueError, match="max_dist"):
            f(d, d, max_dist=-1.0)
        with pytest.raises(ValueError, match="descriptors"):
            f(d, d[:, :4])
        with pytest.raises(ValueError, match="descriptors"):
            f(d[0], d)
        with pytest.raises(ValueError, match="norm"):
            f(d, d, norm="cosine")
        with pytest.raises(ValueError, match="uint8"):
            f(d, d, norm="hamming")
    for r in (0.0, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="ratio"):
            matcher.match_smnn(d, d, ratio=r)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["l2", "hamming"])
@pytest.mark.parametrize("mutual", [False, True])
def test_restatement_is_match_snn_at_decide_0(norm, mutual):
    rng = np.random.default_rng(5)
    for n1, n2 in ((40, 33), (7, 1), (5, 2), (30, 30)):
        if norm == "l2":
            d1 = rng.integers(0, 4, (n1, 6)).astype(np.float32); d2 = rng.integers(0, 4, (n2, 6)).astype(np.float32)   # many ties and near rows
        else:
            d1 = rng.integers(0, 256, (n1, 4), dtype=np.uint8); d2 = rng.integers(0, 256, (n2, 4), dtype=np.uint8)
        for ratio in (0.5, 0.9, 1.0):
            q, t, _ = mo.match_snn(d1, d2, ratio, mutual, norm)
            q2, t2 = dr.tentatives(d1, d2, ratio, mutual, None, norm)
            assert np.array_equal(q, q2) and np.array_equal(t, t2)
            idx, dist = mo.knn2(d1, d2, norm); back, bdist = mo.knn2(d2, d1, norm) if mutual else (None, None)
            # the guided form differs exactly where slot 1 is missing
            g = dr.decide_guided(idx, dist, ratio, back, bdist); u = dr.decide(idx, dist, ratio, back, bdist)
            assert np.array_equal(g & (idx[:, 1] >= 0), u) and (n2 != 1 or (g.any() and not u.any()))
    for sel, n in (("every2", 65), ("sweep", 513)):
        sc = vr.rank_scene("F", sel, n)
        q, t = dr.tentatives(sc["d1"], sc["d2"], sc["ratio"], mutual, None, sc["norm"])
        assert np.array_equal(q, sc["kept"][mutual]) and np.array_equal(t, sc["train_of"][q])


@pytest.mark.parametrize("norm", vr.NORMS)
@pytest.mark.parametrize("seed", [0, 1])
def test_the_designed_scene_keeps_what_it_states(norm, seed):
    sc = dr.scene(norm, seed=seed)
    idx, dist = mo.knn2(sc["d1"], sc["d2"], "l2" if norm == "l2_u8" else norm)
    assert sorted(set(dist[:, 0].tolist())) == [0.0, 1.0, 2.0]           # the same small integers under every norm
    assert np.array_equal(idx[:, 0], sc["train_of"])
    for (ratio, mutual, md), want in dr.KEPT.items():
        q, t = dr.tentatives(sc["d1"], sc["d2"], ratio, mutual, md, norm)
        assert list(q) == want and np.array_equal(t, sc["train_of"][q]), (ratio, mutual, md)
    assert set(dr.ROWS) == set(range(dr.N1))


@pytest.mark.parametrize("norm", vr.NORMS)
def test_the_one_word_scene_and_the_widened_scene_keep_what_they_state(norm):
    sc = dr.scalar_scene(norm)
    assert sc["d1"].shape[1] == (1 if norm == "l2" else 4)
    idx, dist = mo.knn2(sc["d1"], sc["d2"], "l2" if norm == "l2_u8" else norm)
    assert dist.tolist() == [[0, 10], [1, 9], [2, 8], [2, 9], [0, 11]] and np.array_equal(idx[:, 0], sc["train_of"])
    for key, want in dr.SCALAR_KEPT.items():
        q, t = dr.tentatives(sc["d1"], sc["d2"], *key, norm)
        assert list(q) == want and np.array_equal(t, sc["train_of"][q]), key
    for dim in {"l2": (64, 65), "l2_u8": (64, 128, 256), "hamming": (256, 260)}[norm]:
        wide = dr.widened(dr.scene(norm), dim)
        for key, want in dr.KEPT.items():
            assert list(dr.tentatives(wide["d1"], wide["d2"], *key, norm)[0]) == want, (dim, key)


def test_designed_pairs_of_verify_ref_under_the_new_rules():
    """what the GPU tests rely on: exact copies have d0 = 0, so max_dist = 0 changes nothing; NO_RATIO keeps every query of a pair with a
    train row, also with a single one"""
    sc = vr.count_scene("F", 8, 0)
    for mutual in (False, True):
        assert np.array_equal(dr.tentatives(sc["d1"], sc["d2"], 0.9, mutual, 0.0, sc["norm"])[0], sc["kept"][mutual])
    one = vr.designed_pair("F", 9, [], train="one")
    q, t = dr.tentatives(one["d1"], one["d2"], None, False, None)
    assert list(q) == list(range(9)) and not t.any()
    assert len(dr.tentatives(one["d1"], one["d2"], 0.9, False, None)[0]) == 0
    assert list(dr.tentatives(one["d1"], one["d2"], None, True, None)[0]) == [0]      # the one train row's nearest query


# ---- three broken restatements, each rejected by a scene --------------------------------------------------------------------------------
def _keep(sc, ratio, mutual, md, broken):
    norm = "l2" if sc["norm"] == "l2_u8" else sc["norm"]
    idx, dist = mo.knn2(sc["d1"], sc["d2"], norm); back, bdist = mo.knn2(sc["d2"], sc["d1"], norm)
    flags, r, mu, m = dr.rule_flags(ratio, mutual, md)
    return np.flatnonzero(broken(idx, dist, np.float32(r), back if mu else None, bdist, flags, np.float32(m)))


def _strict_max_dist(idx, dist, r, back, bdist, flags, md):
    keep = dr.decide(idx, dist, r, back, bdist, flags & ~MAX_DIST)
    return keep & (dist[:, 0] < md) if flags & MAX_DIST else keep        # the defect: < instead of <=


def _back_ratio_at_the_query_row(idx, dist, r, back, bdist, flags, md):
    keep = dr.decide(idx, dist, r, back, bdist, flags & ~BACK_RATIO, md)
    i = np.clip(np.arange(len(idx)), 0, len(back) - 1)                   # the defect: row i of the reverse search instead of row idx[i][0]
    return keep & (back[i, 1] >= 0) & (bdist[i, 0] < r * bdist[i, 1]) if flags & BACK_RATIO else keep


def _no_ratio_demands_slot_1(idx, dist, r, back, bdist, flags, md):
    return dr.decide(idx, dist, r, back, bdist, flags, md) & (idx[:, 1] >= 0)          # the defect


def test_broken_restatements_are_rejected():
    sc = dr.scene("l2")
    key = (None, True, 1.0)
    assert list(_keep(sc, *key, dr.decide)) == dr.KEPT[key]
    assert list(_keep(sc, *key, _strict_max_dist)) != dr.KEPT[key]       # loses the rows at d0 == max_dist
    key = (dr.RATIO, "ratio", None)
    hit = [list(_keep(dr.scene(n, seed=s), *key, _back_ratio_at_the_query_row)) != dr.KEPT[key] for n in vr.NORMS for s in (0, 1)]
    assert all(hit), hit
    one = vr.designed_pair("F", 9, [], train="one")
    assert list(_keep(one, None, False, None, dr.decide)) == list(range(9))
    assert list(_keep(one, None, False, None, _no_ratio_demands_slot_1)) == []
