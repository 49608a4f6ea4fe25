"""GPU: the decision rule at the row widths where the matcher kernels change path (1 / 64 / 65 words, every l2_u8 instance), through the C
entry points on stores that start at a non-zero row, and the estimator half of the pair-list, FGINN-list and F+H calls under a rule against
the CPU restatement (tests/decide_ref.py, tests/verify_ref.py); the unchanged-output check for the pair-list families; FGINN inside the
gate under max_dist; and the contract "no model, no inliers" on the call as it was before the rule."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, tensor_api
from tests import decide_ref as dr
from tests import pairs_ref
from tests import verify_ref as vr
from tests.test_gpu_decide import CTR, F_ANY, LIST, _kp, _restated, _same, _stated, _stores, _t

pytestmark = pytest.mark.gpu
NORM_CODE = {"l2": 0, "hamming": 1, "l2_u8": 4}
WIDTHS = [("l2", 1), ("l2", 64), ("l2", 65), ("l2_u8", 4), ("l2_u8", 64), ("l2_u8", 128), ("l2_u8", 256), ("hamming", 4), ("hamming", 256),
          ("hamming", 260)]                                              # 1 / 64 / 65 words; l2_u8 stops at 64 words and has three instances


# ---- row widths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,dim", WIDTHS)
def test_rules_at_the_row_widths_of_the_matcher_kernels(norm, dim):
    one_word = dim == (1 if norm == "l2" else 4)
    sc = dr.scalar_scene(norm) if one_word else dr.widened(dr.scene(norm), dim)
    kept = dr.SCALAR_KEPT if one_word else dr.KEPT
    assert sc["d1"].shape[1] == dim
    n1, n2 = sc["n1"], sc["n2"]
    args = (_t(_kp(n1, 4)), _t(_kp(n2, 5)), _t(sc["d1"]), _t(sc["d2"]), [n1], [n2])
    for key, rows in kept.items():
        ratio, mutual, md = key
        want = np.full(n1, -1, np.int32); want[rows] = sc["train_of"][rows]
        assert np.array_equal(_restated(sc["d1"], sc["d2"], [n1], [n2], norm, *key), want), key
        kw = dict(ratio=ratio, mutual=mutual, max_dist=md, norm=norm)
        r = tensor_api.match_and_verify_batch_tensors(*args, **kw)
        assert np.array_equal(r[1].cpu().numpy(), want) and int(r[4][0]) == len(rows), key
        g = tensor_api.guided_match_batch_tensors(*args, _t(F_ANY[None]), px_th=1e9, **kw)      # two rows on either side everywhere: both forms agree
        assert np.array_equal(g[0].cpu().numpy(), want), key
        q, t, _ = tensor_api.match_snn_tensors(args[2], args[3], ratio, mutual, norm, max_dist=md)
        assert np.array_equal(q.cpu().numpy(), rows) and np.array_equal(t.cpu().numpy(), sc["train_of"][rows]), key


# ---- the C entry points on stores that start at a non-zero row --------------------------------------------------------------------------
J1, J2 = 3, 5                                                            # rows in front of side 1 / side 2 that belong to nobody
OFFSET_KEYS = [(dr.RATIO, "ratio", None), (None, True, 1.0), (dr.RATIO, False, 1.0), (dr.RATIO, True, None)]


def _mp(norm, dim, key, size40):
    """the match params of a key; size40: the 40-byte struct also where the rule is decide = 0"""
    rule = matcher.check_rule(*key)
    if rule.decide == 0 and not size40:
        return _lib.MatchParams(NORM_CODE[norm], dim, rule.ratio, rule.mutual)
    return _lib.MatchParamsEx(NORM_CODE[norm], dim, rule.ratio, rule.mutual, None, rule.decide, rule.max_dist)


@pytest.mark.parametrize("norm", vr.NORMS)
@pytest.mark.parametrize("key", OFFSET_KEYS, ids=repr)
def test_c_entry_points_with_a_non_zero_first_offset(norm, key):
    """Side 1 starts at row 3 and side 2 at row 5 of their arrays; the rows in front are copies of real rows, so reading them would change
    the answers.  Every key keeps fewer than 8 queries per pair, so no estimator runs.  The last key is decide = 0 in a 40-byte struct."""
    import torch
    scs, D1, D2, c1, c2, K1, K2 = _stores(norm)
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    N1, N2 = len(D1), len(D2)
    a = _t(np.concatenate([D1[5:5 + J1], D1])); b = _t(np.concatenate([D2[2:2 + J2], D2]))
    k1 = _t(np.concatenate([K1[:J1], K1])); k2 = _t(np.concatenate([K2[:J2], K2]))
    o1 = (J1 + np.r_[0, np.cumsum(c1)]).astype(np.int64); o2 = (J2 + np.r_[0, np.cumsum(c2)]).astype(np.int64)
    K = len(c1); pr = np.ascontiguousarray(LIST, np.int32); KL = len(pr)
    mp = _mp(norm, D1.shape[1], key, True); prm = matcher.estimator_params("F", max_iters=2000); gp = _lib.GuideParams(0, 0, 1e9)
    dev = a.device; s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    new = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device=dev)                                       # noqa: E731
    want_b = np.concatenate([_stated(sc, key) for sc in scs])                                                          # image p against image p
    want_l = np.concatenate([_stated(scs[j], key) for _, j in LIST])
    n_kept = len(dr.KEPT[key])
    # the ragged batch: per-query outputs live at the queries' own (absolute) rows
    seeds = new((max(K, KL),), torch.int32, 7); M = new((KL, 9), torch.float64, 0); st = new((KL, 16), torch.int32, 0)
    match = new((J1 + N1,), torch.int32, -7); inl = new((J1 + N1,), torch.uint8, 9); cnt = np.zeros(KL, np.int32)
    _lib.check(L.mi_degensac_match_verify_batch_dev(0, C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), o2.ctypes.data_as(lp),
                                                    k1.data_ptr(), k2.data_ptr(), 2, K, C.byref(prm), seeds.data_ptr(), 0, s, M.data_ptr(),
                                                    match.data_ptr(), inl.data_ptr(), st.data_ptr(), cnt.ctypes.data_as(ip)))
    m = match.cpu().numpy()
    assert np.array_equal(m[J1:], want_b) and (m[:J1] == -7).all() and list(cnt[:K]) == [n_kept] * K
    assert not inl.cpu().numpy()[J1:].any() and (inl.cpu().numpy()[:J1] == 9).all() and not M.cpu().numpy().any()
    # the pair list: outputs from row 0, pair after pair
    po = np.r_[0, np.cumsum(np.asarray(c1)[pr[:, 0]])]; n = int(po[-1])
    match = new((n,), torch.int32, -7); inl = new((n,), torch.uint8, 9)
    _lib.check(L.mi_degensac_match_verify_pairs_dev(0, C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), K, o2.ctypes.data_as(lp), K,
                                                    k1.data_ptr(), k2.data_ptr(), 2, pr.ctypes.data_as(ip), KL, C.byref(prm), seeds.data_ptr(), 0, s,
                                                    M.data_ptr(), match.data_ptr(), inl.data_ptr(), st.data_ptr(), cnt.ctypes.data_as(ip)))
    assert np.array_equal(match.cpu().numpy(), want_l) and list(cnt) == [n_kept] * KL and not inl.cpu().numpy().any()
    # guided, both layouts (every row passes the gate; both forms of the rule agree on this scene)
    Ms = _t(np.tile(F_ANY.ravel(), (KL, 1)))
    idx = new((J1 + N1, 2), torch.int32, -7); dist = new((J1 + N1, 2), torch.float32, -7.0); match = new((J1 + N1,), torch.int32, -7)
    _lib.check_match(L.mi_degensac_match_guided_batch_dev(C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), o2.ctypes.data_as(lp),
                                                          k1.data_ptr(), k2.data_ptr(), 2, K, Ms.data_ptr(), C.byref(gp), 0, s, idx.data_ptr(),
                                                          dist.data_ptr(), match.data_ptr(), None, cnt.ctypes.data_as(ip)))
    m = match.cpu().numpy()
    assert np.array_equal(m[J1:], want_b) and (m[:J1] == -7).all() and (idx.cpu().numpy()[:J1] == -7).all() and list(cnt[:K]) == [n_kept] * K
    idx = new((n, 2), torch.int32, -7); dist = new((n, 2), torch.float32, -7.0); match = new((n,), torch.int32, -7)
    _lib.check_match(L.mi_degensac_match_guided_pairs_dev(C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), K, o2.ctypes.data_as(lp), K,
                                                          pr.ctypes.data_as(ip), KL, k1.data_ptr(), k2.data_ptr(), 2, Ms.data_ptr(), C.byref(gp), 0, s,
                                                          idx.data_ptr(), dist.data_ptr(), match.data_ptr(), None, cnt.ctypes.data_as(ip)))
    assert np.array_equal(match.cpu().numpy(), want_l) and list(cnt) == [n_kept] * KL
    # and the restatement on the device's own 2-NN outputs says the same
    (e1,), (e2,), ec1, ec2, _ = pairs_ref.expand((D1,), c1, (D2,), c2, LIST)
    assert np.array_equal(_restated(e1, e2, ec1, ec2, norm, *key), want_l)
    assert np.array_equal(_restated(e1, e2, ec1, ec2, norm, *key, guided=True), want_l)


# ---- the estimator half of the pair-list families -----------------------------------------------------------------------------------------
H_BUDGET = dict(vr.BUDGET["H"], laf_consistensy_coef=-1.0)               # the stores hold [n, 2] keypoints: no frames for H
EST_LIST = [(1, 1), (0, 0), (2, 2), (0, 1), (3, 3), (1, 0)]
EST_SEEDS = [301, 302, 303, 304, 305, 306]


def _est_stores():
    """four images per store from designed pairs of verify_ref (image i of store 1 = the queries, of store 2 = the train rows of pair i):
    two eligible pairs, a short one, one with a single train row"""
    scs = [vr.designed_pair("F", 64, np.arange(1, 64, 2), seed=61), vr.designed_pair("F", 70, np.arange(0, 70, 3), seed=62),
           vr.designed_pair("F", 40, [1, 9, 20, 33, 39], seed=63), vr.designed_pair("F", 30, [], train="one", seed=64)]
    cat = lambda k: np.concatenate([s[k] for s in scs])                                                               # noqa: E731
    return scs, cat("k1"), cat("k2"), cat("d1"), cat("d2"), [s["n1"] for s in scs], [s["n2"] for s in scs]


def _ref_entry(port, model, scs, i, j, seed, key):
    """the restatement of list entry (i, j) under a rule; H on [n, 2] rows under H_BUDGET"""
    a, b = scs[i], scs[j]
    if model == "F":
        return dr.pair_ref(port, "F", a["k1"], b["k2"], a["d1"], b["d2"], seed, *key, "l2")
    q, t = dr.tentatives(a["d1"], b["d2"], *key, "l2")
    est = None
    if len(q) >= 4:
        M, mask, stt = port.find_homography(a["k1"][q], b["k2"][t], H_BUDGET["px_th"], H_BUDGET["conf"], H_BUDGET["max_iters"], 2, True, 0.0, seed=seed)
        M = np.asarray(M, float)
        est = (np.linalg.inv(M.T), mask, (stt["samples"], stt["lo_runs"], stt["I"])) if np.abs(M).sum() != 0 else \
            (M, np.zeros(len(q), bool), (stt["samples"], stt["lo_runs"], stt["I"]))
    return vr.result("H", a["n1"], q, t, est)


def _entries(M, match, inl, st, cnt, po):
    M, match, inl, st = (x.cpu().numpy() for x in (M, match, inl, st))
    return [dict(model=M[p], match=match[po[p]:po[p + 1]], inlier=inl[po[p]:po[p + 1]], cnt=int(cnt[p]), counters=tuple(int(c) for c in st[p, CTR]))
            for p in range(len(cnt))]


@pytest.mark.parametrize("key", [(0.9, "ratio", None), (0.9, True, 0.0), (None, True, 0.0)], ids=repr)
def test_estimator_half_of_the_pair_list_fginn_list_and_fh_calls(oracle_port, key):
    scs, K1, K2, D1, D2, c1, c2 = _est_stores()
    ratio, mutual, md = key
    T = [_t(K1), _t(K2), _t(D1), _t(D2)]
    kw = dict(ratio=ratio, mutual=mutual, max_dist=md, seeds=EST_SEEDS)
    want_f = [_ref_entry(oracle_port, "F", scs, i, j, EST_SEEDS[p], key) for p, (i, j) in enumerate(EST_LIST)]
    want_h = [_ref_entry(oracle_port, "H", scs, i, j, EST_SEEDS[p], key) for p, (i, j) in enumerate(EST_LIST)]
    assert sum(w["cnt"] >= 8 for w in want_f) >= 2 and any(w["cnt"] < 4 for w in want_f)      # eligible and short entries in one list
    r = tensor_api.match_and_verify_pairs_tensors(*T, c1, c2, EST_LIST, **kw, **vr.BUDGET["F"])
    for p, got in enumerate(_entries(*r)):
        assert not vr.disagreements(got, want_f[p]), ("pairs", p, vr.disagreements(got, want_f[p]))
    fh = tensor_api.match_and_verify_fh_pairs_tensors(*T, c1, c2, EST_LIST, **kw, f_params=vr.BUDGET["F"], h_params=H_BUDGET)
    F, H, match, inf, inh, stf, sth, summ, cnt, po = fh
    for p, got in enumerate(_entries(F, match, inf, stf, cnt, po)):
        assert not vr.disagreements(got, want_f[p]), ("fh F", p, vr.disagreements(got, want_f[p]))
    for p, got in enumerate(_entries(H, match, inh, sth, cnt, po)):
        assert not vr.disagreements(got, want_h[p]), ("fh H", p, vr.disagreements(got, want_h[p]))
    want_s = [[w["cnt"], w["inlier"].sum(), h["inlier"].sum(), (w["inlier"] & h["inlier"]).sum()] for w, h in zip(want_f, want_h)]
    assert np.array_equal(summ.cpu().numpy(), np.asarray(want_s, np.int32))
    # the F+H batch call on the entries' copied rows
    (e_k1, e_d1), (e_k2, e_d2), ec1, ec2, _ = pairs_ref.expand((K1, D1), c1, (K2, D2), c2, EST_LIST)
    fb = tensor_api.match_and_verify_fh_batch_tensors(_t(e_k1), _t(e_k2), _t(e_d1), _t(e_d2), ec1, ec2, **kw, f_params=vr.BUDGET["F"], h_params=H_BUDGET)
    assert _same(fb[:9], fh[:9], stats=(5, 6))
    if mutual != "ratio" and ratio is not None:                          # the FGINN list: radius 0 is the plain second neighbour
        f = tensor_api.match_and_verify_fginn_pairs_tensors(*T, c1, c2, EST_LIST, 0.0, **kw, **vr.BUDGET["F"])
        for p, got in enumerate(_entries(*f)):
            assert not vr.disagreements(got, want_f[p]), ("fginn pairs", p)


def test_pair_list_families_are_unchanged_at_decide_0_and_under_a_max_dist_above_every_d0():
    scs, K1, K2, D1, D2, c1, c2 = _est_stores()
    T = [_t(K1), _t(K2), _t(D1), _t(D2)]
    base = dict(ratio=0.9, mutual=True, seeds=EST_SEEDS)
    for md in (1e30, 40.0):
        a = tensor_api.match_and_verify_pairs_tensors(*T, c1, c2, EST_LIST, **base, **vr.BUDGET["F"])
        b = tensor_api.match_and_verify_pairs_tensors(*T, c1, c2, EST_LIST, **base, max_dist=md, **vr.BUDGET["F"])
        assert _same(a, b) and a[0].abs().sum() > 0
        a = tensor_api.match_and_verify_fginn_pairs_tensors(*T, c1, c2, EST_LIST, 10.0, **base, **vr.BUDGET["F"])
        b = tensor_api.match_and_verify_fginn_pairs_tensors(*T, c1, c2, EST_LIST, 10.0, **base, max_dist=md, **vr.BUDGET["F"])
        assert _same(a, b)
        a = tensor_api.match_and_verify_fh_pairs_tensors(*T, c1, c2, EST_LIST, **base, f_params=vr.BUDGET["F"], h_params=H_BUDGET)
        b = tensor_api.match_and_verify_fh_pairs_tensors(*T, c1, c2, EST_LIST, **base, max_dist=md, f_params=vr.BUDGET["F"], h_params=H_BUDGET)
        assert _same(a, b, stats=(5, 6))
        Ms = a[0]
        for fg in (None, 10.0):
            ga = tensor_api.guided_match_pairs_tensors(*T, c1, c2, EST_LIST, Ms, ratio=0.9, mutual=True, fginn_th=fg)
            gb = tensor_api.guided_match_pairs_tensors(*T, c1, c2, EST_LIST, Ms, ratio=0.9, mutual=True, fginn_th=fg, max_dist=md)
            assert _same(ga, gb, stats=()) and (ga[0] >= 0).any()


# ---- FGINN inside the gate under max_dist -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", vr.NORMS)
def test_guided_batch_with_fginn_th_under_max_dist(norm):
    sc = dr.scene(norm); n1, n2 = sc["n1"], sc["n2"]
    args = (_t(_kp(n1, 4)), _t(_kp(n2, 5)), _t(sc["d1"]), _t(sc["d2"]), [n1], [n2], _t(F_ANY[None]))
    for mutual in (False, True):
        # radius 0: slot 1 is the plain second gated row, the decision is decide_guided on the plain 2-NN
        g = tensor_api.guided_match_batch_tensors(*args, px_th=1e9, ratio=dr.RATIO, mutual=mutual, fginn_th=0.0, max_dist=1.0, norm=norm)
        want = _restated(sc["d1"], sc["d2"], [n1], [n2], norm, dr.RATIO, mutual, 1.0, guided=True)
        assert np.array_equal(g[0].cpu().numpy(), want)
        if not mutual:
            assert np.array_equal(want, _stated(sc, (dr.RATIO, False, 1.0)))
        # a radius nothing reaches: slot 1 is empty, the guided ratio test passes, and max_dist alone decides (with mutual: the mutual check too)
        g = tensor_api.guided_match_batch_tensors(*args, px_th=1e9, ratio=dr.RATIO, mutual=mutual, fginn_th=1e9, max_dist=1.0, norm=norm)
        rows = dr.KEPT[(None, True, 1.0)] if mutual else [0, 1, 3, 4, 5, 7, 8, 9]          # every query at d0 <= 1
        assert list(np.flatnonzero(g[0].cpu().numpy() >= 0)) == rows and (g[2].cpu().numpy()[:, 1] == np.inf).all()
        assert np.array_equal(g[0].cpu().numpy()[rows], sc["train_of"][rows])


# ---- no model, no inliers: the contract of the call as it was -------------------------------------------------------------------------
def test_a_pair_without_a_model_has_no_inliers_in_the_existing_call(oracle_port):
    """8 tentatives of the plain ratio test whose train keypoints are one point: the estimator runs and finds no model.  The call returns a
    zero model and NO inliers, whatever mask the estimator left; tests/decide_ref.pair_ref states the same for the rules."""
    sc = vr.designed_pair("F", 40, [1, 5, 9, 20, 21, 30, 33, 39], seed=77)
    k2 = sc["k2"].copy(); k2[sc["train_of"][sc["kept"][False]]] = [100.0, 200.0]
    r = tensor_api.match_and_verify_batch_tensors(_t(sc["k1"]), _t(k2), _t(sc["d1"]), _t(sc["d2"]), [sc["n1"]], [sc["n2"]], ratio=0.9, seeds=[5],
                                                  **vr.BUDGET["F"])
    assert int(r[4][0]) == 8 and int(r[3][0, 0]) > 0                      # eligible, and estimated
    assert not r[0].cpu().numpy().any() and not r[2].cpu().numpy().any()
    want = dr.pair_ref(oracle_port, "F", sc["k1"], k2, sc["d1"], sc["d2"], 5, 0.9, False, None, "l2")
    assert not want["model"].any() and not want["inlier"].any() and want["counters"] == tuple(int(c) for c in r[3].cpu().numpy()[0, CTR])
