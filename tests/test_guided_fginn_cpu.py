"""FGINN inside the gate of guided matching without a device: the restatement of tests/guided_fginn_ref.py judged on its own (r = 0 is the
plain guided restatement; the twin scenes and the keep rule; every slot-1 distance inside the float64 bound of tests/matcher_ref.py;
broken restatements told apart on the inputs the GPU tests use; the stated needy counts of those inputs), every refusal of the six C
entry points (before a device is looked for) and of the Python keywords."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import fginn_ref as fr, guided_fginn_ref as gf, guided_ref as gr, matcher_ref as mr

EINVAL = -1
R = 10.0
NEEDY = [0, 1, 15, 16, 17, 63, 64, 65]
FLUSH = ["exact64", "carry63", "excluded", "chunks", "tie_lo", "tie_hi"]


def _oracle(P, s, model, r=R, px=None, mutual=False, norm="l2", **kw):
    px = px if px is not None else (1.0 if model == "F" else 3.0)
    return gf.oracle(P, model, 0, px, s[4], s[0], s[1], s[2], s[3], norm, r, 0.9, mutual, **kw)


def _inputs():
    """(name, scene, model, px, norm) of the shared scenes"""
    out = [(k, gf.flush_scene(k), "F", 1.0, "l2") for k in FLUSH] + [("offband", gf.offband_scene(), "F", 1.0, "l2")]
    out += [("radius", gf.radius_scene(), "H", 1e100, "l2"), ("radius_below", gf.radius_scene(True), "H", 1e100, "l2")]
    for model, norm, width in (("H", "l2", 8), ("F", "l2", 8), ("H", "hamming", 32), ("F", "l2_u8", 32)):
        out += [(f"twin{n}", gf.twin_scene(5, n + 9, 90 + n, width, norm, n, model), model, 3.0, norm) for n in (0, 17, 65)]
    return out


# ---- the restatement ----
def test_radius_zero_is_the_plain_guided_restatement(oracle_port):
    for name, s, model, px, norm in _inputs():
        for mutual in (False, True):
            gi, gd, gm, gn = gf.oracle(oracle_port, model, 0, px, s[4], s[0], s[1], s[2], s[3], norm, 0.0, 0.9, mutual)
            d1, d2 = (s[2], s[3]) if norm != "l2_u8" else (s[2].astype(np.float32), s[3].astype(np.float32))
            wi, wd, wm = gr.oracle(oracle_port, model, 0, px, s[4], s[0], s[1], d1, d2, "hamming" if norm == "hamming" else "l2", 0.9, mutual)
            assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gm, wm), name
            assert not gn.any(), name


@pytest.mark.parametrize("model,norm,width", [("H", "l2", 8), ("F", "l2", 8), ("H", "hamming", 32), ("F", "l2_u8", 32)])
def test_stated_needy_counts_of_the_twin_scenes(oracle_port, model, norm, width):
    for n in NEEDY:
        for n1 in (n, n + 9):
            s = gf.twin_scene(4 if n1 == n else 5, n1, 90 + n, width, norm, n, model)
            idx, dist, match, needy = _oracle(oracle_port, s, model, px=3.0, norm=norm)
            assert int(needy.sum()) == n and needy[:n].all(), (n, n1)
            assert (match[:n] >= 0).all()


def test_stated_needy_counts_and_answers_of_the_edge_scenes(oracle_port):
    for n_q in (1, 17):
        for k in FLUSH:
            s = gf.flush_scene(k, n_q)
            idx, dist, match, needy = _oracle(oracle_port, s, "F")
            assert needy.all() and (idx[:, 0] == s[5]).all() and (idx[:, 1] == s[6]).all(), k
        s = gf.offband_scene(n_q)
        idx, dist, match, needy = _oracle(oracle_port, s, "F")
        assert needy.all() and (idx[:, 0] == 1).all() and (idx[:, 1] == 3).all()
    for below, r, want in ((False, 10.0, 2), (True, 10.0, 3), (False, np.nextafter(10.0, 11.0), 3), (True, np.nextafter(10.0, 0.0), 2)):
        idx, dist, match, needy = _oracle(oracle_port, gf.radius_scene(below), "H", r=float(r), px=1e100)
        assert needy.all() and (idx[:, 1] == want).all(), (below, r)


@pytest.mark.parametrize("model", ["F", "H"])
def test_twin_scene_plain_guided_drops_the_twinned_queries_and_the_new_rule_keeps_them(oracle_port, model):
    n_tw = 40
    s = gf.twin_scene(7, 150, 200, 32, "l2", n_tw, model)
    gi, gd, gm = gr.oracle(oracle_port, model, 0, 3.0, s[4], s[0], s[1], s[2], s[3], "l2", 0.9, False)
    idx, dist, match, needy = _oracle(oracle_port, s, model, px=3.0)
    assert (gm[:n_tw] == -1).all() and int((gm >= 0).sum()) == 150 - n_tw          # plain guided: exactly the twinned queries are lost
    assert int(needy.sum()) == n_tw and (match[:150] >= 0).all()
    assert int((match >= 0).sum()) - int((gm >= 0).sum()) == n_tw
    assert set(match[:n_tw] % 160) <= set(range(n_tw))                   # each to its own row or that row's twin (rows 160 ..)


def test_keep_rule_a_query_whose_only_companions_are_twins_is_kept(oracle_port):
    """under H nothing but the correct row and its twin is gated: slot 1 = -1 / inf, and the query is a match (the guided rule: nothing
    competes with it).  The unguided FGINN filter (fginn_ref.keep) would drop it."""
    s = gf.twin_scene(7, 30, 50, 8, "l2", 10, "H")
    idx, dist, match, needy = _oracle(oracle_port, s, "H", px=3.0)
    assert needy[:10].all() and (idx[:10, 0] >= 0).all() and (idx[:10, 1] == -1).all() and np.isposinf(dist[:10, 1]).all()
    assert (match[:10] == idx[:10, 0]).all()
    assert not fr.keep(idx, dist, 0.9)[:10].any()


def test_every_slot_1_distance_is_inside_the_float64_bound(oracle_port):
    seen = 0
    for name, s, model, px, norm in _inputs():
        if norm != "l2":
            continue
        idx, dist, match, needy = gf.oracle(oracle_port, model, 0, px, s[4], s[0], s[1], s[2], s[3], norm, R, 0.9, False)
        D = mr.dist64(s[2], s[3], "l2")
        g = mr.g_bound(s[2].shape[1])
        have = np.flatnonzero(idx[:, 1] >= 0)
        De = D[have, idx[have, 1]]
        assert (np.abs(dist[have, 1].astype(np.float64) - De) <= g * De).all(), name
        ok = gf.second_mask(gr.gate_matrix(oracle_port, model, 0, px, s[4], s[0], s[1]), idx[:, 0], s[1], R)
        best = np.where(ok, D, np.inf).min(axis=1) if ok.shape[1] else np.full(len(idx), np.inf)
        assert (De <= best[have] * (1 + g) / (1 - g)).all() and np.isinf(best[idx[:, 1] < 0]).all(), name
        seen += len(have)
    assert seen > 50


# ---- broken restatements are told apart on the shared inputs ----
def _ungated_anchor(D):
    def second(G, i0, k2, r):
        from oracle import matcher_np as mo
        return G & fr.ok_mask(mo.top2(D)[0][:, 0], k2, r)
    return second


def _anchor_competes(G, i0, k2, r):
    ok = gf.second_mask(G, i0, k2, r)
    q = np.flatnonzero(i0 >= 0)
    ok[q, i0[q]] = True
    return ok


def _greater_than(G, i0, k2, r):
    k2 = np.asarray(k2, np.float64); an = np.clip(i0, 0, None)
    dx = k2[None, :, 0] - k2[an, 0][:, None]; dy = k2[None, :, 1] - k2[an, 1][:, None]
    ok = G & (dx * dx + dy * dy > r * r) & (np.arange(len(k2))[None, :] != i0[:, None])
    ok[i0 < 0] = False
    return ok


def test_broken_restatements_are_rejected(oracle_port):
    s = gf.offband_scene()
    good = _oracle(oracle_port, s, "F")
    bad = _oracle(oracle_port, s, "F", second=_ungated_anchor(gf.dmat(s[2], s[3], "l2")))
    assert (good[0][:, 1] == 3).all() and (bad[0][:, 1] == 1).all()   # the exclusion against the ungated nearest row: the true anchor competes
    for k in FLUSH:
        s = gf.flush_scene(k)
        bad = _oracle(oracle_port, s, "F", second=_anchor_competes)
        assert (bad[0][:, 1] == s[5]).all() and (_oracle(oracle_port, s, "F")[0][:, 1] == s[6]).all(), k   # the anchor as its own competitor
    s = gf.radius_scene()
    assert (_oracle(oracle_port, s, "H", px=1e100)[0][:, 1] == 2).all()
    assert (_oracle(oracle_port, s, "H", px=1e100, second=_greater_than)[0][:, 1] == 3).all()               # > instead of >= at the radius
    s = gf.radius_scene(True)
    assert (_oracle(oracle_port, s, "H", px=1e100, second=_greater_than)[0][:, 1] == 3).all()


# ---- the C-ABI: refusals before a device is looked for ----
def _abi(layout, pairs=((0, 1),), off1=(0, 4, 10), off2=(0, 3, 7), n_pairs=None, mp=None, gp=None, kp_dim=2, r=R, data=None):
    """(rc, message) of guided_fginn_knn2_<layout>_dev, guided_fginn_<layout>_dev and guided_fginn_<layout>; every data pointer is null
    unless `data` names the one that stays null while the others hold an address"""
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32); fp = C.POINTER(C.c_float); dp = C.POINTER(C.c_double)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64); pr_ = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    mp = mp or _lib.MatchParams(0, 8, 0.9, True, r)
    gp = gp or _lib.GuideParams(0, 0, 0.5)
    P = dict.fromkeys(("desc1", "desc2", "kp1", "kp2", "models", "idx", "dist", "match"), None)
    if data is not None:
        buf = np.zeros(64); P = {k: (None if k == data else buf.ctypes.data) for k in P}

    def c(x, t):
        return C.cast(x, t) if x is not None else None
    if layout == "pairs":
        n = len(pr_) if n_pairs is None else n_pairs
        lay = (o1.ctypes.data_as(lp), len(o1) - 1, o2.ctypes.data_as(lp), len(o2) - 1, pr_.ctypes.data_as(ip), n)
        calls = [
            lambda: L.mi_degensac_match_guided_fginn_knn2_pairs_dev(mp.norm, P["desc1"], P["desc2"], *lay, mp.dim, P["kp1"], P["kp2"], kp_dim,
                                                                    P["models"], C.byref(gp), r, 0, None, P["idx"], P["dist"]),
            lambda: L.mi_degensac_match_guided_fginn_pairs_dev(C.byref(mp), P["desc1"], P["desc2"], *lay, P["kp1"], P["kp2"], kp_dim, P["models"],
                                                               C.byref(gp), 0, None, P["idx"], P["dist"], P["match"], None, None),
            lambda: L.mi_degensac_match_guided_fginn_pairs(C.byref(mp), P["desc1"], P["desc2"], *lay, c(P["kp1"], dp), c(P["kp2"], dp), kp_dim,
                                                           c(P["models"], dp), C.byref(gp), 0, c(P["idx"], ip), c(P["dist"], fp), c(P["match"], ip),
                                                           None)]
    else:
        n = len(o1) - 1 if n_pairs is None else n_pairs
        lay = (o1.ctypes.data_as(lp), o2.ctypes.data_as(lp))
        calls = [
            lambda: L.mi_degensac_match_guided_fginn_knn2_batch_dev(mp.norm, P["desc1"], P["desc2"], *lay, n, mp.dim, P["kp1"], P["kp2"], kp_dim,
                                                                    P["models"], C.byref(gp), r, 0, None, P["idx"], P["dist"]),
            lambda: L.mi_degensac_match_guided_fginn_batch_dev(C.byref(mp), P["desc1"], P["desc2"], *lay, P["kp1"], P["kp2"], kp_dim, n, P["models"],
                                                               C.byref(gp), 0, None, P["idx"], P["dist"], P["match"], None, None),
            lambda: L.mi_degensac_match_guided_fginn_batch(C.byref(mp), P["desc1"], P["desc2"], *lay, c(P["kp1"], dp), c(P["kp2"], dp), kp_dim, n,
                                                           c(P["models"], dp), C.byref(gp), 0, c(P["idx"], ip), c(P["dist"], fp), c(P["match"], ip),
                                                           None)]
    out, msg = [], []
    for k, f in enumerate(calls):
        if k == 0 and data == "match":                                   # the 2-NN form has no match array: it would go on to a device
            out.append(None); msg.append(b""); continue
        out.append(f()); msg.append(L.mi_degensac_match_last_error())
    return tuple(out), msg


LAYOUTS = ["batch", "pairs"]
ALL = (EINVAL, EINVAL, EINVAL)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("r", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
def test_abi_refuses_a_bad_radius(layout, r):
    for n_pairs in (None, 0):
        rcs, msg = _abi(layout, r=r, n_pairs=n_pairs)
        assert rcs == ALL and all(b"spatial_th" in m for m in msg), (n_pairs, msg)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_abi_refuses_a_bad_second_nn(layout):
    for v in (2, -1):
        mp = _lib.MatchParams(0, 8, 0.9, True, R); mp.second_nn = v
        rcs, msg = _abi(layout, mp=mp)
        assert rcs[1:] == (EINVAL, EINVAL) and all(b"second_nn" in m for m in msg[1:])
        assert _abi(layout, mp=mp, n_pairs=0)[0][1:] == (EINVAL, EINVAL)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", [
    dict(mp=_lib.MatchParams(2, 8, 0.9, False, R)), dict(mp=_lib.MatchParams(4, 260, 0.9, False, R)), dict(mp=_lib.MatchParams(1, 6, 0.9, False, R)),
    dict(mp=_lib.MatchParams(0, 0, 0.9, False, R)), dict(kp_dim=3), dict(kp_dim=0),
    dict(gp=_lib.GuideParams(0, 2, 0.5)), dict(gp=_lib.GuideParams(1, 5, 0.5)), dict(gp=_lib.GuideParams(0, 0, -0.1)),
    dict(gp=_lib.GuideParams(1, 2, float("nan"))),
], ids=lambda c: f"mp-norm{c['mp'].norm}-dim{c['mp'].dim}" if "mp" in c else repr(c))     # MatchParams' repr holds the object's address
def test_abi_keeps_the_refusals_of_the_plain_guided_calls_whatever_the_list_holds(layout, case):
    assert _abi(layout, **case)[0] == ALL
    assert _abi(layout, n_pairs=0, **case)[0] == ALL


@pytest.mark.parametrize("layout", LAYOUTS)
def test_abi_ratio_struct_size_and_list_defects(layout):
    for ratio in (0.0, -1.0, float("nan"), float("inf")):
        rcs, msg = _abi(layout, mp=_lib.MatchParams(0, 8, ratio, False, R))
        assert rcs[1:] == (EINVAL, EINVAL) and all(b"ratio" in m for m in msg[1:])
    gp = _lib.GuideParams(0, 0, 0.5); gp.struct_size = 8
    assert _abi(layout, gp=gp)[0] == ALL
    assert _abi(layout, n_pairs=-1)[0] == ALL
    for bad in (dict(off1=(0, 6, 4)), dict(off2=(0, 8, 7)), dict(off2=(-1, 3, 7))):
        assert _abi(layout, **bad)[0] == ALL, bad
    if layout == "pairs":
        for bad in ([(0, 2)], [(2, 0)], [(0, -1)]):
            assert _abi(layout, pairs=bad)[0] == ALL, bad
    # the plain refusals come first: a bad gate next to a bad radius is the gate's message; a bad ratio next to a bad second_nn the ratio's
    rcs, msg = _abi(layout, kp_dim=3, r=-1.0)
    assert rcs == ALL and all(b"keypoint" in m for m in msg)
    mp = _lib.MatchParams(0, 8, 0.0, False, R); mp.second_nn = 2
    assert all(b"ratio" in m for m in _abi(layout, mp=mp)[1][1:])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_abi_null_pointers_are_refused_and_an_empty_list_returns_zero(layout):
    rcs, msg = _abi(layout)
    assert rcs == ALL and all(b"NULL" in m for m in msg)
    for name in ("desc1", "desc2", "kp1", "kp2", "models", "idx", "dist"):
        rcs, msg = _abi(layout, data=name)
        assert rcs == ALL and all(b"NULL" in m for m in msg), name
    rcs, msg = _abi(layout, data="match")
    assert rcs == (None, EINVAL, EINVAL) and all(b"NULL" in m for m in msg[1:])
    assert _abi(layout, n_pairs=0)[0] == (0, 0, 0)
    assert _abi(layout, n_pairs=0, r=0.0)[0] == (0, 0, 0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_abi_short_struct_size_or_second_nn_zero_is_the_plain_call(layout):
    """a struct_size that does not cover spatial_th: second_nn and the radius are not read, whatever they hold (the layout from before the
    fields); second_nn = 0 leaves the radius unread too.  Both get as far as the NULL check, and an empty list returns 0."""
    for size in (0, _lib.MatchParams.spatial_th.offset, _lib.MatchParams.second_nn.offset):
        mp = _lib.MatchParams(0, 8, 0.9, True, R); mp.struct_size = size; mp.second_nn = 7; mp.spatial_th = float("nan")
        rcs, msg = _abi(layout, mp=mp, r=R)
        assert rcs == ALL and all(b"NULL" in m for m in msg), size
        assert _abi(layout, mp=mp, n_pairs=0)[0][1:] == (0, 0)
    mp = _lib.MatchParams(0, 8, 0.9, True, None); mp.spatial_th = -5.0
    assert all(b"NULL" in m for m in _abi(layout, mp=mp)[1][1:]) and _abi(layout, mp=mp, n_pairs=0)[0][1:] == (0, 0)


def test_the_plain_guided_entry_points_still_ignore_both_fields():
    L = _lib.lib()
    mp = _lib.MatchParams(0, 8, 0.9, True, R); mp.second_nn = 7; mp.spatial_th = float("nan")
    o = np.array([0, 4], np.int64); lp = C.POINTER(C.c_int64); gp = _lib.GuideParams(0, 0, 0.5)
    assert L.mi_degensac_match_guided_batch_dev(C.byref(mp), None, None, o.ctypes.data_as(lp), o.ctypes.data_as(lp), None, None, 2, 0, None,
                                                C.byref(gp), 0, None, None, None, None, None, None) == 0
    assert L.mi_degensac_match_guided_batch_dev(C.byref(mp), None, None, o.ctypes.data_as(lp), o.ctypes.data_as(lp), None, None, 2, 1, None,
                                                C.byref(gp), 0, None, None, None, None, None, None) == EINVAL
    assert b"NULL" in L.mi_degensac_match_last_error()


# ---- the Python keywords ----
COUNTS = [5, 3, 0, 7, 4]
PAIRS = [(3, 1), (1, 3), (0, 0)]
BAD_R = [-1.0, float("nan"), float("inf"), "x", [1.0, 2.0]]


def _lists(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 100, (n, 2)) for n in COUNTS], [rng.normal(size=(n, 8)).astype(np.float32) for n in COUNTS]


@pytest.mark.parametrize("r", BAD_R, ids=repr)
def test_numpy_calls_refuse_a_bad_fginn_th(r):
    kl, dl = _lists()
    I3 = np.tile(np.eye(3), (len(PAIRS), 1, 1))
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.guided_match_pairs(kl, dl, PAIRS, I3, fginn_th=r)
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.guided_match_batch([kl[0]], [kl[1]], [dl[0]], [dl[1]], I3[:1], fginn_th=r)
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.guided_match(kl[0], kl[1], dl[0], dl[1], np.eye(3), fginn_th=r)
    with pytest.raises(ValueError, match="guided_fginn_th"):
        matcher.match_and_verify_batch([kl[0]], [kl[1]], [dl[0]], [dl[1]], guided=True, guided_fginn_th=r)


def test_guided_fginn_th_needs_guided_and_the_pair_list_calls_keep_refusing_guided():
    kl, dl = _lists()
    with pytest.raises(ValueError, match="guided=True"):
        matcher.match_and_verify_batch([kl[0]], [kl[1]], [dl[0]], [dl[1]], guided_fginn_th=R)
    with pytest.raises(ValueError, match="guided=True"):
        matcher.match_and_verify_batch([kl[0]], [kl[1]], [dl[0]], [dl[1]], guided=False, fginn_th=R, guided_fginn_th=R)
    with pytest.raises(ValueError, match="guided_match_pairs"):
        matcher.match_and_verify_pairs(kl, dl, PAIRS, guided=True)
    with pytest.raises(ValueError, match="guided_match_pairs"):
        matcher.match_and_verify_fginn_pairs(kl, dl, PAIRS, R, guided=True)
    with pytest.raises(TypeError):
        matcher.match_and_verify_pairs(kl, dl, PAIRS, guided_fginn_th=R)
    assert matcher.check_guided_fginn_th(False, None) is None and matcher.check_guided_fginn_th(True, None) is None
    assert matcher.check_guided_fginn_th(True, 0) == 0.0 and matcher.check_guided_fginn_th(True, 7) == 7.0


def test_the_other_refusals_come_first():
    kl, dl = _lists()
    with pytest.raises(ValueError, match="models"):
        matcher.guided_match_pairs(kl, dl, PAIRS, np.zeros((2, 3, 3)), fginn_th=-1.0)
    with pytest.raises(ValueError, match="px_th"):
        matcher.guided_match(kl[0], kl[1], dl[0], dl[1], np.eye(3), px_th=-1.0, fginn_th=-1.0)


def test_tensor_calls_check_the_keywords_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    n = int(np.sum(COUNTS))
    d = torch.zeros((n, 8)); k = torch.zeros((n, 2), dtype=torch.float64)
    M = torch.zeros((len(PAIRS), 3, 3), dtype=torch.float64)
    for r in BAD_R:
        with pytest.raises(ValueError, match="fginn_th"):
            tensor_api.guided_match_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, M, fginn_th=r)
        with pytest.raises(ValueError, match="fginn_th"):
            tensor_api.guided_match_batch_tensors(k, k, d, d, COUNTS, COUNTS, torch.zeros((5, 3, 3), dtype=torch.float64), fginn_th=r)
        with pytest.raises(ValueError, match="guided_fginn_th"):
            tensor_api.match_and_verify_batch_tensors(k, k, d, d, COUNTS, COUNTS, guided=True, guided_fginn_th=r)
    with pytest.raises(ValueError, match="guided=True"):
        tensor_api.match_and_verify_batch_tensors(k, k, d, d, COUNTS, COUNTS, guided_fginn_th=R)
    with pytest.raises(ValueError, match="guided"):
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, guided=True)
    with pytest.raises(TypeError):
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, guided_fginn_th=R)
    with pytest.raises(ValueError, match="device"):                     # good keywords, but not on a ROCm device
        tensor_api.guided_match_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, M, fginn_th=R)
