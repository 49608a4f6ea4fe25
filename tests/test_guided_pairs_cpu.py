"""Guided matching over a pair list without a device (matcher.guided_match_pairs, tensor_api.guided_match_pairs_tensors,
include/mi_degensac.h mi_degensac_match_guided_*_pairs*): every ValueError of the argument checks, the refusals of the three C entry
points, which come before a device is looked for, and what "pair list" means for this stage: the restatement of tests/guided_ref.py per
list entry on store slices equals the same restatement on the expansion of tests/pairs_ref.py."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import guided_ref as gr, pairs_ref as pr

EINVAL = -1
# a self pair, a repeated pair, (i, j) with (j, i), descending order; image 2 is empty, image 4 is unused
COUNTS = [5, 3, 0, 7, 4]
PAIRS = [(3, 1), (1, 3), (0, 0), (3, 1), (2, 0), (0, 2), (1, 0)]
K = len(PAIRS)
I3 = np.tile(np.eye(3), (K, 1, 1))


def _lists(counts=COUNTS, dim=8, desc=np.float32, kp_w=2, kp=np.float64, seed=0):
    rng = np.random.default_rng(seed)
    dl = [rng.normal(size=(n, dim)).astype(desc) for n in counts]
    kl = [rng.uniform(0, 100, (n, kp_w)).astype(kp) for n in counts]
    return kl, dl


def _call(pairs=PAIRS, models=I3, lists=None, **kw):
    kl, dl = lists or _lists()
    return matcher.guided_match_pairs(kl, dl, pairs, models, **kw)


# ---- the numpy entry point: refusals before any device ----
@pytest.mark.parametrize("shape", [(K - 1, 3, 3), (K + 1, 3, 3), (K, 9), (K, 3, 4), (K,), (3, 3)])
def test_models_of_the_wrong_k_or_shape(shape):
    with pytest.raises(ValueError, match="models"):
        _call(models=np.zeros(shape))


@pytest.mark.parametrize("dt", [np.float32, np.int64, np.complex128])
def test_models_must_be_float64(dt):
    with pytest.raises(ValueError, match="models"):
        _call(models=I3.astype(dt))


@pytest.mark.parametrize("px_th", [-0.5, -1e-300, float("nan"), "x"])
def test_px_th_must_be_a_non_negative_number(px_th):
    with pytest.raises(ValueError, match="px_th"):
        _call(px_th=px_th)


@pytest.mark.parametrize("model,error_type", [("F", "symm_max"), ("F", "symm_sq_sum"), ("H", "symm_epipolar"), ("F", "nope"), ("H", "")])
def test_error_type_of_the_model_kind(model, error_type):
    with pytest.raises(ValueError, match="Error type"):
        _call(model=model, error_type=error_type)


def _check_args(**kw):
    """check_match_pairs_args on the shapes of the store of _lists()"""
    a = dict(model="F", ratio=0.9, norm=None, d1_shape=(19, 8), d1_dtype=np.float32, d2_shape=(19, 8), d2_dtype=np.float32, k1_shape=(19, 2),
             k1_dtype=np.float64, k2_shape=(19, 2), k2_dtype=np.float64, counts1=COUNTS, counts2=COUNTS, pairs=PAIRS)
    a.update(kw)
    return a


# every list defect that check_match_pairs_args refuses (the cases of tests/test_match_pairs_cpu.py that concern the list and the stores)
LIST_DEFECTS = [
    dict(pairs=[0, 1]), dict(pairs=[(0, 1, 2)]), dict(pairs=np.zeros((2, 2, 2), np.int64)), dict(pairs=np.zeros((3, 2))),
    dict(pairs=[(0.0, 1.0)]), dict(pairs=np.zeros((0, 2), np.int64)),
    dict(pairs=[(0, 1), (-1, 0)]), dict(pairs=[(0, -1)]), dict(pairs=[(5, 0)]), dict(pairs=[(0, 5)]),
]


@pytest.mark.parametrize("bad", LIST_DEFECTS, ids=repr)
def test_list_defects_are_refused_by_the_shared_check_and_by_the_call(bad):
    with pytest.raises(ValueError):
        matcher.check_match_pairs_args(**_check_args(**bad))
    prs = np.asarray(bad["pairs"])
    n = prs.shape[0] if prs.ndim >= 1 else 0
    with pytest.raises(ValueError, match="pair"):
        _call(pairs=bad["pairs"], models=np.tile(np.eye(3), (n, 1, 1)))


def test_the_list_is_checked_before_the_models():
    """a list defect and a models defect together: the list's message comes first, so `models` is judged against a valid K"""
    with pytest.raises(ValueError, match="image index"):
        _call(pairs=[(0, 5)], models=np.zeros((2, 3, 3)))


def test_second_store_goes_together_and_is_indexed_by_the_second_column():
    kl, dl = _lists()
    with pytest.raises(ValueError, match="go together"):
        matcher.guided_match_pairs(kl, dl, [(0, 1)], I3[:1], kps2_list=kl)
    with pytest.raises(ValueError, match="go together"):
        matcher.guided_match_pairs(kl, dl, [(0, 1)], I3[:1], desc2_list=dl)
    with pytest.raises(ValueError, match="one keypoint array"):
        matcher.guided_match_pairs(kl, dl, [(0, 1)], I3[:1], kps2_list=kl[:2], desc2_list=dl)
    with pytest.raises(ValueError, match="image index"):                # store 2 has two images
        matcher.guided_match_pairs(kl, dl, [(0, 2)], I3[:1], kps2_list=kl[:2], desc2_list=dl[:2])
    with pytest.raises(ValueError, match="at least one image"):
        matcher.guided_match_pairs([], [], [(0, 0)], I3[:1])


def test_other_argument_defects():
    with pytest.raises(ValueError, match="model"):
        _call(model="E")
    for r in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ratio"):
            _call(ratio=r)
    with pytest.raises(ValueError, match="descriptors"):
        _call(lists=_lists(desc=np.float64))
    with pytest.raises(ValueError, match="keypoints"):
        _call(lists=_lists(kp_w=3))
    kl, dl = _lists()
    kl[1] = kl[1][:-1]
    with pytest.raises(ValueError, match="keypoint row"):
        _call(lists=(kl, dl))


def test_match_and_verify_pairs_still_refuses_guided_and_names_the_new_call():
    kl, dl = _lists()
    with pytest.raises(ValueError, match="guided_match_pairs"):
        matcher.match_and_verify_pairs(kl, dl, PAIRS, guided=True)
    with pytest.raises(ValueError, match="guided"):
        matcher.check_match_pairs_args(**_check_args(guided=True))
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.match_and_verify_pairs(kl, dl, PAIRS, fginn_th=5.0)


def test_tensor_form_checks_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d = torch.zeros((19, 8)); k = torch.zeros((19, 2), dtype=torch.float64)
    M = torch.zeros((K, 3, 3), dtype=torch.float64)
    call = tensor_api.guided_match_pairs_tensors
    with pytest.raises(ValueError, match="image index"):
        call(k, k, d, d, COUNTS, COUNTS, [(0, 5)], M[:1])
    with pytest.raises(ValueError, match="pairs"):
        call(k, k, d, d, COUNTS, COUNTS, [0, 1], M)
    with pytest.raises(ValueError, match="counts"):
        call(k, k, d, d, [5, 3, 0, 7, 5], COUNTS, PAIRS, M)
    with pytest.raises(ValueError, match="models"):
        call(k, k, d, d, COUNTS, COUNTS, PAIRS, M[:-1])
    with pytest.raises(ValueError, match="models"):
        call(k, k, d, d, COUNTS, COUNTS, PAIRS, M.float())
    with pytest.raises(ValueError, match="models"):
        call(k, k, d, d, COUNTS, COUNTS, PAIRS, M.reshape(K, 9))
    with pytest.raises(ValueError, match="px_th"):
        call(k, k, d, d, COUNTS, COUNTS, PAIRS, M, px_th=float("nan"))
    with pytest.raises(ValueError, match="Error type"):
        call(k, k, d, d, COUNTS, COUNTS, PAIRS, M, model="H", error_type="symm_epipolar")
    with pytest.raises(ValueError, match="keypoints"):
        call(k.float(), k, d, d, COUNTS, COUNTS, PAIRS, M)
    with pytest.raises(ValueError):                             # valid arguments, but not on a ROCm device
        call(k, k, d, d, COUNTS, COUNTS, PAIRS, M)
    with pytest.raises(ValueError):
        call(k, k, d, d, COUNTS, COUNTS, PAIRS, np.zeros((K, 3, 3)))


# ---- the C-ABI: refusals before a device is looked for ----
def _abi(pairs=((0, 1),), off1=(0, 4, 10), off2=(0, 3, 7), n_pairs=None, mp=None, gp=None, kp_dim=2, m1=None, m2=None, data=None):
    """(rc of guided_knn2_pairs_dev, of guided_pairs_dev, of guided_pairs) and their messages; data pointers are null unless `data` is
    given: then every data pointer but the one it names holds an address.  An entry point that does not take the named pointer would see
    no null pointer at all and go on to a device, so it is not called (rc None)."""
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64); pr_ = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    n = len(pr_) if n_pairs is None else n_pairs
    m1 = len(o1) - 1 if m1 is None else m1; m2 = len(o2) - 1 if m2 is None else m2
    mp = mp or _lib.MatchParams(0, 8, 0.9, True)
    gp = gp or _lib.GuideParams(0, 0, 0.5)
    P = dict.fromkeys(("desc1", "desc2", "kp1", "kp2", "models", "idx", "dist", "match"), None)
    if data is not None:
        buf = np.zeros(64); addr = buf.ctypes.data
        P = {k: (None if k == data else addr) for k in P}
    fp = C.POINTER(C.c_float); dp = C.POINTER(C.c_double)

    def c(x, t):
        return C.cast(x, t) if x is not None else None
    out = []; msg = []
    if data == "match":
        out.append(None); msg.append(b"")
    else:
        out.append(L.mi_degensac_match_guided_knn2_pairs_dev(mp.norm, P["desc1"], P["desc2"], o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2,
                                                             pr_.ctypes.data_as(ip), n, mp.dim, P["kp1"], P["kp2"], kp_dim, P["models"], C.byref(gp),
                                                             0, None, P["idx"], P["dist"]))
        msg.append(L.mi_degensac_match_last_error())
    out.append(L.mi_degensac_match_guided_pairs_dev(C.byref(mp), P["desc1"], P["desc2"], o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2,
                                                    pr_.ctypes.data_as(ip), n, P["kp1"], P["kp2"], kp_dim, P["models"], C.byref(gp), 0, None,
                                                    P["idx"], P["dist"], P["match"], None, None))
    msg.append(L.mi_degensac_match_last_error())
    out.append(L.mi_degensac_match_guided_pairs(C.byref(mp), P["desc1"], P["desc2"], o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2,
                                                pr_.ctypes.data_as(ip), n, c(P["kp1"], dp), c(P["kp2"], dp), kp_dim, c(P["models"], dp),
                                                C.byref(gp), 0, c(P["idx"], ip), c(P["dist"], fp), c(P["match"], ip), None))
    msg.append(L.mi_degensac_match_last_error())
    return tuple(out), msg


@pytest.mark.parametrize("case", [
    dict(pairs=[(0, 2)]), dict(pairs=[(2, 0)]), dict(pairs=[(0, 1), (-1, 0)]), dict(pairs=[(0, -1)]), dict(pairs=[(0, 0)], m1=0),   # index out of range
    dict(n_pairs=-1),
    dict(off1=(0, 6, 4)), dict(off2=(0, 8, 7)), dict(off2=(-1, 3, 7)), dict(off1=(-2, 4, 10)),
    # rows beyond the limit, from offsets alone: each store is within it, twice the image is not (output rows; back rows)
    dict(off1=(0, 0x3fffffff), off2=(0, 1), pairs=[(0, 0), (0, 0)]),
    dict(off1=(0, 1), off2=(0, 0x3fffffff), pairs=[(0, 0), (0, 0)]),
    dict(off1=(5, 0x20000005), off2=(0, 1), pairs=[(0, 0)] * 3),
], ids=repr)
def test_abi_refuses_bad_lists(case):
    rcs, msg = _abi(**case)
    assert rcs == (EINVAL, EINVAL, EINVAL)
    assert all(msg)


@pytest.mark.parametrize("mp", [_lib.MatchParams(2, 8, 0.9, False), _lib.MatchParams(4, 260, 0.9, False), _lib.MatchParams(1, 6, 0.9, False),
                                _lib.MatchParams(4, 6, 0.9, False), _lib.MatchParams(0, 0, 0.9, False), _lib.MatchParams(0, -8, 0.9, False)],
                         ids=lambda m: f"norm{m.norm}-dim{m.dim}")
def test_abi_refuses_bad_norms_and_dims(mp):
    assert _abi(mp=mp)[0] == (EINVAL, EINVAL, EINVAL)
    assert _abi(mp=mp, n_pairs=0)[0] == (EINVAL, EINVAL, EINVAL)       # the parameters are judged whatever the list holds


@pytest.mark.parametrize("case", [
    dict(kp_dim=3), dict(kp_dim=0),
    dict(gp=_lib.GuideParams(0, 2, 0.5)),                            # error_type 2 is an H kind
    dict(gp=_lib.GuideParams(1, 5, 0.5)), dict(gp=_lib.GuideParams(1, -1, 0.5)),
    dict(gp=_lib.GuideParams(0, 0, -0.1)), dict(gp=_lib.GuideParams(1, 2, float("nan"))),
], ids=repr)
def test_abi_refuses_bad_guide_params(case):
    assert _abi(**case)[0] == (EINVAL, EINVAL, EINVAL)
    assert _abi(n_pairs=0, **case)[0] == (EINVAL, EINVAL, EINVAL)


def test_abi_refuses_bad_struct_size_homography_flag_and_ratio():
    gp = _lib.GuideParams(0, 0, 0.5); gp.struct_size = 8
    assert _abi(gp=gp)[0] == (EINVAL, EINVAL, EINVAL)
    gp = _lib.GuideParams(0, 0, 0.5); gp.homography = 2
    assert _abi(gp=gp)[0] == (EINVAL, EINVAL, EINVAL)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        rcs, msg = _abi(mp=_lib.MatchParams(0, 8, r, False))
        assert rcs[1:] == (EINVAL, EINVAL) and all(b"ratio" in m for m in msg[1:]), r


def test_abi_null_pointers_on_a_valid_layout_are_refused_not_read():
    rcs, msg = _abi()
    assert rcs == (EINVAL, EINVAL, EINVAL) and all(b"NULL" in m for m in msg)
    for name in ("desc1", "desc2", "kp1", "kp2", "models", "idx", "dist"):
        rcs, msg = _abi(data=name)
        assert rcs == (EINVAL, EINVAL, EINVAL) and all(b"NULL" in m for m in msg), name
    rcs, msg = _abi(data="match")                                       # the 2-NN entry point has no match array
    assert rcs == (None, EINVAL, EINVAL) and all(b"NULL" in m for m in msg[1:])


def test_abi_second_nn_is_ignored():
    """the FGINN fields of match_params are not part of the guided calls: a valid layout with them set gets as far as the NULL check"""
    rcs, msg = _abi(mp=_lib.MatchParams(0, 8, 0.9, False, fginn_th=10.0))
    assert rcs == (EINVAL, EINVAL, EINVAL) and all(b"NULL" in m for m in msg)
    assert _abi(mp=_lib.MatchParams(0, 8, 0.9, False, fginn_th=10.0), n_pairs=0)[0] == (0, 0, 0)


def test_abi_empty_list_returns_zero():
    assert _abi(pairs=np.zeros((0, 2), np.int32), n_pairs=0)[0] == (0, 0, 0)
    assert _abi(pairs=[(9, 9)], n_pairs=0, off1=(0,), off2=(0,))[0] == (0, 0, 0)          # nothing is looked at
    assert _abi(pairs=[(9, 9)], n_pairs=0, off1=(7, 3), off2=(-1,))[0] == (0, 0, 0)


# ---- what "pair list" means for the guided stage ----
@pytest.mark.parametrize("model,et", gr.KINDS)
@pytest.mark.parametrize("mutual", [False, True])
def test_restatement_per_entry_equals_restatement_on_the_expansion(oracle_port, model, et, mutual):
    """tests/guided_ref.oracle on image i against image j under the ENTRY's model, taken straight from the stores, is the same oracle on
    entry p of the expansion; the repeated entry (3, 1) carries two different models and gives two different results"""
    rng = np.random.default_rng(3 + et)
    n = int(np.sum(COUNTS))
    d = rng.normal(size=(n, 8)).astype(np.float32)
    k = rng.uniform(0, 40, (n, 2))
    o = pr.offsets(COUNTS)
    d[o[1]:o[1] + 3] = d[o[3]:o[3] + 3]; k[o[1]:o[1] + 3] = k[o[3]:o[3] + 3]          # images 1 and 3 share rows: true matches
    M = np.stack([np.eye(3) if model == "H" else np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])] * K)
    M[3] = M[3] @ np.array([[1.0, 0, 6.0], [0, 1, 6.0], [0, 0, 1]])      # the repeat of (3, 1) under a shifted model
    M[5] = 0.0
    px = 5.0
    (e1, k1), (e2, k2), c1, c2, po = pr.expand((d, k), COUNTS, (d, k), COUNTS, PAIRS)
    o2 = pr.offsets(c2)
    res = []
    for p, (i, j) in enumerate(PAIRS):
        got = gr.oracle(oracle_port, model, et, px, M[p], k[o[i]:o[i + 1]], k[o[j]:o[j + 1]], d[o[i]:o[i + 1]], d[o[j]:o[j + 1]], "l2", 0.9, mutual)
        want = gr.oracle(oracle_port, model, et, px, M[p], k1[po[p]:po[p + 1]], k2[o2[p]:o2[p + 1]], e1[po[p]:po[p + 1]], e2[o2[p]:o2[p + 1]],
                         "l2", 0.9, mutual)
        for g, w in zip(got, want):
            assert g.shape[0] == COUNTS[i] and np.array_equal(g, w, equal_nan=True), p
        res.append(got)
    assert (res[0][2] >= 0).sum() >= 3                                   # the shared rows match under the identity / same-row model
    assert not np.array_equal(res[0][0], res[3][0])                      # the same (i, j), another model: another result
    assert (res[5][0] == -1).all() and (res[4][0].shape == (0, 2))       # the zero model; the empty query image
