"""FGINN over a pair list without a device (tensor_api.knn_match_fginn_pairs_tensors, match_and_verify_fginn_pairs_tensors,
matcher.match_and_verify_fginn_pairs, include/mi_degensac.h mi_degensac_match_fginn_knn2_pairs_dev and
mi_degensac_match_verify_fginn_pairs[_dev]): every ValueError of the Python calls, every EINVAL of the C entry points (all come before a
device is looked for), the refusals the plain pair-list calls keep, and what "pair list" means for this stage: the restatement of
tests/fginn_ref.py per list entry on store slices equals the same restatement on the expansion of tests/pairs_ref.py."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import fginn_ref as fr, pairs_ref as pr

EINVAL = -1
COUNTS = [5, 3, 0, 7, 4]
PAIRS = [(3, 1), (1, 3), (0, 0), (3, 1), (2, 0), (0, 2), (1, 0)]
K = len(PAIRS)
BAD_TH = [-1.0, -1e-300, float("nan"), float("inf"), -float("inf")]


def _lists(counts=COUNTS, dim=8, desc=np.float32, kp_w=2, kp=np.float64, seed=0):
    rng = np.random.default_rng(seed)
    dl = [rng.normal(size=(n, dim)).astype(desc) for n in counts]
    kl = [rng.uniform(0, 100, (n, kp_w)).astype(kp) for n in counts]
    return kl, dl


def _call(pairs=PAIRS, fginn_th=10.0, lists=None, **kw):
    kl, dl = lists or _lists()
    return matcher.match_and_verify_fginn_pairs(kl, dl, pairs, fginn_th, **kw)


# ---- the numpy entry point ----
@pytest.mark.parametrize("th", BAD_TH + ["x", None])
def test_fginn_th_must_be_a_finite_non_negative_number(th):
    with pytest.raises(ValueError, match="fginn_th"):
        _call(fginn_th=th)


def test_fginn_th_is_required():
    kl, dl = _lists()
    with pytest.raises(TypeError):
        matcher.match_and_verify_fginn_pairs(kl, dl, PAIRS)


@pytest.mark.parametrize("pairs", [[0, 1], [(0, 1, 2)], np.zeros((3, 2)), np.zeros((0, 2), np.int64), [(0, 1), (-1, 0)], [(0, -1)], [(5, 0)], [(0, 5)]],
                         ids=repr)
def test_list_defects(pairs):
    with pytest.raises(ValueError, match="pair"):
        _call(pairs=pairs)


def test_guided_is_refused_and_names_the_call_that_takes_the_models():
    with pytest.raises(ValueError, match="guided_match_pairs"):
        _call(guided=True)


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
    with pytest.raises(ValueError, match="seed"):
        _call(seeds=[1, 2])
    kl, dl = _lists()
    with pytest.raises(ValueError, match="go together"):
        matcher.match_and_verify_fginn_pairs(kl, dl, [(0, 1)], 5.0, kps2_list=kl)
    with pytest.raises(ValueError, match="image index"):                # store 2 has two images
        matcher.match_and_verify_fginn_pairs(kl, dl, [(0, 2)], 5.0, kps2_list=kl[:2], desc2_list=dl[:2])
    kl[1] = kl[1][:-1]
    with pytest.raises(ValueError, match="keypoint row"):
        _call(lists=(kl, dl))


def test_the_plain_pair_list_calls_still_refuse_fginn_and_guided():
    kl, dl = _lists()
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.match_and_verify_pairs(kl, dl, PAIRS, fginn_th=5.0)
    with pytest.raises(ValueError, match="guided"):
        matcher.match_and_verify_pairs(kl, dl, PAIRS, guided=True)
    a = dict(model="F", ratio=0.9, norm=None, d1_shape=(19, 8), d1_dtype=np.float32, d2_shape=(19, 8), d2_dtype=np.float32, k1_shape=(19, 2),
             k1_dtype=np.float64, k2_shape=(19, 2), k2_dtype=np.float64, counts1=COUNTS, counts2=COUNTS, pairs=PAIRS)
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.check_match_pairs_args(**a, fginn_th=5.0)


# ---- the tensor entry points ----
def test_tensor_forms_check_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d = torch.zeros((19, 8)); k = torch.zeros((19, 2), dtype=torch.float64)
    knn = tensor_api.knn_match_fginn_pairs_tensors
    for th in BAD_TH + ["x"]:
        with pytest.raises(ValueError, match="spatial_th"):
            knn(d, d, k, COUNTS, COUNTS, PAIRS, th)
    with pytest.raises(ValueError, match="image index"):
        knn(d, d, k, COUNTS, COUNTS, [(0, 5)])
    with pytest.raises(ValueError, match="image index"):
        knn(d, d, k, COUNTS, COUNTS, [(-1, 0)])
    with pytest.raises(ValueError, match="pairs"):
        knn(d, d, k, COUNTS, COUNTS, [0, 1])
    with pytest.raises(ValueError, match="counts"):
        knn(d, d, k, [5, 3, 0, 7, 5], COUNTS, PAIRS)
    for bad in (k.float(), torch.zeros((19, 3), dtype=torch.float64), torch.zeros((19, 4), dtype=torch.float64), torch.zeros(19, dtype=torch.float64)):
        with pytest.raises(ValueError, match="keypoints"):
            knn(d, d, bad, COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="keypoint row"):
        knn(d, d, k[:-1], COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="tensors"):
        knn(d, d, k.numpy(), COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError):                              # valid arguments, but not on a ROCm device
        knn(d, d, k, COUNTS, COUNTS, PAIRS)
    mv = tensor_api.match_and_verify_fginn_pairs_tensors
    for th in BAD_TH + ["x", None]:
        with pytest.raises(ValueError, match="fginn_th"):
            mv(k, k, d, d, COUNTS, COUNTS, PAIRS, th)
    with pytest.raises(TypeError):
        mv(k, k, d, d, COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="guided_match_pairs"):
        mv(k, k, d, d, COUNTS, COUNTS, PAIRS, 5.0, guided=True)
    with pytest.raises(ValueError, match="image index"):
        mv(k, k, d, d, COUNTS, COUNTS, [(0, 5)], 5.0)
    with pytest.raises(ValueError, match="seed"):
        mv(k, k, d, d, COUNTS, COUNTS, PAIRS, 5.0, seeds=[1])
    with pytest.raises(ValueError):                              # valid arguments, but not on a ROCm device
        mv(k, k, d, d, COUNTS, COUNTS, PAIRS, 5.0)
    # the plain call keeps its refusals
    with pytest.raises(ValueError, match="fginn_th"):
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, fginn_th=5.0)
    with pytest.raises(ValueError, match="guided"):
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, guided=True)


# ---- the C-ABI: refusals before a device is looked for ----
def _abi(pairs=((0, 1),), off1=(0, 4, 10), off2=(0, 3, 7), n_pairs=None, mp=None, kp_dim=2, th=10.0, m1=None, m2=None, data=None, homography=0):
    """(rc of fginn_knn2_pairs_dev, of verify_fginn_pairs_dev, of verify_fginn_pairs) and their messages.  th is the radius of the first and,
    unless mp is given, of the other two.  Data pointers are null unless `data` names one: then every data pointer but that one holds an
    address; an entry point that does not take the named pointer is not called (rc None)."""
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64); pr_ = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    n = len(pr_) if n_pairs is None else n_pairs
    m1 = len(o1) - 1 if m1 is None else m1; m2 = len(o2) - 1 if m2 is None else m2
    mp = mp or _lib.MatchParams(0, 8, 0.9, True, th)
    prm = matcher.estimator_params("H" if homography else "F")
    names = ("desc1", "desc2", "kp1", "kp2", "idx", "dist", "seeds", "model", "match", "inlier")
    P = dict.fromkeys(names, None)
    if data is not None:
        buf = np.zeros(64); addr = buf.ctypes.data
        P = {k: (None if k == data else addr) for k in P}

    def c(x, t):
        return C.cast(x, C.POINTER(t)) if x is not None else None
    out = []; msg = []
    if data in ("kp1", "seeds", "model", "match", "inlier"):
        out.append(None); msg.append(b"")
    else:
        out.append(L.mi_degensac_match_fginn_knn2_pairs_dev(mp.norm, P["desc1"], P["desc2"], o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2,
                                                            pr_.ctypes.data_as(ip), n, mp.dim, P["kp2"], kp_dim, th, 0, None, P["idx"], P["dist"]))
        msg.append(L.mi_degensac_match_last_error())
    if data in ("idx", "dist"):
        out += [None, None]; msg += [b"", b""]
        return tuple(out), msg
    out.append(L.mi_degensac_match_verify_fginn_pairs_dev(homography, C.byref(mp), P["desc1"], P["desc2"], o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp),
                                                          m2, P["kp1"], P["kp2"], kp_dim, pr_.ctypes.data_as(ip), n, C.byref(prm), P["seeds"], 0, None,
                                                          P["model"], P["match"], P["inlier"], None, None))
    msg.append(L.mi_degensac_last_error())
    out.append(L.mi_degensac_match_verify_fginn_pairs(homography, C.byref(mp), P["desc1"], P["desc2"], o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2,
                                                      c(P["kp1"], C.c_double), c(P["kp2"], C.c_double), kp_dim, pr_.ctypes.data_as(ip), n, C.byref(prm),
                                                      c(P["seeds"], C.c_uint32), 0, c(P["model"], C.c_double), c(P["match"], C.c_int32),
                                                      c(P["inlier"], C.c_uint8), None, None))
    msg.append(L.mi_degensac_last_error())
    return tuple(out), msg


ALL = (EINVAL, EINVAL, EINVAL)


@pytest.mark.parametrize("case", [
    dict(pairs=[(0, 2)]), dict(pairs=[(2, 0)]), dict(pairs=[(0, 1), (-1, 0)]), dict(pairs=[(0, -1)]), dict(pairs=[(0, 0)], m1=0),   # index out of range
    dict(n_pairs=-1),
    dict(off1=(0, 6, 4)), dict(off2=(0, 8, 7)), dict(off2=(-1, 3, 7)), dict(off1=(-2, 4, 10)),                                       # offsets
    dict(off1=(0, 0x3fffffff), off2=(0, 1), pairs=[(0, 0), (0, 0)]), dict(off1=(0, 1), off2=(0, 0x3fffffff), pairs=[(0, 0), (0, 0)]),   # the row limit
], ids=repr)
def test_abi_refuses_bad_lists(case):
    rcs, msg = _abi(**case)
    assert rcs == ALL and all(msg)


@pytest.mark.parametrize("th", BAD_TH)
def test_abi_refuses_a_bad_radius_whatever_the_list_holds(th):
    for kw in (dict(), dict(n_pairs=0), dict(pairs=[(0, 9)])):
        rcs, msg = _abi(th=th, **kw)
        assert rcs == ALL and all(b"spatial_th" in m for m in msg), (th, kw)


@pytest.mark.parametrize("kp_dim", [0, 1, 3, 4, 5, 7, -2])
def test_abi_refuses_keypoint_rows_that_are_not_2_or_6_wide(kp_dim):
    assert _abi(kp_dim=kp_dim)[0] == ALL
    assert _abi(kp_dim=kp_dim, n_pairs=0)[0] == ALL


@pytest.mark.parametrize("mp", [_lib.MatchParams(2, 8, 0.9, False, 5.0), _lib.MatchParams(4, 260, 0.9, False, 5.0), _lib.MatchParams(1, 6, 0.9, False, 5.0),
                                _lib.MatchParams(4, 6, 0.9, False, 5.0), _lib.MatchParams(0, 0, 0.9, False, 5.0), _lib.MatchParams(0, -8, 0.9, False, 5.0)],
                         ids=lambda m: f"norm{m.norm}-dim{m.dim}")
def test_abi_refuses_bad_norms_and_dims(mp):
    assert _abi(mp=mp)[0] == ALL
    assert _abi(mp=mp, n_pairs=0)[0] == ALL


def test_abi_refuses_a_bad_ratio_second_nn_and_homography_flag():
    for r in (0.0, -1.0, float("nan"), float("inf")):
        rcs, msg = _abi(mp=_lib.MatchParams(0, 8, r, False, 5.0))
        assert rcs[1:] == (EINVAL, EINVAL) and all(b"ratio" in m for m in msg[1:]), r
    mp = _lib.MatchParams(0, 8, 0.9, False, 5.0); mp.second_nn = 2
    rcs, msg = _abi(mp=mp)
    assert rcs[1:] == (EINVAL, EINVAL) and all(b"second_nn" in m for m in msg[1:])
    assert _abi(homography=2)[0][1:] == (EINVAL, EINVAL)


def test_abi_null_data_with_rows_present_is_refused_not_read():
    rcs, msg = _abi()
    assert rcs == ALL and all(b"NULL" in m for m in msg)
    for name in ("desc1", "desc2", "kp2"):
        rcs, msg = _abi(data=name)
        assert rcs == ALL and all(b"NULL" in m for m in msg), name
    for name in ("idx", "dist"):
        rcs, msg = _abi(data=name)
        assert rcs == (EINVAL, None, None) and b"NULL" in msg[0], name
    for name in ("kp1", "seeds", "model", "match", "inlier"):
        rcs, msg = _abi(data=name)
        assert rcs == (None, EINVAL, EINVAL) and all(b"NULL" in m for m in msg[1:]), name


def test_abi_empty_list_returns_zero():
    assert _abi(pairs=np.zeros((0, 2), np.int32), n_pairs=0)[0] == (0, 0, 0)
    assert _abi(pairs=[(9, 9)], n_pairs=0, off1=(0,), off2=(0,))[0] == (0, 0, 0)          # nothing is looked at
    assert _abi(pairs=[(9, 9)], n_pairs=0, off1=(7, 3), off2=(-1,))[0] == (0, 0, 0)


def test_abi_plain_rule_for_second_nn_0_and_for_the_layout_before_spatial_th():
    """with second_nn = 0, or a struct_size that does not cover spatial_th, the fginn match-and-verify calls are the plain pair-list calls:
    a spatial_th that would be refused is not looked at, and the call gets as far as the NULL check, as the plain calls do"""
    L = _lib.lib()
    for size in (None, 0, 24):
        mp = _lib.MatchParams(0, 8, 0.9, False, None)
        mp.spatial_th = float("nan")
        if size is not None:
            mp.struct_size = size; mp.second_nn = 1
        rcs, msg = _abi(mp=mp)
        assert rcs[1:] == (EINVAL, EINVAL) and all(b"NULL" in m for m in msg[1:]), size
        assert _abi(mp=mp, n_pairs=0)[0][1:] == (0, 0)
    # ... while the plain entry points keep refusing second_nn = 1, with their message
    mp = _lib.MatchParams(0, 8, 0.9, False, 5.0)
    lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    o1 = np.array([0, 4, 10], np.int64); o2 = np.array([0, 3, 7], np.int64); pr_ = np.array([[0, 1]], np.int32)
    prm = matcher.estimator_params("F")
    rc = L.mi_degensac_match_verify_pairs_dev(0, C.byref(mp), None, None, o1.ctypes.data_as(lp), 2, o2.ctypes.data_as(lp), 2, None, None, 2,
                                              pr_.ctypes.data_as(ip), 1, C.byref(prm), None, 0, None, None, None, None, None, None)
    assert rc == EINVAL and b"FGINN" in L.mi_degensac_last_error() and b"not part of the pair-list entry points" in L.mi_degensac_last_error()
    rc = L.mi_degensac_match_verify_pairs(0, C.byref(mp), None, None, o1.ctypes.data_as(lp), 2, o2.ctypes.data_as(lp), 2, None, None, 2,
                                          pr_.ctypes.data_as(ip), 1, C.byref(prm), None, 0, None, None, None, None, None)
    assert rc == EINVAL and b"FGINN" in L.mi_degensac_last_error()


# ---- what "pair list" means for this stage ----
def _stores_of_the_gpu_file(norm):
    """the stores and lists of tests/test_gpu_fginn_pairs.py that come from fginn_ref.twin_scene alone"""
    w = 33 if norm == "l2" else 36
    scenes = [fr.twin_scene(20 + i, 130, 200, w, norm, m) for i, m in enumerate([0, 1, 63, 64, 65])]
    two = ([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes])
    yield two, [(s, s) for s in (3, 4, 0, 2, 1)] + [(0, 4), (4, 2)]
    D, Kp = [], []
    for k, (a, b, kp2) in enumerate(scenes):
        g = np.arange(len(a)) + 37 * (k + 1)
        D += [a, b]; Kp += [np.c_[100.0 * (g % 37), 100.0 * (g // 37)], kp2]
    yield (D, D, Kp), [(2 * s, 2 * s + 1) for s in (4, 2, 0, 3, 1, 0)] + [(9, 9), (1, 0)]


@pytest.mark.parametrize("norm", fr.NORMS)
def test_restatement_per_entry_equals_restatement_on_the_expansion(norm):
    """fginn_ref.fginn on image i against image j with image j's keypoints, taken straight from the stores, is the same restatement on
    entry p of the expansion: idx, dist bits, the needy set and keep"""
    total = 0
    for (D1, D2, K2), pairs in _stores_of_the_gpu_file(norm):
        c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
        (e1,), (e2, ek2), k1, k2, po = pr.expand((np.concatenate(D1),), c1, (np.concatenate(D2), np.concatenate(K2)), c2, pairs)
        o2 = pr.offsets(k2)
        for p, (i, j) in enumerate(pairs):
            got = fr.fginn(D1[i], D2[j], K2[j], 10.0, norm)
            want = fr.fginn(e1[po[p]:po[p + 1]], e2[o2[p]:o2[p + 1]], ek2[o2[p]:o2[p + 1]], 10.0, norm)
            assert got[0].shape == (c1[i], 2)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), p
            assert np.array_equal(got[2], want[2]) and np.array_equal(fr.keep(got[0], got[1], 0.9), fr.keep(want[0], want[1], 0.9)), p
            total += int(got[2].sum())
    assert total >= 2 * (1 + 63 + 64 + 65)
