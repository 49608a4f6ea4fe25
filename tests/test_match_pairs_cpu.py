"""The pair-list calls without a device: exhaustive_pairs, the reference expansion of tests/pairs_ref.py (and the numpy oracle per pair
against the same oracle on the expansion, which pins the helper itself), every ValueError of the argument check, and the refusals of
the C-ABI, which come before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher
from tests import pairs_ref as pr

EINVAL = -1
# a self pair, a repeated pair, (i, j) with (j, i), descending order; image 2 is empty, image 4 is unused
COUNTS = [5, 3, 0, 7, 4]
PAIRS = [(3, 1), (1, 3), (0, 0), (3, 1), (2, 0), (0, 2), (1, 0)]


# ---- exhaustive_pairs ----
@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_exhaustive_pairs(n):
    u = matcher.exhaustive_pairs(n); o = matcher.exhaustive_pairs(n, ordered=True)
    assert u.shape == (n * (n - 1) // 2, 2) and o.shape == (n * (n - 1), 2)
    assert np.issubdtype(u.dtype, np.integer) and np.issubdtype(o.dtype, np.integer)
    assert [tuple(r) for r in u] == [(i, j) for i in range(n) for j in range(n) if i < j]
    assert [tuple(r) for r in o] == [(i, j) for i in range(n) for j in range(n) if i != j]


def test_exhaustive_pairs_refuses_a_negative_count():
    with pytest.raises(ValueError):
        matcher.exhaustive_pairs(-1)


# ---- the expansion ----
def _store(counts, dim=8, seed=0, width=2):
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    return rng.normal(size=(n, dim)).astype(np.float32), rng.uniform(0, 100, (n, width))


def test_expansion_and_pair_offsets():
    d, k = _store(COUNTS)
    tag = np.repeat(np.arange(len(COUNTS)), COUNTS)                       # the image of every store row
    (e1, k1, t1), (e2, k2, t2), c1, c2, po = pr.expand((d, k, tag), COUNTS, (d, k, tag), COUNTS, PAIRS)
    assert list(c1) == [COUNTS[i] for i, _ in PAIRS] and list(c2) == [COUNTS[j] for _, j in PAIRS]
    assert list(po) == [0, 7, 10, 15, 22, 22, 27, 30] and po.dtype == np.int64
    o = pr.offsets(COUNTS); o2 = pr.offsets(c2)
    for p, (i, j) in enumerate(PAIRS):
        assert (t1[po[p]:po[p + 1]] == i).all() and (t2[o2[p]:o2[p + 1]] == j).all()
        assert np.array_equal(e1[po[p]:po[p + 1]], d[o[i]:o[i + 1]]) and np.array_equal(k1[po[p]:po[p + 1]], k[o[i]:o[i + 1]])
        assert np.array_equal(e2[o2[p]:o2[p + 1]], d[o[j]:o[j + 1]]) and np.array_equal(k2[o2[p]:o2[p + 1]], k[o[j]:o[j + 1]])
    # the checker returns the same offsets
    got = matcher.check_match_pairs_args("F", 0.9, None, d.shape, d.dtype, d.shape, d.dtype, k.shape, k.dtype, k.shape, k.dtype, COUNTS, COUNTS, PAIRS)
    assert np.array_equal(got[5], po) and got[5].dtype == np.int64 and got[4].dtype == np.int32 and got[4].tolist() == [list(x) for x in PAIRS]


def test_expansion_of_two_stores_and_of_an_empty_list():
    d1, k1 = _store([2, 0, 3], seed=1); d2, k2 = _store([4, 1], seed=2)
    (e1,), (e2,), c1, c2, po = pr.expand((d1,), [2, 0, 3], (d2,), [4, 1], [(2, 1), (1, 0), (0, 0)])
    assert list(c1) == [3, 0, 2] and list(c2) == [1, 4, 4] and list(po) == [0, 3, 3, 5]
    assert np.array_equal(e1, d1[[2, 3, 4, 0, 1]]) and np.array_equal(e2, d2[[4, 0, 1, 2, 3, 0, 1, 2, 3]])
    (e1,), (e2,), c1, c2, po = pr.expand((d1,), [2, 0, 3], (d2,), [4, 1], np.zeros((0, 2), np.int64))
    assert e1.shape == (0, 8) and e2.shape == (0, 8) and len(c1) == 0 and list(po) == [0]


@pytest.mark.parametrize("norm", ["l2", "hamming"])
@pytest.mark.parametrize("mutual", [False, True])
def test_oracle_per_pair_equals_oracle_on_the_expansion(norm, mutual):
    """pins the reference helper: the numpy matcher on image i against image j, taken straight from the stores, is the numpy matcher on
    pair p of the expansion"""
    rng = np.random.default_rng(3)
    n = int(np.sum(COUNTS))
    d = rng.normal(size=(n, 8)).astype(np.float32) if norm == "l2" else rng.integers(0, 256, (n, 8), dtype=np.uint8)
    o = pr.offsets(COUNTS)
    d[o[1]:o[1] + 3] = d[o[3]:o[3] + 3]                                  # images 1 and 3 share rows: true matches, both directions
    (e1,), (e2,), c1, c2, po = pr.expand((d,), COUNTS, (d,), COUNTS, PAIRS)
    o2 = pr.offsets(c2)
    kept = 0
    for p, (i, j) in enumerate(PAIRS):
        a, b = d[o[i]:o[i + 1]], d[o[j]:o[j + 1]]
        ea, eb = e1[po[p]:po[p + 1]], e2[o2[p]:o2[p + 1]]
        for got, want in zip(mo.knn2(a, b, norm), mo.knn2(ea, eb, norm)):
            assert np.array_equal(got, want), p
        if len(b) == 0:                                                   # (the oracle's mutual check indexes the reverse search's rows)
            assert (mo.knn2(a, b, norm)[0] == -1).all()
            continue
        for got, want in zip(mo.match_snn(a, b, 0.9, mutual, norm), mo.match_snn(ea, eb, 0.9, mutual, norm)):
            assert np.array_equal(got, want), p
        kept += len(mo.match_snn(a, b, 0.9, mutual, norm)[0])
    assert kept > 0


# ---- the argument check ----
def _args(**kw):
    d, k = _store(COUNTS)
    a = dict(model="F", ratio=0.9, norm=None, d1_shape=d.shape, d1_dtype=d.dtype, d2_shape=d.shape, d2_dtype=d.dtype, k1_shape=k.shape,
             k1_dtype=k.dtype, k2_shape=k.shape, k2_dtype=k.dtype, counts1=COUNTS, counts2=COUNTS, pairs=PAIRS)
    a.update(kw)
    return a


def test_check_accepts_the_list_and_two_stores_of_different_size():
    code, kind, o1, o2, p, po, sd = matcher.check_match_pairs_args(**_args(seeds=list(range(len(PAIRS)))))
    assert code == matcher.NORM_L2 and kind == "xy" and list(o1) == [0, 5, 8, 8, 15, 19] and sd.dtype == np.uint32 and list(sd) == list(range(7))
    got = matcher.check_match_pairs_args(**_args(d2_shape=(6, 8), k2_shape=(6, 2), counts2=[6], pairs=[(4, 0), (0, 0)]))
    assert list(got[3]) == [0, 6] and list(got[5]) == [0, 4, 9] and got[6] is None


@pytest.mark.parametrize("bad", [
    dict(pairs=[0, 1]), dict(pairs=[(0, 1, 2)]), dict(pairs=np.zeros((2, 2, 2), np.int64)), dict(pairs=np.zeros((3, 2))),       # shape, dtype
    dict(pairs=[(0.0, 1.0)]), dict(pairs=np.zeros((0, 2), np.int64)),                                                        # float, K = 0
    dict(pairs=[(0, 1), (-1, 0)]), dict(pairs=[(0, -1)]), dict(pairs=[(5, 0)]), dict(pairs=[(0, 5)]),                       # -1, M
    dict(d2_shape=(6, 8), k2_shape=(6, 2), counts2=[6], pairs=[(0, 1)]),                                                     # M2 = 1
    dict(guided=True), dict(fginn_th=10.0), dict(fginn_th=0.0),
    dict(seeds=[1, 2, 3]), dict(seeds=[[1] * 7]), dict(seeds=list(range(8))),
    dict(counts1=[5, 3, 0, 7, 5]), dict(counts2=[19.0]), dict(counts1=[-1, 20]), dict(counts1=[[19]]),
    dict(model="E"), dict(ratio=0.0), dict(d2_dtype=np.uint8), dict(k2_shape=(18, 2)), dict(k1_shape=(19, 3), k2_shape=(19, 3)),
], ids=repr)
def test_check_refuses(bad):
    with pytest.raises(ValueError):
        matcher.check_match_pairs_args(**_args(**bad))


def test_numpy_entry_point_checks_before_the_device():
    d, k = _store(COUNTS)
    o = pr.offsets(COUNTS)
    dl = [d[o[i]:o[i + 1]] for i in range(5)]; kl = [k[o[i]:o[i + 1]] for i in range(5)]
    for kw in (dict(pairs=[(0, 5)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, 1)], guided=True), dict(pairs=[(0, 1)], fginn_th=5.0),
               dict(pairs=[(0, 1)], seeds=[1, 2]), dict(pairs=[(0, 1)], desc2_list=dl), dict(pairs=[(0, 1)], kps2_list=kl[:2], desc2_list=dl),
               dict(pairs=[(0, 2)], kps2_list=kl[:2], desc2_list=dl[:2])):
        pairs = kw.pop("pairs")
        with pytest.raises(ValueError):
            matcher.match_and_verify_pairs(kl, dl, pairs, **kw)
    with pytest.raises(ValueError):
        matcher.match_and_verify_pairs([], [], [(0, 0)])


def test_tensor_form_checks_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d = torch.zeros((19, 8)); k = torch.zeros((19, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="image index"):
        tensor_api.knn_match_pairs_tensors(d, d, COUNTS, COUNTS, [(0, 5)])
    with pytest.raises(ValueError, match="pairs"):
        tensor_api.knn_match_pairs_tensors(d, d, COUNTS, COUNTS, [0, 1])
    with pytest.raises(ValueError, match="guided"):
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, guided=True)
    with pytest.raises(ValueError, match="fginn_th"):
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, fginn_th=10.0)
    with pytest.raises(ValueError, match="seed"):
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS, seeds=[1])
    with pytest.raises(ValueError):                             # valid arguments, but not on a ROCm device
        tensor_api.match_and_verify_pairs_tensors(k, k, d, d, COUNTS, COUNTS, PAIRS)


# ---- the C-ABI: refusals before a device is looked for ----
def _abi(pairs=((0, 1),), off1=(0, 4, 10), off2=(0, 3, 7), n_pairs=None, mp=None, m1=None, m2=None):
    """(rc of knn2_pairs_dev, of verify_pairs_dev, of verify_pairs) with null data pointers"""
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64); pr_ = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    K = len(pr_) if n_pairs is None else n_pairs
    m1 = len(o1) - 1 if m1 is None else m1; m2 = len(o2) - 1 if m2 is None else m2
    mp = mp or _lib.MatchParams(0, 8, 0.9, True)
    prm = _lib.make_params(0.5, 0.99, 1000, 0, True, 0.0)
    out = []
    out.append(L.mi_degensac_match_knn2_pairs_dev(mp.norm, None, None, o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2, pr_.ctypes.data_as(ip), K,
                                                  mp.dim, 0, None, None, None))
    msg = [L.mi_degensac_match_last_error()]
    out.append(L.mi_degensac_match_verify_pairs_dev(0, C.byref(mp), None, None, o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2, None, None, 2,
                                                    pr_.ctypes.data_as(ip), K, C.byref(prm), None, 0, None, None, None, None, None, None))
    msg.append(L.mi_degensac_last_error())
    out.append(L.mi_degensac_match_verify_pairs(1, C.byref(mp), None, None, o1.ctypes.data_as(lp), m1, o2.ctypes.data_as(lp), m2, None, None, 2,
                                                pr_.ctypes.data_as(ip), K, C.byref(prm), None, 0, None, None, None, None, None))
    msg.append(L.mi_degensac_last_error())
    return tuple(out), msg


@pytest.mark.parametrize("case", [
    dict(pairs=[(0, 2)]), dict(pairs=[(2, 0)]), dict(pairs=[(0, 1), (-1, 0)]), dict(pairs=[(0, -1)]), dict(pairs=[(0, 0)], m1=0),   # index out of range
    dict(n_pairs=-1),
    dict(off1=(0, 6, 4)), dict(off2=(-1, 3, 7)),
    # rows beyond the limit, from offsets alone: each store is within it, twice the image is not (output rows; back rows)
    dict(off1=(0, 0x3fffffff), off2=(0, 1), pairs=[(0, 0), (0, 0)]),
    dict(off1=(0, 1), off2=(0, 0x3fffffff), pairs=[(0, 0), (0, 0)]),
    dict(off1=(5, 0x20000005), off2=(0, 1), pairs=[(0, 0)] * 3),
], ids=repr)
def test_abi_refuses_bad_lists(case):
    rcs, msg = _abi(**case)
    assert rcs == (EINVAL, EINVAL, EINVAL)
    assert all(msg)


def test_abi_null_data_pointers_are_refused_not_read():
    """a valid layout with null descriptor / output pointers is EINVAL before a device is looked for"""
    rcs, msg = _abi()
    assert rcs == (EINVAL, EINVAL, EINVAL) and all(b"NULL" in m for m in msg)


def test_abi_refuses_fginn():
    rcs, msg = _abi(mp=_lib.MatchParams(0, 8, 0.9, False, fginn_th=10.0))
    assert rcs[1:] == (EINVAL, EINVAL) and all(b"FGINN" in m for m in msg[1:])
    rcs, msg = _abi(mp=_lib.MatchParams(0, 8, 0.9, False, fginn_th=0.0), n_pairs=0)
    assert rcs[1:] == (EINVAL, EINVAL)
    mp = _lib.MatchParams(0, 8, 0.9, False, fginn_th=10.0); mp.struct_size = 0       # the layout before spatial_th: the plain rule, no refusal
    rcs, msg = _abi(mp=mp, n_pairs=0)
    assert rcs == (0, 0, 0)


@pytest.mark.parametrize("mp", [_lib.MatchParams(2, 8, 0.9, False), _lib.MatchParams(4, 260, 0.9, False), _lib.MatchParams(1, 6, 0.9, False),
                                _lib.MatchParams(0, 0, 0.9, False)], ids=lambda m: f"norm{m.norm}-dim{m.dim}")
def test_abi_refuses_bad_norms(mp):
    assert _abi(mp=mp)[0] == (EINVAL, EINVAL, EINVAL)


def test_abi_empty_list_returns_zero():
    assert _abi(pairs=np.zeros((0, 2), np.int32), n_pairs=0)[0] == (0, 0, 0)
    assert _abi(pairs=[(9, 9)], n_pairs=0, off1=(0,), off2=(0,))[0] == (0, 0, 0)          # nothing is looked at
