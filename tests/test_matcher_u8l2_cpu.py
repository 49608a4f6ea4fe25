"""The uint8 L2 norm (norm "l2_u8", MI_DEGENSAC_NORM_L2_U8 = 4) without a device: the Python argument checks, the C-ABI refusals
(all before the library looks for a device), and the claim the GPU tests rest on — for dim <= 256 the exact integer distance
(tests/matcher_u8_ref.py) and the float32 oracle (oracle/matcher_np.py) on the cast rows agree bit for bit, ties included, while two
deliberately wrong restatements do not."""
import ctypes as C

import numpy as np
import pytest

from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher
from tests import matcher_u8_ref as ur

EINVAL = -1


def _args(dim=128, dt=np.uint8, n1=10, n2=7):
    return ((n1, dim), np.dtype(dt), (n2, dim), np.dtype(dt), (n1, 2), np.float64, (n2, 2), np.float64, [4, n1 - 4], [3, n2 - 3])


# ---- Python checks -------------------------------------------------------------------------------------------------------------
def test_checker_accepts_uint8_rows():
    code, kind, o1, o2 = matcher.check_match_verify_args("F", 0.9, "l2_u8", *_args())
    assert code == matcher.NORM_L2_U8 == 4 and kind == "xy"
    assert list(o1) == [0, 4, 10] and list(o2) == [0, 3, 7]
    assert matcher.check_match_verify_args("H", 0.9, "l2_u8", *_args(dim=256))[0] == 4


def test_checker_refuses_float_rows_and_wide_rows():
    with pytest.raises(ValueError, match="l2_u8"):
        matcher.check_match_verify_args("F", 0.9, "l2_u8", *_args(dt=np.float32))
    with pytest.raises(ValueError, match="256"):
        matcher.check_match_verify_args("F", 0.9, "l2_u8", *_args(dim=257))
    with pytest.raises(ValueError, match="256"):
        matcher.check_match_verify_args("F", 0.9, "l2_u8", *_args(dim=260))


def test_existing_rules_stay():
    assert matcher.check_match_verify_args("F", 0.9, None, *_args())[0] == matcher.NORM_HAMMING         # uint8 without a norm: Hamming
    assert matcher.check_match_verify_args("F", 0.9, None, *_args(dt=np.float32))[0] == matcher.NORM_L2
    with pytest.raises(ValueError, match="L2"):
        matcher.check_match_verify_args("F", 0.9, "l2", *_args())
    with pytest.raises(ValueError, match="norm"):
        matcher.check_match_verify_args("F", 0.9, "l2_u16", *_args())
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)
    code, x, y = matcher._prep(a, a, None)
    assert code == matcher.NORM_HAMMING and x.dtype == np.uint8
    code, x, y = matcher._prep(a, a, "l2")
    assert code == matcher.NORM_L2 and x.dtype == np.float32 and np.array_equal(x, a)


@pytest.mark.parametrize("dim", [5, 6, 7])
def test_prep_pads_to_whole_words(dim):
    rng = np.random.default_rng(dim)
    a = rng.integers(0, 256, (9, dim), dtype=np.uint8); b = rng.integers(0, 256, (4, dim), dtype=np.uint8)
    code, x, y = matcher._prep(a, b, "l2_u8")
    assert code == 4 and x.shape == (9, 8) and y.shape == (4, 8) and x.dtype == y.dtype == np.uint8
    assert x.flags.c_contiguous and y.flags.c_contiguous
    assert np.array_equal(x[:, :dim], a) and np.array_equal(y[:, :dim], b) and not x[:, dim:].any() and not y[:, dim:].any()
    assert np.array_equal(ur.sq_dist(x, y), ur.sq_dist(a, b))          # the zero bytes add nothing
    k = [np.zeros((9, 2))], [np.zeros((4, 2))]
    code, kind, A, B, K1, K2, o1, o2 = matcher._stack_pairs(k[0], k[1], [a], [b], "F", 0.9, "l2_u8", 0)
    A, B, _, _ = matcher._finish_pairs(code, kind, A, B, K1, K2, 0)
    assert code == 4 and np.array_equal(A, x) and np.array_equal(B, y)


def test_prep_refuses_float_rows_and_wide_rows():
    with pytest.raises(ValueError, match="uint8"):
        matcher._prep(np.zeros((3, 8), np.float32), np.zeros((3, 8), np.float32), "l2_u8")
    with pytest.raises(ValueError, match="256"):
        matcher._prep(np.zeros((3, 257), np.uint8), np.zeros((3, 257), np.uint8), "l2_u8")
    assert matcher._prep(np.zeros((3, 256), np.uint8), np.zeros((3, 256), np.uint8), "l2_u8")[0] == 4


def test_tensor_form_checks_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d1 = torch.zeros((10, 8), dtype=torch.uint8); d2 = torch.zeros((7, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="l2_u8"):
        tensor_api.knn_match_batch_tensors(d1.float(), d2.float(), [4, 6], [3, 4], norm="l2_u8")
    with pytest.raises(ValueError, match="256"):
        tensor_api.knn_match_batch_tensors(torch.zeros((10, 260), dtype=torch.uint8), torch.zeros((7, 260), dtype=torch.uint8), [4, 6], [3, 4],
                                           norm="l2_u8")
    with pytest.raises(ValueError):                                    # valid arguments, but not on a ROCm device
        tensor_api.knn_match_batch_tensors(d1, d2, [4, 6], [3, 4], norm="l2_u8")
    with pytest.raises(ValueError):
        tensor_api.knn_match_tensors(d1, d2, norm="l2_u8")


# ---- the C-ABI: refused before the library looks for a device ------------------------------------------------------------------
def _abi(norm, dim):
    """return codes of every matcher entry point that takes a norm (pattern of tests/test_guided_cpu.py::_abi)"""
    L = _lib.lib()
    mp = _lib.MatchParams(norm, dim, 0.9, False); gp = _lib.GuideParams(0, 0, 0.5)
    prm = _lib.make_params(0.5, 0.99, 1000, 0, True, 0.0)
    o1 = np.asarray((0, 4, 10), np.int64); o2 = np.asarray((0, 3, 7), np.int64)
    lp = C.POINTER(C.c_int64); p1 = o1.ctypes.data_as(lp); p2 = o2.ctypes.data_as(lp)
    a = np.zeros((10, dim), np.float32); b = np.zeros((7, dim), np.float32)          # large enough for either element size
    idx = np.zeros((10, 2), np.int32); dist = np.zeros((10, 2), np.float32)
    rc = {}
    rc["match"] = L.mi_degensac_match(norm, a.ctypes.data_as(C.c_void_p), 10, b.ctypes.data_as(C.c_void_p), 7, dim, 0.9, 0, 0,
                                      idx.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(C.POINTER(C.c_float)), None)
    rc["knn2_dev"] = L.mi_degensac_match_knn2_dev(norm, None, 10, None, 7, dim, 0, None, None, None)
    rc["knn2_batch_dev"] = L.mi_degensac_match_knn2_batch_dev(norm, None, None, p1, p2, 2, dim, 0, None, None, None)
    rc["verify_batch_dev"] = L.mi_degensac_match_verify_batch_dev(0, C.byref(mp), None, None, p1, p2, None, None, 2, 2, C.byref(prm), None, 0, None,
                                                                  None, None, None, None, None)
    rc["verify_batch"] = L.mi_degensac_match_verify_batch(1, C.byref(mp), None, None, p1, p2, None, None, 2, 2, C.byref(prm), None, 0, None, None, None,
                                                          None, None)
    rc["guided_batch_dev"] = L.mi_degensac_match_guided_batch_dev(C.byref(mp), None, None, p1, p2, None, None, 2, 2, None, C.byref(gp), 0, None, None,
                                                                  None, None, None, None)
    rc["guided_knn2"] = L.mi_degensac_match_guided_knn2_batch_dev(norm, None, None, p1, p2, 2, dim, None, None, 2, None, C.byref(gp), 0, None, None,
                                                                  None)
    rc["guided_batch"] = L.mi_degensac_match_guided_batch(C.byref(mp), None, None, p1, p2, None, None, 2, 2, None, C.byref(gp), 0, None, None, None,
                                                          None)
    return rc


@pytest.mark.parametrize("norm,dim,words", [(4, 6, "multiple of 4"), (4, 260, "float32"), (4, 0, ""), (2, 8, ""), (3, 8, ""), (5, 8, ""), (-1, 8, "")])
def test_abi_refuses(norm, dim, words):
    rc = _abi(norm, dim)
    assert all(v == EINVAL for v in rc.values()), rc
    L = _lib.lib()
    L.mi_degensac_match_knn2_dev(norm, None, 10, None, 7, dim, 0, None, None, None)
    assert words in L.mi_degensac_match_last_error().decode()
    mp = _lib.MatchParams(norm, dim, 0.9, False); gp = _lib.GuideParams(0, 0, 0.5)
    o = np.asarray((0, 4), np.int64); lp = C.POINTER(C.c_int64)
    L.mi_degensac_match_guided_batch_dev(C.byref(mp), None, None, o.ctypes.data_as(lp), o.ctypes.data_as(lp), None, None, 2, 1, None, C.byref(gp), 0,
                                         None, None, None, None, None, None)
    assert words in L.mi_degensac_match_last_error().decode()


def test_abi_empty_batch_of_the_new_norm_returns_zero():
    L = _lib.lib()
    o = np.zeros(1, np.int64); lp = C.POINTER(C.c_int64)
    mp = _lib.MatchParams(4, 128, 0.9, False); gp = _lib.GuideParams(0, 0, 0.5)
    assert L.mi_degensac_match_knn2_batch_dev(4, None, None, o.ctypes.data_as(lp), o.ctypes.data_as(lp), 0, 256, 0, None, None, None) == 0
    assert L.mi_degensac_match_guided_batch_dev(C.byref(mp), None, None, o.ctypes.data_as(lp), o.ctypes.data_as(lp), None, None, 2, 0, None,
                                                C.byref(gp), 0, None, None, None, None, None, None) == 0


# ---- uint8 L2 == float32 L2 for dim <= 256, on the oracle alone ----------------------------------------------------------------
def test_shapes_cover_the_stated_rows_and_dims():
    s = ur.shapes()
    assert {x[0] for x in s} >= set(ur.ROWS) and {x[1] for x in s} >= set(ur.ROWS) and {x[2] for x in s} >= set(ur.DIMS)


@pytest.mark.parametrize("family", ur.FAMILIES)
def test_integer_reference_equals_the_float32_oracle(family):
    for n1, n2, dim in ur.shapes() + [(40, 50, d) for d in ur.UNPADDED_DIMS]:
        if n1 * n2 * dim > 129 * 1000 * 256:                           # the float32 oracle loops over k on n1 x n2 matrices
            n1, n2 = min(n1, 300), min(n2, 300)
        a, b = ur.descs(family, n1, n2, dim, 1)
        assert ur.same_bits(ur.knn2(a, b), mo.knn2(a, b, "l2")), (family, n1, n2, dim)
        assert ur.sq_dist(a, b).max(initial=0) < 1 << 24


def test_the_extreme_distance_is_exact():
    a = np.zeros((3, 256), np.uint8); b = np.full((4, 256), 255, np.uint8); b[2, 0] = 254
    S = ur.sq_dist(a, b)
    assert S.max() == 256 * 255 * 255 == 16646400 < 1 << 24
    idx, dist = ur.knn2(a, b)
    assert list(idx[0]) == [2, 0] and dist[0, 1] == np.float32(4080.0)                 # sqrt(16646400) = 4080 exactly
    assert ur.same_bits((idx, dist), mo.knn2(a, b, "l2"))
    assert ur.same_bits(ur.knn2(b, a), mo.knn2(b, a, "l2"))                              # every train row ties: lower indices


@pytest.mark.parametrize("bug", ["signed", "drop_word"])
@pytest.mark.parametrize("family", ["uniform", "extremes"])
def test_broken_references_are_rejected(bug, family):
    """the comparison that accepts the reference rejects a byte read as signed without the offset, and a dropped k-word"""
    for n1, n2, dim in [(64, 65, 8), (127, 129, 128), (63, 64, 256)]:
        a, b = ur.descs(family, n1, n2, dim, 1)
        want = mo.knn2(a, b, "l2")
        assert ur.same_bits(ur.knn2(a, b), want)
        assert not ur.same_bits(ur.knn2(a, b, bug), want), (bug, family, n1, n2, dim)
