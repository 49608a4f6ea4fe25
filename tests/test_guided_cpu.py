"""Guided matching (matcher.guided_match_batch / guided_match, tensor_api.guided_match_batch_tensors, the guided=True stage of the
batched match-and-verify calls, include/mi_degensac.h mi_degensac_match_guided_*): the argument checks raise ValueError before a
device is needed, and the C-ABI refuses bad arguments with MI_DEGENSAC_EINVAL before it looks for a device."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher


def _pairs(K=3, n=20, dim=16, desc=np.float32, kp_w=2, kp=np.float64):
    rng = np.random.default_rng(0)
    d1 = [rng.normal(size=(n, dim)).astype(desc) for _ in range(K)]
    d2 = [rng.normal(size=(n + 1, dim)).astype(desc) for _ in range(K)]
    k1 = [rng.uniform(0, 100, (n, kp_w)).astype(kp) for _ in range(K)]
    k2 = [rng.uniform(0, 100, (n + 1, kp_w)).astype(kp) for _ in range(K)]
    return k1, k2, d1, d2


def _call(models=None, **kw):
    k1, k2, d1, d2 = kw.pop("arrays", None) or _pairs()
    if models is None:
        models = np.tile(np.eye(3), (len(d1), 1, 1))
    return matcher.guided_match_batch(k1, k2, d1, d2, models, **kw)


def test_model_must_be_f_or_h():
    with pytest.raises(ValueError, match="model"):
        _call(model="E")


@pytest.mark.parametrize("shape", [(2, 3, 3), (4, 3, 3), (3, 9), (3, 3, 4), (3,)])
def test_models_of_the_wrong_shape(shape):
    with pytest.raises(ValueError, match="models"):
        _call(models=np.zeros(shape))


@pytest.mark.parametrize("dt", [np.float32, np.int64, np.complex128])
def test_models_must_be_float64(dt):
    with pytest.raises(ValueError, match="models"):
        _call(models=np.tile(np.eye(3), (3, 1, 1)).astype(dt))


@pytest.mark.parametrize("px_th", [-0.5, -1e-300, float("nan"), "x"])
def test_px_th_must_be_a_non_negative_number(px_th):
    with pytest.raises(ValueError, match="px_th"):
        _call(px_th=px_th)


@pytest.mark.parametrize("model,error_type", [("F", "symm_max"), ("F", "symm_sq_sum"), ("H", "symm_epipolar"), ("F", "nope"), ("H", "")])
def test_error_type_of_the_model_kind(model, error_type):
    with pytest.raises(ValueError, match="Error type"):
        _call(model=model, error_type=error_type)


@pytest.mark.parametrize("ratio", [0.0, -0.5, float("nan"), float("inf")])
def test_ratio_must_be_finite_and_positive(ratio):
    with pytest.raises(ValueError, match="ratio"):
        _call(ratio=ratio)


def test_shape_and_dtype_mismatches():
    with pytest.raises(ValueError, match="descriptors"):
        _call(arrays=_pairs(desc=np.float64))
    with pytest.raises(ValueError, match="keypoints"):
        _call(arrays=_pairs(kp_w=3))
    k1, k2, d1, d2 = _pairs()
    with pytest.raises(ValueError):
        matcher.guided_match_batch(k1[:2], k2, d1, d2, np.zeros((3, 3, 3)))
    k2[1] = k2[1][:-1]
    with pytest.raises(ValueError, match="keypoint row"):
        matcher.guided_match_batch(k1, k2, d1, d2, np.zeros((3, 3, 3)))
    k1, k2, d1, d2 = _pairs(K=1)
    with pytest.raises(ValueError, match="models"):
        matcher.guided_match(k1[0], k2[0], d1[0], d2[0], np.eye(4))


def test_match_and_verify_checks_guided_arguments_first():
    k1, k2, d1, d2 = _pairs()
    with pytest.raises(ValueError, match="model"):
        matcher.match_and_verify_batch(k1, k2, d1, d2, model="E", guided=True)


def test_tensor_form_checks_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d1 = torch.zeros((10, 8)); d2 = torch.zeros((7, 8)); k1 = torch.zeros((10, 2), dtype=torch.float64); k2 = torch.zeros((7, 2), dtype=torch.float64)
    M = torch.zeros((2, 3, 3), dtype=torch.float64)
    call = tensor_api.guided_match_batch_tensors
    with pytest.raises(ValueError, match="counts"):
        call(k1, k2, d1, d2, [4, 5], [3, 4], M)
    with pytest.raises(ValueError, match="model"):
        call(k1, k2, d1, d2, [4, 6], [3, 4], M, model="X")
    with pytest.raises(ValueError, match="models"):
        call(k1, k2, d1, d2, [4, 6], [3, 4], M[:1])
    with pytest.raises(ValueError, match="models"):
        call(k1, k2, d1, d2, [4, 6], [3, 4], M.float())
    with pytest.raises(ValueError, match="px_th"):
        call(k1, k2, d1, d2, [4, 6], [3, 4], M, px_th=float("nan"))
    with pytest.raises(ValueError, match="Error type"):
        call(k1, k2, d1, d2, [4, 6], [3, 4], M, model="H", error_type="symm_epipolar")
    with pytest.raises(ValueError, match="keypoints"):
        call(k1.float(), k2, d1, d2, [4, 6], [3, 4], M)
    with pytest.raises(ValueError):                             # valid arguments, but not on a ROCm device
        call(k1, k2, d1, d2, [4, 6], [3, 4], M)
    with pytest.raises(ValueError):
        call(k1, k2, d1, d2, [4, 6], [3, 4], np.zeros((2, 3, 3)))


# ---- the C-ABI: every refusal below comes before the library looks for a device ----
def _abi(mp=None, gp=None, kp_dim=2, off1=(0, 4, 10), off2=(0, 3, 7), n_pairs=None):
    L = _lib.lib()
    mp = mp or _lib.MatchParams(0, 8, 0.9, False)
    gp = gp or _lib.GuideParams(0, 0, 0.5)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64)
    K = len(o1) - 1 if n_pairs is None else n_pairs
    lp = C.POINTER(C.c_int64)
    rc_dev = L.mi_degensac_match_guided_batch_dev(C.byref(mp), None, None, o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), None, None, kp_dim, K,
                                                  None, C.byref(gp), 0, None, None, None, None, None, None)
    rc_knn = L.mi_degensac_match_guided_knn2_batch_dev(mp.norm, None, None, o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), K, mp.dim, None, None,
                                                       kp_dim, None, C.byref(gp), 0, None, None, None)
    rc_host = L.mi_degensac_match_guided_batch(C.byref(mp), None, None, o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), None, None, kp_dim, K, None,
                                               C.byref(gp), 0, None, None, None, None)
    return rc_dev, rc_knn, rc_host


EINVAL = -1


@pytest.mark.parametrize("case", [
    dict(mp=_lib.MatchParams(2, 8, 0.9, False)),                     # norm
    dict(mp=_lib.MatchParams(0, 0, 0.9, False)),                     # dim
    dict(mp=_lib.MatchParams(1, 6, 0.9, False)),                     # Hamming dim % 4
    dict(kp_dim=3),
    dict(gp=_lib.GuideParams(0, 2, 0.5)),                            # error_type 2 is an H kind
    dict(gp=_lib.GuideParams(1, 5, 0.5)),
    dict(gp=_lib.GuideParams(1, -1, 0.5)),
    dict(gp=_lib.GuideParams(0, 0, -0.1)),
    dict(gp=_lib.GuideParams(1, 2, float("nan"))),
    dict(off1=(0, 6, 4)),                                            # decreasing
    dict(off2=(-1, 3, 7)),
    dict(n_pairs=-1),
])
def test_abi_refuses_bad_arguments(case):
    assert _abi(**case) == (EINVAL, EINVAL, EINVAL)
    assert _lib.lib().mi_degensac_match_last_error()


def test_abi_refuses_bad_ratio_and_struct_size():
    for r in (0.0, -1.0, float("nan"), float("inf")):
        rc_dev, _, rc_host = _abi(mp=_lib.MatchParams(0, 8, r, False))
        assert (rc_dev, rc_host) == (EINVAL, EINVAL), r
    gp = _lib.GuideParams(0, 0, 0.5); gp.struct_size = 8
    assert _abi(gp=gp) == (EINVAL, EINVAL, EINVAL)


def test_abi_empty_batch_returns_zero():
    assert _abi(off1=(0,), off2=(0,), n_pairs=0) == (0, 0, 0)
