"""Batched match-and-verify (matcher.match_and_verify_batch, tensor_api.match_and_verify_batch_tensors): the argument checks run
in Python before the library is reached, so every one of them raises ValueError on a machine without a GPU."""
import numpy as np
import pytest

from pydegensac_amd import matcher


def _pairs(K=3, n=20, dim=16, desc=np.float32, kp_w=2, kp=np.float64):
    rng = np.random.default_rng(0)
    d1 = [rng.normal(size=(n, dim)).astype(desc) for _ in range(K)]
    d2 = [rng.normal(size=(n + 1, dim)).astype(desc) for _ in range(K)]
    k1 = [rng.uniform(0, 100, (n, kp_w)).astype(kp) for _ in range(K)]
    k2 = [rng.uniform(0, 100, (n + 1, kp_w)).astype(kp) for _ in range(K)]
    return k1, k2, d1, d2


def _call(**kw):
    k1, k2, d1, d2 = kw.pop("arrays", None) or _pairs()
    return matcher.match_and_verify_batch(k1, k2, d1, d2, **kw)


def test_model_must_be_f_or_h():
    with pytest.raises(ValueError, match="model"):
        _call(model="E")


@pytest.mark.parametrize("ratio", [0.0, -0.5, float("nan"), float("inf")])
def test_ratio_must_be_finite_and_positive(ratio):
    with pytest.raises(ValueError, match="ratio"):
        _call(ratio=ratio)


def test_keypoint_rows_of_width_three_are_refused():
    with pytest.raises(ValueError, match="keypoints"):
        _call(arrays=_pairs(kp_w=3))


@pytest.mark.parametrize("kp_w,kp", [(2, np.float32), (4, np.float64), (6, np.float32)])
def test_keypoint_dtypes(kp_w, kp):
    with pytest.raises(ValueError, match="keypoints"):
        _call(arrays=_pairs(kp_w=kp_w, kp=kp))


@pytest.mark.parametrize("desc", [np.float64, np.int32, np.float16])
def test_descriptor_dtypes(desc):
    with pytest.raises(ValueError, match="descriptors"):
        _call(arrays=_pairs(desc=desc))


def test_hamming_needs_uint8():
    with pytest.raises(ValueError, match="Hamming"):
        _call(norm="hamming")
    with pytest.raises(ValueError, match="L2"):
        _call(arrays=_pairs(desc=np.uint8), norm="l2")


def test_mismatched_counts():
    k1, k2, d1, d2 = _pairs()
    with pytest.raises(ValueError):
        matcher.match_and_verify_batch(k1[:2], k2, d1, d2)
    k1[1] = k1[1][:-1]                                           # one keypoint row short of the descriptors
    with pytest.raises(ValueError, match="keypoint row"):
        matcher.match_and_verify_batch(k1, k2, d1, d2)


def test_empty_batch():
    with pytest.raises(ValueError):
        matcher.match_and_verify_batch([], [], [], [])


def test_shape_checks_on_counts():
    """the shared checker as the tensor API calls it: counts against the number of rows, per side"""
    chk = matcher.check_match_verify_args
    ok = dict(model="F", ratio=0.9, norm=None, d1_shape=(10, 8), d1_dtype=np.float32, d2_shape=(7, 8), d2_dtype=np.float32,
              k1_shape=(10, 2), k1_dtype=np.float64, k2_shape=(7, 2), k2_dtype=np.float64, counts1=[4, 6], counts2=[3, 4])
    code, kind, o1, o2 = chk(**ok)
    assert code == matcher.NORM_L2 and kind == "xy" and list(o1) == [0, 4, 10] and list(o2) == [0, 3, 7]
    for bad in (dict(counts1=[4, 5]), dict(counts2=[3, 4, 0]), dict(counts1=[11, -1]), dict(counts1=[4.0, 6.0]),
                dict(d2_shape=(7, 9)), dict(k2_shape=(6, 2)), dict(k1_shape=(10, 4), k1_dtype=np.float32)):
        with pytest.raises(ValueError):
            chk(**{**ok, **bad})
    code, kind, _, _ = chk(**{**ok, "d1_dtype": np.uint8, "d2_dtype": np.uint8, "k1_shape": (10, 4), "k1_dtype": np.float32,
                              "k2_shape": (7, 4), "k2_dtype": np.float32})
    assert code == matcher.NORM_HAMMING and kind == "kpts"


def test_tensor_form_checks_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d1 = torch.zeros((10, 8)); d2 = torch.zeros((7, 8)); k1 = torch.zeros((10, 2), dtype=torch.float64); k2 = torch.zeros((7, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="counts"):
        tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, [4, 5], [3, 4])
    with pytest.raises(ValueError, match="model"):
        tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, [4, 6], [3, 4], model="X")
    with pytest.raises(ValueError, match="keypoints"):
        tensor_api.match_and_verify_batch_tensors(k1.float(), k2, d1, d2, [4, 6], [3, 4])
    with pytest.raises(ValueError, match="descriptors"):
        tensor_api.knn_match_batch_tensors(d1.double(), d2, [4, 6], [3, 4])
    with pytest.raises(ValueError):                             # valid shapes, but not on a ROCm device
        tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, [4, 6], [3, 4])
