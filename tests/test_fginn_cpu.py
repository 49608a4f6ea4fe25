"""The FGINN ratio test without a device: the restatement of tests/fginn_ref.py against the plain 2-NN (r = 0), the twin scene of
the feature, the float64 bound of tests/matcher_ref.py for slot 1, four broken restatements that the scenes must reject, and the
refusals of the Python calls and of the C-ABI, which come before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher
from tests import fginn_ref as fr, matcher_ref as mr

EINVAL = -1
FAMILIES = [("l2", "normal"), ("l2", "sift"), ("l2", "tiny"), ("l2", "subnormal"), ("hamming", "hamming"), ("l2_u8", "hamming")]


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _family(norm, fam, n1=70, n2=130, width=36):
    a, b = mr.descs(3, n1, n2, width, fam)
    rng = np.random.default_rng(9)
    kp2 = rng.uniform(0, 60, (n2, 2))
    return a, b, kp2


@pytest.mark.parametrize("norm,fam", FAMILIES)
def test_radius_zero_is_the_plain_2nn(norm, fam):
    a, b, kp2 = _family(norm, fam)
    idx, dist, needy, _ = fr.fginn(a, b, kp2, 0.0, norm)
    pi, pd = mo.top2(fr.dmat(a, b, norm))
    assert np.array_equal(idx, pi) and np.array_equal(_bits(dist), _bits(pd)) and not needy.any()


@pytest.mark.parametrize("norm", fr.NORMS)
def test_twin_scene_plain_keeps_none_fginn_keeps_all(norm):
    a, b, kp2 = fr.twin_scene(1, 200, 400, 32, norm, 200)
    pi, pd = mo.top2(fr.dmat(a, b, norm))
    assert fr.keep(pi, pd, 0.9).sum() == 0
    idx, dist, needy, _ = fr.fginn(a, b, kp2, 10.0, norm)
    assert needy.all() and fr.keep(idx, dist, 0.9).sum() == 200
    assert np.array_equal(idx[:, 0] % 200, np.arange(200))            # the train row or its twin


@pytest.mark.parametrize("fam", mr.L2_FAMILIES)
@pytest.mark.parametrize("r", [0.0, 8.0, 30.0])
def test_slot1_within_the_float64_bound_among_the_competing_rows(fam, r):
    a, b, kp2 = _family("l2", fam)
    idx, dist, _, ok = fr.fginn(a, b, kp2, r, "l2")
    D = mr.dist64(a, b, "l2"); g = mr.g_bound(a.shape[1])
    have = np.flatnonzero(idx[:, 1] >= 0)
    assert np.array_equal(idx[:, 1] >= 0, ok.any(axis=1)) and len(have) > 0
    assert ok[have, idx[have, 1]].all()
    best = np.where(ok, D, np.inf).min(axis=1)[have]
    De = D[have, idx[have, 1]]
    assert (De <= best * (1 + g) / (1 - g)).all()
    assert (np.abs(dist[have, 1].astype(np.float64) - De) <= g * De).all()


# ---- four broken restatements ------------------------------------------------------------------------------------------------
def _broken(a, b, kp2, r, kind):
    D = fr.dmat(a, b, "l2")
    pi, pd = mo.top2(D)
    n1, n2 = D.shape
    anchor = pi[:, 1] if kind == "anchor_from_i1" else pi[:, 0]
    an = np.clip(anchor, 0, None)
    dx = kp2[None, :, 0] - kp2[an, 0][:, None]; dy = kp2[None, :, 1] - kp2[an, 1][:, None]
    d2 = dx * dx + dy * dy
    ok = d2 > r * r if kind == "gt" else d2 >= r * r
    if kind != "anchor_kept":
        ok &= np.arange(n2)[None, :] != pi[:, 0][:, None]
    si, sd = mo.top2(D, ok)
    if kind == "slot0_excluded":
        return si, sd
    return np.c_[pi[:, 0], si[:, 0]], np.c_[pd[:, 0], sd[:, 0]]


def _radius_scene():
    # one query next to train row 0; rows 1 (at (3, 4), 5 px away) and 2 (far) follow in distance
    b = np.array([[0.0, 0], [1, 0], [2, 0], [3, 0]], np.float32); a = np.array([[0.1, 0]], np.float32)
    kp2 = np.array([[0.0, 0], [3, 4], [100, 100], [0.5, 0]])
    return a, b, kp2


@pytest.mark.parametrize("kind,r", [("gt", 5.0), ("anchor_kept", 0.0), ("anchor_from_i1", 5.0), ("slot0_excluded", 5.0)])
def test_broken_restatements_are_rejected(kind, r):
    a, b, kp2 = _radius_scene()
    idx, dist, _, _ = fr.fginn(a, b, kp2, r, "l2")
    assert list(idx[0]) == [0, 1]                # (3, 4) is exactly 5 away: it competes at r = 5 and at r = 0
    assert list(fr.fginn(a, b, kp2, np.nextafter(5.0, 6.0), "l2")[0][0]) == [0, 2]
    bi, bd = _broken(a, b, kp2, r, kind)
    assert not (np.array_equal(bi, idx) and np.array_equal(_bits(bd), _bits(dist))), kind


# ---- refusals before a device is looked for ----------------------------------------------------------------------------------
BAD_R = [-1.0, -1e-300, float("nan"), float("inf")]


@pytest.mark.parametrize("r", BAD_R + ["x"])
def test_python_calls_refuse_a_bad_radius(r):
    rng = np.random.default_rng(0)
    d1 = rng.normal(size=(20, 8)).astype(np.float32); d2 = rng.normal(size=(21, 8)).astype(np.float32)
    k1 = rng.uniform(0, 100, (20, 2)); k2 = rng.uniform(0, 100, (21, 2))
    with pytest.raises(ValueError, match="spatial_th"):
        matcher.match_fginn(d1, d2, k2, spatial_th=r)
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.match_and_verify_batch([k1], [k2], [d1], [d2], fginn_th=r)
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.check_match_verify_args("F", 0.9, None, d1.shape, d1.dtype, d2.shape, d2.dtype, k1.shape, k1.dtype, k2.shape, k2.dtype, [20], [21],
                                        fginn_th=r)


def test_match_fginn_refuses_keypoints_that_do_not_fit():
    d1 = np.zeros((5, 8), np.float32); d2 = np.zeros((6, 8), np.float32)
    with pytest.raises(ValueError, match="kps2"):
        matcher.match_fginn(d1, d2, np.zeros((5, 2)))
    with pytest.raises(ValueError, match="kps2"):
        matcher.match_fginn(d1, d2, np.zeros((6, 1)))


def test_tensor_call_checks_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d1 = torch.zeros((10, 8)); d2 = torch.zeros((7, 8)); k2 = torch.zeros((7, 2), dtype=torch.float64)
    call = tensor_api.knn_match_fginn_batch_tensors
    for r in BAD_R:
        with pytest.raises(ValueError, match="spatial_th"):
            call(d1, d2, k2, [4, 6], [3, 4], r)
    with pytest.raises(ValueError, match="keypoints"):
        call(d1, d2, k2.float(), [4, 6], [3, 4])
    with pytest.raises(ValueError, match="keypoints"):
        call(d1, d2, torch.zeros((7, 3), dtype=torch.float64), [4, 6], [3, 4])
    with pytest.raises(ValueError, match="counts"):
        call(d1, d2, k2, [4, 5], [3, 4])
    with pytest.raises(ValueError):                                  # valid arguments, but not on a ROCm device
        call(d1, d2, k2, [4, 6], [3, 4])
    with pytest.raises(ValueError, match="ROCm device"):             # [n, 6] keypoint rows pass the layout check too
        call(d1, d2, torch.zeros((7, 6), dtype=torch.float64), [4, 6], [3, 4])


def _abi_knn(r=10.0, kp_dim=2, norm=0, dim=8, off1=(0, 4, 10), off2=(0, 3, 7), n_pairs=None):
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64); lp = C.POINTER(C.c_int64)
    K = len(o1) - 1 if n_pairs is None else n_pairs
    return _lib.lib().mi_degensac_match_fginn_knn2_batch_dev(norm, None, None, o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), K, dim, None, kp_dim,
                                                            r, 0, None, None, None)


def _abi_verify(mp, n_pairs=None, off1=(0, 4, 10), off2=(0, 3, 7)):
    L = _lib.lib(); lp = C.POINTER(C.c_int64)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64)
    K = len(o1) - 1 if n_pairs is None else n_pairs
    prm = _lib.make_params(0.5, 0.99, 1000, 0, True, 0.0)
    rc_dev = L.mi_degensac_match_verify_batch_dev(0, C.byref(mp), None, None, o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), None, None, 2, K,
                                                  C.byref(prm), None, 0, None, None, None, None, None, None)
    rc_host = L.mi_degensac_match_verify_batch(0, C.byref(mp), None, None, o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), None, None, 2, K,
                                               C.byref(prm), None, 0, None, None, None, None, None)
    return rc_dev, rc_host


@pytest.mark.parametrize("case", [dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")), dict(r=-float("inf")), dict(kp_dim=3), dict(norm=2),
                                  dict(dim=0), dict(norm=4, dim=260), dict(off1=(0, 6, 4)), dict(n_pairs=-1)])
def test_abi_knn_refuses_bad_arguments(case):
    assert _abi_knn(**case) == EINVAL
    assert _lib.lib().mi_degensac_match_last_error()


def test_abi_empty_batch_returns_zero():
    assert _abi_knn(off1=(0,), off2=(0,), n_pairs=0) == 0


@pytest.mark.parametrize("r", BAD_R)
def test_abi_verify_refuses_a_bad_radius(r):
    assert _abi_verify(_lib.MatchParams(0, 8, 0.9, False, fginn_th=r)) == (EINVAL, EINVAL)
    assert _abi_verify(_lib.MatchParams(0, 8, 0.9, False, fginn_th=r), n_pairs=0, off1=(0,), off2=(0,)) == (EINVAL, EINVAL)
    assert b"spatial_th" in _lib.lib().mi_degensac_last_error()


def test_abi_verify_refuses_an_unknown_mode():
    mp = _lib.MatchParams(0, 8, 0.9, False); mp.second_nn = 2
    assert _abi_verify(mp, n_pairs=0, off1=(0,), off2=(0,)) == (EINVAL, EINVAL)


@pytest.mark.parametrize("size", [0, 24])
def test_old_layout_match_params_are_accepted(size):
    """a caller built before spatial_th passes struct_size 0 or 24 and anything in its last field: the plain rule, no refusal"""
    assert C.sizeof(_lib.MatchParams) == 32 and _lib.MatchParams.spatial_th.offset == 24
    mp = _lib.MatchParams(0, 8, 0.9, False, fginn_th=-1.0); mp.struct_size = size; mp.second_nn = 7
    assert _abi_verify(mp, n_pairs=0, off1=(0,), off2=(0,)) == (0, 0)
    assert _abi_verify(_lib.MatchParams(0, 8, 0.9, False), n_pairs=0, off1=(0,), off2=(0,)) == (0, 0)
    assert _abi_verify(_lib.MatchParams(0, 8, 0.9, False, fginn_th=0.0), n_pairs=0, off1=(0,), off2=(0,)) == (0, 0)
