"""The refit of F / H on exported correspondence lists without a device (include/mi_degensac.h mi_degensac_refit_lists*,
matcher.refit_correspondences, tensor_api.refit_correspondences_tensors): every refusal of both C entry points with its message (each comes
back as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), K == 0, the Python keyword and shape
checks, the restatement tests/refit_ref.py on small lists whose outcome can be told in advance, three broken restatements that these lists
reject, and the margin that every scene of test_gpu_refit.py must have."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import refit_ref as R

EINVAL = -1
NAMES = ("dev", "host")


def _abi(which, K=2, cap=10, gp="default", max_fits=4, null=()):
    """(rc, message) of one entry point; data pointers hold an address (never read: every call here is refused first) unless in `null`"""
    L = _lib.lib(); buf = np.zeros(64); addr = buf.ctypes.data
    P = lambda name: None if name in null else addr                    # noqa: E731
    if gp == "default":
        gp = _lib.GuideParams(0, 0, 0.5)
    gpp = None if gp is None else C.byref(gp)
    head = (P("pts"), P("off"), P("models"), K, cap, gpp, max_fits, 0)
    outs = (P("models_out"), P("inlier"), None, None, None)
    rc = L.mi_degensac_refit_lists_dev(*head, None, *outs) if which == "dev" else L.mi_degensac_refit_lists(*head, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and part in msg, (which, rc, msg)


def test_tile_constants_and_status_codes_are_mirrored():
    L = _lib.lib()
    assert L.mi_degensac_refit_tile(0) == _lib.REFIT_STEP and L.mi_degensac_refit_tile(1) == _lib.REFIT_GRID and L.mi_degensac_refit_tile(2) == -1
    assert (_lib.REFIT_FIXED, _lib.REFIT_MAX_FITS, _lib.REFIT_SHORT, _lib.REFIT_BAD_FIT, _lib.REFIT_WORSE, _lib.REFIT_TRUNCATED) == \
        (R.FIXED, R.MAX_FITS, R.SHORT, R.BAD_FIT, R.WORSE, R.TRUNCATED) == tuple(range(6))


def test_negative_counts():
    _refused(b"n_entries", K=-1)
    _refused(b"cap", cap=-1)
    _refused(b"cap", cap=0x40000000)
    _refused(b"max_fits", max_fits=-1)
    _refused(b"n_entries", K=-1, cap=-1, max_fits=-1)                  # in this order


def test_guide_params():
    _refused(b"guide params", gp=None)
    gp = _lib.GuideParams(0, 0, 0.5); gp.struct_size = 8
    _refused(b"struct_size", gp=gp)
    gp = _lib.GuideParams(0, 0, 0.5); gp.homography = 2
    _refused(b"homography", gp=gp)
    for g in (_lib.GuideParams(0, 2, 0.5), _lib.GuideParams(0, -1, 0.5), _lib.GuideParams(1, 5, 0.5), _lib.GuideParams(1, -1, 0.5)):
        _refused(b"error_type", gp=g)
        _refused(b"error_type", gp=g, K=0, cap=0)
    for px in (-1.0, float("nan"), -0.0 - 1e-300):
        _refused(b"px_th", gp=_lib.GuideParams(0, 0, px))
        _refused(b"px_th", gp=_lib.GuideParams(1, 4, px))


def test_null_pointers():
    _refused(b"corr_offsets", null=("off",))
    _refused(b"corr_offsets", null=("off",), K=0, cap=0)
    _refused(b"models", null=("models",))
    _refused(b"models", null=("models_out",))
    _refused(b"pts", null=("pts",))
    _refused(b"inlier", null=("inlier",))
    _refused(b"guide params", gp=None, null=("off", "pts"))           # the parameters come first


def test_k0_and_cap0_succeed_without_a_device():
    for which in NAMES:
        rc, _ = _abi(which, K=0, cap=0, null=("pts", "models", "models_out", "inlier"))
        assert rc == 0, which


# ---- the Python checks ----
def _np(K=2, cap=10):
    return np.zeros((cap, 4)), np.zeros(K + 1, np.int64), np.zeros((K, 3, 3))


@pytest.mark.parametrize("kw, part", [
    (dict(model="E"), "model"), (dict(error_type="nope"), "Error type"), (dict(model="F", error_type="symm_max"), "Error type"),
    (dict(px_th=-1.0), "px_th"), (dict(px_th=float("nan")), "px_th"), (dict(px_th="x"), "px_th"),
    (dict(max_fits=-1), "max_fits"), (dict(max_fits=1.5), "max_fits"), (dict(max_fits=True), "max_fits"),
])
def test_keyword_checks(kw, part):
    pts, off, M = _np()
    with pytest.raises(ValueError, match=part):
        matcher.refit_correspondences(pts, off, M, **kw)


def test_shape_and_dtype_checks():
    pts, off, M = _np()
    bad = [(pts[:, :3], off, M, "pts"), (pts.astype(np.float32), off, M, "pts"), (pts.ravel(), off, M, "pts"),
           (pts, off.astype(np.int32), M, "corr_offsets"), (pts, off.reshape(1, -1), M, "corr_offsets"), (pts, off[:0], M, "corr_offsets"),
           (pts, off, M[:1], "models"), (pts, off, M.reshape(2, 9), "models"), (pts, off, M.astype(np.float32), "models")]
    for a, b, c, part in bad:
        with pytest.raises(ValueError, match=part):
            matcher.check_refit_args(a.shape, a.dtype, b.shape, b.dtype, c.shape, c.dtype)
    assert matcher.check_refit_args(pts.shape, pts.dtype, off.shape, off.dtype, M.shape, M.dtype) == (2, 10, 0.5, 0, 4)
    assert matcher.check_refit_args(pts.shape, pts.dtype, off.shape, off.dtype, M.shape, M.dtype, "H", None, "symm_sum", 0) == (2, 10, 1.0, 4, 0)


def test_tensor_call_wants_tensors():
    from pydegensac_amd import tensor_api
    pts, off, M = _np()
    with pytest.raises(ValueError, match="torch tensors"):
        tensor_api.refit_correspondences_tensors(pts, off, M)
    import torch
    with pytest.raises(ValueError, match="ROCm device"):
        tensor_api.refit_correspondences_tensors(torch.from_numpy(pts), torch.from_numpy(off), torch.from_numpy(M))


# ---- the restatement on lists whose outcome can be told in advance ----
def _one(oracle_port, sc, **kw):
    return R.refit(oracle_port, sc["pts"], sc["off"], sc["models"], sc["model"], sc["et"], sc["px_th"], **kw)


@pytest.mark.parametrize("model, n, where", [("F", 600, [64 * k + 3 for k in range(8)]), ("F", 300, list(range(290, 298))),
                                             ("H", 250, [3, 67, 131, 195, 200]), ("H", 40, [0, 5, 9, 20, 21, 39])])
def test_exact_members_are_a_fixed_point_after_one_fit(oracle_port, model, n, where):
    """noise-free rows of the ground truth at `where`, every other row beyond 1000 th: the ground truth's members are exactly `where`, the
    fit on them keeps them, the second pass finds the same set"""
    sc = R.sparse_scene(oracle_port, model, 0, n, where, 71)
    ref = _one(oracle_port, sc)
    assert ref["info"].tolist() == [[len(where), len(where), 1, R.FIXED]]
    assert np.flatnonzero(ref["inlier"]).tolist() == sorted(where)
    again = R.refit(oracle_port, sc["pts"], sc["off"], ref["models"], model, 0)
    assert again["info"].tolist() == [[len(where), len(where), 1, R.FIXED]] and np.array_equal(again["inlier"], ref["inlier"])
    assert R.rel_fro(again["models"][0], ref["models"][0]) <= 1e-9


def test_short_lists_zero_models_and_max_fits_0(oracle_port):
    sc = R.sparse_scene(oracle_port, "F", 0, 300, [1, 60, 64, 127, 128, 255, 299], 72)          # seven members: one short of a fit
    assert _one(oracle_port, sc)["info"].tolist() == [[7, 7, 0, R.SHORT]]
    sc = R.sparse_scene(oracle_port, "H", 0, 100, [0, 50, 99], 73)
    ref = _one(oracle_port, sc)
    assert ref["info"].tolist() == [[3, 3, 0, R.SHORT]] and np.array_equal(ref["models"], sc["models"])
    sc = R.sparse_scene(oracle_port, "F", 0, 100, list(range(10, 30)), 74)
    assert _one(oracle_port, sc, max_fits=0)["info"].tolist() == [[20, 20, 0, R.MAX_FITS]]
    sc["models"][:] = 0.0
    ref = _one(oracle_port, sc)
    assert ref["info"].tolist() == [[0, 0, 0, R.SHORT]] and not ref["inlier"].any() and not ref["models"].any()
    sc["models"][0, 3] = np.nan
    ref = _one(oracle_port, sc)
    assert ref["info"].tolist() == [[0, 0, 0, R.SHORT]] and not ref["inlier"].any()


def test_members_grow_after_one_fit_and_a_losing_fit_is_dropped(oracle_port):
    """the noisy scenes: a start model fitted on 24 inliers gains members when it is refitted on all of its members; where a later fit
    loses members the entry keeps the model and the set it had (WORSE), so members never fall below n0"""
    sc = R.gpu_scenes(oracle_port)["F_len_1"]; ref = R.reference(oracle_port, "F_len_1", 4)
    info = ref["info"]
    assert (info[:, 1] >= info[:, 0]).all() and (info[:, 1] > info[:, 0]).any() and (info[:, 3] == R.WORSE).any()
    one = R.reference(oracle_port, "F_len_1", 1)["info"]
    assert ((one[:, 1] > one[:, 0]) & (one[:, 2] == 1)).any()
    for p in np.flatnonzero(info[:, 3] == R.WORSE):
        b, e = sc["off"][p], sc["off"][p + 1]
        I, _ = R.members(oracle_port, "F", 1, ref["models"][p], sc["pts"][b:e], R.threshold("F", 1))
        assert len(I) == info[p, 1] and np.array_equal(np.flatnonzero(ref["inlier"][b:e]), I)
        nxt = R.fit(oracle_port, "F", sc["pts"][b:e], I)
        I2, _ = R.members(oracle_port, "F", 1, nxt, sc["pts"][b:e], R.threshold("F", 1))
        assert len(I2) < len(I) or info[p, 2] > 1


def test_offsets_that_are_no_ranges(oracle_port):
    sc = R.offsets_scene(oracle_port)
    ref = _one(oracle_port, sc)
    assert ref["info"][:, 3].tolist()[2:5] == [R.TRUNCATED] * 3 and (ref["info"][2:5, :3] == 0).all()
    assert np.array_equal(ref["models"][2:5], sc["models"][2:5]) and not ref["inlier"][50:60].any()
    assert ref["info"][5, 0] > 0 and ref["inlier"][60:100].sum() == ref["info"][5, 1]


def test_broken_restatements_are_rejected(oracle_port):
    """`<` for `<=`: a threshold that equals a row's residual (H symm_max, where th = px_th itself); accepting a smaller set: a scene
    with a WORSE entry; fitting on all rows instead of the members: any scene with outliers"""
    sc = R.lengths_scene(oracle_port, "H", 2, [60], 81)
    d = R.resid(oracle_port, "H", 2, sc["models"][0], sc["pts"])
    sc["px_th"] = float(np.sort(d)[20])
    good = _one(oracle_port, sc, max_fits=0); lt = _one(oracle_port, sc, max_fits=0, broken="lt")
    assert good["info"][0, 0] == 21 and lt["info"][0, 0] == 20
    sc = R.gpu_scenes(oracle_port)["F_len_1"]
    good = R.reference(oracle_port, "F_len_1", 4); small = _one(oracle_port, sc, broken="smaller")
    assert not np.array_equal(good["info"], small["info"]) and (small["info"][:, 3] != R.WORSE).all()
    allrows = _one(oracle_port, sc, broken="allrows")
    assert not np.array_equal(good["inlier"], allrows["inlier"]) and allrows["info"][:, 1].sum() < good["info"][:, 1].sum()


def test_every_gpu_scene_keeps_its_margin(oracle_port):
    """no residual of any model the restatement visits lies within 1e-6 th of th, in any scene test_gpu_refit.py uses and at every max_fits
    it uses (the models of max_fits 0 and 1 are the first of those of 4)"""
    for name, sc in R.gpu_scenes(oracle_port).items():
        m = R.min_margin(oracle_port, sc, R.reference(oracle_port, name, 4))
        assert m > R.MARGIN, (name, m)
