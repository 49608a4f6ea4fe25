"""The refit of F / H on exported correspondence lists without a device (include/mi_degensac.h mi_degensac_refit_lists*,
matcher.refit_correspondences, tensor_api.refit_correspondences_tensors): every refusal of both C entry points with its message (each comes
back as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), K == 0, the Python keyword and shape
checks, the restatement tests/refit_ref.py on small lists whose outcome can be told in advance, three broken restatements that these lists
reject, the margin that every scene of test_gpu_refit.py must have, and the scenes fixed by member count (refit_ref.MEMBER_STORES): their
outcome, the oracle's fit against a plain numpy least-squares solution, and the teeth of a comparison of bytes."""
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


# ---- the scenes fixed by member count: the unit entry of the non-minimal fits ----
def _entries(oracle_port, name):
    """(scene, p, m, where, rows of the entry) of every entry of a member store"""
    sc = R.gpu_scenes(oracle_port)[name]
    return [(sc, p, sc["m"][p], sc["where"][p], sc["pts"][sc["off"][p]:sc["off"][p + 1]]) for p in range(len(sc["m"]))]


def test_member_stores_hold_the_counts_the_solvers_switch_at(oracle_port):
    """the catalogue of the member stores: every count of both sides of 16 | 17 (F) and 12 | 13 (H), of the 8-term unroll, the wave, the
    stride of 256 threads and 512, and members that are never a contiguous range of rows"""
    S = R.gpu_scenes(oracle_port)
    assert S["F_members_0"]["m"] == list(R.F_COUNTS) + [24] * 3 and S["H_members_0"]["m"] == list(R.H_COUNTS) + [13] * 3
    assert R.F_COUNTS == (8, 9, 15, 16, 17, 18, 23, 24, 25, 63, 64, 65, 255, 256, 257, 511, 512, 513)
    assert R.H_COUNTS == (4, 5, 11, 12, 13, 14, 19, 20, 21, 63, 64, 65, 255, 256, 257, 513)
    assert S["F_members_1"]["m"] == [16, 17] and all(S[f"H_members_{et}"]["m"] == [12, 13] for et in (1, 2, 3, 4))
    for fr in R.MEMBER_FRAMES:
        assert S[f"F_frame_{fr}"]["m"] == [16, 17, 64, 257] and S[f"H_frame_{fr}"]["m"] == [12, 13, 64, 257]
    assert S["F_rankdef"]["m"] == [9, 20] == S["H_rankdef"]["m"]
    for name in R.MEMBER_STORES:
        for sc, p, m, where, rows in _entries(oracle_port, name):
            assert len(where) == m and (np.diff(where) > 0).all() and where[-1] - where[0] >= m           # sorted, not one range
    late, edges, wave = S["F_members_0"]["where"][-3:]
    assert late.min() >= 1024 and {0, 1023, 1024, 1099} <= set(edges.tolist()) and wave.min() >= 640 and wave.max() < 700
    late, edges, wave = S["H_members_0"]["where"][-3:]
    assert late.min() >= 1024 and {0, 1023, 1024, 1099} <= set(edges.tolist()) and wave.min() >= 640 and wave.max() < 700
    for k in "FH":                                                     # rank-deficient: 3 distinct rows in 9, 6 in 20
        for (sc, p, m, where, rows), d in zip(_entries(oracle_port, f"{k}_rankdef"), (3, 6)):
            assert len(np.unique(rows[where], axis=0)) == d


@pytest.mark.parametrize("name", list(R.MEMBER_STORES))
def test_member_scene_is_a_fixed_point_after_one_fit(oracle_port, name):
    """at max_fits = 1 every member scene gives info == [m, m, 1, FIXED] and its inlier rows are exactly `where`: the members of the
    start model are known in advance, the one fit runs on exactly them, and its model is the output.  That holds for the two
    rank-deficient F sets and the repeated H sets too, at the seeds refit_ref._PICKED names.  The one exception is H on 4 rows: the
    reference's u2h at len == 4 (Htools.c:106-114, restated in oracle/dg_oracle.c u2h) transposes its 9 x 8 system as if it were 9 x 9
    and zeroes the last row, so its null vector is (0, ..., 0, 1) for ANY four rows, noise-free ones included; under that model no
    row is a member, the entry ends WORSE with the start model kept, and the 4-row fit shows in info and the mask only."""
    sc = R.gpu_scenes(oracle_port)[name]
    ref = R.reference(oracle_port, name, 1)
    for _, p, m, where, rows in _entries(oracle_port, name):
        b = sc["off"][p]
        if sc["model"] == "H" and m == 4:
            assert ref["info"][p].tolist() == [4, 4, 1, R.WORSE] and np.array_equal(ref["models"][p], sc["models"][p])
            assert R.fit(oracle_port, "H", rows, where).tolist() == [0.0] * 8 + [1.0]
        else:
            assert ref["info"][p].tolist() == [m, m, 1, R.FIXED], (p, m, ref["info"][p])
            assert ref["models"][p].tobytes() == R.fit(oracle_port, sc["model"], rows, where).tobytes()
        assert np.array_equal(np.flatnonzero(ref["inlier"][b:b + len(rows)]), where)
    assert np.array_equal(R.reference(oracle_port, name, 4)["info"], ref["info"])          # a fixed point stays one


K_F, K_H = 360.0, 2.9


def test_oracle_fit_is_the_plain_least_squares_model(oracle_port):
    """The oracle's u2f / u2h (R.fit) on every member set against R.plain_fit, an independent float64 numpy solution (Hartley
    normalisation, design matrix, np.linalg.svd, rank 2 by a second SVD, denormalisation), as sign-aligned relative Frobenius distance of
    the unit-norm models.  Oracle against numpy only: the device is never the yardstick.  The bound is k eps |N|_2 / (l8 - l9) of the
    9 x 9 normal matrix N of the design matrix the solver works on (normalised; raw for F on 8 rows): the first-order change of the
    eigenvector under a relative perturbation eps of N, and the oracle forms N.  Measured worst distance / (eps |N| / gap) over all scenes:
    F 45.0 (511 members; 40.1 at 256, 37.1 at 24 in the second step; the rank-2 step and the denormalisation to pixels are not in the
    first-order term), H 0.351 (257 members, normalised frame; 0.304 in the pixel frame); k is 8 x that, per model kind: 360 and 2.9.
    Left out: the rank-deficient scenes (the gap is 0 and the model is not determined) and H on 4 rows (the reference's 4-row u2h
    returns (0, ..., 0, 1), see test_member_scene_is_a_fixed_point_after_one_fit, which is no least-squares model)."""
    worst = {"F": 0.0, "H": 0.0}
    for name in R.MEMBER_STORES:
        if "rankdef" in name:
            continue
        for sc, p, m, where, rows in _entries(oracle_port, name):
            if sc["model"] == "H" and m == 4:
                continue
            N, Z = R.plain_fit(sc["model"], rows[where])
            d = R.aligned_rel_fro(R.fit(oracle_port, sc["model"], rows, where), N); gb = R.gap_bound(Z)
            worst[sc["model"]] = max(worst[sc["model"]], d / gb)
            assert d <= (K_F if sc["model"] == "F" else K_H) * gb, (name, p, m, d, gb, d / gb)
    print("worst distance / (eps |N| / gap):", worst)


def test_plain_fit_finds_a_planted_model():
    """the numpy reference itself: noise-free rows of a known F / H give that model back to 1e-9 (its own conventions are the drivers')"""
    for model in "FH":
        rows, _, gt = R._rows(model, 40, 5, ratio=1.0, sigma=0.0)
        assert R.aligned_rel_fro(R.plain_fit(model, rows)[0], gt) <= 1e-9, model


@pytest.mark.parametrize("name", ["F_members_0", "H_members_0"])
def test_a_wrong_order_or_a_missing_member_changes_the_bits(oracle_port, name):
    """teeth of the bit-level comparison: for every count of every solver variant (F 8, 9 .. 16, 17 .. 513; H 4, 5 .. 12, 13 .. 513) the
    oracle's fit on the members in reversed list order, and on the members without the last one, differs from the proper fit in at
    least one bit: a wrong summation order or an off-by-one gather cannot pass a comparison of bytes"""
    seen = {}
    for sc, p, m, where, rows in _entries(oracle_port, name):
        M = R.fit(oracle_port, sc["model"], rows, where)
        assert R.fit(oracle_port, sc["model"], rows, where[::-1]).tobytes() != M.tobytes(), (m, "reversed")
        assert R.fit(oracle_port, sc["model"], rows, where[:-1]).tobytes() != M.tobytes(), (m, "without the last")
        small = m <= (16 if sc["model"] == "F" else 12)
        seen[small] = seen.get(small, 0) + 1
    assert seen[True] >= 3 and seen[False] >= 3


def test_every_gpu_scene_keeps_its_margin(oracle_port):
    """no residual of any model the restatement visits lies within 1e-6 th of th, in any scene test_gpu_refit.py uses and at every max_fits
    it uses (the models of max_fits 0 and 1 are the first of those of 4)"""
    for name, sc in R.gpu_scenes(oracle_port).items():
        m = R.min_margin(oracle_port, sc, R.reference(oracle_port, name, 4))
        assert m > R.MARGIN, (name, m)
