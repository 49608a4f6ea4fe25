"""The relative pose from a homography without a device (include/mi_degensac.h mi_degensac_pose_h_lists*, matcher.homography_pose,
tensor_api.homography_pose_tensors, select_pose): every refusal of both C entry points with its message and its place in the order (each
comes back as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), K == 0 and cap == 0, the Python
keyword and shape checks, the restatement tests/pose_h_ref.py on exact planar scenes and pure rotations whose outcome is the generator's,
the edge of rotation_eps, a plane seen from behind, a reflection, a rank-2 matrix, three broken restatements that these scenes reject,
the margin that every scene of test_gpu_pose_h.py must have, and select_pose on a hand-written table."""
import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import pose_h_ref as Hr
from tests import pose_ref as R

EINVAL = -1
NAMES = ("dev", "host")


def _abi(which, K=2, cap=10, n_cams=4, cos_min=0.5, rot_eps=1e-3, null=()):
    """(rc, message) of one entry point; data pointers hold an address (never read: every call here is refused first) unless in `null`"""
    L = _lib.lib(); buf = np.zeros(64); addr = buf.ctypes.data
    P = lambda name: None if name in null else addr                    # noqa: E731
    head = (P("pts"), P("off"), None, P("H"), P("cams"), n_cams, None, K, cap, cos_min, rot_eps, 0)
    outs = (P("pose"), P("front"), P("info"), P("normal"), P("tod"), None, None, None, None, None, None)
    rc = L.mi_degensac_pose_h_lists_dev(*head, None, *outs) if which == "dev" else L.mi_degensac_pose_h_lists(*head, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and part in msg, (which, rc, msg)


def test_tile_constants_and_status_codes_are_mirrored():
    L = _lib.lib()
    assert L.mi_degensac_pose_h_tile(0) == _lib.POSE_H_STEP == 1024 and L.mi_degensac_pose_h_tile(1) == _lib.POSE_H_GRID == 256
    assert L.mi_degensac_pose_h_tile(2) == -1
    assert (_lib.POSE_OK, _lib.POSE_BAD_MODEL, _lib.POSE_BAD_CAMERA, _lib.POSE_TRUNCATED, _lib.POSE_EMPTY, _lib.POSE_ROTATION) == \
        (Hr.OK, Hr.BAD_MODEL, Hr.BAD_CAMERA, Hr.TRUNCATED, Hr.EMPTY, Hr.ROTATION) == tuple(range(6))


def test_refusals_and_their_order():
    _refused(b"n_entries", K=-1)
    _refused(b"cap < 0", cap=-1)
    _refused(b"0x3fffffff", cap=0x40000000)
    _refused(b"n_cams", n_cams=-1)
    for c in (float("nan"), 1.0000001, -1.5, float("inf")):
        _refused(b"cos_min", cos_min=c)
    for e in (float("nan"), -1e-300, -1.0, -float("inf")):
        _refused(b"rotation_eps", rot_eps=e)
    _refused(b"corr_offsets", null=("off",))
    _refused(b"corr_offsets", null=("off",), K=0, cap=0)
    _refused(b"H and cams", null=("H",))
    _refused(b"H and cams", null=("cams",))
    for name in ("pose", "info", "normal", "tod"):
        _refused(b"pose, info, normal and t_over_d", null=(name,))
    _refused(b"pts and front", null=("pts",))
    _refused(b"pts and front", null=("front",))
    # each refusal hides every later one
    later = ("off", "H", "pose", "pts")
    _refused(b"n_entries", K=-1, cap=-1, n_cams=-1, cos_min=2.0, rot_eps=-1.0, null=later)
    _refused(b"cap < 0", cap=-1, n_cams=-1, cos_min=2.0, rot_eps=-1.0, null=later)
    _refused(b"n_cams", n_cams=-1, cos_min=2.0, rot_eps=-1.0, null=later)
    _refused(b"cos_min", cos_min=2.0, rot_eps=-1.0, null=later)
    _refused(b"rotation_eps", rot_eps=-1.0, null=later)
    _refused(b"corr_offsets", null=later)
    _refused(b"H and cams", null=("H", "pose", "pts"))
    _refused(b"pose, info", null=("pose", "pts"))
    for e in (0.0, 1.0, float("inf")):                                 # allowed: refused later, for the pointer
        _refused(b"pts and front", rot_eps=e, null=("pts",))


def test_k0_and_cap0_succeed_without_a_device():
    for which in NAMES:
        rc, _ = _abi(which, K=0, cap=0, n_cams=0, null=("pts", "H", "cams", "pose", "front", "info", "normal", "tod"))
        assert rc == 0, which


# ---- the Python checks ----
def _np(K=2, cap=10):
    return np.zeros((cap, 4)), np.zeros(K + 1, np.int64), np.zeros((K, 3, 3)), np.ones((K, 8))


@pytest.mark.parametrize("kw, part", [
    (dict(min_parallax_deg=-1.0), "min_parallax_deg"), (dict(min_parallax_deg=float("nan")), "min_parallax_deg"),
    (dict(rotation_eps=-1e-9), "rotation_eps"), (dict(rotation_eps=float("nan")), "rotation_eps"), (dict(rotation_eps="x"), "rotation_eps"),
    (dict(rotation_eps=True), "rotation_eps"),
    (dict(cams2=np.ones((3, 4))), "cams2"), (dict(pairs=np.zeros((2, 2), np.int32)), "cams1"), (dict(pairs=np.zeros((3, 2), np.int32)), "pairs"),
    (dict(keep=np.zeros(9, bool)), "keep"), (dict(keep=np.zeros(10, np.int32)), "keep"),
])
def test_keyword_checks(kw, part):
    pts, off, M, cams = _np()
    with pytest.raises(ValueError, match=part):
        matcher.homography_pose(pts, off, M, cams, **kw)


def test_shape_and_dtype_checks():
    pts, off, M, cams = _np()
    chk = lambda a, b, c, d, **kw: matcher.check_pose_h_args(a.shape, a.dtype, b.shape, b.dtype, c.shape, c.dtype, d.shape, d.dtype, **kw)  # noqa: E731
    bad = [(pts[:, :3], off, M, cams, "pts"), (pts.astype(np.float32), off, M, cams, "pts"), (pts, off.astype(np.int32), M, cams, "corr_offsets"),
           (pts, off, M[:1], cams, "one homography per entry"), (pts, off, M.reshape(2, 9), cams, "models"),
           (pts, off, M.astype(np.float32), cams, "models"), (pts, off, M, cams[:1], "cams1"), (pts, off, M, cams.astype(np.float32), "cams1")]
    for a, b, c, d, part in bad:
        with pytest.raises(ValueError, match=part):
            chk(a, b, c, d)
    assert chk(pts, off, M, cams) == (2, 10, 2, None, R.cos_min(1.5), 1e-3)
    assert chk(pts, off, M, np.ones((5, 4)), pairs=((2, 2), np.dtype(np.int32)), rotation_eps=0) == (2, 10, 5, None, R.cos_min(1.5), 0.0)
    with pytest.raises(TypeError):
        matcher.homography_pose(pts, off, M, cams, px_th=1.0)


def test_tensor_call_wants_tensors():
    from pydegensac_amd import tensor_api
    pts, off, M, cams = _np()
    with pytest.raises(ValueError, match="torch tensors"):
        tensor_api.homography_pose_tensors(pts, off, M, cams)
    import torch
    with pytest.raises(ValueError, match="ROCm device"):
        tensor_api.homography_pose_tensors(*(torch.from_numpy(x) for x in (pts, off, M, cams)))
    with pytest.raises(ValueError, match="rotation_eps"):
        tensor_api.homography_pose_tensors(*(torch.from_numpy(x) for x in (pts, off, M, cams)), rotation_eps=-1.0)


# ---- the restatement on exact scenes ----
def _exact_scene(n=40, **kw):
    return Hr._scene([Hr.planar_entry(n, k, 50, **kw) for k in range(len(Hr.POSES))], 1.5)


def test_exact_planar_scenes_give_the_generators_pose():
    """all four candidates solve G = R + (t / d) n^T with R in SO(3) and |n| = 1; the chosen one is the generator's pose, normal and
    t / d to the 1e-9 of test_pose_cpu.py (the restatement alone: the figures it reaches are printed); every row is front; the runner-up
    is strictly below; the independent decomposition holds the same four"""
    sc = _exact_scene()
    out = Hr.from_candidates(sc)
    worst = 0.0
    for k in range(len(Hr.POSES)):
        c1, c2 = sc["cams"][2 * k], sc["cams"][2 * k + 1]
        dec = Hr.decompose(sc["H"][k], c1, c2)
        assert dec["status"] == Hr.OK
        G = dec["G"]
        for q in range(4):
            Rq = dec["cand"][q, :9].reshape(3, 3); tq = dec["cand"][q, 9:]; nq = dec["normal"][q]
            assert np.abs(G - (Rq + dec["tod"][q] * np.outer(tq, nq))).max() <= Hr.TOL
            assert np.abs(Rq @ Rq.T - np.eye(3)).max() <= Hr.TOL and abs(np.linalg.det(Rq) - 1) <= Hr.TOL
            assert abs(np.linalg.norm(nq) - 1) <= Hr.TOL and abs(np.linalg.norm(tq) - 1) <= Hr.TOL
        for q in range(2):                                             # the header's order
            assert np.array_equal(dec["cand"][q, :9], dec["cand"][q + 2, :9]) and np.array_equal(dec["cand"][q, 9:], -dec["cand"][q + 2, 9:])
            assert np.array_equal(dec["normal"][q], -dec["normal"][q + 2])
        Rg, tg, ng, todg = Hr.truth(k)
        err = max(np.abs(out["pose"][k, :9] - Rg.ravel()).max(), np.abs(out["pose"][k, 9:] - tg).max(), np.abs(out["normal"][k] - ng).max(),
                  abs(out["t_over_d"][k] - todg))
        worst = max(worst, err)
        assert err <= Hr.TOL, (k, err)
        used, front, second, wide, st = out["info"][k]
        assert st == Hr.OK and used == front == 40 and second < front, out["info"][k]
        b, e = sc["off"][k], sc["off"][k + 1]
        assert out["front"][b:e].all()
        st2, cd, nr, td = Hr.candidates_svd(sc["H"][k], c1, c2)
        assert st2 == Hr.OK and Hr.same_set(dec["cand"], dec["normal"], cd, nr)
        assert np.abs(np.linalg.norm(td, axis=1) - dec["tod"]).max() <= Hr.TOL
    print("largest error of the restatement against the generator:", worst)


def test_exact_rotations_and_the_edge_of_rotation_eps():
    for k in range(len(Hr.ROTS)):
        rows, H, c1, c2 = Hr.rotation_entry(30, k, 51)
        sc = Hr._scene([(rows, H, c1, c2)], 1.5)
        out = Hr.from_candidates(sc)
        assert out["info"][0].tolist() == [30, 30, 0, 0, Hr.ROTATION]
        assert np.abs(out["pose"][0, :9] - Hr.ROTS[k].ravel()).max() <= Hr.TOL and not out["pose"][0, 9:].any()
        assert not out["normal"].any() and not out["t_over_d"].any() and out["front"].all()
        assert np.isnan(out["X"]).all() and np.isnan(out["depth"]).all() and (out["cosang"] > 1 - 1e-12).all()
        st, cd, _, _ = Hr.candidates_svd(H, c1, c2)
        assert st == Hr.ROTATION and np.abs(cd[0] - out["pose"][0]).max() <= Hr.TOL
    c1, c2 = R.cam_of(0), R.cam_of(7)
    for ratio, want in ((0.999e-3, Hr.ROTATION), (1.001e-3, Hr.OK), (0.0, Hr.ROTATION)):
        H = Hr.near_rotation_h(ratio, c1, c2)[0]
        assert Hr.decompose(H, c1, c2)["status"] == want, ratio
        assert Hr.candidates_svd(H, c1, c2)[0] == want
    H = Hr.near_rotation_h(1e-6, c1, c2)[0]
    assert Hr.decompose(H, c1, c2, rotation_eps=0.0)["status"] == Hr.OK and Hr.decompose(H, c1, c2, rotation_eps=1.0)["status"] == Hr.ROTATION


def test_behind_reflection_and_rank_two():
    S = Hr.gpu_scenes()
    out = Hr.from_candidates(S["behind"])
    assert out["info"][0, 4] == Hr.OK and out["info"][0, 1] < out["info"][0, 0] and out["info"][1, 1] == out["info"][1, 0] == 40
    # a reflection (det < 0 as given) is the same homography: the same pose
    sc = _exact_scene()
    neg = dict(sc); neg["H"] = -sc["H"]
    a, b = Hr.from_candidates(sc), Hr.from_candidates(neg)
    assert np.abs(a["pose"] - b["pose"]).max() <= Hr.TOL and np.array_equal(a["info"], b["info"])
    assert all(np.linalg.det(Hr.decompose(neg["H"][k], sc["cams"][2 * k], sc["cams"][2 * k + 1])["G"]) > 0 for k in range(len(Hr.POSES)))
    # rank 2: a column of zeros stays zero under the rotations, sigma3 == 0
    m = Hr.from_candidates(S["models"])
    assert m["info"][:, 4].tolist() == [Hr.BAD_MODEL] * 3 + [Hr.OK] * 2 + [Hr.BAD_MODEL] + [Hr.OK] * 2
    assert not m["pose"][5].any() and not m["cand"][5].any()
    for k in (3, 4, 7):                                                # x 1e150, x 1e-150, x -1: the generator's pose all the same
        assert np.abs(m["pose"][k, :9] - Hr.truth(k)[0].ravel()).max() <= Hr.TOL and np.abs(m["pose"][k, 9:] - Hr.truth(k)[1]).max() <= Hr.TOL
    one = np.array([1.0, 1.0, 0.0, 0.0])
    assert Hr.decompose(np.array([[1.0, 2, 3], [4, 5, 6], [5, 7, 9]]), one, one)["status"] in (Hr.OK, Hr.BAD_MODEL)      # rank 2 to rounding: no error


@pytest.mark.parametrize("broken", ["unsorted", "unnormalised"])
def test_broken_decompositions_are_rejected(broken):
    """sigma left in column order and a t that is not normalised give a pose that is not the generator's"""
    sc = _exact_scene()
    out = Hr.from_candidates(sc, broken=broken)
    bad = 0
    for k in range(len(Hr.POSES)):
        Rg, tg, ng, _ = Hr.truth(k)
        err = max(np.abs(out["pose"][k, :9] - Rg.ravel()).max(), np.abs(out["pose"][k, 9:] - tg).max(), np.abs(out["normal"][k] - ng).max())
        if not (out["info"][k, 4] == Hr.OK and err <= Hr.TOL and out["info"][k, 2] < out["info"][k, 1]):
            bad += 1
    assert bad >= (len(Hr.POSES) if broken == "unnormalised" else 1), bad


def test_a_dropped_plane_side_test_is_rejected():
    """On a row of the plane lambda1 > 0 and n . d1 > 0 say the same (X = lambda1 d1 and n . X = d > 0), so exact scenes cannot see the
    plane-side test; a mismatched row can triangulate in front of both cameras on a ray that never meets the plane.  The scenes with
    outliers that test_gpu_pose_h.py compares bit for bit have such rows under the other solution's plane, which cuts their field of view:
    without the test the counts differ."""
    sc = Hr.gpu_scenes()["lengths"]
    a, b = Hr.from_candidates(sc), Hr.from_candidates(sc, broken="no_side")
    assert (b["info"][:, 2] >= a["info"][:, 2]).all() and (b["info"][:, 2] > a["info"][:, 2]).sum() >= 8          # the runner-up gains rows
    assert not np.array_equal(a["cand_front"], b["cand_front"])
    ex = _exact_scene()
    assert np.array_equal(Hr.from_candidates(ex)["front"], Hr.from_candidates(ex, broken="no_side")["front"])


def test_gpu_scenes_have_a_margin():
    """front > runner-up for every entry of every scene of test_gpu_pose_h.py that has a pose from a plane and at least 8 used rows"""
    seen = 0
    for name, sc in Hr.gpu_scenes().items():
        info = Hr.from_candidates(sc)["info"]
        for p in np.flatnonzero((info[:, 4] == Hr.OK) & (info[:, 0] >= 8)):
            assert info[p, 1] > info[p, 2], (name, p, info[p])
            seen += 1
    assert seen > 250
    st = set()
    for sc in Hr.gpu_scenes().values():
        st |= set(Hr.from_candidates(sc)["info"][:, 4].tolist())
    assert st == set(range(6))


def test_gpu_scenes_agree_with_the_independent_decomposition():
    for name, sc in Hr.gpu_scenes().items():
        K = len(sc["off"]) - 1
        for p in range(K):
            i1, i2 = Hr.cam_rows(sc, p)
            st, dec = Hr.entry_status(sc["H"][p], sc["cams"], i1, i2, 0, 0, 0, sc.get("rotation_eps", Hr.ROT_EPS))
            if dec is None:
                continue
            st2, cd, nr, _ = Hr.candidates_svd(sc["H"][p], sc["cams"][i1], sc["cams"][i2])
            if (name, p) == ("models", 6):                             # rank 2 to rounding: sigma3 is noise on both sides
                continue
            assert st == st2, (name, p, st, st2)
            if st == Hr.OK:
                assert Hr.same_set(dec["cand"], dec["normal"], cd, nr), (name, p)
            elif st == Hr.ROTATION:
                assert np.abs(dec["cand"][0] - cd[0]).max() <= Hr.TOL


def test_select_pose_on_a_table():
    K = 6
    cls = np.array([2, 2, 2, 1, 0, 2], np.int8)
    Rf = np.arange(K * 9, dtype=np.float64).reshape(K, 3, 3); Rh = -Rf - 1
    tf = np.arange(K * 3, dtype=np.float64).reshape(K, 3); th = -tf - 1
    off = np.array([0, 2, 4, 6, 8, 10, 12], np.int64)
    ff = np.array([1, 0] * 6, bool); fh = ~ff
    inf = np.array([[2, 1, 0, 1, Hr.OK]] * K, np.int32); inf[1, 4] = Hr.BAD_MODEL; inf[5, 4] = Hr.EMPTY
    inh = np.array([[2, 1, 1, 0, Hr.OK], [2, 1, 0, 0, Hr.ROTATION], [0, 0, 0, 0, Hr.BAD_MODEL], [2, 1, 1, 0, Hr.OK], [2, 1, 1, 0, Hr.OK],
                    [0, 0, 0, 0, Hr.EMPTY]], np.int32)
    Rs, ts, fs, ins, use_h, edge = matcher.select_pose(cls, (Rf, tf, ff, inf), (Rh, th, fh, inh), off)
    assert use_h.tolist() == [True, True, False, False, False, False]
    assert edge.tolist() == [True, True, True, True, True, False]
    for k in range(K):
        src = (Rh, th, inh) if use_h[k] else (Rf, tf, inf)
        assert np.array_equal(Rs[k], src[0][k]) and np.array_equal(ts[k], src[1][k]) and np.array_equal(ins[k], src[2][k])
        assert np.array_equal(fs[2 * k:2 * k + 2], (fh if use_h[k] else ff)[2 * k:2 * k + 2])
    assert matcher.select_pose(cls, (Rf, tf, ff, inf), (Rh, th, fh, inh))[2] is None
    with pytest.raises(ValueError, match="cls"):
        matcher.select_pose(cls[:5], (Rf, tf, ff, inf), (Rh, th, fh, inh))
    with pytest.raises(ValueError, match="corr_offsets"):
        matcher.select_pose(cls, (Rf, tf, ff, inf), (Rh, th, fh, inh), off[:-1])
