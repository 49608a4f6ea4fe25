"""The relative pose on exported correspondence lists without a device (include/mi_degensac.h mi_degensac_pose_lists*,
matcher.relative_pose, tensor_api.relative_pose_tensors): every refusal of both C entry points with its message and its place in the order
(each comes back as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), K == 0 and cap == 0, the
Python keyword and shape checks, the restatement tests/pose_ref.py on exact scenes whose outcome is the generator's own cameras, three
broken restatements that these scenes reject, the margin that every scene of test_gpu_pose.py must have, and pose_config."""
import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from pydegensac_amd import synthetic as syn
from tests import pose_ref as R

EINVAL = -1
NAMES = ("dev", "host")


def _abi(which, K=2, cap=10, n_cams=4, cos_min=0.5, null=()):
    """(rc, message) of one entry point; data pointers hold an address (never read: every call here is refused first) unless in `null`"""
    L = _lib.lib(); buf = np.zeros(64); addr = buf.ctypes.data
    P = lambda name: None if name in null else addr                    # noqa: E731
    head = (P("pts"), P("off"), None, P("F"), P("cams"), n_cams, None, K, cap, cos_min, 0)
    outs = (P("pose"), P("front"), P("info"), None, None, None, None, None)
    rc = L.mi_degensac_pose_lists_dev(*head, None, *outs) if which == "dev" else L.mi_degensac_pose_lists(*head, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and part in msg, (which, rc, msg)


def test_tile_constants_and_status_codes_are_mirrored():
    L = _lib.lib()
    assert L.mi_degensac_pose_tile(0) == _lib.POSE_STEP == 1024 and L.mi_degensac_pose_tile(1) == _lib.POSE_GRID == 256
    assert L.mi_degensac_pose_tile(2) == -1
    assert (_lib.POSE_OK, _lib.POSE_BAD_MODEL, _lib.POSE_BAD_CAMERA, _lib.POSE_TRUNCATED, _lib.POSE_EMPTY) == \
        (R.OK, R.BAD_MODEL, R.BAD_CAMERA, R.TRUNCATED, R.EMPTY) == tuple(range(5))


def test_refusals_and_their_order():
    _refused(b"n_entries", K=-1)
    _refused(b"cap < 0", cap=-1)
    _refused(b"0x3fffffff", cap=0x40000000)
    _refused(b"n_cams", n_cams=-1)
    for c in (float("nan"), 1.0000001, -1.5, float("inf")):
        _refused(b"cos_min", cos_min=c)
    _refused(b"corr_offsets", null=("off",))
    _refused(b"corr_offsets", null=("off",), K=0, cap=0)
    _refused(b"F and cams", null=("F",))
    _refused(b"F and cams", null=("cams",))
    _refused(b"pose and info", null=("pose",))
    _refused(b"pose and info", null=("info",))
    _refused(b"pts and front", null=("pts",))
    _refused(b"pts and front", null=("front",))
    # each refusal hides every later one
    _refused(b"n_entries", K=-1, cap=-1, n_cams=-1, cos_min=2.0, null=("off", "F", "pose", "pts"))
    _refused(b"cap < 0", cap=-1, n_cams=-1, cos_min=2.0, null=("off", "F", "pose", "pts"))
    _refused(b"n_cams", n_cams=-1, cos_min=2.0, null=("off", "F", "pose", "pts"))
    _refused(b"cos_min", cos_min=2.0, null=("off", "F", "pose", "pts"))
    _refused(b"corr_offsets", null=("off", "F", "pose", "pts"))
    _refused(b"F and cams", null=("F", "pose", "pts"))
    _refused(b"pose and info", null=("pose", "pts"))
    for c in (-1.0, 1.0, 0.0):                                         # the closed ends are allowed: refused later, for the pointer
        _refused(b"pts and front", cos_min=c, null=("pts",))


def test_k0_and_cap0_succeed_without_a_device():
    for which in NAMES:
        rc, _ = _abi(which, K=0, cap=0, n_cams=0, null=("pts", "F", "cams", "pose", "front", "info"))
        assert rc == 0, which


# ---- the Python checks ----
def _np(K=2, cap=10):
    return np.zeros((cap, 4)), np.zeros(K + 1, np.int64), np.zeros((K, 3, 3)), np.ones((K, 8))


@pytest.mark.parametrize("kw, part", [
    (dict(min_parallax_deg=-1.0), "min_parallax_deg"), (dict(min_parallax_deg=181), "min_parallax_deg"), (dict(min_parallax_deg="x"), "min_parallax_deg"),
    (dict(min_parallax_deg=float("nan")), "min_parallax_deg"), (dict(min_parallax_deg=True), "min_parallax_deg"),
    (dict(cams2=np.ones((3, 4))), "cams2"), (dict(pairs=np.zeros((2, 2), np.int32)), "cams1"), (dict(pairs=np.zeros((3, 2), np.int32)), "pairs"),
    (dict(pairs=np.zeros((2, 2))), "pairs"), (dict(keep=np.zeros(9, bool)), "keep"), (dict(keep=np.zeros(10, np.int32)), "keep"),
])
def test_keyword_checks(kw, part):
    pts, off, M, cams = _np()
    with pytest.raises(ValueError, match=part):
        matcher.relative_pose(pts, off, M, cams, **kw)


def test_shape_and_dtype_checks():
    pts, off, M, cams = _np()
    table = np.ones((5, 4)); pr = ((2, 2), np.dtype(np.int32))
    chk = lambda a, b, c, d, **kw: matcher.check_pose_args(a.shape, a.dtype, b.shape, b.dtype, c.shape, c.dtype, d.shape, d.dtype, **kw)  # noqa: E731
    bad = [(pts[:, :3], off, M, cams, "pts"), (pts.astype(np.float32), off, M, cams, "pts"), (pts.ravel(), off, M, cams, "pts"),
           (pts, off.astype(np.int32), M, cams, "corr_offsets"), (pts, off.reshape(1, -1), M, cams, "corr_offsets"), (pts, off[:0], M, cams, "corr_offsets"),
           (pts, off, M[:1], cams, "models"), (pts, off, M.reshape(2, 9), cams, "models"), (pts, off, M.astype(np.float32), cams, "models"),
           (pts, off, M, cams[:1], "cams1"), (pts, off, M, cams[:, :4], "cams1"), (pts, off, M, cams.astype(np.float32), "cams1")]
    for a, b, c, d, part in bad:
        with pytest.raises(ValueError, match=part):
            chk(a, b, c, d)
    with pytest.raises(ValueError, match="cams2"):
        chk(pts, off, M, table, pairs=pr, cams2=((3, 5), np.dtype(np.float64)))
    with pytest.raises(ValueError, match="cams2"):
        chk(pts, off, M, table, pairs=pr, cams2=((3, 4), np.dtype(np.float32)))
    assert chk(pts, off, M, cams) == (2, 10, 2, None, R.cos_min(1.5))
    assert chk(pts, off, M, table, pairs=pr, min_parallax_deg=0) == (2, 10, 5, None, 1.0)
    assert chk(pts, off, M, table, pairs=pr, cams2=((3, 4), np.dtype(np.float64)), keep=((10,), np.dtype(bool)), min_parallax_deg=180)[:4] == (2, 10, 5, 3)


def test_tensor_call_wants_tensors():
    from pydegensac_amd import tensor_api
    pts, off, M, cams = _np()
    with pytest.raises(ValueError, match="torch tensors"):
        tensor_api.relative_pose_tensors(pts, off, M, cams)
    import torch
    with pytest.raises(ValueError, match="ROCm device"):
        tensor_api.relative_pose_tensors(*(torch.from_numpy(x) for x in (pts, off, M, cams)))


# ---- the generator's cameras ----
def test_collection_cameras_are_the_ones_image_collection_projects_with():
    """noise-free keypoints of two images that show the same cloud point satisfy x2^T F x1 = 0 for the F of collection_cameras"""
    m = 5
    K, poses = syn.collection_cameras(m)
    kps, descs = syn.image_collection(m=m, n=200, inlier_ratio=1.0, sigma=0.0, dim=8, seed=4, desc_sigma=0.0)
    cam = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    assert cam.tolist() == [syn.FOCAL, syn.FOCAL, syn.IMG_W / 2, syn.IMG_H / 2] and len(poses) == m
    for i, j in ((0, 4), (3, 1)):
        Rr, t = R.relative(poses, i, j)
        F = R.f_from_pose(Rr, t, cam, cam); F /= np.linalg.norm(F)
        d = np.abs(descs[i][:, None, :] - descs[j][None, :, :]).sum(2)          # desc_sigma = 0: the same cloud point has the same descriptor
        match = d.argmin(1)
        assert (d.min(1) == 0).all()
        x1 = np.concatenate([kps[i], np.ones((200, 1))], 1); x2 = np.concatenate([kps[j][match], np.ones((200, 1))], 1)
        r = np.abs(np.einsum("ni,ij,nj->n", x2, F, x1)) / (np.linalg.norm(x1, axis=1) * np.linalg.norm(x2, axis=1))
        assert r.max() < 1e-12, (i, j, r.max())
    again, _ = syn.image_collection(m=m, n=200, inlier_ratio=1.0, sigma=0.0, dim=8, seed=4, desc_sigma=0.0)
    assert all(np.array_equal(a, b) for a, b in zip(kps, again))


# ---- the restatement on exact scenes ----
@pytest.mark.parametrize("i, j", R.PAIRS)
def test_exact_scene_gives_the_generators_pose(i, j):
    """F from collection_cameras, noise-free rows: the chosen pose is the ground truth to 1e-9, every row is front, the runner-up has none"""
    rows, F, Rg, tg, ci, cj = R.pair_rows(50, i, j, 31)
    sc = R._scene([(rows, F * 7.5, ci, cj)], 1.5)
    ref = R.reference(sc)
    assert ref["info"][0, :3].tolist() == [50, 50, 0] and ref["info"][0, 4] == R.OK and ref["front"].all()
    assert np.abs(ref["pose"][0, :9].reshape(3, 3) - Rg).max() <= R.TOL and np.abs(ref["pose"][0, 9:] - tg).max() <= R.TOL
    # the midpoint of exact rays is the point itself: X in the frame of camera i reprojects onto the rows
    X = ref["X"]; x = X[:, :2] / X[:, 2:3] * ci[:2] + ci[2:]
    assert np.abs(x - rows[:, :2]).max() < 1e-9 and (ref["depth"] > 0).all() and (ref["cosang"] < 1).all()
    assert np.abs(ref["depth"][:, 0] - X[:, 2]).max() < 1e-9


def test_pure_rotation_has_no_wide_row():
    """two views from one centre: whatever candidate is given, the rays of a row are parallel and no row is wide"""
    rng = np.random.default_rng(5)
    a = 0.3; Rg = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    cam = R.cam_of(0, False); X = np.stack([rng.uniform(-2, 2, 60), rng.uniform(-1.5, 1.5, 60), rng.uniform(4, 8, 60)], 1)
    rows = np.concatenate([syn._project(R.kmat(cam), np.eye(3), np.zeros(3), X), syn._project(R.kmat(cam), Rg, np.zeros(3), X)], 1)
    sc = R._scene([(rows, np.eye(3), cam, cam)], 1.5)
    for t in ([1.0, 0, 0], [0, 0.6, 0.8]):
        cand = np.array([np.concatenate([Rg.ravel(), s * np.array(t)]) for s in (1, -1, 1, -1)])
        ref = R.from_candidates(sc, [cand])
        assert ref["info"][0, 0] == 60 and ref["info"][0, 3] == 0 and (ref["cosang"] > R.cos_min(0.001)).all()
    assert matcher.pose_config(ref["info"]).tolist() == [2]


def test_broken_restatements_are_rejected():
    """`>=` for `>`: the exact scene's row 0 has lambda1 = lambda2 = 0; F^T for F and the cameras swapped: the pose of an exact scene is no
    longer the generator's"""
    sc = R.exact_scene()
    cand = np.array([np.concatenate([np.eye(3).ravel(), s * np.array([1.0, 0, 0])]) for s in (1, -1)] +
                    [np.concatenate([np.diag([1.0, -1, -1]).ravel(), s * np.array([1.0, 0, 0])]) for s in (1, -1)])
    good = R.from_candidates(sc, [cand]); ge = R.from_candidates(sc, [cand], "ge")
    assert good["depth"][0].tolist() == [0.0, 0.0] and not good["front"][0] and ge["front"][0]
    assert good["info"][0].tolist() == [30, 28, 0, 28, R.OK] and ge["info"][0, 1] == 29
    l1, l2, cs, X, den = R.rows_rule(cand[0], sc["cams"][0], sc["cams"][1], sc["pts"])
    assert den[1] == 0.0 and not good["front"][1] and not (good["depth"][1] > 0).any()          # den == 0: what IEEE division gives
    assert R.same_set(R.svd_candidates_of(sc)[0], cand)
    rows, F, Rg, tg, ci, cj = R.pair_rows(50, 6, 3, 32)
    sc = R._scene([(rows, F, ci, cj)], 1.5)
    for broken in ("Ft", "swap"):
        ref = R.reference(sc, broken)
        err = max(np.abs(ref["pose"][0, :9].reshape(3, 3) - Rg).max(), np.abs(ref["pose"][0, 9:] - tg).max())
        assert err > 1e-3, (broken, err)
    assert np.abs(R.reference(sc)["pose"][0, 9:] - tg).max() <= R.TOL


def _all_scenes():
    return dict(R.gpu_scenes(), decomposition_edges=R.edge_scene())


def test_decomposition_restated_agrees_with_numpys_svd():
    """pose_ref.decompose, which test_gpu_pose.py demands bit for bit, on every entry of its scenes: the same four candidates as
    numpy's SVD to TOL, the header's slot order, c2 = -R^T t; BAD_MODEL exactly where the independent status says so or the rank is below 2"""
    n = 0
    for name, sc in _all_scenes().items():
        for p, (d, s) in enumerate(zip(R.decompose_scene(sc), R.svd_candidates_of(sc))):
            if d is None:
                continue
            if d["status"] != R.OK:
                assert not d["cand"].any() and (s is None or (name, p) == ("decomposition_edges", 6)), (name, p)
                continue
            n += 1
            assert s is not None and R.same_set(d["cand"], s), (name, p)
            c = d["cand"]
            assert np.array_equal(c[0, :9], c[1, :9]) and np.array_equal(c[2, :9], c[3, :9]) and np.array_equal(c[0, 9:], -c[1, 9:])
            assert np.array_equal(c[0, 9:], c[2, 9:]) and np.array_equal(c[2, 9:], -c[3, 9:])
            for q in range(4):
                assert np.abs(d["c2"][q] + c[q, :9].reshape(3, 3).T @ c[q, 9:]).max() < 1e-15
    assert n > 350


def test_decomposition_edges_are_what_they_claim():
    sc = R.edge_scene(); dec = dict(zip(R.EDGES, R.decompose_scene(sc)))
    assert np.diff(sc["off"]).tolist() == [1] * 7 and len(R.EDGES) == 7
    E = {k: sc["F"][i].reshape(3, 3) for i, k in enumerate(R.EDGES)}
    assert [dec[k]["status"] for k in R.EDGES] == [R.OK] * 6 + [R.BAD_MODEL] and not dec["rank1"]["cand"].any()
    assert round(np.linalg.det(E["rank2"])) == 0 and np.abs(E["rank2"]).max() == 8 and np.array_equal(E["rank2"], np.round(E["rank2"]))
    assert np.array_equal(E["equal_sigma"] @ E["equal_sigma"].T @ E["equal_sigma"], 729.0 * E["equal_sigma"])          # E E^T E = sigma^2 E, in integers
    assert not dec["diagonal"]["rotated"] and all(dec[k]["rotated"] for k in R.EDGES if k != "diagonal")
    assert dec["negative_det"]["det"][0] < 0 and dec["tiny"]["det"][0] > 0
    assert np.abs(sc["F"][4]).max() < 1e-150 and np.abs(sc["F"][5]).max() > 1e140
    assert dec["tiny"]["cand"].tobytes() != dec["huge"]["cand"].tobytes() and R.same_set(dec["tiny"]["cand"], dec["huge"]["cand"])
    assert np.linalg.matrix_rank(E["rank1"]) == 1 and E["rank1"].all()


def test_reordered_jacobi_is_rejected_by_the_bits_only():
    """a Jacobi rule that takes the column pairs of a sweep as (0 1) (1 2) (0 2) converges as the header's does: on every entry of every
    scene its candidates are numpy's to TOL, which is all that the comparison with the SVD asks.  The bitwise comparison of
    test_candidates_equal_restatement rejects it in every scene that has an entry with a rotation to apply."""
    for name, sc in _all_scenes().items():
        good = R.decompose_scene(sc); bad = R.decompose_scene(sc, "order"); svd = R.svd_candidates_of(sc)
        differ = 0
        for g, b, s in zip(good, bad, svd):
            if g is None or g["status"] != R.OK:
                assert g is None or not b["cand"].any()
                continue
            assert b["status"] == R.OK and R.same_set(b["cand"], s), name
            differ += g["cand"].tobytes() != b["cand"].tobytes()
        assert differ > 0 or name == "exact", name          # (the exact scene's E is [t]x of a unit axis: nothing to rotate)
    sc = R.gpu_scenes()["lengths"]
    assert all(g["cand"].tobytes() != b["cand"].tobytes() for g, b in zip(R.decompose_scene(sc), R.decompose_scene(sc, "order")))


def test_every_gpu_scene_entry_with_a_pose_has_a_clear_winner():
    """every entry of every scene of test_gpu_pose.py that has a pose and at least 8 used rows has front > runner-up in the restatement:
    the condition under which the GPU tests compare the chosen pose.  No such entry is left out: the assertion runs over all of them, and
    each scene must hold at least one (all but the scene that is made of refused cameras and one good entry holds several)."""
    for name, sc in R.gpu_scenes().items():
        info = R.reference(sc)["info"]
        sel = (info[:, 4] == R.OK) & (info[:, 0] >= 8)
        assert sel.any() or name == "nonessential", name          # (six random rows per entry there: its models fit no rows)
        assert (info[sel, 1] > info[sel, 2]).all(), (name, info[sel & (info[:, 1] <= info[:, 2])])


def test_scene_catalogue_holds_the_edges():
    S = R.gpu_scenes()
    assert np.diff(S["lengths"]["off"]).tolist() == R.LENGTHS == [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
    assert S["lengths"]["off"][0] == 3 and len(S["lengths"]["pts"]) == S["lengths"]["off"][-1] + 5
    assert len(S["many"]["off"]) - 1 == 300 > _lib.POSE_GRID and (S["many"]["idx"] == 0).any(axis=1).sum() == 112
    k = S["keep"]; b = int(k["off"][1])
    assert np.flatnonzero(k["keep"][b:b + 1100]).min() >= 1024 + 64 and np.diff(k["off"]).tolist() == [0, 1100, 0, 700, 90, 0]
    b = int(k["off"][3]); w = np.flatnonzero(k["keep"][b:b + 700]) // 64
    assert w.tolist() == list(range(11)) and not k["keep"][int(k["off"][4]):].any()
    st = lambda n: R.reference(S[n])["info"][:, 4].tolist()          # noqa: E731
    assert st("offsets") == [R.OK, R.TRUNCATED, R.TRUNCATED, R.TRUNCATED, R.OK]
    assert st("models") == [R.BAD_MODEL] * 3 + [R.OK] * 3 and st("cameras") == [R.BAD_CAMERA] * 5 + [R.OK]
    assert st("keep") == [R.EMPTY, R.OK, R.EMPTY, R.OK, R.EMPTY, R.EMPTY]
    seen = {s for n in S for s in st(n)}
    assert seen == {R.OK, R.BAD_MODEL, R.BAD_CAMERA, R.TRUNCATED, R.EMPTY}
    mix = R.reference(S["lengths"])["info"]
    assert ((mix[:, 3] > 0) & (mix[:, 3] < mix[:, 1])).any() and (mix[:, 2] > 0).any()          # wide is a proper subset somewhere


def test_scaled_models_have_the_same_candidates():
    sc = R.gpu_scenes()["models"]
    for p in (3, 4):
        unscaled = R.candidates_svd(sc["F"][p] * (1e-150 if p == 3 else 1e150), sc["cams"][2 * p], sc["cams"][2 * p + 1])
        assert R.same_set(R.candidates_svd(sc["F"][p], sc["cams"][2 * p], sc["cams"][2 * p + 1]), unscaled)


def test_nonessential_fixtures_are_what_they_claim(tmp_path):
    """the three matrices of pose_ref.NONORTH_F: rank 2, sigma2 well below sigma1, and the reference's 3 x 3 routine (csrc/dg_mat3.h,
    compiled for the host as tests/test_mat3_cpu.py does) returns a V on them that is not orthogonal, while numpy's candidates are
    rotations: a decomposition must not rest on that V"""
    import ctypes as C
    import os
    import subprocess
    out = str(tmp_path / "libmat3_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mat3_host.cpp"),
                           "-o", out])
    host = C.CDLL(out); dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))          # noqa: E731
    one = np.array([1.0, 1.0, 0.0, 0.0])
    for F in R.NONORTH_F:
        A = np.array(F).reshape(3, 3); s = np.linalg.svd(A, compute_uv=False)
        assert np.abs(A).max() == 1.0 and s[2] < 1e-15 and 0.04 < s[1] / s[0] < 0.2
        w = A.ravel().copy(); v = np.zeros(9); d = np.zeros(3)
        host.t_svd3_right(dp(w), dp(v), dp(d)); V = v.reshape(3, 3)
        assert np.abs(V.T @ V - np.eye(3)).max() > 1e-2
        Rs = R.candidates_svd(A, one, one)[:, :9].reshape(4, 3, 3)
        assert np.abs(Rs @ Rs.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    assert R.reference(R.gpu_scenes()["nonessential"])["info"][:, 4].tolist() == [R.OK] * 3


def test_pose_config_table_and_its_strict_edges():
    info = np.array([[100, 50, 3, 1, R.OK],        # front == 0.5 used: supported (strict <); one wide row: parallax
                     [100, 49, 3, 9, R.OK],        # front < 0.5 used: undecided
                     [100, 90, 3, 0, R.OK],        # no wide row: panoramic
                     [100, 10, 3, 0, R.OK],        # no wide row wins over a weak pose
                     [0, 0, 0, 0, R.EMPTY], [0, 0, 0, 0, R.BAD_MODEL], [0, 0, 0, 0, R.BAD_CAMERA], [0, 0, 0, 0, R.TRUNCATED]], np.int32)
    assert matcher.pose_config(info).tolist() == [1, 0, 2, 2, 0, 0, 0, 0]
    assert matcher.pose_config(info, min_front_ratio=0.49).tolist()[:2] == [1, 1]
    edge = np.array([[100, 80, 0, 8, R.OK], [100, 80, 0, 9, R.OK]], np.int32)
    assert matcher.pose_config(edge, min_wide_ratio=0.1).tolist() == [2, 1]          # wide == 0.1 front is still panoramic (<=)
    assert matcher.pose_config(edge, min_front_ratio=0.8, min_wide_ratio=0.0).tolist() == [1, 1]
    assert matcher.pose_config(edge, min_front_ratio=0.81).tolist() == [0, 0]
    assert matcher.pose_config(np.zeros((0, 5), np.int32)).dtype == np.int8
    for bad in (np.zeros((2, 4), np.int32), np.zeros((2, 5)), np.zeros(5, np.int32)):
        with pytest.raises(ValueError, match="info"):
            matcher.pose_config(bad)
