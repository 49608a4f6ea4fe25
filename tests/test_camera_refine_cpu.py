"""The refinement of camera poses against tracks without a device (include/mi_degensac.h mi_degensac_camera_refine_tracks*,
matcher.refine_cameras, tensor_api.refine_cameras_tensors): every refusal of both C entry points with its message and its place in the
order (each comes back as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), the zero sizes, the
Python keyword, shape and dtype checks, and the restatement tests/camera_refine_ref.py itself: its Jacobian against central differences
of its own residual through its own update, exact and noisy scenes, every status on a scene written by hand, the order of the sums and
the image-major table on numbers written by hand, four broken restatements that these tests reject, and the scene invariant."""
import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import camera_refine_ref as Q

EINVAL = -1
NAMES = ("dev", "host")
ALL = ("off", "obs", "kps", "X", "cams", "out")
# Noise-free scenes, the largest |pose entry - generator's| after the restatement's run: measured 1.24e-14 over the scenes of
# test_exact_scenes_end_at_the_generators_pose (worst: an image of 3 observations, a square system whose conditioning amplifies the
# rounding of the keypoints), and 1.16e-14 between the restatement and an independent Gauss-Newton (numpy.linalg.solve, exponential map,
# no damping) on the same scenes.  The bound is that figure times 80: both runs stop at a cost of some 1e-25 px^2, where the last step is
# rounding noise of either method.
BOUND = 1e-12


def _abi(which, T=2, M=10, rows=7, n_images=3, trials=20, ftol=1e-12, null=()):
    """(rc, message) of one entry point; data pointers hold an address (never read: every call here is refused first) unless in `null`"""
    L = _lib.lib(); buf = np.zeros(64); addr = buf.ctypes.data
    A = lambda name: None if name in null else addr                    # noqa: E731
    mid = (A("kps"), rows, A("cams"), A("cams"), n_images, A("X"), None, None, T, M, trials, ftol, 0)
    outs = (A("out"), A("out"), A("out"), None, None, None)
    if which == "dev":
        rc = L.mi_degensac_camera_refine_tracks_dev(A("off"), A("obs"), A("obs"), None, *mid, None, *outs)
    else:
        rc = L.mi_degensac_camera_refine_tracks(A("off"), A("obs"), A("obs"), -1, *mid, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and part in msg, (which, rc, msg)


def test_tile_constants_and_status_codes_are_mirrored():
    L = _lib.lib()
    assert [L.mi_degensac_camera_refine_tile(i) for i in range(4)] == [_lib.CAMREF_STEP, _lib.CAMREF_GRID, _lib.CAMREF_GROUP, -1]
    assert (_lib.CAMREF_CONVERGED, _lib.CAMREF_STALLED, _lib.CAMREF_MAX_TRIALS, _lib.CAMREF_FIXED, _lib.CAMREF_BEHIND, _lib.CAMREF_NOT_FINITE,
            _lib.CAMREF_SHORT, _lib.CAMREF_BAD_POSE, _lib.CAMREF_BAD_CAMERA) == \
        (Q.CONVERGED, Q.STALLED, Q.MAX_TRIALS, Q.FIXED, Q.BEHIND, Q.NOT_FINITE, Q.SHORT, Q.BAD_POSE, Q.BAD_CAMERA) == tuple(range(9))


def test_refusals_and_their_order():
    nan = float("nan")
    _refused(b"n_tracks_max < 0", T=-1)
    _refused(b"too many tracks", T=0x40000000)
    _refused(b"n_obs_max < 0", M=-1)
    _refused(b"too many observations", M=0x40000000)
    for r in (-1, 0x80000000):
        _refused(b"rows", rows=r)
    _refused(b"n_images", n_images=-1)
    for m in (-1, 101, 1 << 20):
        _refused(b"max_trials", trials=m)
    for f in (nan, -1e-300, -1.0):
        _refused(b"ftol", ftol=f)
    _refused(b"track_offsets", null=("off",))
    _refused(b"track_offsets", null=("off",), T=0, M=0, n_images=0)
    _refused(b"obs and obs_image", null=("obs",))
    _refused(b"NULL argument: kps", null=("kps",))
    _refused(b"NULL argument: X", null=("X",))
    _refused(b"cams and poses", null=("cams",))
    _refused(b"poses_out, cost and info", null=("out",))
    # each refusal hides every later one
    bad = dict(M=-1, rows=-1, n_images=-1, trials=-1, ftol=nan, null=ALL)
    order = [("T", b"n_tracks_max < 0"), ("M", b"n_obs_max < 0"), ("rows", b"rows"), ("n_images", b"n_images"), ("trials", b"max_trials"), ("ftol", b"ftol")]
    kw = dict(bad, T=-1)
    for key, part in order:
        _refused(part, **kw)
        kw.pop(key)                                                    # (the default of the key is a good value)
    for i, part in enumerate((b"track_offsets", b"obs and obs_image", b"NULL argument: kps", b"NULL argument: X", b"cams and poses",
                              b"poses_out, cost and info")):
        _refused(part, null=ALL[i:])
    for m, f in ((0, 0.0), (100, float("inf"))):                       # the closed ends are allowed: refused later
        _refused(b"cams and poses", trials=m, ftol=f, null=("cams",))
    # nothing is asked of a table that is empty
    _refused(b"cams and poses", M=0, null=("obs", "cams"))
    _refused(b"cams and poses", rows=0, null=("kps", "cams"))
    _refused(b"cams and poses", T=0, null=("X", "cams"))


def test_all_sizes_zero_succeed_without_a_device():
    for which in NAMES:
        rc, _ = _abi(which, T=0, M=0, rows=0, n_images=0, null=ALL[1:])
        assert rc == 0, which


# ---- the Python checks ----
def _np(T=2, M=10, rows=7, n=3):
    return (np.zeros(T + 1, np.int64), np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros((rows, 2)), np.ones((n, 4)), np.zeros((n, 3, 3)),
            np.zeros((n, 3)), np.zeros((T, 3)))


@pytest.mark.parametrize("kw, part", [
    (dict(max_trials=-1), "max_trials"), (dict(max_trials=101), "max_trials"), (dict(max_trials=2.0), "max_trials"), (dict(max_trials=True), "max_trials"),
    (dict(ftol=-1e-9), "ftol"), (dict(ftol=float("nan")), "ftol"), (dict(ftol="x"), "ftol"), (dict(ftol=True), "ftol"),
    (dict(n_tracks=1.5), "n_tracks"), (dict(n_tracks=True), "n_tracks"), (dict(max_iters=3), "unknown keyword 'max_iters'"),
    (dict(with_obs=True), "unknown keyword 'with_obs'"), (dict(obs_keep=np.zeros(9, np.uint8)), "obs_keep"), (dict(obs_keep=np.zeros(10, np.int32)), "obs_keep"),
    (dict(refine=np.zeros(4, bool)), "refine should"), (dict(refine=np.zeros(3)), "refine should"), (dict(refine=np.zeros((3, 1), np.uint8)), "refine should"),
])
def test_keyword_checks(kw, part):
    with pytest.raises(ValueError, match=part):
        matcher.refine_cameras(*_np(), **kw)


def test_shape_and_dtype_checks():
    a = _np()
    chk = lambda *v, **kw: matcher.check_camera_refine_args(*[x for y in v for x in (y.shape, y.dtype)], **kw)          # noqa: E731
    assert chk(*a) == (2, 10, 7, 3, 20, 1e-12)
    assert chk(*a, obs_keep=((10,), np.dtype(bool)), refine=((3,), np.dtype(np.uint8)), max_trials=0, ftol=0) == (2, 10, 7, 3, 0, 0.0)

    def swap(i, x):
        return a[:i] + (x,) + a[i + 1:]
    bad = [(swap(0, a[0].astype(np.int32)), "track_offsets"), (swap(1, a[1].astype(np.int64)), "obs should"), (swap(2, a[2][:9]), "obs_image"),
           (swap(3, a[3].astype(np.float32)), "kps"), (swap(3, a[3][:, :1]), "kps"), (swap(4, a[4][:, :3]), "cams"), (swap(5, a[5][:2]), "R should"),
           (swap(6, a[6].astype(np.float32)), "t should"), (swap(7, a[7][:1]), "X should"), (swap(7, a[7].astype(np.float32)), "X should"),
           (swap(7, np.zeros((2, 4))), "X should"), (swap(7, np.zeros(6)), "X should")]
    for args, part in bad:
        with pytest.raises(ValueError, match=part):
            chk(*args)
    with pytest.raises(ValueError, match="n_tracks"):
        chk(*a, n_tracks=((2,), np.dtype(np.int64)))


def test_tensor_form_refuses_before_a_device_is_needed():
    import torch
    from pydegensac_amd import tensor_api as T
    a = _np()
    with pytest.raises(ValueError, match="unknown keyword 'with_obs'"):
        T.refine_cameras_tensors(*a, with_obs=True)
    with pytest.raises(ValueError, match="must be torch tensors"):
        T.refine_cameras_tensors(*a)
    t = [torch.from_numpy(x) for x in a]
    with pytest.raises(ValueError, match="must be torch tensors"):
        T.refine_cameras_tensors(*t, refine=np.ones(3, np.uint8))
    with pytest.raises(ValueError, match="X should"):
        T.refine_cameras_tensors(*t[:7], t[7].float())
    with pytest.raises(ValueError, match="obs_keep"):
        T.refine_cameras_tensors(*t, obs_keep=torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="max_trials"):
        T.refine_cameras_tensors(*t, max_trials=101)
    with pytest.raises(ValueError, match="same ROCm device"):
        T.refine_cameras_tensors(*t)


# ---- the restatement ----
def _image(sc, m):
    io, iobs, tof = Q.table(sc)
    pos = iobs[io[m]:io[m + 1]].astype(np.int64)
    return Q.image_obs(sc, pos, tof), len(pos)


def _jacobian_mismatch(broken=None):
    """the largest |central difference of the residual through update() - Jacobian entry|, relative to the largest entry of its column"""
    sc = Q.gpu_scenes()["empty"]
    worst = 0.0
    for m in (2, 6):
        o, n = _image(sc, m)
        pose = sc["poses"][m]; cam = sc["cams"][m]
        rx, ry, zc, jx, jy = Q.jacobian(o, pose, cam)
        h = 1e-6
        for k in range(6):
            d = np.zeros(6); d[k] = h
            _, _, _, _, rxp, ryp = Q.project(o, Q.update(pose, list(d), broken), cam)
            _, _, _, _, rxm, rym = Q.project(o, Q.update(pose, list(-d), broken), cam)
            for num, ana in (((rxp - rxm) / (2 * h), jx[k]), ((ryp - rym) / (2 * h), jy[k])):
                worst = max(worst, float(np.abs(num[:n] - ana[:n]).max() / max(1.0, np.abs(ana[:n]).max())))
    return worst


def test_jacobian_against_central_differences_through_the_update():
    """central differences of a residual of some 10 px with h = 1e-6: the truncation h^2 |J'''| and the rounding 1e-16 * 1e3 / h both lie
    far below 1e-5 of the largest entry of a column (some 1e3)"""
    assert _jacobian_mismatch() <= 1e-5


def _gauss_newton(sc, m, iters=30):
    """an independent float64 Gauss-Newton on image m: numpy.linalg.solve on J^T J, the exponential map on the left, no damping"""
    io, iobs, tof = Q.table(sc)
    pos = iobs[io[m]:io[m + 1]]
    x = sc["kps"][sc["obs"][pos]]; X = sc["X"][tof[pos]]
    fx, fy, cx, cy = sc["cams"][m]
    R = sc["poses"][m, :9].reshape(3, 3).copy(); t = sc["poses"][m, 9:].copy()
    for _ in range(iters):
        Xc = X @ R.T + t; P = X @ R.T
        r = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx - x[:, 0], fy * Xc[:, 1] / Xc[:, 2] + cy - x[:, 1]], 1)
        J = np.zeros((len(X), 2, 6))
        for i in range(len(X)):
            z = Xc[i, 2]; p = P[i]
            D = np.array([[fx / z, 0, -fx * Xc[i, 0] / z ** 2], [0, fy / z, -fy * Xc[i, 1] / z ** 2]])
            S = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
            J[i] = D @ np.hstack([-S, np.eye(3)])
        Jm = J.reshape(-1, 6)
        d = np.linalg.solve(Jm.T @ Jm, -Jm.T @ r.ravel())
        R = Q.rodrigues(d[:3]) @ R; t = t + d[3:]
    return np.concatenate([R.ravel(), t])


def _exact_scenes():
    return [(Q.gpu_scenes()["exact"], 20)] + [(Q.make_scene([3, 4, 6, 10, 100, 700], seed=s, sigma=0.0, T=720), 40) for s in (11, 12, 13)]


def test_exact_scenes_end_at_the_generators_pose():
    worst = [0.0, 0.0]
    for sc, trials in _exact_scenes():
        r = Q.reference(sc, max_trials=trials)
        for m in range(len(sc["cams"])):
            g = _gauss_newton(sc, m)
            worst[0] = max(worst[0], float(np.abs(r["poses"][m] - sc["truth"][m]).max())); worst[1] = max(worst[1], float(np.abs(r["poses"][m] - g).max()))
        assert (r["info"][:, 3] <= Q.MAX_TRIALS).all() and (r["cost"][:, 1] < 1e-18).all()
    print("exact scenes: worst against the generator", worst[0], "against the independent Gauss-Newton", worst[1])
    assert worst[0] <= BOUND and worst[1] <= BOUND, worst


def test_noisy_scenes_end_below_the_cost_of_the_generators_pose():
    for name in ("counts", "empty", "many"):
        sc = Q.gpu_scenes()[name]
        r = Q.reference(sc)
        at_truth = Q.reference(dict(sc, poses=sc["truth"]), max_trials=0)
        ran = r["info"][:, 3] <= Q.MAX_TRIALS
        assert ran.sum() >= 4 and (r["cost"][ran, 1] < at_truth["cost"][ran, 0]).all() and (r["cost"][ran, 1] < r["cost"][ran, 0]).all()
        assert np.array_equal(at_truth["cost"][ran, 0], at_truth["cost"][ran, 1]) and (at_truth["info"][ran, 3] == Q.MAX_TRIALS).all()
        err = r["err"]; io, iobs = r["io"], r["iobs"]
        for m in np.flatnonzero(ran)[:5]:                              # err is the cost, position by position
            pos = iobs[io[m]:io[m + 1]]
            assert np.isclose((err[pos] ** 2).sum(), r["cost"][m, 1], rtol=1e-12)
        assert np.isnan(err).sum() == len(err) - r["info"][ran, 0].sum()


def test_every_status_by_hand():
    sc = Q.hand_scene()
    r = Q.reference(sc)
    assert r["info"][:, 3].tolist() == [Q.BAD_CAMERA, Q.BAD_POSE, Q.SHORT, Q.NOT_FINITE, Q.BEHIND, Q.FIXED, Q.STALLED, Q.CONVERGED, Q.CONVERGED]
    assert r["info"][:, 0].tolist() == [8, 8, 2, 5, 8, 8, 8, 8, 8]
    assert np.isnan(r["cost"][:4]).all() and r["cost"][4, 0] == r["cost"][4, 1] > 0 and r["cost"][5].tolist() == [2.5, 2.5]          # 8 (0.25 + 0.0625)
    assert r["cost"][6].tolist() == [0.0, 0.0] and r["info"][6].tolist() == [8, 16, 0, Q.STALLED]
    assert not r["info"][:6, 1:3].any()
    same = [0, 1, 2, 3, 4, 5, 6]
    assert np.array_equal(r["poses"][same], sc["poses"][same], equal_nan=True)
    assert r["cost"][7, 1] == r["cost"][8, 1] or abs(r["cost"][7, 1] - r["cost"][8, 1]) < 1e-9          # one minimum from two starts
    written = np.isfinite(r["err"])
    assert set(sc["img"][written].tolist()) == {5, 6, 7, 8} and np.allclose(r["err"][sc["img"] == 5], np.hypot(0.5, 0.25))
    two = Q.reference(sc, max_trials=2)
    assert two["info"][6:, 3].tolist() == [Q.MAX_TRIALS] * 3 and two["info"][6:, 1].tolist() == [2, 2, 2]
    zero = Q.reference(sc, max_trials=0)
    assert zero["info"][6:].tolist() == [[8, 0, 0, Q.MAX_TRIALS]] * 3 and np.array_equal(zero["cost"][6:, 0], zero["cost"][6:, 1])
    # precedence: a bad camera hides a bad pose, a bad pose hides a short image
    both = dict(sc, poses=sc["poses"].copy()); both["poses"][0, 3] = np.inf; both["poses"][2, 0] = np.nan
    assert Q.reference(both)["info"][[0, 2], 3].tolist() == [Q.BAD_CAMERA, Q.BAD_POSE]


def _seq_sum(terms, used):
    acc = np.zeros(terms.shape[1])
    for i in np.flatnonzero(used):                                     # (numpy's own sum is pairwise)
        acc = acc + terms[i]
    return acc


def test_order_of_the_sums_by_hand():
    big = 1e16
    # inside a wave: lane 0 holds 1e16, lane 1 holds 1, lane 32 holds -1e16: the tree takes v[0] + v[32] first, so the 1 survives
    t = np.zeros((256, 1)); t[0] = big; t[1] = 1.0; t[32] = -big
    u = np.ones(256, bool)
    assert Q.tree_sum(t, u)[0] == 1.0 and ((big + 1.0) - big) == 0.0
    # a thread's own terms come first: i = 0 and i = 256 are both thread 0's
    t = np.zeros((512, 1)); t[0] = big; t[256] = 1.0; t[32] = -big
    assert Q.tree_sum(t, np.ones(512, bool))[0] == 0.0
    # the waves: ((w0 + w1) + w2) + w3
    t = np.zeros((256, 1)); t[0] = big; t[64] = 1.0; t[128] = -big; t[192] = 1.0
    assert Q.tree_sum(t, u)[0] == 1.0 and (big + 1.0) + (-big + 1.0) == 0.0
    # a term that is not used adds nothing, not even a NaN
    t = np.ones((256, 2)); t[7] = np.nan; u2 = u.copy(); u2[7] = False
    assert Q.tree_sum(t, u2).tolist() == [255.0, 255.0]


def _hand_table():
    """4 tracks over 3 images and 9 positions, position 8 a tail fill: track 0 = positions 0 .. 3 (images 2, 0, 2: two keypoints of image
    2), track 1 = 3 .. 5 (images 0, 1), track 2 empty, track 3 = 5 .. 8 (images 1, 0, 2); the tests below replace the offsets"""
    return dict(off=np.array([0, 3, 5, 5, 8], np.int64),
                obs=np.array([0, 1, 2, 3, 4, 5, 6, 7, -1], np.int32), img=np.array([2, 0, 2, 0, 1, 1, 0, 2, -1], np.int32), nt=None, kps=np.ones((8, 2)),
                cams=np.ones((3, 4)), poses=np.zeros((3, 12)), X=np.ones((4, 3)), keep=None, refine=None)


def test_image_major_table_by_hand():
    sc = _hand_table()
    sc["off"] = np.array([0, 3, 5, 4, 4], np.int64)                    # tracks 2 and 3 own nothing: (5, 4) decreases, (4, 4) is empty
    io, iobs, tof = Q.table(sc)
    assert io.tolist() == [0, 2, 3, 5] and iobs.tolist() == [1, 3, 4, 0, 2, -1, -1, -1, -1] and tof[:5].tolist() == [0, 0, 0, 1, 1]
    sc["off"] = np.array([0, 3, 5, 5, 8], np.int64)                    # every track whole; position 8 (the fill) belongs to nobody
    io, iobs, tof = Q.table(sc)
    assert io.tolist() == [0, 3, 5, 8] and iobs.tolist() == [1, 3, 6, 4, 5, 0, 2, 7, -1]
    assert Q.table(dict(sc, nt=2))[1].tolist() == [1, 3, 4, 0, 2, -1, -1, -1, -1] and Q.table(dict(sc, nt=0))[0].tolist() == [0, 0, 0, 0]
    assert Q.table(dict(sc, nt=99))[1].tolist() == iobs.tolist() and Q.table(dict(sc, nt=-1))[1].tolist() == [-1] * 9
    sc["off"] = np.array([0, 3, 10, 5, 8], np.int64)                   # track 1 runs beyond M, track 2 decreases
    assert Q.table(sc)[1].tolist() == [1, 6, 5, 0, 2, 7, -1, -1, -1]
    sc["off"] = np.array([0, 3, 5, 5, 8], np.int64)
    X = sc["X"].copy(); X[1, 2] = np.nan
    keep = np.ones(9, np.uint8); keep[6] = 0
    kps = sc["kps"].copy(); kps[7, 1] = np.inf
    assert Q.table(dict(sc, X=X, keep=keep, kps=kps))[1].tolist() == [1, 5, 0, 2, -1, -1, -1, -1, -1]
    img = sc["img"].copy(); img[0] = 3; img[1] = -1
    obs = sc["obs"].copy(); obs[3] = 8
    assert Q.table(dict(sc, img=img, obs=obs))[1].tolist() == [6, 4, 5, 2, 7, -1, -1, -1, -1]


def test_broken_restatements_are_rejected():
    """a right-hand update, an unstable order inside an image, an accept without the Zc test, sums in plain order"""
    # the update on the right: the Jacobian is that of the left one (LM still gets there, by other steps, so the derivative test sees it)
    assert _jacobian_mismatch("right") > 1e-3
    sc = Q.gpu_scenes()["exact"]
    assert not np.array_equal(Q.reference(sc, max_trials=3)["poses"], Q.reference(sc, max_trials=3, broken="right")["poses"])
    # descending positions inside an image: the hand-written table is not met
    hand = _hand_table(); hand["off"] = np.array([0, 3, 5, 5, 8], np.int64)
    assert Q.table(hand)[1].tolist() == [1, 3, 6, 4, 5, 0, 2, 7, -1] != Q.table(hand, broken="unstable")[1].tolist()
    # accepting a trial with an observation behind the camera
    near = Q.gpu_scenes()["near"]; ta = []; tb = []
    a = Q.reference(near, trace=ta); b = Q.reference(near, broken="no_zc", trace=tb)
    assert not any(ta) and any(tb) and not np.array_equal(a["poses"], b["poses"])
    # the sums in plain order
    t = np.zeros((256, 1)); t[0] = 1e16; t[1] = 1.0; t[32] = -1e16
    assert Q.tree_sum(t, np.ones(256, bool))[0] == 1.0 != _seq_sum(t, np.ones(256, bool))[0]


def test_scene_invariant_converging_scenes_converge():
    """what the GPU tests rely on: in the scenes meant to converge every image with at least 4 observations ends CONVERGED by the
    restatement alone; of the 300 small images of `many` a few end their 20 trials on the floor of the cost, so 95 % are asked there"""
    for name in Q.CONVERGING:
        r = Q.reference(Q.gpu_scenes()[name])
        full = r["info"][:, 0] >= 4
        assert full.sum() >= 4 and (r["info"][full, 3] == Q.CONVERGED).all(), name
    r = Q.reference(Q.gpu_scenes()["many"])
    assert (r["info"][:, 3] <= Q.MAX_TRIALS).all() and (r["info"][:, 3] == Q.CONVERGED).mean() >= 0.95
    seen = {s for n in Q.gpu_scenes() for s in Q.reference(Q.gpu_scenes()[n])["info"][:, 3].tolist()}
    assert seen | {Q.MAX_TRIALS} == set(range(9))
