"""The triangulation of tracks without a device (include/mi_degensac.h mi_degensac_triangulate_tracks*, matcher.triangulate_tracks,
tensor_api.triangulate_tracks_tensors): every refusal of both C entry points with its message and its place in the order (each comes
back as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), T == 0 and M == 0, the Python keyword
and shape checks, synthetic.collection_truth against image_collection, and the restatement tests/triangulate_ref.py itself: exact and
noisy scenes, its Jacobian against central differences of its own residual, its linear point against numpy's least squares, every status
on a scene written by hand, the order of the sums on numbers written by hand, three broken restatements that these tests reject, and
the two-view midpoint of tests/pose_ref.py."""
import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from pydegensac_amd import synthetic as syn
from tests import pose_ref as P
from tests import triangulate_ref as Q

EINVAL = -1
NAMES = ("dev", "host")
ALL = ("off", "obs", "X", "kps", "cams")
G = _lib.tri_group()                                                    # the restatement follows the build: 16 in the product, 64 with -DTR_G=64


def _abi(which, T=2, M=10, rows=7, n_images=3, ang=1.5, px=4.0, iters=10, ftol=1e-12, null=()):
    """(rc, message) of one entry point; data pointers hold an address (never read: every call here is refused first) unless in `null`"""
    L = _lib.lib(); buf = np.zeros(64); addr = buf.ctypes.data
    A = lambda name: None if name in null else addr                    # noqa: E731
    tail = (A("kps"), rows, A("cams"), A("cams"), n_images, T, M, ang, px, iters, ftol, 0)
    outs = (A("X"), A("X"), A("X"), A("X"), None, None, None)
    if which == "dev":
        rc = L.mi_degensac_triangulate_tracks_dev(A("off"), A("obs"), A("obs"), None, *tail, None, *outs)
    else:
        rc = L.mi_degensac_triangulate_tracks(A("off"), A("obs"), A("obs"), -1, *tail, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and part in msg, (which, rc, msg)


def test_tile_constants_and_status_codes_are_mirrored():
    L = _lib.lib()
    assert G in (2, 4, 8, 16, 32, 64) and _lib.TRI_CHUNK % G == 0
    assert [L.mi_degensac_triangulate_tile(i) for i in range(5)] == [G, _lib.TRI_GRID, 256 // G, _lib.TRI_CHUNK, -1]
    assert (_lib.TRI_OK, _lib.TRI_NARROW, _lib.TRI_DEGENERATE, _lib.TRI_SHORT, _lib.TRI_TRUNCATED) == \
        (Q.OK, Q.NARROW, Q.DEGENERATE, Q.SHORT, Q.TRUNCATED) == tuple(range(5))


def test_refusals_and_their_order():
    nan = float("nan")
    _refused(b"n_tracks_max < 0", T=-1)
    _refused(b"too many tracks", T=0x40000000)
    _refused(b"n_obs_max < 0", M=-1)
    _refused(b"too many observations", M=0x40000000)
    for r in (-1, 0x80000000):
        _refused(b"rows", rows=r)
    _refused(b"n_images", n_images=-1)
    for a in (nan, -1e-300, 180.0000001, float("inf")):
        _refused(b"min_angle_deg", ang=a)
    for x in (nan, -1e-300, float("-inf")):
        _refused(b"max_reproj_px", px=x)
    for m in (-1, 101, 1 << 20):
        _refused(b"max_iters", iters=m)
    for f in (nan, -1e-300, -1.0):
        _refused(b"ftol", ftol=f)
    _refused(b"track_offsets", null=("off",))
    _refused(b"track_offsets", null=("off",), T=0, M=0)
    _refused(b"obs and obs_image", null=("obs",))
    _refused(b"X, info, cost and cosang", null=("X",))
    _refused(b"NULL argument: kps", null=("kps",))
    _refused(b"cams and poses", null=("cams",))
    # each refusal hides every later one
    bad = dict(M=-1, rows=-1, n_images=-1, ang=nan, px=nan, iters=-1, ftol=nan, null=ALL)
    order = [("T", -1, b"n_tracks_max < 0"), ("M", None, b"n_obs_max < 0"), ("rows", None, b"rows"), ("n_images", None, b"n_images"),
             ("ang", None, b"min_angle_deg"), ("px", None, b"max_reproj_px"), ("iters", None, b"max_iters"), ("ftol", None, b"ftol")]
    kw = dict(bad, T=-1)
    for key, _, part in order:
        _refused(part, **kw)
        kw.pop(key)                                                    # (the default of the key is a good value)
    for i, part in enumerate((b"track_offsets", b"obs and obs_image", b"X, info, cost and cosang", b"NULL argument: kps", b"cams and poses")):
        _refused(part, null=ALL[i:])
    for a, x, m, f in ((0.0, 0.0, 0, 0.0), (180.0, float("inf"), 100, float("inf"))):          # the closed ends are allowed: refused later
        _refused(b"cams and poses", ang=a, px=x, iters=m, ftol=f, null=("cams",))
    # nothing is asked of a table that is empty
    _refused(b"cams and poses", M=0, null=("obs", "cams"))
    _refused(b"cams and poses", rows=0, null=("kps", "cams"))


def test_t0_and_m0_succeed_without_a_device():
    for which in NAMES:
        rc, _ = _abi(which, T=0, M=0, rows=0, n_images=0, null=ALL[1:])
        assert rc == 0, which


# ---- the Python checks ----
def _np(T=2, M=10, rows=7, n=3):
    return np.zeros(T + 1, np.int64), np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros((rows, 2)), np.ones((n, 4)), np.zeros((n, 3, 3)), np.zeros((n, 3))


@pytest.mark.parametrize("kw, part", [
    (dict(max_iters=-1), "max_iters"), (dict(max_iters=101), "max_iters"), (dict(max_iters=2.0), "max_iters"), (dict(max_iters=True), "max_iters"),
    (dict(ftol=-1e-9), "ftol"), (dict(ftol=float("nan")), "ftol"), (dict(ftol="x"), "ftol"), (dict(ftol=True), "ftol"),
    (dict(min_angle_deg=-1), "min_angle_deg"), (dict(min_angle_deg=181), "min_angle_deg"), (dict(min_angle_deg=float("nan")), "min_angle_deg"),
    (dict(max_reproj_px=-1.0), "max_reproj_px"), (dict(max_reproj_px=float("nan")), "max_reproj_px"), (dict(max_reproj_px=None), "max_reproj_px"),
    (dict(n_tracks=1.5), "n_tracks"), (dict(n_tracks=True), "n_tracks"), (dict(max_trials=3), "unknown keyword"), (dict(with_resid=True), "unknown keyword"),
])
def test_keyword_checks(kw, part):
    with pytest.raises(ValueError, match=part):
        matcher.triangulate_tracks(*_np(), **kw)


def test_shape_and_dtype_checks():
    off, obs, img, kps, cams, R, t = _np()
    chk = lambda *a, **kw: matcher.check_triangulate_args(*[x for v in a for x in (v.shape, v.dtype)], **kw)          # noqa: E731
    f32 = lambda x: x.astype(np.float32)                               # noqa: E731
    bad = [((off.astype(np.int32), obs, img, kps, cams, R, t), "track_offsets"), ((off[:0], obs, img, kps, cams, R, t), "track_offsets"),
           ((off.reshape(1, -1), obs, img, kps, cams, R, t), "track_offsets"), ((off, obs.astype(np.int64), img, kps, cams, R, t), "obs should"),
           ((off, obs.reshape(2, 5), img, kps, cams, R, t), "obs should"), ((off, obs, img[:9], kps, cams, R, t), "obs_image"),
           ((off, obs, img.astype(np.int64), kps, cams, R, t), "obs_image"), ((off, obs, img, kps[:, :1], cams, R, t), "kps"),
           ((off, obs, img, f32(kps), cams, R, t), "kps"), ((off, obs, img, kps.ravel(), cams, R, t), "kps"), ((off, obs, img, kps, cams[:, :3], R, t), "cams"),
           ((off, obs, img, kps, f32(cams), R, t), "cams"), ((off, obs, img, kps, cams, R[:2], t), "R should"), ((off, obs, img, kps, cams, R.reshape(3, 9), t), "R should"),
           ((off, obs, img, kps, cams, f32(R), t), "R should"), ((off, obs, img, kps, cams, R, t[:2]), "t should"), ((off, obs, img, kps, cams, R, f32(t)), "t should")]
    for a, part in bad:
        with pytest.raises(ValueError, match=part):
            chk(*a)
    assert chk(off, obs, img, kps, cams, R, t) == (2, 10, 7, 3, 1.5, 4.0, 10, 1e-12)
    wide = np.zeros((7, 6))
    assert chk(off, obs, img, wide, cams, R, t, n_tracks=((1,), np.dtype(np.int64)), min_angle_deg=0, max_reproj_px=np.float32(2), max_iters=np.int64(0),
               ftol=0) == (2, 10, 7, 3, 0.0, 2.0, 0, 0.0)
    for nt in (((2,), np.dtype(np.int64)), ((1,), np.dtype(np.int32))):
        with pytest.raises(ValueError, match="n_tracks"):
            chk(off, obs, img, kps, cams, R, t, n_tracks=nt)


def test_tensor_call_wants_tensors_on_a_device():
    from pydegensac_amd import tensor_api
    import torch
    a = _np()
    with pytest.raises(ValueError, match="torch tensors"):
        tensor_api.triangulate_tracks_tensors(*a)
    ts = [torch.from_numpy(x) for x in a]
    with pytest.raises(ValueError, match="unknown keyword"):
        tensor_api.triangulate_tracks_tensors(*ts, max_trials=3)
    with pytest.raises(ValueError, match="max_iters"):
        tensor_api.triangulate_tracks_tensors(*ts, max_iters=101)
    with pytest.raises(ValueError, match="kps"):
        tensor_api.triangulate_tracks_tensors(*ts[:3], ts[3].float(), *ts[4:])
    with pytest.raises(ValueError, match="same ROCm device"):
        tensor_api.triangulate_tracks_tensors(*ts)


# ---- the generator's truth ----
@pytest.mark.parametrize("args", [dict(), dict(m=5, n=300, inlier_ratio=0.6, sigma=0.3, dim=32, seed=2), dict(m=3, n=41, inlier_ratio=0.33, sigma=0.0, dim=8, seed=9,
                                                                                                            desc_sigma=0.5)])
def test_collection_truth_replays_image_collection(args):
    kps, _ = syn.image_collection(**args)
    X, point, again = syn.collection_truth(**args)
    m = args.get("m", 8); n = args.get("n", 500)
    assert len(point) == len(again) == m and X.shape == (n, 3)
    K, poses = syn.collection_cameras(m)
    for i in range(m):
        assert kps[i].tobytes() == again[i].tobytes()                  # bit for bit
        seen = point[i] >= 0
        assert seen.sum() == int(round(n * args.get("inlier_ratio", 0.5))) and len(set(point[i][seen])) == seen.sum()
        far = np.abs(syn._project(K, *poses[i], X[point[i][seen]]) - kps[i][seen]).max()
        assert far <= 6 * args.get("sigma", 0.1) + 1e-9


# ---- the restatement ----
def _views_scene(views, sigma, seed=0, T=40):
    return Q.make_scene([len(views)] * T, seed=seed, sigma=sigma, views=views)


@pytest.mark.parametrize("views", [(0, 1), (0, 7), (0, 3, 7), tuple(range(8))])
def test_exact_scenes_recover_the_point(views):
    sc = _views_scene(views, 0.0)
    for iters in (0, 10):
        r = Q.reference(sc, G, max_iters=iters)
        assert np.abs(r["X"] - sc["truth"]).max() < 1e-9
        assert (r["info"][:, 4] == Q.OK).all() and (r["info"][:, 0] == len(views)).all() and (r["info"][:, 1] == len(views)).all()
        owned = np.arange(len(sc["obs"]))
        assert r["ok"][owned].all() and (r["depth"] > 3.0).all() and (r["err"] < 1e-7).all()


@pytest.mark.parametrize("sigma", [0.1, 1.0])
def test_noisy_scenes_never_end_above_the_linear_or_the_true_point(sigma):
    for views in ((0, 7), (0, 3, 7), tuple(range(8))):
        sc = _views_scene(views, sigma, seed=3)
        r = Q.reference(sc, G)
        assert (r["cost"][:, 1] <= r["cost"][:, 0]).all() and (r["info"][:, 3] <= 10).all() and (r["info"][:, 2] <= r["info"][:, 3]).all()
        T = len(sc["truth"]); L = len(views)
        o = Q.gather(sc, sc["off"][:T, None] + np.arange(L)[None], np.ones((T, L), bool))
        rx, ry, _, _, _ = Q.residual(o, sc["truth"])
        assert (r["cost"][:, 1] <= (rx * rx + ry * ry).sum(1) * (1 + 1e-12)).all()
        assert np.abs(r["X"] - sc["truth"]).max() < 0.6 * sigma + 0.02
        one = Q.reference(sc, G, max_iters=1)
        assert (one["info"][:, 3] <= 1).all()


def test_jacobian_against_central_differences():
    sc = _views_scene(tuple(range(8)), 1.0, seed=5, T=6)
    T = 6; L = 8
    o = Q.gather(sc, sc["off"][:T, None] + np.arange(L)[None], np.ones((T, L), bool))
    X = sc["truth"] + 0.05
    _, _, _, jx, jy = Q.residual(o, X)
    h = 1e-6
    for j in range(3):
        e = np.zeros(3); e[j] = h
        ax, ay = Q.residual(o, X + e)[:2]; bx, by = Q.residual(o, X - e)[:2]
        assert np.abs((ax - bx) / (2 * h) - jx[j]).max() < 1e-5 and np.abs((ay - by) / (2 * h) - jy[j]).max() < 1e-5


def test_linear_point_against_lstsq():
    for views in ((0, 1), (0, 3, 7), tuple(range(8))):
        sc = _views_scene(views, 1.0, seed=6, T=10)
        r = Q.reference(sc, G, max_iters=0)
        for k in range(10):
            A = []; b = []
            for p in range(sc["off"][k], sc["off"][k + 1]):
                i = sc["img"][p]; R = sc["poses"][i, :9].reshape(3, 3); t = sc["poses"][i, 9:]
                x, y = sc["kps"][sc["obs"][p]]
                d = np.array([(x - sc["cams"][i, 2]) / sc["cams"][i, 0], (y - sc["cams"][i, 3]) / sc["cams"][i, 1], 1.0])
                w = R.T @ d; w /= np.linalg.norm(w)
                Pm = np.eye(3) - np.outer(w, w)
                A.append(Pm); b.append(Pm @ (-R.T @ t))
            X = np.linalg.lstsq(np.concatenate(A), np.concatenate(b), rcond=None)[0]
            assert np.abs(X - r["X"][k]).max() < 1e-9


def test_every_status_by_hand():
    sc = Q.hand_scene()
    r = Q.reference(sc, G)
    assert r["info"][:, 4].tolist() == [Q.SHORT, Q.DEGENERATE, Q.DEGENERATE, Q.NARROW, Q.OK, Q.OK, Q.OK, Q.TRUNCATED]
    assert r["info"][:, 0].tolist() == [1, 2, 2, 2, 3, 2, 2, 0]
    assert np.isnan(r["X"][[0, 1, 2, 7]]).all() and np.isnan(r["cost"][[0, 1, 2, 7]]).all() and np.isnan(r["cosang"][[0, 1, 2, 7]]).all()
    assert np.abs(r["X"][3] - [0, 0, 400.0]).max() < 1e-6 and r["cosang"][3] > Q.cos_min_of(1.5) and r["info"][3, 1] == 2          # NARROW keeps everything
    assert np.abs(r["X"][5] - [0.2, 0.1, 4.0]).max() < 1e-9 and np.abs(r["X"][6] - [0.1, 0.3, 6.0]).max() < 1e-9
    # the point behind camera 2: written, and that observation is neither front nor ok
    b = int(sc["off"][4])
    assert np.isfinite(r["X"][4]).all() and r["depth"][b + 2] < 0 and r["ok"][b + 2] == 0 and (r["depth"][b:b + 2] > 0).all()
    assert np.isnan(r["err"][:int(sc["off"][3])]).all() and not r["ok"][:int(sc["off"][3])].any()          # tracks without a point write nothing
    z = Q.reference(Q.zero_depth_scene(), G)
    assert z["depth"].tolist()[1::2] == [0.0, 0.0] and not z["ok"].any() and z["X"][0, 0] == 0.0 and z["info"][0].tolist() == [4, 0, 0, 0, Q.OK]
    assert np.isinf(z["cost"]).all() and np.isinf(z["err"][1::2]).all() and (z["depth"][0::2] > 3.0).all()          # no step from a cost that is not finite


def test_order_of_the_sums_by_hand():
    """1, 2^-53 and -1 spread over lanes and steps: the sum depends on the order, and the restatement has the header's"""
    e = 2.0 ** -53
    t = np.zeros((1, 2 * G, 1)); u = np.ones((1, 2 * G), bool)
    t[0, 0, 0] = 1.0; t[0, G, 0] = e; t[0, 1, 0] = e; t[0, G // 2, 0] = -1.0
    # lane 0: 1 + e = 1 (ties to even); lane 1: e; lane G / 2: -1.  m = G / 2: lane 0 takes 1 + -1 = 0; .. m = 1: 0 + e
    assert Q.lane_sum(t, u, G)[0, 0] == e
    t2 = t.copy(); t2[0, G, 0] = 0.0; t2[0, 2, 0] = e                 # now lanes 1 and 2 hold e each: (1 + -1) .. + (e + e)
    assert Q.lane_sum(t2, u, G)[0, 0] == 2 * e
    u2 = u.copy(); u2[0, G // 2] = False                               # an observation that is not used adds nothing: the -1 is gone, 1 + e = 1
    assert Q.lane_sum(t, u2, G)[0, 0] == 1.0
    # per lane in ascending position: (1 + e) + e = 1, but lane order reversed would give 1 + 2e
    t3 = np.zeros((1, 3 * G, 1)); u3 = np.ones((1, 3 * G), bool)
    t3[0, 0, 0] = 1.0; t3[0, G, 0] = e; t3[0, 2 * G, 0] = e
    assert Q.lane_sum(t3, u3, G)[0, 0] == 1.0
    t3[0, 0, 0] = e; t3[0, 2 * G, 0] = 1.0
    assert Q.lane_sum(t3, u3, G)[0, 0] == 1.0 + 2 * e


@pytest.mark.parametrize("broken", ["drop", "centre", "sign"])
def test_broken_restatements_are_rejected(broken):
    sc = _views_scene((0, 3, 7), 1.0, seed=8)
    good = Q.reference(sc, G); bad = Q.reference(sc, G, broken=broken)
    if broken == "drop":
        assert (bad["info"][:, 0] == 2).all() and not np.array_equal(good["X"], bad["X"])
    elif broken == "centre":
        assert np.abs(bad["X"] - sc["truth"]).max() > 1.0 > np.abs(good["X"] - sc["truth"]).max()
    else:                                                              # a step uphill is never accepted
        assert not bad["info"][:, 2].any() and (bad["info"][:, 3] == 1).all() and good["info"][:, 2].all()
        assert (good["cost"][:, 1] < bad["cost"][:, 1]).all()


def test_two_views_equal_the_pose_calls_midpoint():
    """a two-image store with poses (I, 0) and the (R, t) of pose_ref's relative pose: the same geometry through different arithmetic"""
    K, poses = syn.collection_cameras(8)
    Rg, tg = P.relative(poses, 0, 7)
    cams = np.tile([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], (2, 1)).astype(np.float64)
    ps = np.stack([np.concatenate([np.eye(3).ravel(), np.zeros(3)]), np.concatenate([Rg.ravel(), tg])])
    rng = np.random.default_rng(11); n = 30
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 8, n)], 1)
    x1 = Q.project(cams, ps, 0, X) + rng.normal(0, 0.5, (n, 2)); x2 = Q.project(cams, ps, 1, X) + rng.normal(0, 0.5, (n, 2))
    sc = dict(off=2 * np.arange(n + 1, dtype=np.int64), obs=np.arange(2 * n, dtype=np.int32), img=np.tile([0, 1], n).astype(np.int32), nt=None,
              kps=np.stack([x1, x2], 1).reshape(2 * n, 2), cams=cams, poses=ps)
    r = Q.reference(sc, G, max_iters=0)
    # the two-ray midpoint, written out independently: the closest points of the two rays, halfway
    for k in range(n):
        d1 = np.array([(x1[k, 0] - cams[0, 2]) / cams[0, 0], (x1[k, 1] - cams[0, 3]) / cams[0, 1], 1.0])
        d2 = Rg.T @ np.array([(x2[k, 0] - cams[1, 2]) / cams[1, 0], (x2[k, 1] - cams[1, 3]) / cams[1, 1], 1.0]); c2 = -Rg.T @ tg
        a, b, c = d1 @ d1, d1 @ d2, d2 @ d2; d, e = d1 @ c2, d2 @ c2; den = a * c - b * b
        l1 = (c * d - b * e) / den; l2 = (b * d - a * e) / den
        mid = 0.5 * (l1 * d1 + c2 + l2 * d2)
        assert np.abs(mid - r["X"][k]).max() <= 1e-9 * np.abs(mid).max()
