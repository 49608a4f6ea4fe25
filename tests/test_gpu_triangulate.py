"""GPU: triangulation of tracks under known camera poses (include/mi_degensac.h mi_degensac_triangulate_tracks*,
csrc/mi_triangulate.hip) against tests/triangulate_ref.py.  Everything is demanded BIT FOR BIT: from the device's own inputs the
restatement gives X, info, cost, cosang, err, ok and depth at full length, fills included, with guard elements around every output.
Track lengths sit at the edges of a group of G lanes (G - 1, G, G + 1, 2 G, 2 G + 1), of a wave and of the staging area of the pair pass
(63 .. 65), and beyond it (257, 2049: chunk against chunk)."""
import ctypes as C
import functools

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import triangulate_ref as Q

pytestmark = pytest.mark.gpu
GUARD = 8                                                              # guard elements on each side of an output
PER = dict(X=3, info=5, cost=2, cosang=1, err=1, ok=1, depth=1)
PER_OBS = ("err", "ok", "depth")
FILL = dict(X=-7.0, info=-5, cost=-7.0, cosang=-7.0, err=-3.0, ok=9, depth=-3.0)
DT = dict(info="int32", ok="uint8")
SCENES = ["lengths", "last_step", "one_per_g", "many", "stride", "ranges", "hand", "zero_depth", "bad"]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _tile():
    L = _lib.lib()
    return tuple(L.mi_degensac_triangulate_tile(i) for i in range(3))


def _scenes():
    return Q.gpu_scenes(*_tile())


@functools.lru_cache(maxsize=None)
def _want(name, nt="scene", **kw):
    """the restatement on a scene of the catalogue: computed once, shared, never written to"""
    sc = _scenes()[name]
    if nt != "scene":
        sc = dict(sc, nt=nt)
    return Q.reference(sc, _tile()[0], **kw)


def _outs(torch, T, M):
    out = {}
    for k, per in PER.items():
        n = M if k in PER_OBS else T
        buf = torch.full(((n + 2 * GUARD) * per,), FILL[k], dtype=getattr(torch, DT.get(k, "float64")), device="cuda")
        out[k] = (buf, buf[GUARD * per:(GUARD + n) * per])
    return out


def _call(torch, sc, nt="scene", min_angle_deg=1.5, max_reproj_px=4.0, max_iters=10, ftol=1e-12, outs=None, stream=None, skip=()):
    """mi_degensac_triangulate_tracks_dev on the scene with guarded outputs (outs: the buffers of an earlier call, reused as they are;
    skip: the optional outputs passed as NULL).  Returns (dict of numpy results, outs)."""
    T = len(sc["off"]) - 1; M = len(sc["obs"])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    off, obs, img, kps, cams, poses = (t(sc[k]) for k in ("off", "obs", "img", "kps", "cams", "poses"))
    n = sc["nt"] if nt == "scene" else nt
    ntd = None if n is None else torch.tensor([n], dtype=torch.int64, device="cuda")
    if outs is None:
        outs = _outs(torch, T, M)
    s = torch.cuda.current_stream() if stream is None else stream
    d = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()          # noqa: E731
    p = lambda k: None if k in skip else outs[k][1].data_ptr()         # noqa: E731
    rc = _lib.lib().mi_degensac_triangulate_tracks_dev(d(off), d(obs), d(img), d(ntd), d(kps), len(sc["kps"]), d(cams), d(poses), len(sc["cams"]), T, M,
                                                       min_angle_deg, max_reproj_px, max_iters, ftol, 0, C.c_void_p(s.cuda_stream),
                                                       *(p(k) for k in PER))
    _lib.check_match(rc)
    s.synchronize()
    res = {}
    for k, (buf, view) in outs.items():
        whole = buf.cpu().numpy(); per = PER[k]
        assert (whole[:GUARD * per] == FILL[k]).all() and (whole[len(whole) - GUARD * per:] == FILL[k]).all(), f"{k}: a guard element was written"
        body = whole[GUARD * per:len(whole) - GUARD * per]
        if k in skip:
            assert (body == FILL[k]).all(), f"{k}: written although NULL was passed"
            continue
        res[k] = body.reshape((-1, per) if per > 1 else (-1,))
    return res, outs


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def _same(got, want):
    assert np.array_equal(got["info"], want["info"]), (np.flatnonzero((got["info"] != want["info"]).any(axis=1))[:8], got["info"][:8], want["info"][:8])
    for k in got:
        w = want[k].reshape(got[k].shape)
        assert _bits(got[k], w), (k, np.flatnonzero(~((got[k] == w) | (np.isnan(got[k]) & np.isnan(w))).reshape(len(w), -1).all(axis=1))[:8])


def test_scene_list_is_the_catalogue():
    G, grid, gpw = _tile()
    assert sorted(SCENES) == sorted(_scenes())
    assert G == _lib.tri_group() and grid == _lib.TRI_GRID and gpw * G == 256 and _lib.lib().mi_degensac_triangulate_tile(3) == _lib.TRI_CHUNK == 64
    S = _scenes()
    assert np.diff(S["lengths"]["off"]).tolist() == Q.lengths_of(G) and S["lengths"]["off"][0] == 3
    assert {0, 1, 2, 3, G - 1, G, G + 1, 2 * G, 2 * G + 1, 63, 64, 65, 257, 2049} == set(Q.lengths_of(G))
    assert len(S["stride"]["off"]) - 1 == grid * gpw + 1               # a second stride step runs
    assert len(S["many"]["off"]) - 1 == 320 and S["many"]["nt"] == 300 and (S["many"]["off"][300:] == S["many"]["off"][300]).all()
    assert (S["many"]["obs"][-9:] == -1).all() and (S["many"]["img"][-9:] == -1).all()
    seen = {s for n in SCENES for s in _want(n)["info"][:, 4].tolist()}
    assert seen == set(range(5))                                       # every status
    assert _want("zero_depth")["depth"].tolist()[1::2] == [0.0, 0.0]   # Zc exactly 0


@pytest.mark.parametrize("name", SCENES)
def test_triangulate_equals_restatement(torch, name):
    """every scene: lengths at the edges with a non-zero first offset and unowned positions behind, used observations in the last lane
    step only and one per G, 300 tracks with the tails of the tracks call, one track more than a full grid, ranges across and beyond M
    and decreasing, every status by hand, Zc exactly 0, inputs that are not finite or out of range, two keypoints of one image"""
    got, _ = _call(torch, _scenes()[name])
    want = _want(name)
    _same(got, want)
    point = want["info"][:, 4] <= Q.NARROW
    assert np.isfinite(got["X"][point]).all() and np.isnan(got["X"][~point]).all() and np.isnan(got["cost"][~point]).all()


@pytest.mark.parametrize("max_iters, ftol", [(0, 1e-12), (1, 1e-12), (10, 0.0), (10, 1.0)])
def test_scalars(torch, max_iters, ftol):
    for name in ("lengths", "hand", "bad"):
        got, _ = _call(torch, _scenes()[name], max_iters=max_iters, ftol=ftol)
        _same(got, _want(name, max_iters=max_iters, ftol=ftol))
        point = got["info"][:, 4] <= Q.NARROW
        assert (got["info"][:, 3] <= max_iters).all()
        if max_iters == 0:                                             # the linear point
            assert not got["info"][:, 2:4].any() and _bits(got["cost"][point, 0], got["cost"][point, 1])
        if ftol == 1.0:                                                # the first accepted step ends the run
            assert (got["info"][:, 2] <= 1).all()


def test_err_at_the_bound_and_cosang_at_the_bound(torch):
    """max_reproj_px equal to an observation's error keeps it ok, the float64 below does not; a min_angle_deg whose cosine is a track's
    cosang leaves it OK, the next bound below makes it NARROW"""
    sc = _scenes()["many"]
    base = _want("many")
    p = int(np.flatnonzero(base["ok"] == 1)[5]); e = float(base["err"][p])
    for px, flag in ((e, 1), (float(np.nextafter(e, 0.0)), 0)):
        got, _ = _call(torch, sc, max_reproj_px=px)
        _same(got, _want("many", max_reproj_px=px))
        assert got["ok"][p] == flag
    k = int(np.flatnonzero(base["info"][:, 4] == Q.NARROW)[0]); c = float(base["cosang"][k])
    at, above = Q.angle_at_bound(c)
    for deg, status in ((at, Q.OK), (above, Q.NARROW)):
        got, _ = _call(torch, sc, min_angle_deg=deg)
        _same(got, _want("many", min_angle_deg=deg))
        assert got["info"][k, 4] == status and got["cosang"][k] == c


@pytest.mark.parametrize("nt", [None, 0, 1, 150, 300, 320, 5000, -4])
def test_n_tracks_below_at_above_and_none(torch, nt):
    got, _ = _call(torch, _scenes()["many"], nt=nt)
    _same(got, _want("many", nt=nt))
    n = 320 if nt is None else min(max(nt, 0), 320)
    assert (got["info"][n:] == [0, 0, 0, 0, Q.SHORT]).all() and np.isnan(got["X"][n:]).all()


def test_null_optional_outputs(torch):
    sc = _scenes()["lengths"]
    full, _ = _call(torch, sc)
    part, _ = _call(torch, sc, skip=PER_OBS)
    assert sorted(part) == ["X", "cosang", "cost", "info"] and all(_bits(part[k], full[k]) for k in part)
    part, _ = _call(torch, sc, skip=("err", "depth"))
    assert "ok" in part and all(_bits(part[k], full[k]) for k in part)


def test_outputs_reused_and_ten_identical_calls(torch):
    """a long scene, then a short one into the same buffers (what the first call left must not show), then ten calls with identical bytes"""
    a = _scenes()["lengths"]; b = _scenes()["hand"]
    _, outs = _call(torch, a)
    T, M = len(b["off"]) - 1, len(b["obs"])
    n = lambda k: M if k in PER_OBS else T                             # noqa: E731
    small = {k: (buf[:(n(k) + 2 * GUARD) * PER[k]], buf[GUARD * PER[k]:(GUARD + n(k)) * PER[k]]) for k, (buf, _) in outs.items()}
    for k, (buf, view) in small.items():                               # the guard behind the shorter body
        buf[len(buf) - GUARD * PER[k]:] = FILL[k]
    got, _ = _call(torch, b, outs=small)
    _same(got, _want("hand"))
    sc = _scenes()["many"]
    first, o2 = _call(torch, sc)
    for _ in range(9):
        again, _ = _call(torch, sc, outs=o2)
        for k in first:
            assert first[k].tobytes() == again[k].tobytes(), k


def test_same_bytes_whichever_tracks_came_before(torch):
    """the 300 tracks in reverse order: every group meets other tracks before and beside each of its own, and every track has the same
    bytes"""
    sc = _scenes()["many"]; T = 300
    order = np.arange(T)[::-1]
    lens = np.diff(sc["off"][:T + 1])[order]
    rev = dict(sc); rev["off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64); rev["nt"] = None
    take = np.concatenate([np.arange(sc["off"][k], sc["off"][k + 1]) for k in order])
    rev["obs"] = sc["obs"][take].copy(); rev["img"] = sc["img"][take].copy()
    got, _ = _call(torch, rev)
    want = _want("many")
    for k in ("X", "info", "cost", "cosang"):
        assert _bits(got[k], want[k][:T][order]), k
    for k in PER_OBS:
        assert _bits(got[k], want[k][take]), k


def test_second_stream(torch):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = _call(torch, _scenes()["many"], stream=s)
    _same(got, _want("many"))


def test_t0_and_m0(torch):
    L = _lib.lib()
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    tail = (1.5, 4.0, 10, 1e-12, 0, None)
    assert L.mi_degensac_triangulate_tracks_dev(off.data_ptr(), None, None, None, None, 0, None, None, 0, 0, 0, *tail, *([None] * 7)) == 0
    # T == 0 with observations: the fills are all that is written
    obs = torch.zeros(5, dtype=torch.int32, device="cuda"); er = torch.zeros(5, dtype=torch.float64, device="cuda")
    okf = torch.ones(5, dtype=torch.uint8, device="cuda")
    assert L.mi_degensac_triangulate_tracks_dev(off.data_ptr(), obs.data_ptr(), obs.data_ptr(), None, None, 0, None, None, 0, 0, 5, *tail, None, None, None,
                                                None, er.data_ptr(), okf.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.isnan(er.cpu().numpy()).all() and not okf.cpu().numpy().any()
    # T > 0 with M == 0 and no tables at all: every track is short or truncated
    off = torch.tensor([0, 0, 3], dtype=torch.int64, device="cuda")
    X = torch.zeros((2, 3), dtype=torch.float64, device="cuda"); cost = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    ca = torch.zeros(2, dtype=torch.float64, device="cuda"); info = torch.ones((2, 5), dtype=torch.int32, device="cuda")
    assert L.mi_degensac_triangulate_tracks_dev(off.data_ptr(), None, None, None, None, 0, None, None, 0, 2, 0, *tail, X.data_ptr(), info.data_ptr(),
                                                cost.data_ptr(), ca.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [[0, 0, 0, 0, Q.SHORT], [0, 0, 0, 0, Q.TRUNCATED]]
    assert np.isnan(X.cpu().numpy()).all() and np.isnan(cost.cpu().numpy()).all() and np.isnan(ca.cpu().numpy()).all()


def _split(sc):
    n = len(sc["cams"])
    return sc["off"], sc["obs"], sc["img"], sc["kps"], sc["cams"], sc["poses"][:, :9].reshape(n, 3, 3), np.ascontiguousarray(sc["poses"][:, 9:])


def test_numpy_form():
    for name, kw in (("lengths", {}), ("bad", dict(max_iters=1, ftol=0.5, min_angle_deg=3.0, max_reproj_px=1.0))):
        sc = _scenes()[name]
        res = matcher.triangulate_tracks(*_split(sc), with_obs=True, **kw)
        got = dict(zip(PER, res)); got["ok"] = got["ok"].astype(np.uint8)
        _same(got, _want(name, **kw))
    sc = _scenes()["many"]
    res = matcher.triangulate_tracks(*_split(sc), n_tracks=150)
    assert len(res) == 4
    _same(dict(zip(PER, res)), {k: v for k, v in _want("many", nt=150).items() if k not in PER_OBS})


def test_tensor_form_takes_wide_keypoints(torch):
    """kps [rows, 6] with x, y in front, a non-contiguous R, n_tracks as the device word"""
    from pydegensac_amd import tensor_api as T
    sc = _scenes()["many"]
    off, obs, img, kps, cams, R, t = _split(sc)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    wide = np.concatenate([kps, np.full((len(kps), 4), np.nan)], 1)
    Rt = c(R.transpose(0, 2, 1)).transpose(1, 2)
    res = T.triangulate_tracks_tensors(c(off), c(obs), c(img), c(wide), c(cams), Rt, c(t), n_tracks=torch.tensor([300], device="cuda"), with_obs=True)
    got = {k: v.cpu().numpy() for k, v in zip(PER, res)}; got["ok"] = got["ok"].astype(np.uint8)
    _same(got, _want("many"))
    short = T.triangulate_tracks_tensors(c(off), c(obs), c(img), c(kps), c(cams), c(R), c(t))
    assert len(short) == 4 and short[0].shape == (320, 3) and short[1].dtype == torch.int32 and short[2].shape == (320, 2) and short[3].shape == (320,)


def test_chain_export_tracks_triangulate_without_sync(torch):
    """match_and_verify_pairs_tensors -> correspondences_pairs_tensors(store_rows) -> tracks_tensors -> triangulate_tracks_tensors on a
    small collection with the generator's cameras: the last two run under torch's synchronisation check, so nothing is read back between
    them.  From the device's own tables the restatement gives every output bit for bit.  Against collection_truth, the point of every
    consistent track all of whose keypoints are the same cloud point, with status OK, lies within BOUND of it.
    BOUND: the restatement on this scene's tables (the chain before the call is deterministic, so they are the same on every run) has
    its largest such error at 0.0476 over 251 tracks (sigma = 0.3 px, f = 800, depth 4 .. 8, two to five views on an arc of half a
    radian: a pair of neighbouring views has a baseline of 0.75 and some 0.03 of depth per 0.3 px); times 2."""
    BOUND = 2 * 0.0476
    from pydegensac_amd import synthetic as syn
    from pydegensac_amd import tensor_api as T
    m = 5
    args = dict(m=m, n=300, inlier_ratio=0.6, sigma=0.3, dim=32, seed=2)
    kps, descs = syn.image_collection(**args)
    cloud, point, _ = syn.collection_truth(**args)
    cams, poses = Q.cameras(m)
    counts = [len(k) for k in kps]
    k = torch.from_numpy(np.ascontiguousarray(np.concatenate(kps)[:, :2], dtype=np.float64)).cuda()
    d = torch.from_numpy(np.concatenate(descs).astype(np.float32)).cuda()
    pairs = matcher.exhaustive_pairs(m)
    ver = T.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.8, max_iters=2000)
    rows, co, total, entry = T.correspondences_pairs_tensors(ver[1], counts, counts, pairs, keep=ver[2], store_rows=True)[:4]
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    cm, Rm, tv = c(cams), c(poses[:, :9].reshape(m, 3, 3)), c(poses[:, 9:])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        track, nt, to, obs, oi, ti, no = T.tracks_tensors(rows, counts, total)
        res = T.triangulate_tracks_tensors(to, obs, oi, k, cm, Rm, tv, n_tracks=nt, with_obs=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = {kk: v.cpu().numpy() for kk, v in zip(PER, res)}; got["ok"] = got["ok"].astype(np.uint8)
    sc = dict(off=to.cpu().numpy(), obs=obs.cpu().numpy(), img=oi.cpu().numpy(), nt=int(nt.item()), kps=k.cpu().numpy(), cams=cams, poses=poses)
    _same(got, Q.reference(sc, _tile()[0]))
    n = sc["nt"]; pt = np.concatenate(point)
    worst = 0.0; judged = 0
    for j in range(n):
        members = sc["obs"][sc["off"][j]:sc["off"][j + 1]]
        ids = pt[members]
        if ti.cpu().numpy()[j] == len(members) and ids[0] >= 0 and (ids == ids[0]).all() and got["info"][j, 4] == Q.OK:
            worst = max(worst, float(np.abs(got["X"][j] - cloud[ids[0]]).max())); judged += 1
    print("chain: tracks", n, "judged", judged, "worst error", worst)
    assert judged >= 50 and worst <= BOUND, (judged, worst)
