"""GPU: refinement of camera poses against triangulated tracks (include/mi_degensac.h mi_degensac_camera_refine_tracks*,
csrc/mi_camera_refine.hip) against tests/camera_refine_ref.py.  Everything is demanded BIT FOR BIT: from the device's own inputs the
restatement gives the poses, cost, info, err, img_offsets and img_obs at full length, fills included, with guard elements around every
output.  Observation counts per image sit at the edges of a wave and of a row-pass step (63 .. 65, 255 .. 257, 511 .. 513, 1023 .. 1025)
and beyond (2049)."""
import ctypes as C
import functools

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import camera_refine_ref as Q

pytestmark = pytest.mark.gpu
GUARD = 8                                                              # guard elements on each side of an output
PER = dict(poses=12, cost=2, info=4, err=1, io=1, iobs=1)
FILL = dict(poses=-7.0, cost=-7.0, info=-5, err=-3.0, io=-9, iobs=-9)
DT = dict(info="int32", io="int64", iobs="int32")
OPTIONAL = ("err", "io", "iobs")
SCENES = ["counts", "masks", "empty", "many", "edges", "poses", "hand", "exact", "near"]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _scenes():
    return Q.gpu_scenes()


@functools.lru_cache(maxsize=None)
def _want(name, nt="scene", **kw):
    """the restatement on a scene of the catalogue: computed once, shared, never written to"""
    sc = _scenes()[name]
    if nt != "scene":
        sc = dict(sc, nt=nt)
    return Q.reference(sc, **kw)


def _len(k, n, M):
    return M if k in ("err", "iobs") else n + 1 if k == "io" else n


def _outs(torch, n, M):
    out = {}
    for k, per in PER.items():
        ln = _len(k, n, M)
        buf = torch.full(((ln + 2 * GUARD) * per,), FILL[k], dtype=getattr(torch, DT.get(k, "float64")), device="cuda")
        out[k] = (buf, buf[GUARD * per:(GUARD + ln) * per])
    return out


def _call(torch, sc, nt="scene", max_trials=20, ftol=1e-12, outs=None, stream=None, skip=(), alias=False):
    """mi_degensac_camera_refine_tracks_dev on the scene with guarded outputs (outs: the buffers of an earlier call, reused as they are;
    skip: the optional outputs passed as NULL; alias: the input poses are the output buffer).  Returns (dict of numpy results, outs)."""
    T = len(sc["off"]) - 1; M = len(sc["obs"]); n = len(sc["cams"])
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    off, obs, img, kps, cams, poses, X, keep, ref = (t(sc[k]) for k in ("off", "obs", "img", "kps", "cams", "poses", "X", "keep", "refine"))
    v = sc["nt"] if nt == "scene" else nt
    ntd = None if v is None else torch.tensor([v], dtype=torch.int64, device="cuda")
    if outs is None:
        outs = _outs(torch, n, M)
    if alias:
        outs["poses"][1].copy_(poses.reshape(-1)); poses = outs["poses"][1]
    s = torch.cuda.current_stream() if stream is None else stream
    d = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()          # noqa: E731
    p = lambda k: None if k in skip or outs[k][1].numel() == 0 else outs[k][1].data_ptr()         # noqa: E731
    rc = _lib.lib().mi_degensac_camera_refine_tracks_dev(d(off), d(obs), d(img), d(ntd), d(kps), len(sc["kps"]), d(cams), d(poses), n, d(X), d(keep), d(ref),
                                                         T, M, max_trials, ftol, 0, C.c_void_p(s.cuda_stream), *(p(k) for k in PER))
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
    L = _lib.lib()
    assert sorted(SCENES) == sorted(_scenes())
    assert [L.mi_degensac_camera_refine_tile(i) for i in range(4)] == [_lib.CAMREF_STEP, _lib.CAMREF_GRID, _lib.CAMREF_GROUP, -1]
    S = _scenes()
    assert _want("counts")["info"][:, 0].tolist() == Q.COUNTS and S["counts"]["off"][0] == 3 and (S["counts"]["obs"][-5:] == -1).all()
    assert {0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049} == set(Q.COUNTS)
    assert _want("masks")["info"][:3, 0].tolist() == [64, 4, 3]        # the last wave only, one per wave, exactly 3 among 300
    assert (S["masks"]["img"] == 2).sum() == 300
    assert _want("empty")["info"][:, 0].tolist() == Q.EMPTY and Q.EMPTY[0] == Q.EMPTY[-1] == 0
    assert len(S["many"]["cams"]) == 300 > _lib.CAMREF_GRID            # a second stride step runs
    seen = {s for n in SCENES for s in _want(n)["info"][:, 3].tolist()} | set(_want("hand", max_trials=2)["info"][:, 3].tolist())
    assert seen == set(range(9))                                       # every status
    assert _want("hand")["info"][:, 3].tolist() == [Q.BAD_CAMERA, Q.BAD_POSE, Q.SHORT, Q.NOT_FINITE, Q.BEHIND, Q.FIXED, Q.STALLED, Q.CONVERGED, Q.CONVERGED]


@pytest.mark.parametrize("name", SCENES)
def test_refine_equals_restatement(torch, name):
    """every scene: counts at the edges with a non-zero first offset and unowned positions behind, used observations in the last wave only,
    one per wave and 3 among 300, images without observations first, last and in runs, 300 images, ranges beyond M, decreasing and
    negative, NaN rows of X, indices out of range, keypoints that are not finite, two keypoints of one image, poses and cameras that are
    zero, NaN, inf and 1e+-150, every status by hand, exact data, trial poses that put observations behind the camera"""
    got, _ = _call(torch, _scenes()[name])
    want = _want(name)
    _same(got, want)
    ran = want["info"][:, 3] <= Q.FIXED
    assert np.isfinite(got["cost"][ran]).all() and (got["cost"][ran, 1] <= got["cost"][ran, 0]).all()
    none = want["info"][:, 3] >= Q.NOT_FINITE
    assert np.isnan(got["cost"][none]).all() and _bits(got["poses"][~ran], np.asarray(_scenes()[name]["poses"]).reshape(-1, 12)[~ran])


@pytest.mark.parametrize("max_trials, ftol", [(0, 1e-12), (1, 1e-12), (2, 1e-12), (100, 1e-12), (20, 0.0), (20, 1.0), (100, 0.0)])
def test_scalars(torch, max_trials, ftol):
    for name in ("counts", "hand", "poses"):
        got, _ = _call(torch, _scenes()[name], max_trials=max_trials, ftol=ftol)
        _same(got, _want(name, max_trials=max_trials, ftol=ftol))
        assert (got["info"][:, 1] <= max_trials).all()
        ran = got["info"][:, 3] <= Q.MAX_TRIALS
        if max_trials == 0:                                            # scores only
            assert not got["info"][:, 1:3].any() and _bits(got["cost"][ran, 0], got["cost"][ran, 1]) and (got["info"][ran, 3] == Q.MAX_TRIALS).all()
        if ftol == 1.0:                                                # the first accepted step ends the run
            assert (got["info"][:, 2] <= 1).all()
        if ftol == 0.0:                                                # no accepted step can end it
            assert not (got["info"][:, 3] == Q.CONVERGED).any()


@pytest.mark.parametrize("nt", [None, 0, 1, 300, 600, 601, 5000, -4])
def test_n_tracks_below_at_above_and_none(torch, nt):
    got, _ = _call(torch, _scenes()["many"], nt=nt)
    _same(got, _want("many", nt=nt))
    if nt in (0, -4):
        assert (got["info"][:, 3] == Q.SHORT).all() and (got["iobs"] == -1).all() and not got["io"].any()


def test_masks(torch):
    """obs_keep all zero; refine all zero and mixed; the triangulation's kind of mask as bool bytes"""
    sc = _scenes()["empty"]
    M = len(sc["obs"]); n = len(sc["cams"])
    none = dict(sc, keep=np.zeros(M, np.uint8))
    got, _ = _call(torch, none)
    _same(got, Q.reference(none))
    assert (got["info"][:, 3] == Q.SHORT).all() and np.isnan(got["err"]).all() and (got["iobs"] == -1).all()
    fixed = dict(sc, refine=np.zeros(n, np.uint8))
    got, _ = _call(torch, fixed)
    _same(got, Q.reference(fixed))
    full = got["info"][:, 0] >= 3
    assert (got["info"][full, 3] == Q.FIXED).all() and _bits(got["poses"], sc["poses"]) and _bits(got["cost"][:, 0], got["cost"][:, 1])
    assert np.isfinite(got["err"]).sum() == got["info"][full, 0].sum()
    mixed = dict(sc, refine=(np.arange(n) % 3 == 0).astype(np.uint8) * 255, keep=(np.arange(M) % 5 != 0).astype(np.uint8) * 7)
    got, _ = _call(torch, mixed)
    _same(got, Q.reference(mixed))


def test_null_optional_outputs(torch):
    sc = _scenes()["counts"]
    full, _ = _call(torch, sc)
    for skip in (OPTIONAL, ("err",), ("io",), ("iobs",), ("io", "iobs")):
        part, _ = _call(torch, sc, skip=skip)
        assert sorted(part) == sorted(set(PER) - set(skip)) and all(_bits(part[k], full[k]) for k in part)


def test_output_pose_aliases_the_input(torch):
    for name in ("many", "poses"):
        got, _ = _call(torch, _scenes()[name], alias=True)
        _same(got, _want(name))


def test_outputs_reused_and_ten_identical_calls(torch):
    """a long scene, then a short one into the same buffers (what the first call left must not show), then ten calls with identical bytes"""
    a = _scenes()["counts"]; b = _scenes()["hand"]
    _, outs = _call(torch, a)
    n, M = len(b["cams"]), len(b["obs"])
    ln = lambda k: _len(k, n, M)                                       # noqa: E731
    small = {k: (buf[:(ln(k) + 2 * GUARD) * PER[k]], buf[GUARD * PER[k]:(GUARD + ln(k)) * PER[k]]) for k, (buf, _) in outs.items()}
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


def test_same_bytes_whichever_images_a_workgroup_handled_before(torch):
    """the 300 images renumbered in reverse: every workgroup meets other images before each of its own, and every image has the same bytes"""
    sc = _scenes()["many"]; n = len(sc["cams"])
    rev = dict(sc); new = n - 1 - np.arange(n)
    rev["img"] = np.where(sc["img"] >= 0, n - 1 - sc["img"], sc["img"]).astype(np.int32)
    rev["cams"] = sc["cams"][new].copy(); rev["poses"] = sc["poses"][new].copy()
    got, _ = _call(torch, rev)
    want = _want("many")
    for k in ("poses", "cost", "info"):
        assert _bits(got[k], want[k][new]), k
    assert _bits(got["err"], want["err"])                              # track-major: the positions did not move


def test_second_stream(torch):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = _call(torch, _scenes()["many"], stream=s)
    _same(got, _want("many"))


def test_zero_sizes(torch):
    L = _lib.lib()
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    tail = (20, 1e-12, 0, None)
    assert L.mi_degensac_camera_refine_tracks_dev(off.data_ptr(), None, None, None, None, 0, None, None, 0, None, None, None, 0, 0, *tail, *([None] * 6)) == 0
    # no images, with observations: the fills are all that is written
    obs = torch.zeros(5, dtype=torch.int32, device="cuda"); er = torch.zeros(5, dtype=torch.float64, device="cuda")
    io = torch.ones(1, dtype=torch.int64, device="cuda"); iobs = torch.zeros(5, dtype=torch.int32, device="cuda")
    assert L.mi_degensac_camera_refine_tracks_dev(off.data_ptr(), obs.data_ptr(), obs.data_ptr(), None, None, 0, None, None, 0, None, None, None, 0, 5, *tail,
                                                  None, None, None, er.data_ptr(), io.data_ptr(), iobs.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.isnan(er.cpu().numpy()).all() and io.item() == 0 and (iobs.cpu().numpy() == -1).all()
    # images without tracks and without observations: every image is SHORT, or has a bad camera
    cams = torch.tensor([[1.0, 1, 0, 0], [0.0, 1, 0, 0]], dtype=torch.float64, device="cuda"); poses = torch.arange(24, dtype=torch.float64, device="cuda")
    out = torch.zeros(24, dtype=torch.float64, device="cuda"); cost = torch.zeros(4, dtype=torch.float64, device="cuda")
    info = torch.ones((2, 4), dtype=torch.int32, device="cuda"); io = torch.ones(3, dtype=torch.int64, device="cuda")
    assert L.mi_degensac_camera_refine_tracks_dev(off.data_ptr(), None, None, None, None, 0, cams.data_ptr(), poses.data_ptr(), 2, None, None, None, 0, 0, *tail,
                                                  out.data_ptr(), cost.data_ptr(), info.data_ptr(), None, io.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [[0, 0, 0, Q.SHORT], [0, 0, 0, Q.BAD_CAMERA]] and not io.cpu().numpy().any()
    assert np.isnan(cost.cpu().numpy()).all() and (out == poses).all()


def _split(sc):
    n = len(sc["cams"])
    return sc["off"], sc["obs"], sc["img"], sc["kps"], sc["cams"], sc["poses"][:, :9].reshape(n, 3, 3), np.ascontiguousarray(sc["poses"][:, 9:]), sc["X"]


def _pack(res, keys):
    got = dict(zip(keys, res))
    got["poses"] = np.concatenate([np.asarray(got.pop("R")).reshape(-1, 9), np.asarray(got.pop("t"))], 1)
    return got


def test_numpy_form():
    for name, kw in (("counts", {}), ("hand", dict(max_trials=2, ftol=0.5)), ("masks", {})):
        sc = _scenes()[name]
        res = matcher.refine_cameras(*_split(sc), obs_keep=sc["keep"], refine=sc["refine"], with_err=True, with_table=True, **kw)
        _same(_pack(res, ("R", "t", "cost", "info", "err", "io", "iobs")), _want(name, **kw))
    sc = _scenes()["many"]
    res = matcher.refine_cameras(*_split(sc), n_tracks=300)
    assert len(res) == 4
    _same(_pack(res, ("R", "t", "cost", "info")), {k: v for k, v in _want("many", nt=300).items() if k not in OPTIONAL})
    res = matcher.refine_cameras(*_split(sc), with_table=True)
    assert len(res) == 6 and _bits(res[4], _want("many")["io"]) and _bits(res[5], _want("many")["iobs"])


def test_tensor_form_takes_wide_keypoints_and_bool_masks(torch):
    """kps [rows, 6] with x, y in front, a non-contiguous R, n_tracks as the device word, bool masks"""
    from pydegensac_amd import tensor_api as T
    sc = _scenes()["masks"]
    off, obs, img, kps, cams, R, t, X = _split(sc)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    wide = np.concatenate([kps, np.full((len(kps), 4), np.nan)], 1)
    Rt = c(R.transpose(0, 2, 1)).transpose(1, 2)
    res = T.refine_cameras_tensors(c(off), c(obs), c(img), c(wide), c(cams), Rt, c(t), c(X), n_tracks=torch.tensor([len(off) - 1], device="cuda"),
                                   obs_keep=c(sc["keep"]).bool(), refine=torch.ones(len(cams), dtype=torch.bool, device="cuda"), with_err=True,
                                   with_table=True)
    _same(_pack([v.cpu().numpy() for v in res], ("R", "t", "cost", "info", "err", "io", "iobs")), _want("masks"))
    short = T.refine_cameras_tensors(c(off), c(obs), c(img), c(kps), c(cams), c(R), c(t), c(X))
    n = len(cams)
    assert len(short) == 4 and short[0].shape == (n, 3, 3) and short[1].shape == (n, 3) and short[2].shape == (n, 2) and short[3].dtype == torch.int32


def _collection(torch, m, n, seed):
    """verify -> export on a small collection: (keypoints, counts, rows, total, cams, true poses) on the device / host"""
    from pydegensac_amd import synthetic as syn
    from pydegensac_amd import tensor_api as T
    args = dict(m=m, n=n, inlier_ratio=0.6, sigma=0.3, dim=32, seed=seed)
    kps, descs = syn.image_collection(**args)
    K, ps = syn.collection_cameras(m)
    cams = np.tile([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], (m, 1)).astype(np.float64)
    poses = np.ascontiguousarray(np.stack([np.concatenate([R.ravel(), t]) for R, t in ps]))
    counts = [len(k) for k in kps]
    k = torch.from_numpy(np.ascontiguousarray(np.concatenate(kps)[:, :2], dtype=np.float64)).cuda()
    d = torch.from_numpy(np.concatenate(descs).astype(np.float32)).cuda()
    pairs = matcher.exhaustive_pairs(m)
    ver = T.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.8, max_iters=2000)
    rows, co, total = T.correspondences_pairs_tensors(ver[1], counts, counts, pairs, keep=ver[2], store_rows=True)[:3]
    return k, counts, rows, total, cams, poses


def test_chain_export_tracks_triangulate_refine_triangulate_without_sync(torch):
    """export -> tracks_tensors -> triangulate_tracks_tensors -> refine_cameras_tensors -> triangulate_tracks_tensors on a small
    collection under perturbed poses: the last four run under torch's synchronisation check, so nothing is read back between them.  From
    the device's own tables and points the restatement gives every output of the refinement bit for bit."""
    from pydegensac_amd import tensor_api as T
    m = 5
    k, counts, rows, total, cams, truth = _collection(torch, m, 300, 2)
    start = Q.perturb(truth, 0.005, 0.01, seed=3)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    cm, Rm, tv = c(cams), c(start[:, :9].reshape(m, 3, 3)), c(start[:, 9:])
    fix = torch.tensor([0, 0, 1, 1, 1], dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        track, nt, to, obs, oi, ti, no = T.tracks_tensors(rows, counts, total)
        X, tinfo, tcost, cosang, terr, ok, depth = T.triangulate_tracks_tensors(to, obs, oi, k, cm, Rm, tv, n_tracks=nt, with_obs=True)
        res = T.refine_cameras_tensors(to, obs, oi, k, cm, Rm, tv, X, n_tracks=nt, obs_keep=ok, refine=fix, with_err=True, with_table=True)
        X2 = T.triangulate_tracks_tensors(to, obs, oi, k, cm, res[0], res[1], n_tracks=nt)[0]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = _pack([v.cpu().numpy() for v in res], ("R", "t", "cost", "info", "err", "io", "iobs"))
    sc = dict(off=to.cpu().numpy(), obs=obs.cpu().numpy(), img=oi.cpu().numpy(), nt=int(nt.item()), kps=k.cpu().numpy(), cams=cams, poses=start,
              X=X.cpu().numpy(), keep=ok.cpu().numpy().astype(np.uint8), refine=fix.cpu().numpy())
    _same(got, Q.reference(sc))
    assert got["info"][:2, 3].tolist() == [Q.FIXED, Q.FIXED] and (got["info"][2:, 3] <= Q.MAX_TRIALS).all() and (got["info"][:, 0] >= 20).all()
    assert np.isfinite(X2.cpu().numpy()).any()
    both = np.isfinite(got["err"])                                     # next to the triangulation's err: the same positions are written
    assert both.sum() == got["info"][:, 0].sum() and np.isfinite(terr.cpu().numpy()[both]).all()


def test_two_rounds_of_alternation_lower_the_summed_cost(torch):
    """6 images x 200 points, poses off by 0.01 rad and 0.02: triangulate <-> refine_cameras twice with the first two cameras held; the
    summed cost of the second round's start is below the first round's start, and each round's end below its start"""
    from pydegensac_amd import tensor_api as T
    m = 6
    k, counts, rows, total, cams, truth = _collection(torch, m, 200, 4)
    start = Q.perturb(truth, 0.01, 0.02, seed=5); start[:2] = truth[:2]
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    cm, Rm, tv = c(cams), c(start[:, :9].reshape(m, 3, 3)), c(start[:, 9:])
    fix = torch.tensor([0, 0, 1, 1, 1, 1], dtype=torch.uint8, device="cuda")
    track, nt, to, obs, oi, ti, no = T.tracks_tensors(rows, counts, total)
    sums = []
    for _ in range(2):
        X, _, _, _, _, ok, _ = T.triangulate_tracks_tensors(to, obs, oi, k, cm, Rm, tv, n_tracks=nt, with_obs=True)
        if not sums:
            keep = ok                                                  # one set of observations for both rounds: the sums are comparable
        Rm, tv, cost, info = T.refine_cameras_tensors(to, obs, oi, k, cm, Rm, tv, X, n_tracks=nt, obs_keep=keep, refine=fix)
        assert (info[:, 3] <= Q.FIXED).all()
        sums.append(cost.sum(0).cpu().numpy())
    print("alternation: summed cost per round (start, end)", sums)
    assert sums[0][1] < sums[0][0] and sums[1][1] < sums[1][0] and sums[1][1] < sums[0][1]
