"""GPU: refinement of relative poses on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_refine_lists*,
csrc/mi_pose_refine.hip) against tests/pose_refine_ref.py.  Everything is demanded BIT FOR BIT: from the device's own inputs the
restatement gives pose_out, cost, info, resid and F, with guard elements around every output.  Entry lengths sit at the edges of the rule
(4, 5, 6 rows), of a wave (63 .. 65), of a load of the workgroup (255 .. 257, 511 .. 513) and of a step of the row pass (1023 .. 1025,
2049 = a third step)."""
import ctypes as C
import functools

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import pose_ref as P
from tests import pose_refine_ref as Q

pytestmark = pytest.mark.gpu
G = 8                                                                  # guard elements on each side of an output
PER = dict(pose=12, cost=2, info=4, resid=1, F=9)
FILL = dict(pose=-7.0, cost=-7.0, info=-5, resid=-3.0, F=-7.0)
SCENES = ["lengths", "keep", "many", "offsets", "poses", "cameras", "bad_rows", "rotation"]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _want(name, max_trials=20, ftol=1e-12):
    """the restatement on a scene of the catalogue: computed once, shared, never written to"""
    return Q.reference(Q.gpu_scenes()[name], max_trials, ftol)


def _outs(torch, K, cap):
    out = {}
    for k, per in PER.items():
        n = cap if k == "resid" else K
        buf = torch.full(((n + 2 * G) * per,), FILL[k], dtype=torch.int32 if k == "info" else torch.float64, device="cuda")
        out[k] = (buf, buf[G * per:(G + n) * per])
    return out


def _call(torch, sc, max_trials=20, ftol=1e-12, outs=None, stream=None, skip=(), alias=False):
    """mi_degensac_pose_refine_lists_dev on the scene with guarded outputs (outs: the buffers of an earlier call, reused as they are; skip:
    the optional outputs passed as NULL; alias: pose_out is the input pose array itself).  Returns (dict of numpy results, outs)."""
    K = len(sc["off"]) - 1; cap = len(sc["pts"])
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    pts, off, cams, idx, keep = t(sc["pts"]), t(sc["off"]), t(sc["cams"]), t(sc["idx"]), t(sc["keep"])
    if outs is None:
        outs = _outs(torch, K, cap)
    if alias:
        outs["pose"][1].copy_(t(sc["pose"]).reshape(-1))
        pose = outs["pose"][1]
    else:
        pose = t(sc["pose"])
    s = torch.cuda.current_stream() if stream is None else stream
    d = lambda x: None if x is None else x.data_ptr()                  # noqa: E731
    p = lambda k: None if k in skip else outs[k][1].data_ptr()         # noqa: E731
    rc = _lib.lib().mi_degensac_pose_refine_lists_dev(d(pts), d(off), d(keep), d(pose), d(cams), len(sc["cams"]), d(idx), K, cap, max_trials, ftol, 0,
                                                      C.c_void_p(s.cuda_stream), p("pose"), p("cost"), p("info"), p("resid"), p("F"))
    _lib.check_match(rc)
    s.synchronize()
    res = {}
    for k, (buf, view) in outs.items():
        whole = buf.cpu().numpy(); per = PER[k]
        assert (whole[:G * per] == FILL[k]).all() and (whole[len(whole) - G * per:] == FILL[k]).all(), f"{k}: a guard element was written"
        body = whole[G * per:len(whole) - G * per]
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
        assert _bits(got[k], w), (k, np.flatnonzero((got[k] != w).reshape(len(w), -1).any(axis=1))[:8])


def test_scene_list_is_the_catalogue():
    assert sorted(SCENES) == sorted(Q.gpu_scenes())
    L = _lib.lib()
    assert L.mi_degensac_pose_refine_tile(1) == _lib.REFINE_GRID == 256 < 300 and L.mi_degensac_pose_refine_tile(0) == _lib.REFINE_STEP == 1024
    S = Q.gpu_scenes()
    assert np.diff(S["lengths"]["off"]).tolist() == Q.LENGTHS and S["lengths"]["off"][0] == 3 and len(S["lengths"]["pts"]) == S["lengths"]["off"][-1] + 5
    assert len(S["many"]["off"]) - 1 == 300
    seen = {s for n in SCENES for s in _want(n)["info"][:, 3].tolist()} | set(_want("lengths", 1)["info"][:, 3].tolist())
    assert seen == set(range(8))                                       # every status


@pytest.mark.parametrize("name", SCENES)
def test_refine_equals_restatement(torch, name):
    """every scene: lengths at the edges, a non-zero o[0] and unowned rows behind, used rows in the last wave only, one per wave and exactly
    5 among 300, keep all zero, empty entries first, last and between, 300 entries on a grid of 256, ranges that cross cap / start beyond
    it / decrease, zero / NaN / inf / 1e+-150 start poses, refused cameras and camera indices, rows that are not finite, a pure rotation"""
    got, _ = _call(torch, Q.gpu_scenes()[name])
    want = _want(name)
    _same(got, want)
    run = want["info"][:, 3] <= Q.MAX_TRIALS
    assert np.isfinite(got["pose"][run]).all() and np.isfinite(got["cost"][run]).all() and (got["cost"][run, 1] <= got["cost"][run, 0]).all()
    assert np.isnan(got["cost"][~run]).all()


@pytest.mark.parametrize("max_trials, ftol", [(0, 1e-12), (1, 1e-12), (20, 0.0), (20, 1.0), (100, 0.0)])
def test_scalars(torch, max_trials, ftol):
    for name in ("lengths", "keep"):
        got, _ = _call(torch, Q.gpu_scenes()[name], max_trials, ftol)
        _same(got, _want(name, max_trials, ftol))
        run = got["info"][:, 3] <= Q.MAX_TRIALS
        if max_trials == 0:                                            # scores only
            assert (got["info"][run, 3] == Q.MAX_TRIALS).all() and not got["info"][run, 1:3].any() and _bits(got["pose"], Q.gpu_scenes()[name]["pose"])
            assert np.array_equal(got["cost"][run, 0], got["cost"][run, 1])
        if ftol == 1.0:                                                # the first accepted step ends the run
            assert (got["info"][run & (got["info"][:, 3] == Q.CONVERGED), 2] == 1).all()


def test_null_optional_outputs_and_aliased_pose(torch):
    sc = Q.gpu_scenes()["lengths"]
    full, _ = _call(torch, sc)
    part, _ = _call(torch, sc, skip=("resid", "F"))
    assert sorted(part) == ["cost", "info", "pose"] and all(_bits(part[k], full[k]) for k in part)
    part, _ = _call(torch, sc, skip=("resid",))
    assert "F" in part and all(_bits(part[k], full[k]) for k in part)
    for name in ("lengths", "many", "poses", "offsets"):               # pose_out is the pose array itself
        got, _ = _call(torch, Q.gpu_scenes()[name], alias=True)
        _same(got, _want(name))


def test_outputs_reused_and_ten_identical_calls(torch):
    """a long scene, then a short one into the same buffers (what the first call left must not show), then ten calls with identical bytes"""
    a = Q.gpu_scenes()["lengths"]; b = Q.gpu_scenes()["offsets"]
    _, outs = _call(torch, a)
    K, cap = len(b["off"]) - 1, len(b["pts"])
    small = {k: (buf[:((cap if k == "resid" else K) + 2 * G) * PER[k]], buf[G * PER[k]:(G + (cap if k == "resid" else K)) * PER[k]]) for k, (buf, _) in outs.items()}
    for k, (buf, view) in small.items():                               # the guard behind the shorter body
        buf[len(buf) - G * PER[k]:] = FILL[k]
    got, _ = _call(torch, b, outs=small)
    _same(got, _want("offsets"))
    sc = Q.gpu_scenes()["keep"]
    first, o2 = _call(torch, sc)
    for _ in range(9):
        again, _ = _call(torch, sc, outs=o2)
        for k in first:
            assert first[k].tobytes() == again[k].tobytes(), k


def test_same_bytes_whichever_entries_came_before(torch):
    """the 300 entries in reverse order: every workgroup meets other entries before each of its own, and every entry has the same bytes"""
    sc = Q.gpu_scenes()["many"]; K = len(sc["off"]) - 1
    order = np.arange(K)[::-1]
    lens = np.diff(sc["off"])[order]
    rev = dict(sc); rev["off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rev["pts"] = np.concatenate([sc["pts"][sc["off"][p]:sc["off"][p + 1]] for p in order]); rev["idx"] = sc["idx"][order].copy(); rev["pose"] = sc["pose"][order].copy()
    got, _ = _call(torch, rev)
    want = _want("many")
    for k in ("pose", "cost", "info", "F"):
        assert _bits(got[k], want[k][order]), k
    assert _bits(got["resid"], np.concatenate([want["resid"][sc["off"][p]:sc["off"][p + 1]] for p in order]))


def test_second_stream(torch):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = _call(torch, Q.gpu_scenes()["many"], stream=s)
    _same(got, _want("many"))


def test_k0_and_cap0(torch):
    L = _lib.lib()
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.mi_degensac_pose_refine_lists_dev(None, off.data_ptr(), None, None, None, 0, None, 0, 0, 20, 1e-12, 0, None, *([None] * 5)) == 0
    # K == 0 with rows: the fill is all that is written
    pts = torch.zeros((5, 4), dtype=torch.float64, device="cuda"); rs = torch.zeros(5, dtype=torch.float64, device="cuda")
    assert L.mi_degensac_pose_refine_lists_dev(pts.data_ptr(), off.data_ptr(), None, None, None, 0, None, 0, 5, 20, 1e-12, 0, None, None, None, None,
                                               rs.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.isnan(rs.cpu().numpy()).all()
    # K > 0 with cap == 0: every entry is short or truncated
    off = torch.tensor([0, 0, 3], dtype=torch.int64, device="cuda")
    pose = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0]] * 2, dtype=torch.float64, device="cuda")
    cams = torch.tensor([[800.0, 800, 500, 375]] * 4, dtype=torch.float64, device="cuda")
    out = torch.zeros((2, 12), dtype=torch.float64, device="cuda"); cost = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    info = torch.ones((2, 4), dtype=torch.int32, device="cuda")
    assert L.mi_degensac_pose_refine_lists_dev(None, off.data_ptr(), None, pose.data_ptr(), cams.data_ptr(), 4, None, 2, 0, 20, 1e-12, 0, None,
                                               out.data_ptr(), cost.data_ptr(), info.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [[0, 0, 0, Q.SHORT], [0, 0, 0, Q.TRUNCATED]] and np.isnan(cost.cpu().numpy()).all()
    assert np.array_equal(out.cpu().numpy(), pose.cpu().numpy())


def _as_results(K, res):
    Rm, t, cost, info, resid, F = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in res)
    return dict(pose=np.concatenate([Rm.reshape(K, 9), t], 1), cost=cost, info=info, resid=resid, F=F.reshape(K, 9))


def test_numpy_form_per_entry_cameras_and_keep():
    sc = Q.gpu_scenes()["lengths"]; K = len(sc["off"]) - 1
    res = matcher.refine_pose(sc["pts"], sc["off"], sc["pose"][:, :9].reshape(K, 3, 3), sc["pose"][:, 9:], sc["cams"].reshape(K, 8), with_resid=True,
                              with_F=True)
    _same(_as_results(K, res), _want("lengths"))
    sc = Q.gpu_scenes()["keep"]; K = len(sc["off"]) - 1
    res = matcher.refine_pose(sc["pts"], sc["off"], sc["pose"][:, :9].reshape(K, 3, 3), sc["pose"][:, 9:], sc["cams"], pairs=sc["idx"],
                              keep=sc["keep"].astype(bool), max_trials=1, ftol=0.5, with_resid=True, with_F=True)
    _same(_as_results(K, res), _want("keep", 1, 0.5))
    assert len(matcher.refine_pose(sc["pts"], sc["off"], sc["pose"][:, :9].reshape(K, 3, 3), sc["pose"][:, 9:], sc["cams"], pairs=sc["idx"])) == 4
    # the same call without any optional output: R, t, cost and info are the bits of the call above
    bare = matcher.refine_pose(sc["pts"], sc["off"], sc["pose"][:, :9].reshape(K, 3, 3), sc["pose"][:, 9:], sc["cams"], pairs=sc["idx"],
                               keep=sc["keep"].astype(bool), max_trials=1, ftol=0.5)
    assert len(bare) == 4 and all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(bare, res[:4]))


def test_tensor_form_by_index_shared_camera_and_two_stores(torch):
    """cameras by index on one table, then the same list over two stores: store 2 holds the cameras in another order, and an image of
    store 1 beyond its table must not reach into store 2's rows"""
    from pydegensac_amd import tensor_api as T
    sc = Q.gpu_scenes()["many"]; K = len(sc["off"]) - 1
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    Rm, tv = c(sc["pose"][:, :9].reshape(K, 3, 3)), c(sc["pose"][:, 9:])
    res = T.refine_pose_tensors(c(sc["pts"]), c(sc["off"]), Rm, tv, c(sc["cams"]), pairs=c(sc["idx"]), with_resid=True, with_F=True)
    one = _as_results(K, res)
    _same(one, _want("many"))
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4]); inv = np.argsort(perm)
    pairs2 = np.stack([sc["idx"][:, 0], inv[sc["idx"][:, 1]]], 1).astype(np.int64)
    pairs2[7, 0] = 9                                                   # beyond store 1 (8 images): would be row 1 of store 2
    res = T.refine_pose_tensors(c(sc["pts"]), c(sc["off"]), Rm, tv, c(sc["cams"]), pairs=c(pairs2), cams2=c(sc["cams"][perm]), with_resid=True, with_F=True)
    two = _as_results(K, res)
    assert two["info"][7].tolist() == [0, 0, 0, Q.BAD_CAMERA] and _bits(two["pose"][7], sc["pose"][7]) and not two["F"][7].any()
    keep = np.ones(K, bool); keep[7] = False
    rows = np.ones(len(sc["pts"]), bool); rows[sc["off"][7]:sc["off"][8]] = False
    for k in one:
        sel = rows if k == "resid" else keep
        assert _bits(one[k][sel], two[k][sel]), k
    short = T.refine_pose_tensors(c(sc["pts"]), c(sc["off"]), Rm, tv, c(sc["cams"]), pairs=c(sc["idx"]))
    assert len(short) == 4 and short[0].shape == (K, 3, 3) and short[1].shape == (K, 3) and short[2].shape == (K, 2) and short[3].dtype == torch.int32


def test_chain_verify_export_refit_pose_refine_without_sync_and_F_fed_back(torch):
    """match_and_verify_pairs_tensors -> correspondences_pairs_tensors -> refit -> pose -> refine on a small collection: the last three run
    under torch's synchronisation check, so nothing is read back between them.  From the device's own inputs the restatement gives the
    refine call's outputs bit for bit; the returned F goes back into relative_pose_tensors and correspondences_pairs_tensors(models=F)."""
    from pydegensac_amd import synthetic as syn
    from pydegensac_amd import tensor_api as T
    m = 4
    kps, descs = syn.image_collection(m=m, n=300, inlier_ratio=0.6, sigma=0.1, dim=32, seed=2)
    Kc, poses = syn.collection_cameras(m)
    counts = [len(k) for k in kps]
    k = torch.from_numpy(np.ascontiguousarray(np.concatenate(kps)[:, :2], dtype=np.float64)).cuda()
    d = torch.from_numpy(np.concatenate(descs).astype(np.float32)).cuda()
    pairs = matcher.exhaustive_pairs(m)
    ver = T.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.8, max_iters=2000)
    F = ver[0]
    rows, co, total, entry, pts, resid = T.correspondences_pairs_tensors(ver[1], counts, counts, pairs, keep=ver[2], kps1=k, kps2=k, models=F)
    cam = [Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]
    cams = torch.tensor([cam] * m, dtype=torch.float64, device="cuda")
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        M, inl, info_r = T.refit_correspondences_tensors(pts, co, F, "F")
        Rm, t, front, info = T.relative_pose_tensors(pts, co, M, cams, pairs=pr, keep=inl)
        R2, t2, cost, info2, rs, F2 = T.refine_pose_tensors(pts, co, Rm, t, cams, pairs=pr, keep=front, with_resid=True, with_F=True)
        back = T.relative_pose_tensors(pts, co, F2, cams, pairs=pr, keep=front)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    K = len(pairs)
    sc = dict(pts=pts.cpu().numpy(), off=co.cpu().numpy(), cams=cams.cpu().numpy(), idx=np.asarray(pairs, np.int32), keep=front.cpu().numpy().astype(np.uint8),
              pose=np.concatenate([Rm.cpu().numpy().reshape(K, 9), t.cpu().numpy()], 1))
    got = _as_results(K, (R2, t2, cost, info2, rs, F2))
    _same(got, Q.reference(sc))
    assert (got["info"][:, 3] == Q.CONVERGED).all() and (got["info"][:, 0] == info.cpu().numpy()[:, 1]).all()
    # the refined pose is the generator's to a degree (the bounds of the pose call's own chain test), and the pose call on the returned F finds it again with every row in front
    Rb, tb, fb, ib = (x.cpu().numpy() for x in back)
    for p, (i, j) in enumerate(np.asarray(pairs)):
        Rg, tg = P.relative(poses, int(i), int(j))
        assert P.rot_err_deg(got["pose"][p, :9], Rg) < 1.0 and P.dir_err_deg(got["pose"][p, 9:], tg) < 5.0, (p, P.dir_err_deg(got["pose"][p, 9:], tg))
        assert np.abs(Rb[p] - got["pose"][p, :9].reshape(3, 3)).max() < 1e-9 and np.abs(tb[p] - got["pose"][p, 9:]).max() < 1e-9
    assert (ib[:, 4] == 0).all() and (ib[:, 0] == got["info"][:, 0]).all()
    # the export takes the returned F as its models: the same rows, a finite residual on every one of them
    again = T.correspondences_pairs_tensors(ver[1], counts, counts, pairs, keep=ver[2], kps1=k, kps2=k, models=F2)
    n = int(total.item())
    assert torch.equal(again[4][:n], pts[:n]) and bool(torch.isfinite(again[5][:n]).all())          # (rows behind `total` are NaN)
