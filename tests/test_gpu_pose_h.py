"""GPU: relative pose from a homography on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_h_lists*,
csrc/mi_pose_h.hip) against tests/pose_h_ref.py.  The device's candidates equal the independent numpy decomposition (numpy.linalg.svd,
Faugeras' closed form) as a set, to 1e-9, and the restatement of the header's rule bit for bit.  Everything behind the candidates is
demanded BIT FOR BIT from the device's own candidates and normals: cand_front, front, info, X, depth, cosang, normal and t_over_d, with
guard elements around every output.  Entry lengths sit at the edges of a wave (63 .. 65), of a load of the workgroup (255 .. 257) and of a
step of the row pass (1023 .. 1025, 2049 = a third step)."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import pose_h_ref as Hr
from tests import pose_ref as R

pytestmark = pytest.mark.gpu
G = 8                                                                  # guard elements on each side of an output
PER = dict(pose=12, front=1, info=5, normal=3, t_over_d=1, X=3, depth=2, cosang=1, cand=48, cand_normal=12, cand_front=4)
FILL = dict(pose=-7.0, front=77, info=-5, normal=-7.0, t_over_d=-7.0, X=-3.0, depth=-3.0, cosang=-3.0, cand=-7.0, cand_normal=-7.0, cand_front=-5)
ROWWISE = ("front", "X", "depth", "cosang")
OPTIONAL = ("X", "depth", "cosang", "cand", "cand_normal", "cand_front")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _outs(torch, K, cap):
    dt = {k: torch.float64 for k in PER}
    dt.update(front=torch.uint8, info=torch.int32, cand_front=torch.int32)
    out = {}
    for k, per in PER.items():
        n = cap if k in ROWWISE else K
        buf = torch.full(((n + 2 * G) * per,), FILL[k], dtype=dt[k], device="cuda")
        out[k] = (buf, buf[G * per:(G + n) * per])
    return out


def _call(torch, sc, outs=None, stream=None, skip=()):
    """mi_degensac_pose_h_lists_dev on the scene with guarded outputs (outs: the buffers of an earlier call, reused as they are; skip: the
    optional outputs passed as NULL).  Returns (dict of numpy results, outs)."""
    K = len(sc["off"]) - 1; cap = len(sc["pts"])
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    pts, off, H, cams, idx, keep = t(sc["pts"]), t(sc["off"]), t(sc["H"]), t(sc["cams"]), t(sc["idx"]), t(sc["keep"])
    if outs is None:
        outs = _outs(torch, K, cap)
    s = torch.cuda.current_stream() if stream is None else stream
    d = lambda x: None if x is None else x.data_ptr()                  # noqa: E731
    p = lambda k: None if k in skip else outs[k][1].data_ptr()         # noqa: E731
    cm = sc["cos_min"] if "cos_min" in sc else R.cos_min(sc["deg"])
    rc = _lib.lib().mi_degensac_pose_h_lists_dev(d(pts), d(off), d(keep), d(H), d(cams), len(sc["cams"]), d(idx), K, cap, cm,
                                                 sc.get("rotation_eps", Hr.ROT_EPS), 0, C.c_void_p(s.cuda_stream), *(p(k) for k in PER))
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
    return a.shape == b.shape and a.tobytes() == b.tobytes() if a.dtype.kind != "f" else \
        a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def _compare(sc, got, skip_svd=()):
    """the whole comparison of one call: candidates as a set against numpy's SVD and bit for bit against the restatement of the header,
    everything else bit for bit from the device's own candidates"""
    K = len(sc["off"]) - 1
    own = Hr.from_candidates(sc)                                       # the restatement alone
    if "cand" in got and "cand_normal" in got:
        cand = got["cand"].reshape(K, 4, 12); nrm = got["cand_normal"].reshape(K, 4, 3)
        for p in range(K):
            st = own["info"][p, 4]
            if st in (Hr.TRUNCATED, Hr.BAD_CAMERA, Hr.BAD_MODEL):
                assert not cand[p].any() and not nrm[p].any(), p
                continue
            i1, i2 = Hr.cam_rows(sc, p)
            st2, cd, nr, _ = Hr.candidates_svd(sc["H"][p], sc["cams"][i1], sc["cams"][i2], sc.get("rotation_eps", Hr.ROT_EPS))
            if p in skip_svd:
                continue
            if cand[p, 0, 9:].any():                                   # four solutions of a plane
                assert st2 == Hr.OK and Hr.same_set(cand[p], nrm[p], cd, nr), (p, cand[p], cd)
                Rs = cand[p][:, :9].reshape(4, 3, 3)
                assert np.abs(Rs @ Rs.transpose(0, 2, 1) - np.eye(3)).max() <= Hr.TOL and np.abs(np.linalg.det(Rs) - 1).max() <= Hr.TOL
                for q in range(2):                                     # the header's order
                    assert np.array_equal(cand[p][q, :9], cand[p][q + 2, :9]) and np.array_equal(cand[p][q, 9:], -cand[p][q + 2, 9:])
                    assert np.array_equal(nrm[p][q], -nrm[p][q + 2])
            else:                                                      # a rotation
                assert st2 == Hr.ROTATION and np.abs(cand[p, 0] - cd[0]).max() <= Hr.TOL and not cand[p, 1:].any() and not nrm[p].any()
        want = Hr.from_candidates(sc, cand, nrm)
        assert _bits(got["cand"].reshape(K, 4, 12), own["cand"]) and _bits(got["cand_normal"].reshape(K, 4, 3), own["cand_normal"])
    else:
        want = own
    assert np.array_equal(got["info"], want["info"]), np.flatnonzero((got["info"] != want["info"]).any(axis=1))[:8]
    if "cand_front" in got:
        assert np.array_equal(got["cand_front"], want["cand_front"])
    assert _bits(got["pose"], want["pose"]) and _bits(got["normal"], want["normal"])
    assert _bits(got["t_over_d"], own["t_over_d"])                     # |t / d| is not in the candidates: the restatement's own
    for k in ROWWISE:
        if k in got:
            assert _bits(got[k], want[k].reshape(got[k].shape)), (k, np.flatnonzero((got[k] != want[k].reshape(got[k].shape)).reshape(len(sc["pts"]), -1).any(axis=1))[:8])
    bad = ~np.isin(got["info"][:, 4], (Hr.OK, Hr.ROTATION))
    assert not got["pose"][bad].any() and not got["info"][bad, :4].any() and not got["normal"][bad].any() and not got["t_over_d"][bad].any()
    return want


SCENES = ["lengths", "lengths_exact", "keep", "many", "offsets", "models", "cameras", "bad_rows", "noisy_models", "rotations", "behind"]
SKIP_SVD = {"models": (6,)}                                            # rank 2 to rounding: sigma3 is noise, numpy's need not be the device's


def test_scene_list_is_the_catalogue():
    assert sorted(SCENES) == sorted(Hr.gpu_scenes())
    assert _lib.lib().mi_degensac_pose_h_tile(1) == _lib.POSE_H_GRID < 300 and _lib.lib().mi_degensac_pose_h_tile(0) == _lib.POSE_H_STEP == 1024


@pytest.mark.parametrize("name", SCENES)
def test_pose_equals_restatement(torch, name):
    """every scene: lengths at the tile edges, a non-zero o[0] and unowned rows behind, used rows in the last wave only and one per wave,
    keep all zero, empty entries first, last and between, 300 entries on a grid of 256, ranges that cross cap / start beyond it /
    decrease, zero / NaN / inf / 1e+-150 / rank-2 / mirrored models, refused cameras and camera indices, rows that are not finite, models as
    an estimator returns them, pure rotations and the two sides of rotation_eps, a plane seen from behind"""
    sc = Hr.gpu_scenes()[name]
    got, _ = _call(torch, sc)
    _compare(sc, got, SKIP_SVD.get(name, ()))


def test_every_status_and_the_fills(torch):
    S = Hr.gpu_scenes(); seen = set()
    for name in ("keep", "offsets", "models", "cameras", "rotations"):
        sc = S[name]
        got, _ = _call(torch, sc)
        seen |= set(got["info"][:, 4].tolist())
        own = np.zeros(len(sc["pts"]), bool); tri = np.zeros(len(sc["pts"]), bool)
        for p, (b, e) in enumerate(zip(sc["off"][:-1], sc["off"][1:])):
            if got["info"][p, 4] in (Hr.OK, Hr.ROTATION):
                own[b:e] = True if sc["keep"] is None else sc["keep"][b:e] != 0
                tri[b:e] = own[b:e] & (got["info"][p, 4] == Hr.OK)
        assert not got["front"][~own].any() and np.isnan(got["cosang"][~own]).all() and np.isfinite(got["cosang"][own]).all()
        assert np.isnan(got["X"][~tri]).all() and np.isnan(got["depth"][~tri]).all() and np.isfinite(got["depth"][tri]).all()
    assert seen == set(range(6))


def test_null_optional_outputs(torch):
    sc = Hr.gpu_scenes()["lengths"]
    full, _ = _call(torch, sc)
    part, _ = _call(torch, sc, skip=OPTIONAL)
    assert sorted(part) == ["front", "info", "normal", "pose", "t_over_d"] and all(_bits(part[k], full[k]) for k in part)
    part, _ = _call(torch, sc, skip=("depth", "cand", "cand_normal"))
    assert all(_bits(part[k], full[k]) for k in part) and "X" in part and "cand_front" in part


def test_outputs_reused_and_ten_identical_calls(torch):
    """a long scene, then a short one into the same buffers (what the first call left must not show), then ten calls with identical bytes"""
    a = Hr.gpu_scenes()["lengths"]; b = Hr.gpu_scenes()["offsets"]
    _, outs = _call(torch, a)
    K, cap = len(b["off"]) - 1, len(b["pts"])
    small = {k: (buf, buf[G * PER[k]:(G + (cap if k in ROWWISE else K)) * PER[k]]) for k, (buf, _) in outs.items()}
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    pts, off, H, cams = t(b["pts"]), t(b["off"]), t(b["H"]), t(b["cams"])
    s = torch.cuda.current_stream(); p = lambda k: small[k][1].data_ptr()          # noqa: E731
    _lib.check_match(_lib.lib().mi_degensac_pose_h_lists_dev(pts.data_ptr(), off.data_ptr(), None, H.data_ptr(), cams.data_ptr(), len(b["cams"]), None, K,
                                                             cap, R.cos_min(b["deg"]), Hr.ROT_EPS, 0, C.c_void_p(s.cuda_stream), *(p(k) for k in PER)))
    s.synchronize()
    got = {k: v[1].cpu().numpy().reshape((-1, PER[k]) if PER[k] > 1 else (-1,)) for k, v in small.items()}
    _compare(b, got)
    sc = Hr.gpu_scenes()["keep"]
    first, o2 = _call(torch, sc)
    for _ in range(9):
        again, _ = _call(torch, sc, outs=o2)
        for k in first:
            assert first[k].tobytes() == again[k].tobytes(), k


def test_same_bytes_whichever_entries_came_before(torch):
    """the 300 entries in reverse order: every workgroup handles other entries before a given one, and the entry's bytes are the same"""
    sc = Hr.gpu_scenes()["many"]; K = len(sc["off"]) - 1
    a, _ = _call(torch, sc)
    lens = np.diff(sc["off"]); order = np.arange(K)[::-1]
    off = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int64)
    rv = dict(sc, off=off, H=sc["H"][order], idx=sc["idx"][order],
              pts=np.concatenate([sc["pts"][sc["off"][p]:sc["off"][p + 1]] for p in order] + [sc["pts"][sc["off"][-1]:]]))
    b, _ = _call(torch, rv)
    for k in a:
        if k in ROWWISE:
            for j, p in enumerate(order):
                assert _bits(a[k][sc["off"][p]:sc["off"][p + 1]], b[k][off[j]:off[j + 1]]), (k, p)
        else:
            assert _bits(a[k][order], b[k]), k


def test_second_stream(torch):
    sc = Hr.gpu_scenes()["many"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = _call(torch, sc, stream=s)
    _compare(sc, got)


def test_k0_and_cap0(torch):
    L = _lib.lib()
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.mi_degensac_pose_h_lists_dev(None, off.data_ptr(), None, None, None, 0, None, 0, 0, 0.5, 1e-3, 0, None, *([None] * 11)) == 0
    # K == 0 with rows: the fills are all that is written
    pts = torch.zeros((5, 4), dtype=torch.float64, device="cuda"); fr = torch.full((5,), 9, dtype=torch.uint8, device="cuda")
    X = torch.zeros((5, 3), dtype=torch.float64, device="cuda"); cs = torch.zeros(5, dtype=torch.float64, device="cuda")
    assert L.mi_degensac_pose_h_lists_dev(pts.data_ptr(), off.data_ptr(), None, None, None, 0, None, 0, 5, 0.5, 1e-3, 0, None, None, fr.data_ptr(), None,
                                          None, None, X.data_ptr(), None, cs.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert not fr.cpu().numpy().any() and np.isnan(X.cpu().numpy()).all() and np.isnan(cs.cpu().numpy()).all()
    # K > 0 with cap == 0: every entry is empty or truncated
    off = torch.tensor([0, 0, 3], dtype=torch.int64, device="cuda"); H = torch.eye(3, dtype=torch.float64, device="cuda").repeat(2, 1, 1)
    H[0, 0, 2] = 50.0
    cams = torch.tensor([[800.0, 800, 500, 375]] * 4, dtype=torch.float64, device="cuda")
    pose = torch.ones((2, 12), dtype=torch.float64, device="cuda"); info = torch.ones((2, 5), dtype=torch.int32, device="cuda")
    nrm = torch.ones((2, 3), dtype=torch.float64, device="cuda"); tod = torch.ones(2, dtype=torch.float64, device="cuda")
    assert L.mi_degensac_pose_h_lists_dev(None, off.data_ptr(), None, H.data_ptr(), cams.data_ptr(), 4, None, 2, 0, 0.5, 1e-3, 0, None, pose.data_ptr(),
                                          None, info.data_ptr(), nrm.data_ptr(), tod.data_ptr(), *([None] * 6)) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [[0, 0, 0, 0, Hr.EMPTY], [0, 0, 0, 0, Hr.TRUNCATED]]
    assert not pose.cpu().numpy().any() and not nrm.cpu().numpy().any() and not tod.cpu().numpy().any()


def _as_results(K, cap, res):
    Rm, t, front, info, nrm, tod, X, depth, cosang, cand, cn, cf = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in res)
    return dict(pose=np.concatenate([Rm.reshape(K, 9), t], 1), front=front.astype(np.uint8), info=info, normal=nrm, t_over_d=tod, X=X, depth=depth,
                cosang=cosang, cand=cand.reshape(K, 48), cand_normal=cn.reshape(K, 12), cand_front=cf)


def test_numpy_form_both_model_forms_and_keep():
    sc = Hr.gpu_scenes()["lengths"]; K = len(sc["off"]) - 1
    Hm = sc["H"].reshape(K, 3, 3)
    res = matcher.homography_pose(sc["pts"], sc["off"], Hm, sc["cams"].reshape(K, 8), min_parallax_deg=sc["deg"], with_points=True, with_candidates=True)
    one = _as_results(K, len(sc["pts"]), res)
    _compare(sc, one)
    # the driver's form of the same models: the same poses to the conversion's rounding, and the caller's form H x1 ~ x2 on the rows
    drv = matcher._h_driver_form(Hm)
    res = matcher.homography_pose(sc["pts"], sc["off"], drv, sc["cams"].reshape(K, 8), min_parallax_deg=sc["deg"], driver_form=True)
    assert len(res) == 6 and np.array_equal(res[3][:, 4], one["info"][:, 4])
    assert np.abs(np.concatenate([res[0].reshape(K, 9), res[1]], 1) - one["pose"]).max() <= Hr.TOL
    sc = Hr.gpu_scenes()["keep"]; K = len(sc["off"]) - 1
    res = matcher.homography_pose(sc["pts"], sc["off"], sc["H"].reshape(K, 3, 3), sc["cams"], pairs=sc["idx"], keep=sc["keep"].astype(bool),
                                  min_parallax_deg=sc["deg"], with_points=True, with_candidates=True)
    _compare(sc, _as_results(K, len(sc["pts"]), res))
    bare = matcher.homography_pose(sc["pts"], sc["off"], sc["H"].reshape(K, 3, 3), sc["cams"], pairs=sc["idx"], keep=sc["keep"].astype(bool),
                                   min_parallax_deg=sc["deg"])
    assert len(bare) == 6 and all(a.tobytes() == b.tobytes() for a, b in zip(bare, res[:6]))


def test_tensor_form_by_index_shared_camera_and_two_stores(torch):
    from pydegensac_amd import tensor_api as T
    sc = Hr.gpu_scenes()["many"]; K = len(sc["off"]) - 1; cap = len(sc["pts"])
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    res = T.homography_pose_tensors(c(sc["pts"]), c(sc["off"]), c(sc["H"].reshape(K, 3, 3)), c(sc["cams"]), pairs=c(sc["idx"]),
                                    min_parallax_deg=sc["deg"], with_points=True, with_candidates=True)
    one = _as_results(K, cap, res)
    _compare(sc, one)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4]); inv = np.argsort(perm)
    pairs2 = np.stack([sc["idx"][:, 0], inv[sc["idx"][:, 1]]], 1).astype(np.int64)
    pairs2[7, 0] = 9                                                   # beyond store 1 (8 images): would be row 1 of store 2
    res = T.homography_pose_tensors(c(sc["pts"]), c(sc["off"]), c(sc["H"].reshape(K, 3, 3)), c(sc["cams"]), pairs=c(pairs2), cams2=c(sc["cams"][perm]),
                                    min_parallax_deg=sc["deg"], with_points=True, with_candidates=True)
    two = _as_results(K, cap, res)
    assert two["info"][7].tolist() == [0, 0, 0, 0, Hr.BAD_CAMERA]
    keep = np.ones(K, bool); keep[7] = False
    rows = np.ones(cap, bool); rows[sc["off"][7]:sc["off"][8]] = False
    for k in one:
        sel = rows if k in ROWWISE else keep
        assert _bits(one[k][sel], two[k][sel]), k
    drv = T._h_driver_form(c(sc["H"].reshape(K, 3, 3)))
    short = T.homography_pose_tensors(c(sc["pts"]), c(sc["off"]), drv, c(sc["cams"]), pairs=c(sc["idx"]), driver_form=True)
    assert len(short) == 6 and short[0].shape == (K, 3, 3) and short[1].shape == (K, 3) and short[2].dtype == torch.bool and short[4].shape == (K, 3)
    assert np.abs(short[0].cpu().numpy().reshape(K, 9) - one["pose"][:, :9]).max() <= Hr.TOL


def test_chain_fh_verify_export_pose_select_refine_average_without_sync(torch):
    """F + H verify -> export under H -> homography_pose_tensors -> select_pose_tensors -> refine_pose_tensors -> average_rotations_tensors
    on a small planar collection: everything behind the export runs under torch's synchronisation check.  The exported rows have a small
    residual under the H that goes into the pose call, and the poses are the generator's to a degree."""
    from pydegensac_amd import synthetic as syn
    from pydegensac_amd import tensor_api as T
    m = 4
    kps, descs, truth = syn.planar_collection(m=m, n=300, inlier_ratio=0.7, sigma=0.1, dim=32, seed=3)
    Kc = truth["K"]
    counts = [len(k) for k in kps]
    k = torch.from_numpy(np.ascontiguousarray(np.concatenate(kps)[:, :2], dtype=np.float64)).cuda()
    d = torch.from_numpy(np.concatenate(descs).astype(np.float32)).cuda()
    pairs = matcher.exhaustive_pairs(m)
    ver = T.match_and_verify_fh_pairs_tensors(k, k, d, d, counts, counts, pairs, ratio=0.8)
    F, Hm, match, inl_f, inl_h, summary = ver[0], ver[1], ver[2], ver[3], ver[4], ver[7]
    rows, co, total, entry, pts, resid = T.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inl_h, kps1=k, kps2=k, models=Hm, model="H")
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * m, dtype=torch.float64, device="cuda")
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pose_f = T.relative_pose_tensors(pts, co, F, cams, pairs=pr)
        pose_h = T.homography_pose_tensors(pts, co, Hm, cams, pairs=pr)
        nF = summary[:, 1].double(); nH = summary[:, 2].double()
        cls = torch.where(torch.maximum(nF, nH) < 15, 0, torch.where(nH > 0.8 * nF, 2, 1))
        Rs, ts, front, info, use_h, edge = T.select_pose_tensors(cls, pose_f, pose_h, co)
        Rr, tr, cost, info_r = T.refine_pose_tensors(pts, co, Rs, ts, cams, pairs=pr, keep=front)
        avg = T.average_rotations_tensors(pr, Rr, m, weight=info[:, 3].double(), edge_keep=edge)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(resid[:int(total)].abs().max()) < 4.0                 # the exported rows fit the H that went in (x2 ~ H x1)
    assert np.array_equal(cls.cpu().numpy(), matcher.two_view_config(summary.cpu().numpy()))
    info = info.cpu().numpy(); Rs = Rs.cpu().numpy(); ts = ts.cpu().numpy()
    assert use_h.cpu().numpy().all() and (info[:, 4] == Hr.OK).all() and (info[:, 1] > info[:, 2]).all() and (info[:, 1] >= 0.9 * info[:, 0]).all()
    assert int(front.sum()) == int(info[:, 1].sum()) and edge.cpu().numpy().all()
    for p, (i, j) in enumerate(np.asarray(pairs)):
        Rg, tg = R.relative(truth["poses"], int(i), int(j))
        assert R.rot_err_deg(Rs[p], Rg) < 1.0 and R.dir_err_deg(ts[p], tg) < 5.0, (p, R.rot_err_deg(Rs[p], Rg), R.dir_err_deg(ts[p], tg))
    Ra = avg[0].cpu().numpy()
    for i in range(m):
        Rg = truth["poses"][i][0] @ truth["poses"][0][0].T
        assert R.rot_err_deg(Ra[i] @ Ra[0].T, Rg) < 1.0, i
