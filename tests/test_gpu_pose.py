"""GPU: relative pose and triangulation on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_lists*, csrc/mi_pose.hip)
against tests/pose_ref.py.  The decomposition is compared with numpy's SVD: the device's four candidates equal numpy's four as a set, to
1e-9, and BIT FOR BIT with the restatement of the header's rule (pose_ref.decompose).  Everything behind the candidates is demanded BIT FOR BIT: from the device's own candidates and cameras the restatement gives
cand_front, front, info, X, depth and cosang, with guard elements around every output.  The chosen pose is compared with the restatement
on numpy's candidates to 1e-9 wherever front > runner-up (test_pose_cpu.py asserts that for every entry of these scenes that has a pose and
at least 8 used rows).  Entry lengths sit at the edges of a wave (63 .. 65), of a load of the workgroup (255 .. 257) and of a step of the row
pass (1023 .. 1025, 2049 = a third step)."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import pose_ref as R

pytestmark = pytest.mark.gpu
G = 8                                                                  # guard elements on each side of an output
PER = dict(pose=12, front=1, info=5, X=3, depth=2, cosang=1, cand=48, cand_front=4)
FILL = dict(pose=-7.0, front=77, info=-5, X=-3.0, depth=-3.0, cosang=-3.0, cand=-7.0, cand_front=-5)
ROWWISE = ("front", "X", "depth", "cosang")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _outs(torch, K, cap):
    dt = dict(pose=torch.float64, front=torch.uint8, info=torch.int32, X=torch.float64, depth=torch.float64, cosang=torch.float64,
              cand=torch.float64, cand_front=torch.int32)
    out = {}
    for k, per in PER.items():
        n = cap if k in ROWWISE else K
        buf = torch.full(((n + 2 * G) * per,), FILL[k], dtype=dt[k], device="cuda")
        out[k] = (buf, buf[G * per:(G + n) * per])
    return out


def _call(torch, sc, outs=None, stream=None, skip=()):
    """mi_degensac_pose_lists_dev on the scene with guarded outputs (outs: the buffers of an earlier call, reused as they are; skip: the
    optional outputs passed as NULL).  Returns (dict of numpy results, outs)."""
    K = len(sc["off"]) - 1; cap = len(sc["pts"])
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    pts, off, F, cams, idx, keep = t(sc["pts"]), t(sc["off"]), t(sc["F"]), t(sc["cams"]), t(sc["idx"]), t(sc["keep"])
    if outs is None:
        outs = _outs(torch, K, cap)
    s = torch.cuda.current_stream() if stream is None else stream
    d = lambda x: None if x is None else x.data_ptr()                  # noqa: E731
    p = lambda k: None if k in skip else outs[k][1].data_ptr()         # noqa: E731
    cm = sc["cos_min"] if "cos_min" in sc else R.cos_min(sc["deg"])
    rc = _lib.lib().mi_degensac_pose_lists_dev(d(pts), d(off), d(keep), d(F), d(cams), len(sc["cams"]), d(idx), K, cap, cm, 0,
                                               C.c_void_p(s.cuda_stream), p("pose"), p("front"), p("info"), p("X"), p("depth"), p("cosang"),
                                               p("cand"), p("cand_front"))
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


def _compare(sc, got):
    """the whole comparison of one call: candidates as a set against numpy's, everything else bit for bit from the device's candidates,
    the chosen pose against the all-numpy reference where it is determined"""
    K = len(sc["off"]) - 1
    cand = got["cand"].reshape(K, 4, 12)
    own = R.svd_candidates_of(sc)
    ref = R.reference(sc)
    for p in range(K):
        if own[p] is None or ref["info"][p, 4] in (R.TRUNCATED, R.BAD_CAMERA):
            assert not cand[p].any(), p
        else:
            assert R.same_set(cand[p], own[p]), (p, cand[p], own[p])
            Rs = cand[p][:, :9].reshape(4, 3, 3)
            assert np.abs(Rs @ Rs.transpose(0, 2, 1) - np.eye(3)).max() <= R.TOL and np.abs(np.linalg.det(Rs) - 1).max() <= R.TOL
            assert np.array_equal(cand[p][0, :9], cand[p][1, :9]) and np.array_equal(cand[p][0, 9:], -cand[p][1, 9:])          # the header's order
            assert np.array_equal(cand[p][2, :9], cand[p][3, :9]) and np.array_equal(cand[p][2, 9:], -cand[p][3, 9:])
            assert np.array_equal(cand[p][0, 9:], cand[p][2, 9:])
    want = R.from_candidates(sc, cand)
    assert np.array_equal(got["info"], want["info"]), np.flatnonzero((got["info"] != want["info"]).any(axis=1))[:8]
    assert np.array_equal(got["cand_front"], want["cand_front"])
    assert _bits(got["pose"], want["pose"])
    for k in ROWWISE:
        if k in got:
            assert _bits(got[k], want[k].reshape(got[k].shape)), (k, np.flatnonzero((got[k] != want[k].reshape(got[k].shape)).reshape(len(sc["pts"]), -1).any(axis=1))[:8])
    # the chosen pose against numpy's own, wherever the winner is clear in the all-numpy reference
    clear = (ref["info"][:, 4] == R.OK) & (ref["info"][:, 1] > ref["info"][:, 2])
    assert np.array_equal(got["info"][:, 4], ref["info"][:, 4])
    for p in np.flatnonzero(clear):
        assert np.abs(got["pose"][p] - ref["pose"][p]).max() <= R.TOL, (p, got["pose"][p], ref["pose"][p])
        assert sc.get("fragile") or got["info"][p].tolist() == ref["info"][p].tolist(), p
    bad = got["info"][:, 4] != R.OK
    assert not got["pose"][bad].any() and not got["info"][bad, :4].any()
    return want


SCENES = ["lengths", "lengths_exact", "keep", "many", "offsets", "models", "cameras", "bad_rows", "noisy_models", "nonessential", "exact"]


def test_scene_list_is_the_catalogue():
    assert sorted(SCENES) == sorted(R.gpu_scenes())
    assert _lib.lib().mi_degensac_pose_tile(1) == _lib.POSE_GRID < 300 and _lib.lib().mi_degensac_pose_tile(0) == _lib.POSE_STEP == 1024


@pytest.mark.parametrize("name", SCENES)
def test_pose_equals_restatement(torch, name):
    """every scene: lengths at the tile edges, a non-zero o[0] and unowned rows behind, used rows in the last wave only and one per wave,
    keep all zero, empty entries first, last and between, 300 entries on a grid of 256, ranges that cross cap / start beyond it /
    decrease, zero / NaN / inf / 1e+-150 models, refused cameras and camera indices, rows that are not finite, models that are no essential matrices (sigma1 != sigma2 of rank 3 by a hair; rank 2 with sigma2 << sigma1, on which the
    reference's 3 x 3 routine returns a V that is not orthogonal), lambda == 0 and den == 0"""
    sc = R.gpu_scenes()[name]
    got, _ = _call(torch, sc)
    _compare(sc, got)


@pytest.mark.parametrize("name", SCENES + ["decomposition_edges"])
def test_candidates_equal_restatement(torch, name):
    """the four candidates BIT FOR BIT against pose_ref.decompose, the header's decomposition operation for operation (numpy's SVD above
    holds them to 1e-9 only, which a Jacobi rule in another operation order passes: test_pose_cpu.py shows one); every scene, and the
    edges of the decomposition with one row per entry: rank 2 exactly, sigma1 == sigma2, columns orthogonal as given, a negative
    determinant before the flip, F x 1e-150 and x 1e150, and rank 1 (BAD_MODEL, zeros)"""
    sc = R.edge_scene() if name == "decomposition_edges" else R.gpu_scenes()[name]
    K = len(sc["off"]) - 1
    got, _ = _call(torch, sc)
    want = R.decompose_scene(sc)
    cand = np.array([np.zeros((4, 12)) if d is None else d["cand"] for d in want])
    assert _bits(got["cand"].reshape(K, 4, 12), cand), [p for p in range(K) if not _bits(got["cand"].reshape(K, 4, 12)[p], cand[p])][:8]
    model = np.array([d is not None and d["status"] == R.OK for d in want])
    assert np.array_equal(np.isin(got["info"][:, 4], (R.OK, R.EMPTY)), model)
    if name == "decomposition_edges":
        assert got["info"][:, 4].tolist() == [R.OK] * 6 + [R.BAD_MODEL] and not got["cand"][6].any() and got["cand"][:6].any(axis=1).all()


def test_every_status_and_the_fills(torch):
    S = R.gpu_scenes(); seen = set()
    for name in ("keep", "offsets", "models", "cameras"):
        sc = S[name]
        got, _ = _call(torch, sc)
        seen |= set(got["info"][:, 4].tolist())
        own = np.zeros(len(sc["pts"]), bool)
        for p, (b, e) in enumerate(zip(sc["off"][:-1], sc["off"][1:])):
            if got["info"][p, 4] == R.OK:
                own[b:e] = True if sc["keep"] is None else sc["keep"][b:e] != 0
        assert not got["front"][~own].any() and np.isnan(got["X"][~own]).all() and np.isnan(got["depth"][~own]).all() and np.isnan(got["cosang"][~own]).all()
        assert np.isfinite(got["cosang"][own]).all()
    assert seen == {R.OK, R.BAD_MODEL, R.BAD_CAMERA, R.TRUNCATED, R.EMPTY}
    got, _ = _call(torch, S["models"])
    assert R.same_set(got["cand"][3].reshape(4, 12), R.candidates_svd(S["models"]["F"][3] * 1e-150, *S["models"]["cams"][6:8]))
    assert R.same_set(got["cand"][4].reshape(4, 12), R.candidates_svd(S["models"]["F"][4] * 1e150, *S["models"]["cams"][8:10]))


def test_lambda_zero_den_zero_and_cosang_at_cos_min(torch):
    sc = dict(R.gpu_scenes()["exact"])
    got, _ = _call(torch, sc)
    assert got["depth"][0].tolist() == [0.0, 0.0] and got["front"][0] == 0          # lambda exactly 0 is not front
    l1, l2, cs, X, den = R.rows_rule(got["pose"][0], sc["cams"][0], sc["cams"][1], sc["pts"])
    assert den[1] == 0.0 and got["front"][1] == 0 and not (got["depth"][1] > 0).any()
    assert got["info"][0].tolist() == [30, 28, 0, 28, R.OK]
    # cosang exactly at cos_min is wide (<=), one unit in the last place below it is not
    fr = np.flatnonzero(got["front"]); c = np.sort(got["cosang"][fr]); at = float(c[len(c) // 2])
    n_le = int((got["cosang"][fr] <= at).sum())
    for cm, n in ((at, n_le), (float(np.nextafter(at, -1.0)), n_le - int((got["cosang"][fr] == at).sum()))):
        sc["cos_min"] = cm
        g, _ = _call(torch, sc)
        assert g["info"][0, 3] == n, (cm, g["info"][0])
        _compare(sc, g)
    assert 0 < n_le < len(fr) + 1


def test_null_optional_outputs(torch):
    sc = R.gpu_scenes()["lengths"]
    full, _ = _call(torch, sc)
    part, _ = _call(torch, sc, skip=("X", "depth", "cosang", "cand", "cand_front"))
    assert sorted(part) == ["front", "info", "pose"] and all(_bits(part[k], full[k]) for k in part)
    part, _ = _call(torch, sc, skip=("depth", "cand"))
    assert all(_bits(part[k], full[k]) for k in part) and "X" in part and "cand_front" in part


def test_outputs_reused_and_ten_identical_calls(torch):
    """a long scene, then a short one into the same buffers (what the first call left must not show), then ten calls with identical bytes"""
    a = R.gpu_scenes()["lengths"]; b = R.gpu_scenes()["offsets"]
    _, outs = _call(torch, a)
    K, cap = len(b["off"]) - 1, len(b["pts"])
    small = {k: (buf, buf[G * PER[k]:(G + (cap if k in ROWWISE else K)) * PER[k]]) for k, (buf, _) in outs.items()}
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    pts, off, F, cams = t(b["pts"]), t(b["off"]), t(b["F"]), t(b["cams"])
    s = torch.cuda.current_stream(); p = lambda k: small[k][1].data_ptr()          # noqa: E731
    _lib.check_match(_lib.lib().mi_degensac_pose_lists_dev(pts.data_ptr(), off.data_ptr(), None, F.data_ptr(), cams.data_ptr(), len(b["cams"]), None, K, cap,
                                                           R.cos_min(b["deg"]), 0, C.c_void_p(s.cuda_stream), *(p(k) for k in PER)))
    s.synchronize()
    got = {k: v[1].cpu().numpy().reshape((-1, PER[k]) if PER[k] > 1 else (-1,)) for k, v in small.items()}
    _compare(b, got)
    sc = R.gpu_scenes()["keep"]
    first, o2 = _call(torch, sc)
    for _ in range(9):
        again, _ = _call(torch, sc, outs=o2)
        for k in first:
            assert first[k].tobytes() == again[k].tobytes(), k


def test_second_stream(torch):
    sc = R.gpu_scenes()["many"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = _call(torch, sc, stream=s)
    _compare(sc, got)


def test_k0_and_cap0(torch):
    L = _lib.lib()
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.mi_degensac_pose_lists_dev(None, off.data_ptr(), None, None, None, 0, None, 0, 0, 0.5, 0, None, *([None] * 8)) == 0
    # K == 0 with rows: the fills are all that is written
    pts = torch.zeros((5, 4), dtype=torch.float64, device="cuda"); fr = torch.full((5,), 9, dtype=torch.uint8, device="cuda")
    X = torch.zeros((5, 3), dtype=torch.float64, device="cuda"); cs = torch.zeros(5, dtype=torch.float64, device="cuda")
    assert L.mi_degensac_pose_lists_dev(pts.data_ptr(), off.data_ptr(), None, None, None, 0, None, 0, 5, 0.5, 0, None, None, fr.data_ptr(), None,
                                        X.data_ptr(), None, cs.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert not fr.cpu().numpy().any() and np.isnan(X.cpu().numpy()).all() and np.isnan(cs.cpu().numpy()).all()
    # K > 0 with cap == 0: every entry is empty or truncated
    off = torch.tensor([0, 0, 3], dtype=torch.int64, device="cuda"); F = torch.ones((2, 9), dtype=torch.float64, device="cuda")
    F[0, 4] = 2.0
    cams = torch.tensor([[800.0, 800, 500, 375]] * 4, dtype=torch.float64, device="cuda")
    pose = torch.ones((2, 12), dtype=torch.float64, device="cuda"); info = torch.ones((2, 5), dtype=torch.int32, device="cuda")
    assert L.mi_degensac_pose_lists_dev(None, off.data_ptr(), None, F.data_ptr(), cams.data_ptr(), 4, None, 2, 0, 0.5, 0, None, pose.data_ptr(), None,
                                        info.data_ptr(), None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [[0, 0, 0, 0, R.EMPTY], [0, 0, 0, 0, R.TRUNCATED]] and not pose.cpu().numpy().any()


def _as_results(K, cap, res):
    Rm, t, front, info, X, depth, cosang, cand, cf = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in res)
    return dict(pose=np.concatenate([Rm.reshape(K, 9), t], 1), front=front.astype(np.uint8), info=info, X=X, depth=depth, cosang=cosang,
                cand=cand.reshape(K, 48), cand_front=cf)


def test_numpy_form_per_entry_cameras_and_keep():
    sc = R.gpu_scenes()["lengths"]; K = len(sc["off"]) - 1
    res = matcher.relative_pose(sc["pts"], sc["off"], sc["F"].reshape(K, 3, 3), sc["cams"].reshape(K, 8), min_parallax_deg=sc["deg"], with_points=True,
                                with_candidates=True)
    _compare(sc, _as_results(K, len(sc["pts"]), res))
    sc = R.gpu_scenes()["keep"]; K = len(sc["off"]) - 1
    res = matcher.relative_pose(sc["pts"], sc["off"], sc["F"].reshape(K, 3, 3), sc["cams"], pairs=sc["idx"], keep=sc["keep"].astype(bool),
                                min_parallax_deg=sc["deg"], with_points=True, with_candidates=True)
    _compare(sc, _as_results(K, len(sc["pts"]), res))
    assert len(matcher.relative_pose(sc["pts"], sc["off"], sc["F"].reshape(K, 3, 3), sc["cams"], pairs=sc["idx"])) == 4
    # the same call without any optional output: R, t, front and info are the bits of the call above
    bare = matcher.relative_pose(sc["pts"], sc["off"], sc["F"].reshape(K, 3, 3), sc["cams"], pairs=sc["idx"], keep=sc["keep"].astype(bool),
                                 min_parallax_deg=sc["deg"])
    assert len(bare) == 4 and all(a.tobytes() == b.tobytes() for a, b in zip(bare, res[:4]))


def test_tensor_form_by_index_shared_camera_and_two_stores(torch):
    """cameras by index (image 0 is camera 1 or 2 of 112 entries), then the same list over two stores: store 2 holds the cameras in another
    order, and an image of store 1 beyond its table must not reach into store 2's rows"""
    from pydegensac_amd import tensor_api as T
    sc = R.gpu_scenes()["many"]; K = len(sc["off"]) - 1; cap = len(sc["pts"])
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    res = T.relative_pose_tensors(c(sc["pts"]), c(sc["off"]), c(sc["F"].reshape(K, 3, 3)), c(sc["cams"]), pairs=c(sc["idx"]),
                                  min_parallax_deg=sc["deg"], with_points=True, with_candidates=True)
    one = _as_results(K, cap, res)
    _compare(sc, one)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4]); inv = np.argsort(perm)
    pairs2 = np.stack([sc["idx"][:, 0], inv[sc["idx"][:, 1]]], 1).astype(np.int64)
    pairs2[7, 0] = 9                                                   # beyond store 1 (8 images): would be row 1 of store 2
    res = T.relative_pose_tensors(c(sc["pts"]), c(sc["off"]), c(sc["F"].reshape(K, 3, 3)), c(sc["cams"]), pairs=c(pairs2), cams2=c(sc["cams"][perm]),
                                  min_parallax_deg=sc["deg"], with_points=True, with_candidates=True)
    two = _as_results(K, cap, res)
    assert two["info"][7].tolist() == [0, 0, 0, 0, R.BAD_CAMERA]
    keep = np.ones(K, bool); keep[7] = False
    rows = np.ones(cap, bool); rows[sc["off"][7]:sc["off"][8]] = False
    for k in one:
        sel = rows if k in ROWWISE else keep
        assert _bits(one[k][sel], two[k][sel]), k
    short = T.relative_pose_tensors(c(sc["pts"]), c(sc["off"]), c(sc["F"].reshape(K, 3, 3)), c(sc["cams"]), pairs=c(sc["idx"]))
    assert len(short) == 4 and short[0].shape == (K, 3, 3) and short[1].shape == (K, 3) and short[2].dtype == torch.bool


def test_chain_verify_export_refit_pose_without_sync(torch):
    """match_and_verify_pairs_tensors -> correspondences_pairs_tensors -> refit -> pose on a small collection: the refit and the pose call
    (with the refit's inlier as keep) run under torch's synchronisation check, so nothing is read back between them, and the poses are the generator's to a degree"""
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
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * m, dtype=torch.float64, device="cuda")
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        M, inl, info_r = T.refit_correspondences_tensors(pts, co, F, "F")
        Rm, t, front, info = T.relative_pose_tensors(pts, co, M, cams, pairs=pr, keep=inl)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    info = info.cpu().numpy(); Rm = Rm.cpu().numpy(); t = t.cpu().numpy()
    assert (info[:, 4] == R.OK).all() and (info[:, 0] == info_r.cpu().numpy()[:, 1]).all() and int(front.sum()) == int(info[:, 1].sum())
    assert (info[:, 1] > info[:, 2]).all() and (info[:, 1] >= 0.9 * info[:, 0]).all()
    for p, (i, j) in enumerate(np.asarray(pairs)):
        Rg, tg = R.relative(poses, int(i), int(j))
        assert R.rot_err_deg(Rm[p], Rg) < 1.0 and R.dir_err_deg(t[p], tg) < 5.0, (p, R.rot_err_deg(Rm[p], Rg), R.dir_err_deg(t[p], tg))
