"""GPU: the refit of F / H on exported correspondence lists (include/mi_degensac.h mi_degensac_refit_lists*, csrc/mi_refit.hip) against its
restatement over the CPU oracle (tests/refit_ref.py).  Equality only: inlier and info bit for bit at full length with guard elements
around every output, models to 1e-9 relative Frobenius in driver form (the project's standing bound against its restatement), resid bit
for bit against the oracle's residual of the device's own output model.  The scenes are refit_ref.gpu_scenes; test_refit_cpu.py asserts
for each of them that no residual of a visited model lies within 1e-6 th of th, the condition under which the masks can be demanded bit
for bit.  Entry LENGTHS sit at the edges of a wave (63 .. 65), of a load of the workgroup (255 .. 257) and of a step of the scoring pass
(1023 .. 1025, 2049 = a third step); at 70 % inliers they say little about which solver ran.  MEMBER COUNTS sit at the solver edges: the
member stores (refit_ref.MEMBER_STORES) hold entries whose members under the start model are known in advance, 8 .. 513 of them for F
and 4 .. 513 for H, on both sides of the solver switches (F 16 | 17, H 4 | 5 and 12 | 13), of the 8-term unroll of the normal-matrix
loop, of the wave, of the stride of 256 threads and of 512.  At max_fits = 1 such an entry is "gather these rows, run the driver's solver
for that count, return the model": there the model is demanded BIT FOR BIT against the oracle's fit (dg_oracle_u2f / dg_oracle_u2h) on
the same rows, in the pixel frame, in three other frames, under every error type, on rank-deficient sets, and independent of which
entries the workgroup fitted before."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import refit_ref as R

pytestmark = pytest.mark.gpu
G = 8                                                                  # guard elements on each side of an output


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _guarded(torch, n, dtype, fill, per=1):
    """(whole buffer, the slice an entry point writes, the guard's fill)"""
    buf = torch.full(((n + 2 * G) * per,), fill, dtype=dtype, device="cuda")
    return buf, buf[G * per:(G + n) * per]


def _call(torch, sc, max_fits=4, outs=None, stream=None):
    """mi_degensac_refit_lists_dev on the scene with guarded outputs (outs: the buffers of an earlier call, reused as they are).  Returns
    (dict of numpy results, outs)."""
    K = len(sc["off"]) - 1; cap = len(sc["pts"])
    pts = torch.from_numpy(sc["pts"]).cuda(); off = torch.from_numpy(sc["off"]).cuda(); M = torch.from_numpy(sc["models"]).cuda()
    if outs is None:
        outs = dict(models=_guarded(torch, K, torch.float64, -7.0, 9), user=_guarded(torch, K, torch.float64, -7.0, 9),
                    inlier=_guarded(torch, cap, torch.uint8, 77), info=_guarded(torch, K, torch.int32, -5, 4),
                    resid=_guarded(torch, cap, torch.float64, -3.0))
    gp = _lib.GuideParams(sc["model"] == "H", sc["et"], R.DEFAULT_PX[sc["model"]] if sc["px_th"] is None else sc["px_th"])
    s = torch.cuda.current_stream() if stream is None else stream
    p = lambda k: outs[k][1].data_ptr()                                # noqa: E731
    rc = _lib.lib().mi_degensac_refit_lists_dev(pts.data_ptr(), off.data_ptr(), M.data_ptr(), K, cap, C.byref(gp), max_fits, 0,
                                                C.c_void_p(s.cuda_stream), p("models"), p("inlier"), p("user"), p("info"), p("resid"))
    _lib.check_match(rc)
    s.synchronize()
    fills = dict(models=-7.0, user=-7.0, inlier=77, info=-5, resid=-3.0)
    res = {}
    for k, (buf, view) in outs.items():
        whole = buf.cpu().numpy(); per = {"models": 9, "user": 9, "info": 4}.get(k, 1)
        assert (whole[:G * per] == fills[k]).all() and (whole[len(whole) - G * per:] == fills[k]).all(), f"{k}: a guard element was written"
        res[k] = whole[G * per:len(whole) - G * per].reshape((-1, per) if per > 1 else (-1,))
    return res, outs


def _owned(sc):
    """bool [cap]: the rows of the entries that are whole"""
    cap = len(sc["pts"]); own = np.zeros(cap, bool)
    for b, e in zip(sc["off"][:-1], sc["off"][1:]):
        if 0 <= b <= e <= cap:
            own[b:e] = True
    return own


def _compare(oracle_port, sc, got, ref):
    assert np.array_equal(got["info"], ref["info"]), np.flatnonzero((got["info"] != ref["info"]).any(axis=1))[:8]
    assert np.array_equal(got["inlier"], ref["inlier"]), np.flatnonzero(got["inlier"] != ref["inlier"])[:8]
    for p in range(len(ref["models"])):
        d = R.rel_fro(got["models"][p], ref["models"][p])
        assert d <= 1e-9, (p, d, got["info"][p])
    # resid: bit for bit the oracle's residual of the device's own model on owned rows, NaN elsewhere
    want = np.full(len(sc["pts"]), np.nan); cap = len(sc["pts"])
    for p, (b, e) in enumerate(zip(sc["off"][:-1], sc["off"][1:])):
        if 0 <= b <= e <= cap and e > b:
            want[b:e] = R.resid(oracle_port, sc["model"], sc["et"], got["models"][p], sc["pts"][b:e])
    nan = np.isnan(want)
    assert np.isnan(got["resid"][nan]).all()
    assert np.array_equal(got["resid"][~nan].view(np.int64), want[~nan].view(np.int64)), np.flatnonzero(got["resid"].view(np.int64) != want.view(np.int64))[:8]
    assert not got["inlier"][~_owned(sc)].any()


SCENES = ["F_len_0", "F_len_1", "H_len_0", "H_len_1", "H_len_2", "H_len_3", "H_len_4", "F_px2", "F_8_per_wave", "F_8_last_wave", "F_7_of_300",
          "H_4_per_wave", "H_4_last_wave", "H_3_of_200", "F_many", "H_many", "F_offsets", "H_offsets", "F_models", "H_models", "H_models_3",
          "F_bad_rows", "H_bad_rows"] + list(R.MEMBER_STORES)


def test_scene_list_is_the_catalogue(oracle_port):
    assert sorted(SCENES) == sorted(R.gpu_scenes(oracle_port))


@pytest.mark.parametrize("name", SCENES)
def test_refit_equals_restatement(torch, oracle_port, name):
    """every scene at max_fits = 4: lengths at the tile and solver edges, empty entries first, last and between, a non-zero o[0], unowned
    rows behind, every error type, member counts exactly at 8 / 4 and one below, members in the last wave only and one per wave, 300
    entries on a grid of 256 workgroups, ranges that cross cap / start beyond it / decrease, zero / NaN / inf / 1e+-150 start models,
    rows that are not finite, the member stores (member counts at the solver edges, other frames, rank-deficient sets)"""
    sc = R.gpu_scenes(oracle_port)[name]
    got, _ = _call(torch, sc, 4)
    _compare(oracle_port, sc, got, R.reference(oracle_port, name, 4))
    assert sc["model"] == "H" or np.array_equal(got["user"], got["models"], equal_nan=True)          # F: the user form is the model


@pytest.mark.parametrize("max_fits", [0, 1])
@pytest.mark.parametrize("name", ["F_len_1", "H_len_0", "H_len_3"])
def test_max_fits_0_and_1(torch, oracle_port, name, max_fits):
    sc = R.gpu_scenes(oracle_port)[name]
    got, _ = _call(torch, sc, max_fits)
    ref = R.reference(oracle_port, name, max_fits)
    _compare(oracle_port, sc, got, ref)
    assert (got["info"][:, 2] <= max_fits).all()
    if max_fits == 0:
        assert np.array_equal(got["models"], sc["models"]) and (got["info"][:, 3] == R.MAX_FITS).all()


# ---- the non-minimal fits bit for bit, through max_fits = 1 on entries whose members are known in advance ----
def _ulps(a, b):
    """the largest distance of two models in units of the last place, -1 where the two are not comparable that way"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()) or (np.signbit(a) != np.signbit(b)).any():
        return -1
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max())


def _fit_is_the_output(info_row):
    """one fit was run and kept: its model is models_out (FIXED; MAX_FITS where the one fit gained members)"""
    return info_row[2] == 1 and info_row[3] in (R.FIXED, R.MAX_FITS)


def _bits(torch, oracle_port, name):
    """the member store at max_fits = 1: the standing comparison, then models_out of every entry whose fit is the output has the bytes of
    the oracle's fit on the rows at `where`.  Every entry is one (all but H on 4 rows, whose reference fit keeps no member: see
    test_refit_cpu.test_member_scene_is_a_fixed_point_after_one_fit).  Every differing entry is reported, not the first."""
    sc = R.gpu_scenes(oracle_port)[name]
    got, _ = _call(torch, sc, 1)
    _compare(oracle_port, sc, got, R.reference(oracle_port, name, 1))
    bad = []; checked = 0
    for p, where in enumerate(sc["where"]):
        if not _fit_is_the_output(got["info"][p]):
            continue
        want = R.fit(oracle_port, sc["model"], sc["pts"][sc["off"][p]:sc["off"][p + 1]], where)
        checked += 1
        if got["models"][p].tobytes() != want.tobytes():
            bad.append((p, sc["m"][p], _ulps(got["models"][p], want), R.rel_fro(got["models"][p], want)))
    print(name, "entries checked", checked, "differing (entry, members, ulps, rel)", bad)
    assert not bad, bad
    assert checked == len(sc["m"]) - sum(1 for m in sc["m"] if sc["model"] == "H" and m == 4)
    return got


@pytest.mark.parametrize("name", ["F_members_0", "F_members_1", "H_members_0", "H_members_1", "H_members_2", "H_members_3", "H_members_4"])
def test_fit_carries_the_oracles_bits(torch, oracle_port, name):
    """dg_u2f_small_w (8 = the 9 x 8 null vector, 9 .. 16), dg_u2f_big (17 .. 513), dg_u2h_small_w (5 .. 12) and dg_u2h_big (13 .. 513) as
    the refit calls them (no LDS table, the global path of dg_lsq_seq_par with a staging slice of 2 len): every operation is meant to be
    the reference's IEEE sequence, sums in list order, no contraction, so the model is demanded byte for byte.  Members are never a
    contiguous range; three entries have them in the second step of the pass only, at rows 0 / 1023 / 1024 / n - 1, and inside the last
    partly filled wave.  The error type changes which rows are members, not the fit: types other than 0 at the switch counts only."""
    _bits(torch, oracle_port, name)


@pytest.mark.parametrize("name", [f"{k}_frame_{fr}" for k in "FH" for fr in R.MEMBER_FRAMES] + ["F_rankdef", "H_rankdef"])
def test_fit_carries_the_oracles_bits_in_other_frames_and_on_rank_deficient_sets(torch, oracle_port, name):
    """the same demand with coordinates x 37 + 5000 / x 37 - 9000, centred x 1e-3 and x 1e4 (px_th and the start model in the frame) at
    the switch counts, 64 and 257; and on member sets that do not determine the model (3 distinct rows in 9, 6 in 20), where the
    eigenvector taken among the (near-)zero eigenvalues is the eigen-solver's order, which DESIGN.md section 4 says is the restatement's"""
    _bits(torch, oracle_port, name)


def _entry_bytes(sc, got, p):
    b, e = int(sc["off"][p]), int(sc["off"][p + 1])
    return tuple(x.tobytes() for x in (got["models"][p], got["user"][p], got["info"][p], got["inlier"][b:e], got["resid"][b:e]))


@pytest.mark.parametrize("name", ["F_members_0", "H_members_0"])
def test_fit_does_not_depend_on_what_the_workgroup_fitted_before(torch, oracle_port, name):
    """LDS that survives an entry (rf_shared.lsq, cand, prep, the popcount words): the entries of the store (a) one workgroup each,
    (b) REFIT_GRID - 1 empty entries between two of them, so that workgroup 0 takes them all one after the other, small fits after big
    ones, (c) the same in reversed order, so that every fit has another predecessor, (d) each alone in a call of its own.  models,
    models_user, info and the entry's slices of inlier and resid must be the same bytes in all four."""
    entries = R.member_entries(oracle_port, name); E = len(entries)
    sc = R.gpu_scenes(oracle_port)[name]
    got, _ = _call(torch, sc, 1)
    want = [_entry_bytes(sc, got, p) for p in range(E)]
    for order in (list(range(E)), list(range(E))[::-1]):
        st = R.concat_scenes(entries, order, stride=_lib.REFIT_GRID)
        assert len(st["off"]) - 1 == (E - 1) * _lib.REFIT_GRID + 1
        g, _ = _call(torch, st, 1)
        for k, q in enumerate(order):
            assert _entry_bytes(st, g, k * _lib.REFIT_GRID) == want[q], (order[0], q, sc["m"][q])
        empty = np.ones(len(st["m"]), bool); empty[::_lib.REFIT_GRID] = False
        assert (g["info"][empty] == [0, 0, 0, R.SHORT]).all()
    for q, one in enumerate(entries):
        g, _ = _call(torch, one, 1)
        assert _entry_bytes(one, g, 0) == want[q], ("alone", q, sc["m"][q])


def test_grid_takes_a_second_step():
    assert _lib.lib().mi_degensac_refit_tile(1) == _lib.REFIT_GRID < 300 and _lib.lib().mi_degensac_refit_tile(0) == _lib.REFIT_STEP == 1024


def test_outputs_reused_across_two_calls_and_ten_identical_repeats(torch, oracle_port):
    """a long scene, then a short one into the same buffers (what the first call left must not show), then ten calls with identical bytes"""
    a = R.gpu_scenes(oracle_port)["F_len_0"]; b = R.gpu_scenes(oracle_port)["F_offsets"]
    _, outs = _call(torch, a, 4)
    K, cap = len(b["off"]) - 1, len(b["pts"])
    small = {k: (buf, buf[G * per:(G + n) * per]) for k, (buf, _), per, n in
             [("models", outs["models"], 9, K), ("user", outs["user"], 9, K), ("inlier", outs["inlier"], 1, cap), ("info", outs["info"], 4, K),
              ("resid", outs["resid"], 1, cap)]}
    pts = torch.from_numpy(b["pts"]).cuda(); off = torch.from_numpy(b["off"]).cuda(); M = torch.from_numpy(b["models"]).cuda()
    gp = _lib.GuideParams(0, 0, 0.5); s = torch.cuda.current_stream()
    p = lambda k: small[k][1].data_ptr()                               # noqa: E731
    _lib.check_match(_lib.lib().mi_degensac_refit_lists_dev(pts.data_ptr(), off.data_ptr(), M.data_ptr(), K, cap, C.byref(gp), 4, 0,
                                                            C.c_void_p(s.cuda_stream), p("models"), p("inlier"), p("user"), p("info"), p("resid")))
    s.synchronize()
    got = {k: v[1].cpu().numpy().reshape((-1, {"models": 9, "user": 9, "info": 4}[k]) if k in ("models", "user", "info") else (-1,))
           for k, v in small.items()}
    _compare(oracle_port, b, got, R.reference(oracle_port, "F_offsets", 4))
    sc = R.gpu_scenes(oracle_port)["H_len_3"]
    first, o2 = _call(torch, sc, 4)
    for _ in range(9):
        again, _ = _call(torch, sc, 4, outs=o2)
        for k in first:
            assert first[k].tobytes() == again[k].tobytes(), k


def test_second_stream(torch, oracle_port):
    sc = R.gpu_scenes(oracle_port)["H_len_0"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = _call(torch, sc, 4, stream=s)
    _compare(oracle_port, sc, got, R.reference(oracle_port, "H_len_0", 4))


def test_k0_and_cap0(torch):
    gp = _lib.GuideParams(0, 0, 0.5); L = _lib.lib()
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.mi_degensac_refit_lists_dev(None, off.data_ptr(), None, 0, 0, C.byref(gp), 4, 0, None, None, None, None, None, None) == 0
    # K == 0 with rows: the fills are all that is written
    pts = torch.zeros((5, 4), dtype=torch.float64, device="cuda"); inl = torch.full((5,), 9, dtype=torch.uint8, device="cuda")
    res = torch.zeros(5, dtype=torch.float64, device="cuda")
    assert L.mi_degensac_refit_lists_dev(pts.data_ptr(), off.data_ptr(), None, 0, 5, C.byref(gp), 4, 0, None, None, inl.data_ptr(), None, None,
                                         res.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not inl.cpu().numpy().any() and np.isnan(res.cpu().numpy()).all()
    # K > 0 with cap == 0: every entry is empty or truncated
    off = torch.tensor([0, 0, 3], dtype=torch.int64, device="cuda"); M = torch.ones((2, 9), dtype=torch.float64, device="cuda")
    out = torch.zeros((2, 9), dtype=torch.float64, device="cuda"); info = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    assert L.mi_degensac_refit_lists_dev(None, off.data_ptr(), M.data_ptr(), 2, 0, C.byref(gp), 4, 0, None, out.data_ptr(), None, None,
                                         info.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [[0, 0, 0, R.SHORT], [0, 0, 0, R.TRUNCATED]] and (out.cpu().numpy() == 1).all()


def test_numpy_entry_point(oracle_port):
    sc = R.gpu_scenes(oracle_port)["F_len_1"]; ref = R.reference(oracle_port, "F_len_1", 4)
    M, inl, info, resid = matcher.refit_correspondences(sc["pts"], sc["off"], sc["models"].reshape(-1, 3, 3), "F", None, "symm_epipolar", max_fits=4,
                                                        with_resid=True)
    _compare(oracle_port, sc, dict(models=M.reshape(-1, 9), inlier=inl.astype(np.uint8), info=info, resid=resid), ref)


def test_host_form_without_optional_outputs_equals_the_device_form(torch):
    """mi_degensac_refit_lists with models_user, info and resid NULL, on 2 entries with one empty: models_out and inlier are what the device
    form writes on the same inputs, bit for bit"""
    rng = np.random.default_rng(5)
    pts = rng.uniform(0.0, 100.0, (9, 4)); pts[:, 3] = pts[:, 1]; pts[8, 3] += 50.0          # 8 rows on y2 = y1, one far off it
    sc = dict(pts=pts, off=np.array([0, 0, 9], np.int64), models=np.tile([0.0, 0, 0, 0, 0, -1, 0, 1, 0], (2, 1)), model="F", et=0, px_th=0.5)
    dev, _ = _call(torch, sc)
    assert dev["info"][0].tolist() == [0, 0, 0, R.SHORT] and dev["info"][1, 0] == 8
    out = np.full((2, 9), -7.0); inl = np.full(9, 77, np.uint8); gp = _lib.GuideParams(False, 0, 0.5)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)          # noqa: E731
    _lib.check_match(_lib.lib().mi_degensac_refit_lists(vp(sc["pts"]), vp(sc["off"]), vp(sc["models"]), 2, 9, C.byref(gp), 4, 0, vp(out), vp(inl),
                                                        None, None, None))
    assert np.array_equal(out.view(np.int64), np.ascontiguousarray(dev["models"]).view(np.int64)) and np.array_equal(inl, dev["inlier"])


def test_h_user_and_driver_form(torch, oracle_port):
    """the tensor call on H: driver_form=True is the C call; driver_form=False converts on the device in both directions, so it is compared
    with the restatement on the driver form the device's own conversion made, and its output with inv(H_c^T) of the driver-form output to
    100 eps cond(H_c) (two 3 x 3 eliminations with pivoting, each backward stable); zero models stay zero"""
    from pydegensac_amd import tensor_api as T
    sc = R.gpu_scenes(oracle_port)["H_len_0"]; K = len(sc["off"]) - 1
    pts = torch.from_numpy(sc["pts"]).cuda(); off = torch.from_numpy(sc["off"]).cuda()
    Md = torch.from_numpy(sc["models"]).cuda().view(K, 3, 3)
    M, inl, info, resid = T.refit_correspondences_tensors(pts, off, Md, "H", driver_form=True, with_resid=True)
    _compare(oracle_port, sc, dict(models=M.cpu().numpy().reshape(K, 9), inlier=inl.cpu().numpy().astype(np.uint8), info=info.cpu().numpy(),
                                   resid=resid.cpu().numpy()), R.reference(oracle_port, "H_len_0", 4))
    Mn = sc["models"].reshape(K, 3, 3).copy()                         # a singular start model (a degenerate 4-point fit) has no user form
    for q in range(K):
        if not np.isfinite(np.linalg.cond(Mn[q])):
            Mn[q] = R.HC / np.linalg.norm(R.HC)
    user = T._h_user_form(torch.from_numpy(Mn).cuda()).clone(); user[0] = 0.0          # a zero model among them
    back = T._h_driver_form(user)
    ref = R.refit(oracle_port, sc["pts"], sc["off"], back.cpu().numpy().reshape(K, 9), "H", 0)
    Mu, inl_u, info_u = T.refit_correspondences_tensors(pts, off, user, "H")
    Mdrv, _, _ = T.refit_correspondences_tensors(pts, off, back, "H", driver_form=True)
    assert np.array_equal(info_u.cpu().numpy(), ref["info"]) and np.array_equal(inl_u.cpu().numpy().astype(np.uint8), ref["inlier"])
    Mu = Mu.cpu().numpy(); Mdrv = Mdrv.cpu().numpy()
    assert (Mu[0] == 0).all() and (Mdrv[0] == 0).all()
    for p in range(1, K):
        want = np.linalg.inv(Mdrv[p].T)
        assert np.linalg.norm(Mu[p] - want) <= 100 * np.finfo(float).eps * np.linalg.cond(Mdrv[p]) * np.linalg.norm(want), p


def test_chain_verify_guided_export_refit_without_sync(torch):
    """match_and_verify_pairs_tensors -> guided_match_pairs_tensors -> correspondences_pairs_tensors -> refit on a small collection: the
    refit call runs under torch's synchronisation check, and no entry ends with fewer members than its start model had"""
    from pydegensac_amd import synthetic as syn
    from pydegensac_amd import tensor_api as T
    kps, descs = syn.image_collection(m=4, n=300, inlier_ratio=0.6, sigma=0.1, dim=32, seed=2)
    counts = [len(k) for k in kps]
    k = torch.from_numpy(np.ascontiguousarray(np.concatenate(kps)[:, :2], dtype=np.float64)).cuda()
    d = torch.from_numpy(np.concatenate(descs).astype(np.float32)).cuda()
    pairs = matcher.exhaustive_pairs(4)
    ver = T.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.8, max_iters=2000)
    F = ver[0]
    gm = T.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, model="F", ratio=0.9)
    rows, co, total, entry, pts, resid = T.correspondences_pairs_tensors(gm[0], counts, counts, pairs, kps1=k, kps2=k, models=F)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        M, inl, info = T.refit_correspondences_tensors(pts, co, F, "F")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    info = info.cpu().numpy(); co = co.cpu().numpy()
    assert (info[:, 3] != R.TRUNCATED).all() and (info[:, 0] == np.diff(co)).all()          # every guided match passed this model's gate
    assert (info[:, 1] >= info[:, 0]).all() and info[:, 0].sum() > 0
    assert int(inl.sum()) == int(info[:, 1].sum())
