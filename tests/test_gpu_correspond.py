"""GPU: the correspondence export (include/mi_degensac.h mi_degensac_correspondences_*; tensor_api.correspondences_pairs_tensors /
_batch_tensors, matcher.correspondences_pairs / _batch).  Equality only: every result is compared with tests/correspond_ref.py, the
residuals bit for bit with the CPU oracle's metric functions.  The shapes are the smallest at which the three passes can go wrong: row
totals around a thread's 4 rows, a wave's 256, a workgroup's CORR_ROWS and a second step of the scan (CORR_SCAN workgroups), misaligned
match / keep bases, single survivors on both sides of every wave and workgroup boundary, runs of empty entries, entries of one row and
an entry across three workgroups."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, tensor_api
from tests import correspond_ref as cr, guided_ref as gr

pytestmark = pytest.mark.gpu
R, S = _lib.CORR_ROWS, _lib.CORR_SCAN


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _split(N, parts, rng):
    """N rows over `parts` images, some of them empty"""
    cuts = np.sort(rng.integers(0, N + 1, parts - 1)) if N else np.zeros(parts - 1, np.int64)
    c = np.diff(np.concatenate([[0], cuts, [N]])).astype(np.int64)
    if parts > 3:
        c[-1] += c[1]; c[1] = 0                                          # one image that is surely empty
    return c


def _case(N, seed, parts=6):
    """a store of `parts` images with N rows in all and the list that names every image once as the query image, in shuffled order, each
    against a random train image: N output rows.  match holds good rows and -1, -7, nt, nt + 1; keep holds 0, 1, 255."""
    rng = np.random.default_rng([seed, N])
    c = _split(N, parts, rng)
    qi = rng.permutation(parts)
    pairs = np.stack([qi, rng.integers(0, parts, parts)], axis=1)
    _, o2, pr, out = cr.layout(c, c, pairs)
    ent = np.repeat(np.arange(parts), np.diff(out))
    nt = c[pr[ent, 1]]
    match = (rng.random(N) * np.maximum(nt, 1)).astype(np.int32)
    odd = rng.random(N)
    match = np.where(odd < 0.1, -1, np.where(odd < 0.15, -7, np.where(odd < 0.2, nt, np.where(odd < 0.25, nt + 1, match)))).astype(np.int32)
    keep = rng.choice(np.array([0, 1, 255], np.uint8), N)
    return c, pairs, match, keep


def _np(t):
    return None if t is None else t.cpu().numpy()


def _compare(got, want, cap, with_pts=False):
    """got = the tuple of the tensor call (as numpy), want = cr.export(...) with the same capacity: the written prefix, the untouched tail,
    the offsets and the total"""
    rows, co, total, entry, pts, resid = got
    n = len(want["rows"])
    assert int(total[0]) == want["total"] and np.array_equal(co, want["corr_offsets"])
    assert rows.shape == (cap, 2) and np.array_equal(rows[:n], want["rows"]) and (rows[n:] == -1).all()
    if entry is not None:
        assert np.array_equal(entry[:n], want["entry"]) and (entry[n:] == -1).all()
    if with_pts:
        assert np.array_equal(pts[:n].view(np.int64), want["pts"].view(np.int64)) and np.isnan(pts[n:]).all()


def _check(c1, c2, pairs, match, keep=None, store_rows=False, capacity=None, kps1=None, kps2=None, tm=None, tk=None):
    """the tensor call against the restatement; tm / tk: device tensors to pass instead of uploads of match / keep"""
    tm = _t(match) if tm is None else tm
    tk = (None if keep is None else _t(keep)) if tk is None else tk
    tk1 = None if kps1 is None else _t(kps1)
    tk2 = None if kps2 is None else (tk1 if kps2 is kps1 else _t(kps2))
    fn = tensor_api.correspondences_batch_tensors if pairs is None else tensor_api.correspondences_pairs_tensors
    args = (tm, c1, c2) if pairs is None else (tm, c1, c2, pairs)
    got = tuple(_np(x) for x in fn(*args, keep=tk, kps1=tk1, kps2=tk2, store_rows=store_rows, with_entry=True, capacity=capacity))
    prs = cr.identity_pairs(len(c1)) if pairs is None else pairs
    want = cr.export(match, c1, c2, prs, keep=keep, store_rows=store_rows, capacity=capacity, kps1=kps1, kps2=kps2)
    N = len(match)
    _compare(got, want, N if capacity is None else capacity, with_pts=kps1 is not None)
    return got, want


# ---- row counts ----
@pytest.mark.parametrize("N", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 2 * R + 1, (S - 1) * R + 1, S * R, S * R + 1])
def test_row_totals_at_the_edges_of_thread_wave_workgroup_and_scan_step(N):
    c, pairs, match, keep = _case(N, 1)
    got, want = _check(c, c, pairs, match, keep)
    _check(c, c, pairs, match, None, store_rows=True)
    if N >= 64:
        assert 0 < want["total"] < N


@pytest.mark.parametrize("first", [(5, 0), (0, 9), (1027, 3)])
@pytest.mark.parametrize("flags", [0, _lib.CORR_STORE_ROWS])
def test_stores_with_a_non_zero_first_offset(first, flags):
    """the C entry point with offsets that do not start at 0: the stores' pointers are indexed like the offsets, which is the restatement
    on stores with one more image in front"""
    import torch
    c, pairs, match, keep = _case(2 * R + 77, 2)
    kps = np.random.default_rng(5).uniform(0, 100, (int(c.sum()) + max(first), 2))
    c1 = np.concatenate([[first[0]], c]); c2 = np.concatenate([[first[1]], c])
    k1 = kps[:c1.sum()]; k2 = kps[:c2.sum()][::-1].copy()
    want = cr.export(match, c1, c2, pairs + 1, keep=keep, store_rows=bool(flags), kps1=k1, kps2=k2)
    o1 = cr.offsets(c1)[1:].copy(); o2 = cr.offsets(c2)[1:].copy()
    out = _raw("pairs", (o1, o2, np.ascontiguousarray(pairs, np.int32)), _t(match), _t(keep), flags, _t(k1), _t(k2), 2, None, None, len(match))
    torch.cuda.synchronize()
    _compare(tuple(_np(x) for x in out), want, len(match), with_pts=True)


def _raw(name, lay, tm, tk, flags, tk1, tk2, kd, tM, gp, cap, outs=None, want_resid=False):
    """mi_degensac_correspondences_{pairs,batch}_dev on device tensors; lay = (o1, o2, pairs int32 [K, 2]) or (o1, o2).  outs: the six
    output tensors to write into (None = fresh ones, pre-filled).  Returns (rows, corr_offsets, total, entry, pts, resid)."""
    import torch
    dev = _dev(); lp = C.POINTER(C.c_int64)
    if name == "pairs":
        o1, o2, pr = lay; K = len(pr)
        layout = (o1.ctypes.data_as(lp), len(o1) - 1, o2.ctypes.data_as(lp), len(o2) - 1, pr.ctypes.data_as(C.POINTER(C.c_int32)), K)
    else:
        o1, o2 = lay; K = len(o1) - 1
        layout = (o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), K)
    if outs is None:
        outs = (torch.full((cap, 2), -1, dtype=torch.int32, device=dev), torch.full((K + 1,), -5, dtype=torch.int64, device=dev),
                torch.full((1,), -5, dtype=torch.int64, device=dev), torch.full((cap,), -1, dtype=torch.int32, device=dev),
                None if tk1 is None else torch.full((cap, 4), float("nan"), dtype=torch.float64, device=dev),
                torch.full((cap,), float("nan"), dtype=torch.float64, device=dev) if want_resid else None)
    rows, co, total, entry, pts, resid = outs
    p = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    stream = torch.cuda.current_stream(dev)
    rc = getattr(_lib.lib(), f"mi_degensac_correspondences_{name}_dev")(*layout, p(tm), p(tk), flags, p(tk1), p(tk2), kd, p(tM),
                                                                       None if gp is None else C.byref(gp), cap, 0, C.c_void_p(stream.cuda_stream),
                                                                       p(co), p(total), p(rows), p(entry), p(pts), p(resid))
    _lib.check_match(rc)
    return outs


@pytest.mark.parametrize("shift_m,shift_k", [(1, 1), (2, 3), (3, 2), (0, 1), (1, 0)])
def test_match_and_keep_bases_that_are_not_aligned(shift_m, shift_k):
    """slices of larger tensors: match at a 4-byte but not 16-byte boundary, keep at an odd address: the scalar loads, the same result"""
    c, pairs, match, keep = _case(2 * R + 9, 3)
    N = len(match)
    big_m = _t(np.concatenate([np.full(shift_m, 2, np.int32), match, np.full(5, 2, np.int32)]))
    big_k = _t(np.concatenate([np.full(shift_k, 1, np.uint8), keep, np.full(5, 1, np.uint8)]))
    tm, tk = big_m[shift_m:shift_m + N], big_k[shift_k:shift_k + N]
    assert tm.data_ptr() % 16 == 4 * shift_m and tk.data_ptr() % 4 == shift_k % 4
    _check(c, c, pairs, match, keep, tm=tm, tk=tk)
    _check(c, c, pairs, match, keep != 0, tm=tm, tk=tk != 0)          # bool keep


# ---- selection patterns ----
def _plain(N, parts=5, seed=4):
    """a list whose every match value is a good row (train images are not empty): the selection is what keep says"""
    rng = np.random.default_rng([seed, N])
    c = np.maximum(_split(N - parts, parts, rng), 0) + 1
    pairs = np.stack([np.arange(parts), rng.integers(0, parts, parts)], axis=1)
    _, _, pr, out = cr.layout(c, c, pairs)
    nt = c[pr[np.repeat(np.arange(parts), np.diff(out)), 1]]
    return c, pairs, (rng.random(N) * nt).astype(np.int32)


def test_none_all_and_every_second_row():
    N = 2 * R + 1
    c, pairs, match = _plain(N)
    assert _check(c, c, pairs, match, np.zeros(N, np.uint8))[1]["total"] == 0
    assert _check(c, c, pairs, match, None)[1]["total"] == N
    assert _check(c, c, pairs, match, np.full(N, 255, np.uint8))[1]["total"] == N
    assert _check(c, c, pairs, np.full(N, -1, np.int32), None)[1]["total"] == 0
    _check(c, c, pairs, match, (np.arange(N) % 2).astype(np.uint8))
    _check(c, c, pairs, match, ((np.arange(N) + 1) % 2).astype(np.uint8), store_rows=True)


def test_exactly_one_row_on_each_side_of_every_wave_and_workgroup_boundary():
    N = 2 * R + 1
    c, pairs, match = _plain(N)
    tm = _t(match)
    spots = sorted({0, N - 1} | {b + d for b in range(256, N, 256) for d in (-1, 0)} | {3, 4, 255 * 4 + 3})
    for r in spots:
        keep = np.zeros(N, np.uint8); keep[r] = 1
        got, want = _check(c, c, pairs, match, keep, tm=tm)
        assert want["total"] == 1 and int(got[0][0, 1]) == match[r], r


def test_an_empty_workgroup_between_two_full_ones():
    N = 3 * R
    c, pairs, match = _plain(N)
    keep = np.ones(N, np.uint8); keep[R:2 * R] = 0
    assert _check(c, c, pairs, match, keep)[1]["total"] == 2 * R


# ---- entries ----
def test_runs_of_empty_entries_entries_of_one_row_and_an_entry_across_three_workgroups():
    c = np.array([0, R - 5, 1, 2 * R - 10, 0, 1, 7])
    # empty entries at the start (2), in the middle (3 in a run) and at the end (2); image 3 spans workgroups 0, 1 and 2
    pairs = np.array([(0, 1), (4, 6), (1, 3), (2, 2), (0, 0), (4, 1), (0, 6), (3, 1), (5, 6), (4, 4), (0, 3)])
    _, _, pr, out = cr.layout(c, c, pairs)
    N = int(out[-1])
    rng = np.random.default_rng(6)
    nt = c[pr[np.repeat(np.arange(len(pairs)), np.diff(out)), 1]]
    match = (rng.random(N) * nt).astype(np.int32)
    for keep in (None, rng.choice(np.array([0, 1], np.uint8), N), np.zeros(N, np.uint8)):
        got, want = _check(c, c, pairs, match, keep, store_rows=True)
        co = want["corr_offsets"]
        assert co[0] == co[1] == co[2] == 0 and co[4] == co[5] == co[6] == co[7] and co[9] == co[10] == co[11] == want["total"]


def test_many_entries_inside_one_wave():
    c = np.ones(64, np.int64)
    rng = np.random.default_rng(7)
    pairs = np.stack([rng.permutation(64), rng.integers(0, 64, 64)], axis=1)
    match = rng.choice(np.array([0, 0, 0, 1, -1], np.int32), 64)
    got, want = _check(c, c, pairs, match, None, store_rows=True)
    assert np.array_equal(np.diff(want["corr_offsets"]), (match == 0).astype(np.int64))


def test_self_pairs_repeats_both_orders_last_image_first_and_empty_train_images():
    c = np.array([40, 0, 300, 17])
    pairs = np.array([(3, 0), (2, 2), (0, 2), (2, 0), (0, 2), (3, 1), (2, 1), (3, 3), (1, 2)])      # (3, 1), (2, 1): train images of 0 rows
    _, _, pr, out = cr.layout(c, c, pairs)
    N = int(out[-1])
    rng = np.random.default_rng(8)
    match = rng.integers(-1, 45, N).astype(np.int32)
    keep = rng.choice(np.array([0, 1, 255], np.uint8), N)
    kps = rng.uniform(0, 100, (int(c.sum()), 6))
    got, want = _check(c, c, pairs, match, keep, kps1=kps, kps2=kps)
    co = want["corr_offsets"]
    assert co[5] == co[6] == co[7] and want["total"] > 0                  # nothing can be selected against an empty train image
    _check(c, c, pairs, match, None, store_rows=True, kps1=kps, kps2=kps)


def test_two_stores():
    c1 = np.array([9, 0, 130]); c2 = np.array([3, 50, 0, 8])
    pairs = np.array([(2, 1), (0, 3), (2, 0), (1, 1), (0, 2), (2, 3)])
    _, _, pr, out = cr.layout(c1, c2, pairs)
    N = int(out[-1])
    rng = np.random.default_rng(9)
    match = rng.integers(-2, 52, N).astype(np.int32)
    k1 = rng.uniform(0, 100, (int(c1.sum()), 2)); k2 = rng.uniform(0, 100, (int(c2.sum()), 2))
    _check(c1, c2, pairs, match, None, kps1=k1, kps2=k2)
    _check(c1, c2, pairs, match, rng.choice(np.array([0, 1], np.uint8), N), store_rows=True, kps1=k1, kps2=k2)


@pytest.mark.parametrize("store_rows", [False, True])
def test_the_ragged_batch_is_the_pair_list_call_on_the_identity_list(store_rows):
    rng = np.random.default_rng(10)
    c1 = np.array([0, 700, 1, 0, 1500, 33]); c2 = np.array([5, 640, 0, 9, 1400, 33])
    N = int(c1.sum())
    nt = np.repeat(c2, c1)
    match = (rng.random(N) * (nt + 2)).astype(np.int32) - 1
    keep = rng.choice(np.array([0, 1], np.uint8), N)
    k1 = rng.uniform(0, 100, (N, 2)); k2 = rng.uniform(0, 100, (int(c2.sum()), 2))
    b, _ = _check(c1, c2, None, match, keep, store_rows=store_rows, kps1=k1, kps2=k2)
    p, _ = _check(c1, c2, cr.identity_pairs(6), match, keep, store_rows=store_rows, kps1=k1, kps2=k2)
    for x, y in zip(b, p):
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True)


# ---- capacity ----
def test_capacity_cuts_the_arrays_and_nothing_else():
    c, pairs, match, keep = _case(2 * R + 300, 11)
    kps = np.random.default_rng(11).uniform(0, 100, (int(c.sum()), 2))
    total = cr.export(match, c, c, pairs, keep=keep)["total"]
    assert total > R
    for cap in (total, total - 1, 1, 0, None, total + 7):
        got, want = _check(c, c, pairs, match, keep, capacity=cap, kps1=kps, kps2=kps)
        assert want["total"] == total and len(want["rows"]) == min(total, len(match) if cap is None else cap)


@pytest.mark.parametrize("cap_delta", [0, -1, -700])
def test_nothing_is_written_outside_the_arrays(cap_delta):
    """outputs that are slices of larger tensors with guard elements on both sides, rows at a 4-byte and pts at an 8-byte boundary only"""
    import torch
    c, pairs, match, keep = _case(2 * R + 300, 12)
    kps = np.random.default_rng(12).uniform(0, 100, (int(c.sum()), 2))
    total = cr.export(match, c, c, pairs, keep=keep)["total"]
    cap = total + cap_delta
    dev = _dev(); G = 3; K = len(pairs)
    for odd in (0, 1):                                                   # odd = 1: the guard in front is an odd number of elements
        g = G + odd
        B = dict(rows=torch.full((2 * cap + 2 * g,), -9, dtype=torch.int32, device=dev), co=torch.full((K + 1 + 2 * g,), -9, dtype=torch.int64, device=dev),
                 total=torch.full((1 + 2 * g,), -9, dtype=torch.int64, device=dev), entry=torch.full((cap + 2 * g,), -9, dtype=torch.int32, device=dev),
                 pts=torch.full((4 * cap + 2 * g,), -9.0, dtype=torch.float64, device=dev), resid=torch.full((cap + 2 * g,), -9.0, dtype=torch.float64, device=dev))
        outs = (B["rows"][g:g + 2 * cap].view(cap, 2), B["co"][g:g + K + 1], B["total"][g:g + 1], B["entry"][g:g + cap], B["pts"][g:g + 4 * cap].view(cap, 4),
                B["resid"][g:g + cap])
        o = cr.offsets(c)
        M = _t(np.tile(np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]]), (K, 1, 1)).reshape(K, 9))
        _raw("pairs", (o, o, np.ascontiguousarray(pairs, np.int32)), _t(match), _t(keep), 0, _t(kps), _t(kps), 2, M, _lib.GuideParams(0, 0, 0.0), cap, outs=outs)
        torch.cuda.synchronize()
        want = cr.export(match, c, c, pairs, keep=keep, capacity=cap, kps1=kps, kps2=kps)
        n = len(want["rows"])
        assert n == min(total, cap)
        assert np.array_equal(_np(outs[0]), want["rows"]) and np.array_equal(_np(outs[1]), want["corr_offsets"]) and int(outs[2][0]) == total
        assert np.array_equal(_np(outs[3]), want["entry"]) and np.array_equal(_np(outs[4]), want["pts"])
        assert not np.isnan(_np(outs[5])).any() and (_np(outs[5]) != -9.0).all()
        for name, t in B.items():
            t = _np(t)
            assert (t[:g] == -9).all() and (t[-g:] == -9).all(), name


# ---- points and residuals ----
def test_keypoint_layouts():
    import torch
    c, pairs, match, keep = _case(R + 50, 13)
    rng = np.random.default_rng(13)
    k6 = rng.uniform(0, 100, (int(c.sum()), 6))
    _check(c, c, pairs, match, keep, kps1=k6[:, :2].copy(), kps2=k6[:, :2].copy())
    _check(c, c, pairs, match, keep, kps1=k6, kps2=k6)
    k4 = rng.uniform(1, 100, (int(c.sum()), 4)).astype(np.float32)
    t4 = _t(k4)
    xyA = _np(tensor_api.kpts_to_xyA_tensors(t4))
    got = tensor_api.correspondences_pairs_tensors(_t(match), c, c, pairs, keep=_t(keep), kps1=t4, kps2=t4, with_entry=True)
    torch.cuda.synchronize()
    _compare(tuple(_np(x) for x in got), cr.export(match, c, c, pairs, keep=keep, kps1=xyA, kps2=xyA), len(match), with_pts=True)


def _two_view(model, n=700, seed=3):
    """a synthetic two-view pair and the estimator's model for it, in the driver's form (numpy [3, 3])"""
    import pydegensac_amd
    from pydegensac_amd import synthetic
    if model == "F":
        p1, p2, _, _ = synthetic.two_view_fundamental(n, 0.5, 0.3, seed=seed)
        M, _ = pydegensac_amd.findFundamentalMatrix(p1, p2, 0.5, 0.999, 5000, seed=5)
        return p1[:, :2].copy(), p2[:, :2].copy(), np.ascontiguousarray(M, np.float64), np.ascontiguousarray(M, np.float64)
    p1, p2 = synthetic.homography_pairs(n, 0.5, 0.5, seed=seed)[:2]
    H, _ = pydegensac_amd.findHomography(p1, p2, 1.0, 0.999, 5000, seed=5)
    H = np.ascontiguousarray(H, np.float64)
    Hd = _np(tensor_api._h_driver_form(_t(H[None])))[0]                  # the bits the tensor call converts to
    return p1[:, :2].copy(), p2[:, :2].copy(), H, Hd


_TV = {}


def _tv(model):
    if model not in _TV:
        _TV[model] = _two_view(model)
    return _TV[model]


def _resid_call(model, et, p1, p2, M, driver_form, keep=None):
    n = len(p1)
    got = tensor_api.correspondences_batch_tensors(_t(np.arange(n, dtype=np.int32)), [n], [n], keep=None if keep is None else _t(keep), kps1=_t(p1),
                                                   kps2=_t(p2), models=_t(np.asarray(M).reshape(1, 3, 3)), model=model,
                                                   error_type=gr.ERROR_NAMES[model][et], driver_form=driver_form, with_entry=True)
    return tuple(_np(x) for x in got)


@pytest.mark.parametrize("model,et", gr.KINDS)
def test_residuals_are_the_oracles_bits(oracle_port, model, et):
    p1, p2, Mu, Md = _tv(model)
    keep = (np.arange(len(p1)) % 3 != 1).astype(np.uint8)
    rows, co, total, entry, pts, resid = _resid_call(model, et, p1, p2, Md, True, keep)
    n = int(total[0])
    assert n == int(keep.sum()) and np.array_equal(rows[:n, 0], np.flatnonzero(keep)) and np.isnan(resid[n:]).all()
    want = cr.resid(oracle_port, model, et, Md[None], entry[:n], pts[:n])
    assert np.isfinite(want).all() and (want <= gr.th(model, et, 3.0)).sum() > 50           # a model that explains its inliers
    assert cr.same_bits_or_nan(resid[:n], want)
    if model == "H":                                                     # the user-facing H gives the same bits
        r2 = _resid_call(model, et, p1, p2, Mu, False, keep)[5]
        assert np.array_equal(r2.view(np.int64), resid.view(np.int64))


@pytest.mark.parametrize("model,et", gr.KINDS)
def test_residuals_of_degenerate_models_and_keypoints(oracle_port, model, et):
    p1, p2, _, Md = _tv(model)
    p1 = p1[:200].copy(); p2 = p2[:200].copy()
    bad1 = p1.copy(); bad2 = p2.copy()
    bad1[3, 0] = np.inf; bad1[10, 1] = np.nan; bad2[17, 0] = -np.inf; bad2[40, 1] = np.nan; bad1[50] = 1e200; bad2[60] = -1e200
    nanM = Md.copy(); nanM[1, 1] = np.nan
    infM = Md.copy(); infM[0, 2] = np.inf
    for M, a, b in ((np.zeros((3, 3)), p1, p2), (nanM, p1, p2), (infM, p1, p2), (Md * 1e150, p1, p2), (Md * 1e-150, p1, p2), (Md, bad1, bad2)):
        rows, co, total, entry, pts, resid = _resid_call(model, et, a, b, M, True)
        assert int(total[0]) == 200
        want = cr.resid(oracle_port, model, et, np.asarray(M)[None], entry, pts)
        assert cr.same_bits_or_nan(resid, want)


def _collection(m=4, n=300, dim=32, seed=0):
    from pydegensac_amd import synthetic
    kps, descs = synthetic.image_collection(m, n, 0.6, 0.1, dim, seed=seed)
    return np.concatenate(kps), np.concatenate(descs), [n] * m


@pytest.mark.parametrize("model,et", gr.KINDS)
def test_every_guided_match_lies_inside_the_gate_it_passed(model, et):
    """guided_match_pairs_tensors with px_th, then the export with the same models: the export and the gate call the same function, so
    resid <= th holds for every exported correspondence, without a tolerance"""
    k, d, c = _collection()
    pairs = matcher.exhaustive_pairs(4, ordered=True)
    tk, td = _t(k), _t(d)
    name = gr.ERROR_NAMES[model][et]
    M = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, c, c, pairs, model=model, error_type=name)[0]
    px = 4.0
    gm = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, c, c, pairs, M, model=model, px_th=px, error_type=name)[0]
    rows, co, total, entry, pts, resid = (_np(x) for x in tensor_api.correspondences_pairs_tensors(gm, c, c, pairs, kps1=tk, kps2=tk, models=M, model=model,
                                                                                                  error_type=name, with_entry=True))
    n = int(total[0])
    assert n == int((_np(gm) >= 0).sum()) and n > 50
    assert (resid[:n] <= gr.th(model, et, px)).all()


# ---- chains and execution ----
def test_verified_matches_of_a_pair_list_per_entry():
    k, d, c = _collection()
    pairs = matcher.exhaustive_pairs(4, ordered=True)
    tk, td = _t(k), _t(d)
    F, match, inlier, stats, nten, po = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, c, c, pairs, model="F")
    rows, co, total, entry, pts, resid = tensor_api.correspondences_pairs_tensors(match, c, c, pairs, keep=inlier, kps1=tk, kps2=tk, models=F, with_entry=True,
                                                                                  capacity=int(nten.sum()))
    inl = _np(inlier)
    per = np.array([inl[po[p]:po[p + 1]].sum() for p in range(len(pairs))])
    assert np.array_equal(np.diff(_np(co)), per) and int(total[0]) == inl.sum() > 100
    want = cr.export(_np(match), c, c, pairs, keep=inl, capacity=int(nten.sum()), kps1=k, kps2=k)
    _compare(tuple(_np(x) for x in (rows, co, total, entry, pts, resid)), want, int(nten.sum()), with_pts=True)
    tent = tensor_api.correspondences_pairs_tensors(match, c, c, pairs)
    assert np.array_equal(np.diff(_np(tent[1])), nten)                   # keep=None: the tentatives


def test_both_models_overlap_counts():
    k, d, c = _collection()
    pairs = matcher.exhaustive_pairs(4)
    tk, td = _t(k), _t(d)
    out = tensor_api.match_and_verify_fh_pairs_tensors(tk, tk, td, td, c, c, pairs)
    match, inf, inh, summ = out[2], out[3], out[4], _np(out[7])
    co = _np(tensor_api.correspondences_pairs_tensors(match, c, c, pairs, keep=inf & inh)[1])
    assert np.array_equal(np.diff(co), summ[:, 3])
    co = _np(tensor_api.correspondences_pairs_tensors(match, c, c, pairs, keep=inf)[1])
    assert np.array_equal(np.diff(co), summ[:, 1]) and summ[:, 1].sum() > 100


def test_numpy_entry_points(oracle_port):
    c, pairs, match, keep = _case(R + 200, 14)
    rng = np.random.default_rng(14)
    kps = rng.uniform(0, 100, (int(c.sum()), 2))
    o = cr.offsets(c)
    kl = [kps[o[i]:o[i + 1]] for i in range(len(c))]
    M = rng.normal(size=(len(pairs), 3, 3))
    for store_rows in (False, True):
        got = matcher.correspondences_pairs(match, c, c, pairs, keep=keep, kps_list=kl, models=M, model="F", error_type="symm_epipolar",
                                            store_rows=store_rows)
        want = cr.export(match, c, c, pairs, keep=keep, store_rows=store_rows, kps1=kps, kps2=kps)
        wres = cr.resid(oracle_port, "F", 1, M, want["entry"], want["pts"])
        co = want["corr_offsets"]
        assert len(got) == len(pairs)
        for p, g in enumerate(got):
            s = slice(co[p], co[p + 1])
            assert np.array_equal(g["rows"], want["rows"][s]) and np.array_equal(g["pts"], want["pts"][s])
            assert cr.same_bits_or_nan(g["resid"], wres[s])
    got = matcher.correspondences_pairs(match, c, c, pairs)
    assert all(g["pts"] is None and g["resid"] is None for g in got) and sum(len(g["rows"]) for g in got) == cr.export(match, c, c, pairs)["total"]
    # the ragged batch
    c1 = np.array([30, 0, 1200]); c2 = np.array([20, 4, 1100])
    N = int(c1.sum())
    match = (rng.random(N) * (np.repeat(c2, c1) + 1)).astype(np.int32)
    k1 = rng.uniform(0, 100, (N, 2)); k2 = rng.uniform(0, 100, (int(c2.sum()), 2))
    o1, o2 = cr.offsets(c1), cr.offsets(c2)
    got = matcher.correspondences_batch(match, c1, c2, kps1_list=[k1[o1[i]:o1[i + 1]] for i in range(3)], kps2_list=[k2[o2[i]:o2[i + 1]] for i in range(3)])
    want = cr.export(match, c1, c2, cr.identity_pairs(3), kps1=k1, kps2=k2)
    co = want["corr_offsets"]
    for p, g in enumerate(got):
        assert np.array_equal(g["rows"], want["rows"][co[p]:co[p + 1]]) and np.array_equal(g["pts"], want["pts"][co[p]:co[p + 1]])


def test_host_form_with_every_optional_output_equals_the_device_form():
    """mi_degensac_correspondences_pairs with entry, pts and resid given, on 2 entries with one empty and a capacity one below the total:
    what it writes is what the device form writes on the same inputs, bit for bit"""
    import torch
    o = np.array([0, 6, 6, 12], np.int64); pr = np.array([[1, 0], [0, 2]], np.int32)          # image 1 is empty: entry 0 has no row
    match = np.array([0, 7, -1, 3, 5, 2], np.int32); keep = np.array([1, 1, 1, 0, 1, 1], np.uint8)      # rows 0, 4, 5 are selected
    rng = np.random.default_rng(21)
    kps = rng.uniform(0, 100, (12, 2)); M = rng.normal(size=(2, 9)); gp = _lib.GuideParams(False, 0, 0.0); cap = 2
    dev = _raw("pairs", (o, o, pr), _t(match), _t(keep), 0, _t(kps), _t(kps), 2, _t(M), gp, cap, want_resid=True)
    torch.cuda.synchronize()
    dev = [_np(x) for x in dev]
    assert dev[2][0] == 3 and dev[1].tolist() == [0, 0, 3] and dev[3].tolist() == [1, 1]
    host = [np.full((cap, 2), -1, np.int32), np.full(3, -5, np.int64), np.full(1, -5, np.int64), np.full(cap, -1, np.int32),
            np.full((cap, 4), np.nan), np.full(cap, np.nan)]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)          # noqa: E731
    lp = o.ctypes.data_as(C.POINTER(C.c_int64))
    rc = _lib.lib().mi_degensac_correspondences_pairs(lp, 3, lp, 3, pr.ctypes.data_as(C.POINTER(C.c_int32)), 2, vp(match), vp(keep), 0, vp(kps), vp(kps), 2,
                                                      vp(M), C.byref(gp), cap, 0, vp(host[1]), vp(host[2]), vp(host[0]), vp(host[3]), vp(host[4]),
                                                      vp(host[5]))
    _lib.check_match(rc)
    for h, d in zip(host, dev):
        assert h.tobytes() == np.ascontiguousarray(d).tobytes()


def test_a_second_stream():
    import torch
    c, pairs, match, keep = _case(3 * R + 5, 15)
    s = torch.cuda.Stream(device=_dev())
    tm, tk = _t(match), _t(keep)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = tensor_api.correspondences_pairs_tensors(tm, c, c, pairs, keep=tk, with_entry=True)
    s.synchronize()
    _compare(tuple(_np(x) for x in got), cr.export(match, c, c, pairs, keep=keep), len(match))


def test_two_calls_into_the_same_outputs_leave_no_state():
    import torch
    outs = None
    o = pr = None
    for seed in (16, 17, 16):
        c, pairs, match, keep = _case(2 * R + 40, seed)
        o = cr.offsets(c); pr = np.ascontiguousarray(pairs, np.int32)
        outs = _raw("pairs", (o, o, pr), _t(match), _t(keep), 0, None, None, 0, None, None, len(match), outs=outs)
        torch.cuda.synchronize()
        want = cr.export(match, c, c, pairs, keep=keep)
        n = want["total"]
        assert int(outs[2][0]) == n and np.array_equal(_np(outs[1]), want["corr_offsets"])
        assert np.array_equal(_np(outs[0])[:n], want["rows"]) and np.array_equal(_np(outs[3])[:n], want["entry"])


def test_an_empty_list_and_a_list_without_rows():
    import torch
    dev = _dev()
    z = np.zeros(1, np.int64)
    for name, lay in (("pairs", (z, z, np.zeros((0, 2), np.int32))), ("batch", (z, z))):
        outs = _raw(name, lay, None, None, 0, None, None, 0, None, None, 0)
        torch.cuda.synchronize()
        assert int(outs[2][0]) == 0 and int(outs[1][0]) == 0
    co, total = (_np(x) for x in tensor_api.correspondences_pairs_tensors(torch.zeros(0, dtype=torch.int32, device=dev), [0, 0, 0], [4, 0, 2],
                                                                          [(0, 0), (2, 1), (1, 2)])[1:3])
    assert co.tolist() == [0, 0, 0, 0] and int(total[0]) == 0
