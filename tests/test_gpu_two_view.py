"""GPU: match once, verify F and H (tensor_api.match_and_verify_fh_*_tensors, matcher.match_and_verify_fh_*, include/mi_degensac.h
mi_degensac_match_verify_fh_*).  Equality only.  Every result of the new call is compared with (a) the two existing calls, F then H, on
the same inputs, seeds and match parameters: models, inlier rows and the deterministic stats columns bit for bit per model, match and the
tentative counts with either; and (b) tests/two_view_ref.summary_ref on the returned masks.  A subset is also compared with the CPU
restatement of tests/verify_ref.py under verify_ref.BUDGET for both models (masks and counters bit for bit, models to MODEL_RTOL).
Scenes are those of tests/verify_ref.py; tests/test_two_view_cpu.py shows what the restatement of the summary notices."""
import ctypes as C
import functools

import numpy as np
import pytest

import pydegensac_amd as pd
from pydegensac_amd import _lib, matcher, tensor_api
from tests import fginn_ref as fr, pairs_ref as pr, two_view_ref as tv, verify_ref as vr

pytestmark = pytest.mark.gpu

DET = [c for c in range(16) if c not in (12, 13)]      # every stats column but the two device clock readings
CTR = [0, 1, 3]                                        # samples, lo_runs, I
FP, HP = vr.BUDGET["F"], vr.BUDGET["H"]
R = 10.0


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(M):
    import torch
    return M.contiguous().view(torch.int64)


def _same(got, wf, wh, po):
    """got = the new call's tuple (F, H, match, inlier_f, inlier_h, stats_f, stats_h, summary, cnt, ...), wf / wh = the existing call's
    tuple (model, match, inlier, stats, cnt, ...) for F / H: (a) and (b) of the module docstring"""
    import torch
    torch.cuda.synchronize()
    F, H, match, inf, inh, stf, sth, summ, cnt = got[:9]
    assert torch.equal(_bits(F), _bits(wf[0])) and torch.equal(_bits(H), _bits(wh[0]))
    assert torch.equal(match, wf[1]) and torch.equal(match, wh[1])
    assert inf.dtype == torch.bool and inh.dtype == torch.bool and torch.equal(inf, wf[2]) and torch.equal(inh, wh[2])
    assert torch.equal(stf[:, DET], wf[3][:, DET]) and torch.equal(sth[:, DET], wh[3][:, DET])
    assert isinstance(cnt, np.ndarray) and cnt.dtype == np.int64 and np.array_equal(cnt, wf[4]) and np.array_equal(cnt, wh[4])
    s = summ.cpu().numpy()
    assert s.dtype == np.int32 and s.shape == (len(cnt), 4)
    assert np.array_equal(s, tv.summary_ref(match.cpu().numpy(), inf.cpu().numpy(), inh.cpu().numpy(), po))
    assert np.array_equal(s[:, 0], cnt)
    Fn, Hn, sf, sh = F.cpu().numpy(), H.cpu().numpy(), stf.cpu().numpy(), sth.cpu().numpy()
    for p in range(len(cnt)):                            # the follow-on rules: an F from 8 tentatives on, an H from 4 on
        assert bool(Fn[p].any()) <= (cnt[p] >= 8) and bool(Hn[p].any()) <= (cnt[p] >= 4), p
        assert (sf[p, 0] > 0) == (cnt[p] >= 8) and (sh[p, 0] > 0) == (cnt[p] >= 4), p
    return s


def _batch_args(scs, kpts=False):
    k1, k2 = ("k4_1", "k4_2") if kpts else ("k1", "k2")
    c1 = [s["n1"] for s in scs]; c2 = [s["n2"] for s in scs]
    cat = lambda k: _t(np.concatenate([s[k] for s in scs]))          # noqa: E731
    return (cat(k1), cat(k2), cat("d1"), cat("d2"), c1, c2), np.r_[0, np.cumsum(c1)].astype(np.int64)


def _batch_both(scs, seeds, mutual=False, kpts=False, fginn_th=None, fp=FP, hp=HP):
    """the new batch call and the two existing ones on designed pairs of one norm and ratio -> (got, summary, offsets)"""
    args, po = _batch_args(scs, kpts)
    kw = dict(ratio=scs[0]["ratio"], mutual=mutual, seeds=seeds, norm=scs[0]["norm"], fginn_th=fginn_th)
    got = tensor_api.match_and_verify_fh_batch_tensors(*args, f_params=fp, h_params=hp, **kw)
    wf = tensor_api.match_and_verify_batch_tensors(*args, model="F", **fp, **kw)
    wh = tensor_api.match_and_verify_batch_tensors(*args, model="H", **hp, **kw)
    return got, _same(got, wf, wh, po), po


def _vs_restatement(port, got, po, scs, seeds, mutual=False):
    """the new call's rows against the CPU restatement under BUDGET for both models"""
    F, H, match, inf, inh, stf, sth, summ, cnt = [x.cpu().numpy() if hasattr(x, "cpu") else x for x in got[:9]]
    for p, sc in enumerate(scs):
        rows = slice(int(po[p]), int(po[p + 1]))
        want = tv.both_ref(port, sc, seeds[p], mutual)
        for m, M, inl, st in (("F", F, inf, stf), ("H", H, inh, sth)):
            g = dict(model=M[p], match=match[rows], inlier=inl[rows], cnt=int(cnt[p]), counters=tuple(int(c) for c in st[p, CTR]))
            bad = vr.disagreements(g, want[m])
            assert not bad, (p, m, bad, g["cnt"], want[m]["cnt"], g["counters"], want[m]["counters"])
        assert np.array_equal(np.flatnonzero(match[rows] >= 0), sc["kept"][mutual]), p          # the stated tentatives


def _h_close(H_dev, H_host):
    """the user-facing H of the tensor calls (inverted by torch on the device) against that of the numpy calls (inverted by numpy): the same
    driver-form bits through two inversions, so equal to rounding only; zero models are zero in both"""
    return np.array_equal(H_dev.any(axis=(1, 2)), H_host.any(axis=(1, 2))) and np.allclose(H_dev, H_host, rtol=1e-9, atol=0)


# ---- count thresholds: exactly 3 / 4 / 5 / 7 / 8 / 9 tentatives among 300 queries (K = 1) ------------------------------------------------
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("layout,core,dups", [(m, c, d) for m in ("F", "H") for c, d in vr.COUNT_CASES[m]])
def test_count_thresholds(oracle_port, layout, core, dups, mutual):
    norm = vr.NORMS[(core + dups) % 3]
    sc = vr.count_scene(layout, core, dups, norm); seed = 100 + core
    got, s, po = _batch_both([sc], [seed], mutual=mutual)
    n = core + (0 if mutual else dups)
    assert s[0, 0] == n and n in (3, 4, 5, 7, 8, 9)
    F, H = got[0][0], got[1][0]
    assert bool(got[6][0, 0] > 0) == (n >= 4) and bool(got[5][0, 0] > 0) == (n >= 8)
    if n < 8:
        assert not F.any() and not got[3].any() and not got[5].any() and s[0, 1] == 0 == s[0, 3]
    if n < 4:
        assert not H.any() and not got[4].any() and not got[6].any() and s[0, 2] == 0
    _vs_restatement(oracle_port, got, po, [sc], [seed], mutual)


# ---- batch composition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vr.ARRANGEMENTS))
@pytest.mark.parametrize("layout", ["F", "H"])
def test_batch_arrangements(oracle_port, layout, name):
    """12 pairs: all short, all eligible, short first, short last, one eligible pair between short and empty ones.  A short pair of the
    [n, 2] scenes has 5 tentatives (an H, no F), one of the [n, 6] scenes 3 (neither)."""
    scs = vr.batch_scene(layout, name); seeds = vr.batch_seeds(name)
    got, s, po = _batch_both(scs, seeds)
    kinds = vr.ARRANGEMENTS[name]
    assert [int(c >= 8) for c in s[:, 0]] == [int(k == "E") for k in kinds]
    assert [int(4 <= c < 8) for c in s[:, 0]] == [int(k == "S" and layout == "F") for k in kinds]
    if name in ("around_one", "short_last"):
        _vs_restatement(oracle_port, got, po, scs, seeds)


@pytest.mark.parametrize("layout,norm,kpts", [("F", "l2", False), ("H", "l2_u8", False), ("H", "l2_u8", True), ("F", "hamming", False)])
def test_alternating_h_only_and_both(oracle_port, layout, norm, kpts):
    """5 tentatives (H only) | empty | >= 9 (both) ...: the eligible index and the row base of every pair differ between the halves"""
    import torch
    scs = tv.alternating_scenes(layout, norm); seeds = tv.ALTERNATING_SEEDS
    got, s, po = _batch_both(scs, seeds, kpts=kpts)
    assert ["Q" if c == 0 else "5" if c == 5 else "E" for c in s[:, 0]] == list(tv.ALTERNATING)
    stf, sth = got[5].cpu().numpy(), got[6].cpu().numpy()
    for p, k in enumerate(tv.ALTERNATING):
        assert (stf[p, 0] > 0) == (k == "E") and (sth[p, 0] > 0) == (k != "Q"), p
    assert (s[[p for p, k in enumerate(tv.ALTERNATING) if k == "E"], 1] >= 8).all()          # every F found its inliers where they are
    if not kpts:
        _vs_restatement(oracle_port, got, po, scs, seeds)
    # each pair alone gives the same rows
    F, H, match = got[0], got[1], got[2]
    for p in (0, 2, 3, 11):
        one, _, _ = _batch_both([scs[p]], [seeds[p]], kpts=kpts)
        assert torch.equal(_bits(one[0][0]), _bits(F[p])) and torch.equal(_bits(one[1][0]), _bits(H[p]))
        assert torch.equal(one[2], match[int(po[p]):int(po[p + 1])]) and np.array_equal(one[7].cpu().numpy()[0], s[p])


# ---- rank positions over the three keypoint layouts and the three norms ------------------------------------------------------------------
RANK_SIZES = (64, 65, 256, 257, 513, 600)


@pytest.mark.parametrize("n", RANK_SIZES)
@pytest.mark.parametrize("sel", ["every2", "last8"])
@pytest.mark.parametrize("layout,kpts", [("F", False), ("H", False), ("H", True)], ids=["n2", "n6", "kpts4"])
def test_rank_positions(oracle_port, layout, kpts, sel, n):
    sc = vr.rank_scene(layout, sel, n); seed = vr.rank_seed(layout, sel, n)
    got, s, po = _batch_both([sc], [seed], kpts=kpts)
    assert s[0, 0] == len(sc["kept"][False]) >= 8 and s[0, 1] > 0 and s[0, 2] > 0
    if not kpts and sel == "last8":
        _vs_restatement(oracle_port, got, po, [sc], [seed])


def test_rank_scenes_cover_the_three_norms():
    assert {vr.rank_scene(m, sel, n)["norm"] for m in ("F", "H") for sel in ("every2", "last8") for n in RANK_SIZES} == set(vr.NORMS)


# ---- different parameters for the two models in one call ----------------------------------------------------------------------------------
def test_each_side_takes_its_own_parameters():
    scs = tv.alternating_scenes("F")
    fp = dict(px_th=0.75, error_type="symm_epipolar", max_iters=2000, enable_degeneracy_check=False)
    hp = dict(px_th=1.5, error_type="sampson", max_iters=1500, conf=0.99)
    got, s, _ = _batch_both(scs, tv.ALTERNATING_SEEDS, fp=fp, hp=hp)
    base, s0, _ = _batch_both(scs, tv.ALTERNATING_SEEDS)
    assert not np.array_equal(s, s0)                     # ... and the parameters matter


# ---- FGINN --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", vr.NORMS)
def test_fginn_radius_changes_a_stated_kept_set(norm):
    """fginn_ref.twin_scene: query i is a noisy copy of train row i, and the first 7 train rows have a twin 1.5 px away with a near-equal
    descriptor.  Plain rule (fginn_th None, and radius 0): queries 0 .. 6 fail the ratio test against the twin, the kept set is 7 .. 39.
    Radius 10: the twin no longer competes, the kept set is 0 .. 39."""
    a, b, kp2 = fr.twin_scene(31, 40, 60, 33 if norm == "l2" else 36, norm, 7)
    g = np.arange(40)
    kp1 = np.c_[100.0 * (g % 7), 100.0 * (g // 7)]
    sc = dict(k1=kp1, k2=np.ascontiguousarray(kp2[:, :2], np.float64), d1=a, d2=b, n1=40, n2=60, ratio=0.9, norm=norm)
    for th, kept in ((None, np.arange(7, 40)), (0, np.arange(7, 40)), (R, np.arange(40))):
        got, s, _ = _batch_both([sc], [5], fginn_th=th)
        assert np.array_equal(np.flatnonzero(got[2].cpu().numpy() >= 0), kept), th
        assert s[0, 0] == len(kept)


# ---- pair lists -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _collection(layout):
    """tests/test_gpu_fginn_pairs._collection (three views of one scene and a 3-row image, every third keypoint twinned), with two empty
    images behind them: image 5 is used by no list"""
    from tests.test_gpu_fginn_pairs import _collection as base
    xy, k6, desc, counts = base(layout)
    return xy, k6, desc, list(counts) + [0, 0]


# last image first; the 3-row image (short: neither model); a repeat of (1, 0) under two seeds; both orders; a self pair; an empty image on
# either side
LIST = [(4, 0), (3, 0), (2, 1), (1, 0), (1, 2), (1, 0), (0, 1), (0, 0), (0, 4)]
LIST_SEEDS = [1, 9, 11, 4000000000, 3, 77, 7, 123456, 2]
LP = dict(F=dict(max_iters=2000), H=dict(max_iters=2000))


def _pairs_both(k1, k2, d1, d2, c1, c2, pairs, seeds, fginn_th=None, mutual=False, fp=LP["F"], hp=LP["H"], norm=None):
    tk, td = _t(k1), _t(d1)
    args = (tk, tk if k2 is k1 else _t(k2), td, td if d2 is d1 else _t(d2), c1, c2, pairs)          # one store: the same tensors on both sides
    kw = dict(mutual=mutual, seeds=seeds, norm=norm)
    got = tensor_api.match_and_verify_fh_pairs_tensors(*args, fginn_th=fginn_th, f_params=fp, h_params=hp, **kw)
    if fginn_th is None:
        wf = tensor_api.match_and_verify_pairs_tensors(*args, model="F", **fp, **kw)
        wh = tensor_api.match_and_verify_pairs_tensors(*args, model="H", **hp, **kw)
    else:
        wf = tensor_api.match_and_verify_fginn_pairs_tensors(*args, fginn_th, model="F", **fp, **kw)
        wh = tensor_api.match_and_verify_fginn_pairs_tensors(*args, fginn_th, model="H", **hp, **kw)
    assert np.array_equal(got[9], wf[5]) and got[9].dtype == np.int64
    return got, _same(got, wf, wh, got[9]), args


@pytest.mark.parametrize("fginn_th", [None, 0, R])
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("layout", ["F", "H"])
def test_pair_list(layout, mutual, fginn_th):
    import torch
    xy, k6, desc, counts = _collection(layout)
    kps = xy if layout == "F" else k6
    got, s, _ = _pairs_both(kps, kps, desc, desc, counts, counts, LIST, LIST_SEEDS, fginn_th, mutual)
    po = got[9]
    assert list(np.diff(po)) == [counts[i] for i, _ in LIST]
    assert (s[[0, 1, 8]] == [[0, 0, 0, 0], [s[1, 0], 0, 0, 0], [0, 0, 0, 0]]).all() and s[1, 0] < 4          # empty, short, no train rows
    assert (s[[2, 3, 4, 5, 6], 1] >= 8).all() and (s[[2, 3, 4, 5, 6], 0] > 20).all()
    match = got[2].cpu().numpy()
    assert np.array_equal(match[po[3]:po[4]], match[po[5]:po[6]])                                           # the repeat: the same tentatives,
    assert not torch.equal(got[5][3, DET], got[5][5, DET])                                                  # ... another seed, another run
    if fginn_th == R:
        plain, sp, _ = _pairs_both(kps, kps, desc, desc, counts, counts, LIST, LIST_SEEDS, None, mutual)
        assert (s[[2, 3, 4, 6], 0] > sp[[2, 3, 4, 6], 0] + 10).all()                                        # the rule changes the tentatives


def test_two_stores_and_the_numpy_entry_points():
    xy, k6, desc, counts = _collection("F")
    o = pr.offsets(counts)
    kl = [xy[o[i]:o[i + 1]] for i in range(len(counts))]; dl = [desc[o[i]:o[i + 1]] for i in range(len(counts))]
    pairs2 = [(0, 0), (2, 1), (3, 0), (1, 1), (4, 1)]; seeds2 = LIST_SEEDS[:5]
    cases = [(dict(), (xy, xy, desc, desc, counts, counts), LIST, LIST_SEEDS),
             (dict(kps2_list=kl[1:3], desc2_list=dl[1:3]), (xy, xy[o[1]:o[3]], desc, desc[o[1]:o[3]], counts, counts[1:3]), pairs2, seeds2)]
    for second, stores, pairs, seeds in cases:
        for th in (None, R):
            got, s, _ = _pairs_both(*stores, pairs, seeds, th, True)
            F, H, match, inf, inh, stf, sth = (x.cpu().numpy() for x in got[:7]); po = got[9]
            Fh, Hh, mh, ifh, ihh, sh = matcher.match_and_verify_fh_pairs(kl, dl, pairs, mutual=True, fginn_th=th, seeds=seeds, f_params=LP["F"],
                                                                         h_params=LP["H"], **second)
            last = pd.last_stats()
            assert np.array_equal(F, Fh) and _h_close(H, Hh) and np.array_equal(s, sh) and sh.dtype == np.int32
            for p in range(len(pairs)):
                rows = slice(int(po[p]), int(po[p + 1]))
                assert np.array_equal(match[rows], mh[p]) and np.array_equal(inf[rows], ifh[p]) and np.array_equal(inh[rows], ihh[p]), p
                assert [last[p][k] for k in ("samples", "lo_runs", "I")] == list(stf[p, CTR]) and last[p]["tentatives"] == got[8][p], p
                assert [last[p]["homography"][k] for k in ("samples", "lo_runs", "I")] == list(sth[p, CTR]), p
    # the ragged numpy form on the expansion of the first list
    (ek, ed), (ek2, ed2), c1, c2, po = pr.expand((xy, desc), counts, (xy, desc), counts, LIST)
    o1, o2 = pr.offsets(c1), pr.offsets(c2)
    cut = lambda a, oo: [a[oo[p]:oo[p + 1]] for p in range(len(oo) - 1)]          # noqa: E731
    got, s, _ = _pairs_both(xy, xy, desc, desc, counts, counts, LIST, LIST_SEEDS, R, False)
    Fb, Hb, mb, ifb, ihb, sb = matcher.match_and_verify_fh_batch(cut(ek, o1), cut(ek2, o2), cut(ed, o1), cut(ed2, o2), fginn_th=R, seeds=LIST_SEEDS,
                                                                 f_params=LP["F"], h_params=LP["H"])
    assert np.array_equal(got[0].cpu().numpy(), Fb) and _h_close(got[1].cpu().numpy(), Hb) and np.array_equal(s, sb)
    assert np.array_equal(got[3].cpu().numpy(), np.concatenate(ifb)) and np.array_equal(got[4].cpu().numpy(), np.concatenate(ihb))
    assert np.array_equal(got[2].cpu().numpy(), np.concatenate(mb))


def test_batch_form_equals_the_pair_list_on_its_expansion():
    import torch
    xy, k6, desc, counts = _collection("H")
    got, s, _ = _pairs_both(k6, k6, desc, desc, counts, counts, LIST, LIST_SEEDS, R, True)
    (ek, ed), (ek2, ed2), c1, c2, po = pr.expand((k6, desc), counts, (k6, desc), counts, LIST)
    exp = tensor_api.match_and_verify_fh_batch_tensors(_t(ek), _t(ek2), _t(ed), _t(ed2), c1, c2, mutual=True, fginn_th=R, seeds=LIST_SEEDS,
                                                       f_params=LP["F"], h_params=LP["H"])
    torch.cuda.synchronize()
    for a, b in zip(got[:8], exp[:8]):
        assert torch.equal(a[:, DET], b[:, DET]) if a.shape[1:] == (16,) else torch.equal(a, b)
    assert np.array_equal(got[8], exp[8])


# ---- first offsets above zero through the C entry points -----------------------------------------------------------------------------------
def _framed(x, front, back, rng):
    junk = lambda n: rng.integers(0, 5, (n,) + x.shape[1:]).astype(x.dtype)          # noqa: E731
    return _t(np.concatenate([junk(front), x, junk(back)]))


def _c_outputs(K, n):
    import torch
    dev = _dev()
    return dict(F=torch.zeros((K, 9), dtype=torch.float64, device=dev), H=torch.zeros((K, 9), dtype=torch.float64, device=dev),
                match=torch.full((n,), -7, dtype=torch.int32, device=dev), inf=torch.full((n,), 7, dtype=torch.uint8, device=dev),
                inh=torch.full((n,), 7, dtype=torch.uint8, device=dev), stf=torch.zeros((K, 16), dtype=torch.int32, device=dev),
                sth=torch.zeros((K, 16), dtype=torch.int32, device=dev), summ=torch.full((K, 4), -7, dtype=torch.int32, device=dev))


def _c_tail(o, seeds, cnt):
    import torch
    return (seeds.data_ptr(), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream), o["F"].data_ptr(), o["H"].data_ptr(), o["match"].data_ptr(),
            o["inf"].data_ptr(), o["inh"].data_ptr(), o["stf"].data_ptr(), o["sth"].data_ptr(), o["summ"].data_ptr(), cnt.ctypes.data_as(C.POINTER(C.c_int32)))


def _c_check(o, cnt, want, own):
    """the C call's raw outputs against the tensor call `want` on the unframed rows; rows outside `own` untouched"""
    import torch
    torch.cuda.synchronize()
    K = len(cnt)
    assert torch.equal(_bits(o["F"].view(K, 3, 3)), _bits(want[0])) and torch.equal(_bits(tensor_api._h_user_form(o["H"].view(K, 3, 3))), _bits(want[1]))
    assert torch.equal(o["match"][own], want[2]) and torch.equal(o["inf"][own].bool(), want[3]) and torch.equal(o["inh"][own].bool(), want[4])
    assert torch.equal(o["stf"][:, DET], want[5][:, DET]) and torch.equal(o["sth"][:, DET], want[6][:, DET])
    assert torch.equal(o["summ"], want[7]) and np.array_equal(cnt, want[8])
    for k, fill in (("match", -7), ("inf", 7), ("inh", 7)):
        assert (o[k][:own.start] == fill).all() and (o[k][own.stop:] == fill).all(), k


def test_c_batch_entry_whose_first_offsets_are_above_zero():
    scs = tv.alternating_scenes("F"); K = len(scs); seeds = tv.ALTERNATING_SEEDS
    want, _, po = _batch_both(scs, seeds, mutual=True)
    rng = np.random.default_rng(43)
    cat = lambda k: np.concatenate([s[k] for s in scs])          # noqa: E731
    a, k1 = _framed(cat("d1"), 5, 3, rng), _framed(cat("k1"), 5, 3, rng); b, k2 = _framed(cat("d2"), 12, 2, rng), _framed(cat("k2"), 12, 2, rng)
    o1 = po + 5; o2 = np.r_[0, np.cumsum([s["n2"] for s in scs])].astype(np.int64) + 12
    o = _c_outputs(K, a.shape[0]); cnt = np.zeros(K, np.int32)
    d_seeds = _t(np.asarray(seeds, np.uint32).view(np.int32))
    mp = _lib.MatchParams(0, vr.DIM, 0.9, True); pf = matcher.estimator_params("F", **FP); ph = matcher.estimator_params("H", **HP)
    lp = C.POINTER(C.c_int64)
    rc = _lib.lib().mi_degensac_match_verify_fh_batch_dev(C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), o2.ctypes.data_as(lp),
                                                          k1.data_ptr(), k2.data_ptr(), 2, K, C.byref(pf), C.byref(ph), *_c_tail(o, d_seeds, cnt))
    assert rc == 0, _lib.lib().mi_degensac_last_error()
    _c_check(o, cnt, want, slice(int(o1[0]), int(o1[-1])))


def test_c_pair_list_entry_on_stores_whose_first_offsets_are_above_zero():
    xy, k6, desc, counts = _collection("F"); K = len(LIST)
    want, _, _ = _pairs_both(xy, xy, desc, desc, counts, counts, LIST, LIST_SEEDS, R, True)
    rng = np.random.default_rng(44)
    a, k1 = _framed(desc, 6, 3, rng), _framed(xy, 6, 3, rng); b, k2 = _framed(desc, 11, 2, rng), _framed(xy, 11, 2, rng)
    o1 = pr.offsets(counts).astype(np.int64) + 6; o2 = pr.offsets(counts).astype(np.int64) + 11
    n = int(want[9][-1])
    o = _c_outputs(K, n + 4); cnt = np.zeros(K, np.int32)          # four spare rows behind the list's output rows
    d_seeds = _t(np.asarray(LIST_SEEDS, np.uint32).view(np.int32)); prs = np.ascontiguousarray(LIST, np.int32)
    mp = _lib.MatchParams(0, desc.shape[1], 0.9, True, R); pf = matcher.estimator_params("F", **LP["F"]); ph = matcher.estimator_params("H", **LP["H"])
    lp = C.POINTER(C.c_int64); M = len(counts)
    rc = _lib.lib().mi_degensac_match_verify_fh_pairs_dev(C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), M, o2.ctypes.data_as(lp), M,
                                                          k1.data_ptr(), k2.data_ptr(), 2, prs.ctypes.data_as(C.POINTER(C.c_int32)), K, C.byref(pf),
                                                          C.byref(ph), *_c_tail(o, d_seeds, cnt))
    assert rc == 0, _lib.lib().mi_degensac_last_error()
    _c_check(o, cnt, want, slice(0, n))


# ---- the host-pointer form with and without its optional outputs ---------------------------------------------------------------------------
def test_pair_list_host_form_with_and_without_its_optional_outputs():
    """mi_degensac_match_verify_fh_pairs on the stores of tests/test_gpu_match_verify._fold_stores (first offsets above zero; one entry
    short for both models, one that only H can take): F / H / match / inlier_f / inlier_h are the same bytes with stats_f, stats_h,
    summary and counts given, with all four NULL, and with the store passed as two distinct equal copies (both sides uploaded), and they
    are the bytes of the _dev form"""
    import torch
    from tests.test_gpu_match_verify import FOLD_COUNTS, FOLD_LIST, FOLD_RATIO, FOLD_SEEDS, _fold_pairs_host, _fold_scene
    xy, desc = _fold_scene(); K = len(FOLD_LIST)
    tk, td = _t(xy), _t(desc)
    want = tensor_api.match_and_verify_fh_pairs_tensors(tk, tk, td, td, FOLD_COUNTS, FOLD_COUNTS, FOLD_LIST, ratio=FOLD_RATIO, mutual=True,
                                                        seeds=FOLD_SEEDS, f_params=LP["F"], h_params=LP["H"])
    torch.cuda.synchronize()
    cnt = want[8]; n = int(want[9][-1])
    assert list(cnt) == [30, 1, 7, 30] and n == 41 + 40 + 41 + 39
    assert list(want[5][:, 0].cpu().numpy() > 0) == [True, False, False, True] and list(want[6][:, 0].cpu().numpy() > 0) == [True, False, True, True]
    prms = [matcher.estimator_params("F", **LP["F"]), matcher.estimator_params("H", **LP["H"])]
    first = None
    for optional, second in ((True, False), (False, False), (True, True)):
        req = [np.zeros((K, 9)), np.zeros((K, 9)), np.full(n, -7, np.int32), np.full(n, 7, np.uint8), np.full(n, 7, np.uint8)]
        opt = [np.zeros((K, 16), np.int32), np.zeros((K, 16), np.int32), np.full((K, 4), -7, np.int32), np.zeros(K, np.int32)] if optional else [None] * 4
        _fold_pairs_host(_lib.lib().mi_degensac_match_verify_fh_pairs, (), prms, req, opt, second)
        if first is None:
            first = req
            assert torch.equal(_bits(_t(req[0]).view(K, 3, 3)), _bits(want[0]))
            assert torch.equal(_bits(tensor_api._h_user_form(_t(req[1]).view(K, 3, 3))), _bits(want[1]))
            assert np.array_equal(req[2], want[2].cpu().numpy()) and max(req[3].max(), req[4].max()) <= 1
            assert np.array_equal(req[3].astype(bool), want[3].cpu().numpy()) and np.array_equal(req[4].astype(bool), want[4].cpu().numpy())
        for a, b in zip(first, req):
            assert a.tobytes() == b.tobytes(), (optional, second)
        if optional:
            assert np.array_equal(opt[0][:, DET], want[5].cpu().numpy()[:, DET]) and np.array_equal(opt[1][:, DET], want[6].cpu().numpy()[:, DET]), second
            assert np.array_equal(opt[2], want[7].cpu().numpy()) and np.array_equal(opt[3], cnt), second


# ---- a second stream ------------------------------------------------------------------------------------------------------------------------
def test_second_stream_gives_the_same_bits():
    import torch
    xy, k6, desc, counts = _collection("F")
    want, _, args = _pairs_both(xy, xy, desc, desc, counts, counts, LIST, LIST_SEEDS, R, True)
    s = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(s):
        got = tensor_api.match_and_verify_fh_pairs_tensors(*args, mutual=True, seeds=LIST_SEEDS, fginn_th=R, f_params=LP["F"], h_params=LP["H"])
    assert np.array_equal(got[8], want[8])                                                            # host values, before any wait here
    s.synchronize()
    for a, b in zip(got[:8], want[:8]):
        assert torch.equal(a[:, DET], b[:, DET]) if a.shape[1:] == (16,) else torch.equal(a, b)


# ---- end to end: one planar pair, one general pair ------------------------------------------------------------------------------------------
def test_end_to_end_planar_and_general_pair():
    """the expectation (classes 2 and 1, and the counts themselves) comes from the CPU restatement: tests/test_two_view_cpu.py"""
    kps, desc, pairs = tv.e2e_scene()
    counts = [len(d) for d in desc]
    got = tensor_api.match_and_verify_fh_pairs_tensors(_t(np.concatenate(kps)), _t(np.concatenate(kps)), _t(np.concatenate(desc)), _t(np.concatenate(desc)),
                                                       counts, counts, pairs, seeds=tv.E2E_EST_SEEDS, f_params=tv.E2E_PARAMS["F"], h_params=tv.E2E_PARAMS["H"])
    s = got[7].cpu().numpy()
    assert [tuple(r[1:3]) for r in s] == list(tv.E2E_NF_NH) and (s[:, 0] == tv.E2E_N).all()
    assert list(matcher.two_view_config(got[7])) == [2, 1] and list(matcher.two_view_config(s)) == [2, 1]
    Fh, Hh, mh, ifh, ihh, sh = matcher.match_and_verify_fh_pairs(kps, desc, pairs, seeds=tv.E2E_EST_SEEDS, f_params=tv.E2E_PARAMS["F"],
                                                                 h_params=tv.E2E_PARAMS["H"])
    assert np.array_equal(sh, s)


# ---- the chain into guided matching -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual", [False, True])
def test_chain_into_guided_matching(mutual):
    """F and H of the new pair-list call go into guided_match_pairs_tensors as they are: bit for bit what the models of the existing calls give"""
    import torch
    xy, k6, desc, counts = _collection("F")
    got, _, args = _pairs_both(xy, xy, desc, desc, counts, counts, LIST, LIST_SEEDS, R, mutual)
    kw = dict(mutual=mutual, seeds=LIST_SEEDS)
    for model, M in (("F", got[0]), ("H", got[1])):
        old = tensor_api.match_and_verify_fginn_pairs_tensors(*args, R, model=model, **LP[model], **kw)
        g_new = tensor_api.guided_match_pairs_tensors(*args, M, model=model, mutual=mutual)
        g_old = tensor_api.guided_match_pairs_tensors(*args, old[0], model=model, mutual=mutual)
        torch.cuda.synchronize()
        assert torch.equal(g_new[0], g_old[0]) and torch.equal(g_new[1], g_old[1]) and torch.equal(g_new[2].view(torch.int32), g_old[2].view(torch.int32))
        assert np.array_equal(g_new[3], g_old[3]) and int((g_new[0] >= 0).sum()) >= 100, model
