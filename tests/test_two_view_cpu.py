"""Match once, verify F and H, without a device (include/mi_degensac.h mi_degensac_match_verify_fh_*, tensor_api.match_and_verify_fh_*_tensors,
matcher.match_and_verify_fh_*, matcher.two_view_config): every EINVAL of the four C entry points, with a message and before a device is
looked for; the ValueErrors / TypeErrors of the Python calls; two_view_config on a hand-written table; that the numpy restatement of the
summary (tests/two_view_ref.summary_ref) notices a mask shifted across a pair boundary and swapped masks; and the expectation of the
end-to-end scene of tests/test_gpu_two_view.py, from the CPU restatement alone."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import two_view_ref as tv

EINVAL = -1
ENTRIES = ("batch_dev", "batch", "pairs_dev", "pairs")


def _abi(mp=None, kp_dim=2, off1=(0, 4, 10), off2=(0, 3, 7), pairs=((0, 1), (1, 0)), n_pairs=None, prm_f=None, prm_h=None, null=None, ptrs=True, entries=ENTRIES):
    """rc and message of the four entry points on the same arguments.  The batch forms take off1 / off2 as per-pair offsets, the pair-list
    forms as store offsets with `pairs`.  ptrs: every data pointer holds an address (never read by a call that is refused), but the one
    named by `null`; ptrs=False: all are NULL.  entries: the forms to call (a form that would pass every check is left out by its test)."""
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64); pr_ = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    mp = mp or _lib.MatchParams(0, 8, 0.9, True)
    prm_f = prm_f or matcher.estimator_params("F"); prm_h = prm_h or matcher.estimator_params("H")
    buf = np.zeros(64); names = ("desc1", "desc2", "kp1", "kp2", "seeds", "model_f", "model_h", "match", "inlier_f", "inlier_h", "summary")
    P = {k: (buf.ctypes.data if ptrs and k != null else None) for k in names}

    def c(k, t):
        return C.cast(P[k], C.POINTER(t)) if P[k] is not None else None
    out = {}
    for e in entries:
        f = getattr(L, "mi_degensac_match_verify_fh_" + e); dev = e.endswith("_dev")
        if e.startswith("batch"):
            K = min(len(o1), len(o2)) - 1 if n_pairs is None else n_pairs
            layout = (o1.ctypes.data_as(lp), o2.ctypes.data_as(lp))
            tail = (kp_dim, K)
        else:
            K = len(pr_) if n_pairs is None else n_pairs
            layout = (o1.ctypes.data_as(lp), len(o1) - 1, o2.ctypes.data_as(lp), len(o2) - 1)
            tail = (kp_dim, pr_.ctypes.data_as(ip), K)
        if dev:
            rc = f(C.byref(mp), P["desc1"], P["desc2"], *layout, P["kp1"], P["kp2"], *tail, C.byref(prm_f), C.byref(prm_h), P["seeds"], 0, None,
                   P["model_f"], P["model_h"], P["match"], P["inlier_f"], P["inlier_h"], None, None, P["summary"], None)
        else:
            rc = f(C.byref(mp), P["desc1"], P["desc2"], *layout, c("kp1", C.c_double), c("kp2", C.c_double), *tail, C.byref(prm_f), C.byref(prm_h),
                   c("seeds", C.c_uint32), 0, c("model_f", C.c_double), c("model_h", C.c_double), c("match", C.c_int32), c("inlier_f", C.c_uint8),
                   c("inlier_h", C.c_uint8), None, None, c("summary", C.c_int32), None)
        out[e] = (rc, L.mi_degensac_last_error())
    return out


def _all_refuse(res, word=None, entries=ENTRIES):
    for e in entries:
        rc, msg = res[e]
        assert rc == EINVAL and msg, (e, rc, msg)
        if word is not None:
            assert word in msg, (e, msg)


# ---- the C-ABI: refusals before a device is looked for (no device exists where these tests run) ----
def test_the_symbols_exist():
    for e in ENTRIES:
        assert hasattr(_lib.lib(), "mi_degensac_match_verify_fh_" + e)


@pytest.mark.parametrize("mp", [_lib.MatchParams(2, 8, 0.9, False), _lib.MatchParams(3, 8, 0.9, False), _lib.MatchParams(0, 0, 0.9, False),
                                _lib.MatchParams(0, -8, 0.9, False), _lib.MatchParams(1, 6, 0.9, False), _lib.MatchParams(4, 6, 0.9, False),
                                _lib.MatchParams(4, 260, 0.9, False)], ids=lambda m: f"norm{m.norm}-dim{m.dim}")
def test_abi_refuses_bad_norms_and_dims(mp):
    _all_refuse(_abi(mp=mp))
    _all_refuse(_abi(mp=mp, n_pairs=0))


@pytest.mark.parametrize("kp_dim", [0, 1, 3, 4, 5, 7, -2])
def test_abi_refuses_keypoint_rows_that_are_not_2_or_6_wide(kp_dim):
    _all_refuse(_abi(kp_dim=kp_dim), b"keypoint")


@pytest.mark.parametrize("case", [dict(off1=(0, 6, 4)), dict(off2=(0, 8, 7)), dict(off1=(-2, 4, 10)), dict(off2=(-1, 3, 7))], ids=repr)
def test_abi_refuses_bad_offsets(case):
    _all_refuse(_abi(**case), b"offsets")


@pytest.mark.parametrize("pairs", [[(0, 2)], [(2, 0)], [(0, 1), (-1, 0)], [(0, -1)]], ids=repr)
def test_abi_refuses_a_pair_index_outside_its_store(pairs):
    _all_refuse(_abi(pairs=pairs, entries=("pairs_dev", "pairs")), b"image index", ("pairs_dev", "pairs"))


def test_abi_refuses_a_bad_ratio_and_second_nn():
    for r in (0.0, -1.0, float("nan"), float("inf")):
        _all_refuse(_abi(mp=_lib.MatchParams(0, 8, r, False)), b"ratio")
    mp = _lib.MatchParams(0, 8, 0.9, False, 5.0); mp.second_nn = 2
    _all_refuse(_abi(mp=mp), b"second_nn")
    _all_refuse(_abi(mp=None, n_pairs=-1))


@pytest.mark.parametrize("th", [-1.0, -1e-300, float("nan"), float("inf"), -float("inf")])
def test_abi_refuses_a_bad_radius_when_struct_size_covers_it(th):
    _all_refuse(_abi(mp=_lib.MatchParams(0, 8, 0.9, False, th)), b"spatial_th")
    _all_refuse(_abi(mp=_lib.MatchParams(0, 8, 0.9, False, th), n_pairs=0), b"spatial_th")


def test_abi_a_struct_size_that_does_not_cover_spatial_th_means_the_plain_rule():
    """no error of its own: the call gets as far as the NULL check, and the pair-list forms take second_nn = 1 (no FGINN twin)"""
    for size in (0, 24):
        mp = _lib.MatchParams(0, 8, 0.9, False, None)
        mp.spatial_th = float("nan"); mp.struct_size = size; mp.second_nn = 1
        _all_refuse(_abi(mp=mp, ptrs=False), b"NULL")
        assert all(rc == 0 for rc, _ in _abi(mp=mp, n_pairs=0).values())
    _all_refuse(_abi(mp=_lib.MatchParams(0, 8, 0.9, False, 5.0), ptrs=False), b"NULL")          # FGINN is accepted by every form


def test_abi_checks_each_parameter_block_for_its_own_model():
    bad_f = matcher.estimator_params("F"); bad_f.error_type = 2                # fine for H, not for F
    _all_refuse(_abi(prm_f=bad_f), b"fundamental")
    bad_h = matcher.estimator_params("H"); bad_h.error_type = 5
    _all_refuse(_abi(prm_h=bad_h), b"homography")
    ok_h = matcher.estimator_params("H"); ok_h.error_type = 4                  # the same block is refused as F, taken as H
    _all_refuse(_abi(prm_f=ok_h), b"fundamental")
    legacy = matcher.estimator_params("F"); legacy.flags = _lib.FLAG_LEGACY_F  # an F-only flag in the H block
    _all_refuse(_abi(prm_h=legacy), b"LEGACY")
    _all_refuse(_abi(prm_f=bad_f, prm_h=bad_h, ptrs=False))


def test_abi_null_data_with_rows_present_is_refused_not_read():
    _all_refuse(_abi(ptrs=False), b"NULL")
    for name in ("desc1", "desc2", "kp1", "kp2", "seeds", "model_f", "model_h", "match", "inlier_f", "inlier_h"):
        _all_refuse(_abi(null=name), b"NULL")
    _all_refuse(_abi(null="summary", entries=("batch_dev", "pairs_dev")), b"NULL", ("batch_dev", "pairs_dev"))     # not nullable in the _dev forms


def test_abi_valid_arguments_get_as_far_as_the_device():
    """every check passed: what is left is the missing device (with one, the call would run: nothing to show here)"""
    if _lib.lib().mi_degensac_device_count() != 0:
        return
    for e in ("batch_dev", "pairs_dev"):
        rc, msg = _abi(entries=(e,))[e]
        assert rc == -2 and b"no HIP device" in msg, (e, rc, msg)


def test_abi_empty_list_returns_zero():
    assert all(rc == 0 for rc, _ in _abi(n_pairs=0).values())
    assert all(rc == 0 for rc, _ in _abi(n_pairs=0, ptrs=False, off1=(7, 3), off2=(-1,)).values())          # nothing is looked at


# ---- the Python calls ----
COUNTS = [5, 3, 0, 7, 4]
PAIRS = [(3, 1), (1, 3), (0, 0), (3, 1), (2, 0)]


def _lists(counts=COUNTS, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 100, (n, 2)) for n in counts], [rng.normal(size=(n, 8)).astype(np.float32) for n in counts]


def test_params_dicts():
    pf, ph = matcher.two_view_params()
    df, dh = matcher.estimator_params("F"), matcher.estimator_params("H")
    assert bytes(pf) == bytes(df) and bytes(ph) == bytes(dh)                   # missing keys: the two calls' defaults
    pf, ph = matcher.two_view_params(dict(px_th=0.75, error_type="symm_epipolar", enable_degeneracy_check=False), dict(px_th=3.0, error_type="symm_sum"))
    assert (pf.px_th, pf.error_type, pf.enable_degeneracy_check, pf.max_iters) == (0.75, 1, 0, df.max_iters)
    assert (ph.px_th, ph.error_type, ph.conf) == (3.0, 4, dh.conf)
    for kw in (dict(f_params=dict(px=1.0)), dict(h_params=dict(enable_degeneracy_check=False)), dict(h_params=dict(model="H")),
               dict(f_params=dict(guided=True))):
        with pytest.raises(ValueError, match="unknown key"):
            matcher.two_view_params(**kw)
    with pytest.raises(ValueError, match="dict"):
        matcher.two_view_params(f_params=[("px_th", 1.0)])
    with pytest.raises(ValueError):
        matcher.two_view_params(h_params=dict(error_type="nope"))


def test_numpy_calls_check_before_the_device():
    kl, dl = _lists()
    for kw in (dict(f_params=dict(bogus=1)), dict(h_params=dict(bogus=1))):
        with pytest.raises(ValueError, match="unknown key"):
            matcher.match_and_verify_fh_pairs(kl, dl, PAIRS, **kw)
        with pytest.raises(ValueError, match="unknown key"):
            matcher.match_and_verify_fh_batch(kl, kl, dl, dl, **kw)
    with pytest.raises(TypeError):
        matcher.match_and_verify_fh_pairs(kl, dl, PAIRS, guided=True)
    with pytest.raises(TypeError):
        matcher.match_and_verify_fh_batch(kl, kl, dl, dl, guided=True)
    with pytest.raises(ValueError, match="image index"):
        matcher.match_and_verify_fh_pairs(kl, dl, [(0, 5)])
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.match_and_verify_fh_pairs(kl, dl, PAIRS, fginn_th=-1.0)
    with pytest.raises(ValueError, match="fginn_th"):
        matcher.match_and_verify_fh_batch(kl, kl, dl, dl, fginn_th=float("nan"))
    with pytest.raises(ValueError, match="seed"):
        matcher.match_and_verify_fh_pairs(kl, dl, PAIRS, seeds=[1, 2])
    with pytest.raises(ValueError, match="ratio"):
        matcher.match_and_verify_fh_pairs(kl, dl, PAIRS, ratio=0.0)


def test_tensor_calls_check_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    d = torch.zeros((19, 8)); k = torch.zeros((19, 2), dtype=torch.float64)
    fb, fp = tensor_api.match_and_verify_fh_batch_tensors, tensor_api.match_and_verify_fh_pairs_tensors
    for call in (lambda **kw: fb(k, k, d, d, COUNTS, COUNTS, **kw), lambda **kw: fp(k, k, d, d, COUNTS, COUNTS, PAIRS, **kw)):
        with pytest.raises(ValueError, match="unknown key"):
            call(f_params=dict(bogus=1))
        with pytest.raises(ValueError, match="unknown key"):
            call(h_params=dict(enable_degeneracy_check=True))
        with pytest.raises(TypeError):
            call(guided=True)
        with pytest.raises(TypeError):
            call(model="F")
        with pytest.raises(ValueError, match="fginn_th"):
            call(fginn_th=-2.0)
        with pytest.raises(ValueError, match="seed"):
            call(seeds=[1])
        with pytest.raises(ValueError):                                        # valid arguments, but not on a ROCm device
            call()
    with pytest.raises(ValueError, match="tensors"):
        fb(k.numpy(), k, d, d, COUNTS, COUNTS)
    with pytest.raises(ValueError, match="tensors"):
        fp(k, k, d.numpy(), d, COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="same ROCm device"):
        fb(k, k.to("meta"), d, d, COUNTS, COUNTS)
    with pytest.raises(ValueError, match="same ROCm device"):
        fp(k, k, d, d.to("meta"), COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="image index"):
        fp(k, k, d, d, COUNTS, COUNTS, [(0, 5)])
    for f in (fb, fp):
        assert "guided_match_pairs_tensors" in f.__doc__ and "guided_match_batch_tensors" in f.__doc__
    for f in (matcher.match_and_verify_fh_batch, matcher.match_and_verify_fh_pairs):
        assert "guided_match" in f.__doc__


# ---- two_view_config ----
def test_two_view_config_table():
    #            tent  nF   nH  nFH
    table = [((40, 14, 14, 14), 0),          # rejected: max(nF, nH) = 14 < 15 (although nH > 0.8 nF)
             ((40, 15, 3, 3), 1),            # general, at the inlier minimum
             ((40, 3, 15, 3), 2),            # H alone reaches the minimum
             ((90, 20, 16, 16), 1),          # the boundary nH == 0.8 nF: strict, not planar
             ((90, 20, 17, 16), 2),          # one above it
             ((90, 100, 80, 80), 1),         # the boundary again, 0.8 * 100 == 80.0 in float64
             ((90, 100, 81, 80), 2),
             ((30, 0, 15, 0), 2),            # nF == 0 (4 .. 7 tentatives cannot be, but a failed F can): H with enough inliers
             ((6, 0, 6, 0), 0),              # an H-only pair below the minimum
             ((0, 0, 0, 0), 0)]
    s = np.array([row for row, _ in table], np.int32); want = np.array([c for _, c in table], np.int8)
    got = matcher.two_view_config(s)
    assert got.dtype == np.int8 and got.shape == (len(table),) and np.array_equal(got, want), got
    assert np.float64(0.8) * 20.0 == 16.0 and np.float64(0.8) * 100.0 == 80.0          # the boundary rows sit ON the boundary
    assert np.array_equal(matcher.two_view_config(s, min_inliers=4), [2, 1, 2, 1, 2, 1, 2, 2, 2, 0])
    assert np.array_equal(matcher.two_view_config(s, max_h_ratio=0.5)[:5], [0, 1, 2, 2, 2])
    assert matcher.two_view_config(np.zeros((0, 4), np.int32)).shape == (0,)
    torch = pytest.importorskip("torch")
    assert np.array_equal(matcher.two_view_config(torch.from_numpy(s)), want)
    for bad in (np.zeros((3, 3), np.int32), np.zeros(4, np.int32), np.zeros((2, 4))):
        with pytest.raises(ValueError, match="summary"):
            matcher.two_view_config(bad)
    assert "COLMAP" in matcher.two_view_config.__doc__ and "caller" in matcher.two_view_config.__doc__


# ---- the restatement of the summary has power ----
def test_summary_ref_on_designed_masks():
    po = np.array([0, 4, 4, 9, 12])
    match = np.array([3, -1, 0, 1,   2, 2, -1, 0, 4,   -1, -1, 5])
    f = np.array([1, 0, 0, 1,   1, 1, 0, 0, 0,   0, 0, 1], bool)
    h = np.array([1, 0, 1, 0,   0, 1, 0, 1, 1,   0, 0, 0], bool)
    want = np.array([[3, 2, 2, 1], [0, 0, 0, 0], [4, 2, 3, 1], [1, 1, 0, 0]], np.int32)
    got = tv.summary_ref(match, f, h, po)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # a mask shifted by one row across the pair boundaries changes it (row 3 of pair 0 lands in pair 2) ...
    assert not np.array_equal(tv.summary_ref(match, np.roll(f, 1), h, po), want)
    assert not np.array_equal(tv.summary_ref(match, f, np.roll(h, -1), po), want)
    # ... and so do swapped masks, and offsets moved by one row
    assert not np.array_equal(tv.summary_ref(match, h, f, po), want)
    assert np.array_equal(tv.summary_ref(match, h, f, po)[:, [0, 2, 1, 3]], want)
    assert not np.array_equal(tv.summary_ref(match, f, h, np.array([0, 3, 4, 9, 12])), want)


def test_alternating_arrangement_differs_between_the_halves():
    """for every pair behind the first, the eligible index or the row base of the pair differs between the two estimators"""
    scs = tv.alternating_scenes("F")
    cnt = np.array([len(s["kept"][False]) for s in scs])
    assert [("Q" if n == 0 else "5" if n == 5 else "E") for n in cnt] == list(tv.ALTERNATING) and (cnt[cnt > 5] >= 9).all()
    ef = np.cumsum(cnt >= 8) - 1; eh = np.cumsum(cnt >= 4) - 1
    bf = np.r_[0, np.cumsum(np.where(cnt >= 8, cnt, 0))][:-1]; bh = np.r_[0, np.cumsum(np.where(cnt >= 4, cnt, 0))][:-1]
    both = np.flatnonzero(cnt >= 8)
    assert len(both) == 5 and (ef[both] != eh[both]).all() and (bf[both] != bh[both]).all()
    assert len(set(tv.ALTERNATING_SEEDS)) == len(scs)


# ---- the end-to-end scene's expectation, from the CPU restatement alone ----
def test_end_to_end_scene_by_the_restatement(oracle_port):
    s = tv.e2e_ref(oracle_port)
    assert [tuple(r[1:3]) for r in s] == list(tv.E2E_NF_NH), s
    assert (s[:, 0] == tv.E2E_N).all()
    ratio = s[:, 2] / s[:, 1]
    assert not ((ratio > 0.72) & (ratio < 0.88)).any(), ratio                  # not within 10 % of the 0.8 boundary
    assert list(matcher.two_view_config(s)) == [2, 1]
