"""GPU: the F / H estimator kernels at the edges of their tiling and in coordinate frames other than the pixel frame, against the CPU
restatement (oracle/dg_oracle.c).  tests/estimator_shapes.py has the families; tests/test_estimator_shapes_cpu.py shows on the CPU
that they run several local optimisations, DEGENSAC's plane branch and the LAF check, and that every frame keeps its model.

Row counts E = 8, 63 ... 65, 255 ... 257, 511 ... 513, 1023 ... 1025, 2047 ... 2049: both sides of the wave tile of 256 points
(dg_score_tiles.h) and of the workgroup pass steps of 512 / 1024 / 2048 rows; cooperative slices of one row; the sampler's pool stage
at 4096 / 4097; the placement limits, found by bisection.  Tolerances are the project's: masks, residuals, J and counters bit for bit,
models to 1e-9 relative Frobenius; the screens' counts obey inequalities plus two exact cases.  No case is filtered at run time.
The drivers are called through findFundamentalMatrixBatch and through api._batch("H", ...), the call under findHomographyBatch,
which returns the raw model that the restatement returns (findHomographyBatch inverts it)."""
import ctypes as C

import numpy as np
import pytest

import pydegensac_amd as pd
from pydegensac_amd import _lib, api
from pydegensac_amd import synthetic as syn
from tests import estimator_shapes as es
from tests.test_gpu_variants import VARIANT, _check_against_oracle, tune

pytestmark = pytest.mark.gpu

U32 = C.POINTER(C.c_uint32)
VARIANTS = (512, 256, 128)
PLACEMENTS = (1, 2, 0)


def _u(p1, p2):
    """[n, 6] rows x1 y1 1 x2 y2 1 of the restatement's residual routines"""
    n = len(p1); u = np.ones((n, 6)); u[:, 0:2] = p1[:, :2]; u[:, 3:5] = p2[:, :2]
    return u


def _score(p1, p2, models, kind, th):
    """mi_degensac_score_models: (I, J, residuals [n_models, n])"""
    p1 = np.ascontiguousarray(p1[:, :2]); p2 = np.ascontiguousarray(p2[:, :2]); models = np.ascontiguousarray(models, dtype=np.float64)
    nm = len(models); n = len(p1); I = np.zeros(nm, np.uint32); J = np.zeros(nm); R = np.zeros((nm, n))
    _lib.check(_lib.lib().mi_degensac_score_models(_lib.dptr(p1), _lib.dptr(p2), n, 2, _lib.dptr(models), nm, kind, C.c_double(th), 0,
                                                   I.ctypes.data_as(U32), _lib.dptr(J), _lib.dptr(R)))
    return I, J, R


def _screen_f(p1, p2, models, kind, th):
    p1 = np.ascontiguousarray(p1[:, :2]); p2 = np.ascontiguousarray(p2[:, :2]); models = np.ascontiguousarray(models, dtype=np.float64)
    nm = len(models); c1 = np.zeros(nm, np.uint32); c2 = np.zeros(nm, np.uint32)
    _lib.check(_lib.lib().mi_degensac_screen_counts(_lib.dptr(p1), _lib.dptr(p2), len(p1), 2, _lib.dptr(models), nm, kind, C.c_double(th), 0,
                                                    c1.ctypes.data_as(U32), c2.ctypes.data_as(U32)))
    return c1, c2


def _screen_h(p1, p2, models, th):
    p1 = np.ascontiguousarray(p1[:, :2]); p2 = np.ascontiguousarray(p2[:, :2]); models = np.ascontiguousarray(models, dtype=np.float64)
    nm = len(models); n = len(p1); cnt = np.zeros(nm, np.uint32); cand = np.zeros((nm, n), np.uint8)
    _lib.check(_lib.lib().mi_degensac_screen_counts_h(_lib.dptr(p1), _lib.dptr(p2), n, 2, _lib.dptr(models), nm, C.c_double(th), 0,
                                                      cnt.ctypes.data_as(U32), cand.ctypes.data_as(C.POINTER(C.c_uint8))))
    return cnt, cand


def _f_models(Fgt, count, seed):
    """the ground truth, perturbed copies, random ones"""
    rng = np.random.default_rng(seed); f = np.asarray(Fgt, float).ravel(); out = [f]
    for k in range(1, count):
        out.append(f + rng.normal(scale=10.0 ** -(1 + k % 8), size=9) * np.abs(f).max() if k % 3 else rng.normal(size=9))
    return np.ascontiguousarray(np.array(out[:count]))


def _h_models(Hraw, count, seed):
    rng = np.random.default_rng(seed); h = np.asarray(Hraw, float).ravel(); out = [h]
    for k in range(1, count):
        out.append(h * (1 + 10.0 ** -(2 + k % 5) * rng.normal(size=9)) if k % 3 else rng.normal(size=9))
    return np.ascontiguousarray(np.array(out[:count]))


def _f_truth(n):
    return syn.two_view_fundamental(8, 0.5, 0.0, seed=0)[3]          # the generator's geometry does not depend on n or the seed


# ---- 1. unit entry points at the edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", es.E)
def test_score_models_bit_exact_at_tile_edges(oracle_port, n):
    """kinds 0, 1 on the F scene and 10 ... 14 on the H scene of n rows: residuals bit for bit, I equal, J bit for bit (NaN = NaN)"""
    P = oracle_port.lib(); dp = oracle_port.dp; ip = oracle_port.ip
    f1, f2, _ = es.f_scene(n); h1, h2, _ = es.h_scene(n)
    Fm = _f_models(_f_truth(n), 10, n); Hm = _h_models(np.linalg.inv(syn.H_1_6).T, 10, n)
    for kind, th in [(0, 0.25), (1, 0.25), (10, 1.0), (11, 1.0), (12, 1.0), (13, 1.0), (14, 1.0)]:
        a, b, models = (f1, f2, Fm) if kind < 10 else (h1, h2, Hm)
        I, J, R = _score(a, b, models, kind, th); u = _u(a, b)
        for k in range(len(models)):
            d = np.zeros(n); m = models[k].copy()
            if kind == 0:
                P.dg_oracle_FDs(dp(u), dp(m), dp(d), n)
            elif kind == 1:
                P.dg_oracle_FDsSym(dp(u), dp(m), dp(d), n)
            else:
                P.dg_oracle_HDS_full(kind - 10, dp(u), dp(m), dp(d), n)
            lst = np.zeros(n, np.int32)
            S = P.dg_oracle_inlidxs(dp(d), n, C.c_double(th), ip(lst))
            assert np.array_equal(d, R[k], equal_nan=True), (kind, k, int(np.argmax(d != R[k])))
            assert S.I == I[k], (kind, k, S.I, I[k])
            assert S.J == J[k] or (np.isnan(S.J) and np.isnan(J[k])), (kind, k, S.J, J[k])
        assert kind not in (0, 10) or I[0] > 0                        # the ground truth has inliers in every scene


@pytest.mark.parametrize("n", es.E)
def test_screen_counts_at_tile_edges_and_model_batches(n):
    """mi_degensac_screen_counts at 1 / 63 / 64 / 65 / 128 / 129 models (64 per wave): never fewer than the exact band; with every row in
    the band exactly n (a clamped tail row counted twice or a dropped row shows here, not in the inequality); and on noise-free inliers
    plus far outliers with a tiny threshold, level 2 counts exactly the band of the fitted model"""
    p1, p2, _ = es.f_scene(n); models = _f_models(_f_truth(n), max(es.SCREEN_F_MODELS), 100 + n)
    q1, q2, lab, Fq = es.far_outlier_scene(n, seed=900 + n); tiny = 1e-6; huge = 1e15
    for kind in (0, 1):
        _, _, R = _score(p1, p2, models, kind, 1.0)
        _, _, Rq = _score(q1, q2, Fq.reshape(1, 9), kind, tiny)
        exact_q = (Rq < tiny * 9 / 4).sum(axis=1)
        assert exact_q[0] == lab.sum(), (kind, exact_q, lab.sum())    # the band is the inlier set
        for nm in es.SCREEN_F_MODELS:
            for th in (0.25, 4.0):
                c1, c2 = _screen_f(p1, p2, models[:nm], kind, th)
                assert es.superset_ok(c2, R[:nm], th), (kind, nm, th)
                assert es.superset_ok(c1, R[:nm], th), (kind, nm, th)
                assert (c1 <= n).all() and (c2 <= n).all(), (kind, nm, th)
            c1, c2 = _screen_f(p1, p2, models[:nm], kind, huge)
            assert es.all_in_band_ok(c1, R[:nm], huge) and es.all_in_band_ok(c2, R[:nm], huge), (kind, nm, c1, c2)
            rep = np.repeat(Fq.reshape(1, 9), nm, axis=0)             # the fitted model in every slot of the batch
            c1, c2 = _screen_f(q1, q2, rep, kind, tiny)
            assert (c2 == exact_q[0]).all() and (c1 >= exact_q[0]).all(), (kind, nm, c1, c2, exact_q)


@pytest.mark.parametrize("n", es.E)
def test_homography_screen_at_tile_edges_and_model_batches(n):
    """mi_degensac_screen_counts_h at 1 / 3 / 4 / 5 / 7 / 8 / 9 models (four per sweep): the count is the number of candidates, every
    point whose exact HDs is inside the band is a candidate, and with every row in the band the count is exactly n"""
    p1, p2, _ = es.h_scene(n); models = _h_models(np.linalg.inv(syn.H_1_6).T, max(es.SCREEN_H_MODELS), 200 + n); huge = 1e15
    _, _, R = _score(p1, p2, models, 10, 1.0)
    for nm in es.SCREEN_H_MODELS:
        for th in (1.0, 16.0):
            cnt, cand = _screen_h(p1, p2, models[:nm], th)
            assert np.array_equal(cnt, cand.sum(axis=1)), (nm, th)
            assert cand[R[:nm] < th * 9 / 4].all(), (nm, th)
        cnt, cand = _screen_h(p1, p2, models[:nm], huge)
        assert es.all_in_band_ok(cnt, R[:nm], huge) and cand.all(), (nm, cnt)
    assert (R[0] < 9 / 4).sum() > 0                                   # the band of the ground truth is hit


@pytest.mark.parametrize("ssz", [7, 4])
def test_sample_stream_at_pool_edges_both_stages(oracle_port, ssz):
    """300 samples at every size (the small pools are rewritten many times over), parallel and sequential pool stage: 4096 is the last
    size of the parallel stage, 4097 the first of the sequential one; n = sample size is what a homography on 4 rows draws from"""
    L = _lib.lib(); it = es.SAMPLER_ITERS
    for n in es.SAMPLER_NS[ssz]:
        ref = np.zeros((it, ssz), np.int32)
        oracle_port.lib().dg_oracle_sample_stream(C.c_uint(4242 + n), n, ssz, it, oracle_port.ip(ref), None)
        for seq in (0, 1):
            out = np.full((it, ssz), -1, np.int32)
            _lib.check(L.mi_degensac_sample_stream_ex(4242 + n, n, ssz, it, 0, seq, out.ctypes.data_as(C.POINTER(C.c_int32))))
            assert np.array_equal(out[:, ::-1], ref), (ssz, n, seq, int(np.argmax((out[:, ::-1] != ref).any(axis=1))))


# ---- 2. whole drivers at the edges ------------------------------------------------------------------------------------------------------
def _compare(kind, M, mask, st, ref, tag):
    """one pair against the restatement: every shared counter, the mask bit for bit, the raw model to 1e-9 relative Frobenius"""
    Mo, mo, so = ref; Mg = np.asarray(M, float).ravel(); Mo = np.asarray(Mo, float).ravel()
    diff = {k: (st[k], so[k]) for k in (es.F_KEYS if kind == "F" else es.H_KEYS) if st[k] != so[k]}
    assert not diff, (tag, diff)
    assert not st.get("discarded") and not st.get("rerun"), tag
    if np.abs(Mo).sum() == 0:
        assert np.abs(Mg).sum() == 0 and not np.asarray(mask).any(), tag
    else:
        assert np.array_equal(np.asarray(mask, bool), np.asarray(mo, bool)), (tag, int((np.asarray(mask, bool) != mo).sum()))
        rel = np.linalg.norm(Mg - Mo) / np.linalg.norm(Mo)
        assert rel < 1e-9, (tag, rel)


def _run(kind, A, B, seeds, px_th, et=0, laf_coef=0.0, max_iters=None, tuning=0):
    """one batch launch: (models [P, 3, 3] raw, masks, stats)"""
    call = es.F_CALL if kind == "F" else es.H_CALL
    mi = call["max_iters"] if max_iters is None else max_iters
    if kind == "F":
        M, m = pd.findFundamentalMatrixBatch(A, B, px_th, call["conf"], mi, laf_coef, ("sampson", "symm_epipolar")[et], True, True, seeds=seeds, tuning=tuning)
    else:
        M, m = api._batch("H", A, B, px_th, call["conf"], mi, et, True, laf_coef, True, seeds, 0, tuning)
    return np.asarray(M), m, pd.last_stats()


@pytest.mark.parametrize("n", es.E)
def test_drivers_at_tile_edges_every_variant_and_placement(oracle_port, n):
    """the F and the H scene of n rows through 3 workgroup sizes x 3 placements; at 257 / 513 / 1025 also [n, 6] rows with the LAF check"""
    cases = [("F", False), ("H", False)] + ([("F", True), ("H", True)] if n in es.LAF_NS else [])
    for kind, laf in cases:
        p1, p2, seed = (es.f_scene if kind == "F" else es.h_scene)(n, laf)
        ref = es.oracle_e(oracle_port, kind, n, laf)
        for variant in VARIANTS:
            for mode in PLACEMENTS:
                M, m, st = _run(kind, [p1], [p2], [seed], (es.F_CALL if kind == "F" else es.H_CALL)["px_th"], 0, es.LAF_COEF[kind] if laf else 0.0,
                                tuning=tune(variant, mode))
                # "a placement that does not fit the device's LDS is ignored" (include/mi_degensac.h): past the variant's limit a request
                # for points + pool in LDS must come out as the variant's own choice, everywhere else as requested
                want = mode if mode != 1 or n <= _lds_limit(kind, variant) else _placement(kind, n, VARIANT[variant])
                assert st[0]["threads"] == variant and st[0]["placement"] == want, (kind, laf, variant, mode, want, st[0])
                assert want == mode or (kind == "H" and n > 1025), (kind, variant, mode, n)      # every F case and H up to 1025 rows fit
                _compare(kind, M[0], m[0], st[0], ref, (kind, n, laf, variant, mode))


@pytest.mark.parametrize("threads,n", es.COOP_CASES)
def test_cooperative_slices_of_one_row(oracle_port, threads, n):
    """forced helper workgroups at n = pass step + 1 (and 2 steps + 1 at 128 threads): slices are whole steps, so with 3 helpers 513
    rows are units of 512 + 1 rows and 1025 rows 512 + 512 + 1; four pairs per launch, with and without every full pass distributed"""
    A, B, seeds = es.coop_scenes(n)
    for helpers in es.COOP_HELPERS:
        for dist in (0, 1):
            F, m = pd.findFundamentalMatrixBatch(A, B, max_iters=20000, seeds=seeds,
                                                 tuning=tune(threads, 0) | _lib.TUNE_HELPERS(helpers) | (dist * _lib.TUNE_COOP_ALL_PASSES))
            st = pd.last_stats()
            assert all(s_["threads"] == threads and s_["placement"] == 0 for s_ in st), (threads, helpers, dist, st[0])
            _check_against_oracle(oracle_port, A, B, seeds, F, m, st, (threads, n, helpers, dist))


def _placement(kind, n, tuning=_lib.TUNE_LATENCY):
    """the placement reported for one pair of n rows (one sample); default: what the 512-thread variant chooses by itself"""
    rng = np.random.default_rng(n); a = rng.uniform(0, 700, (n, 2)); b = rng.uniform(0, 700, (n, 2))
    return _run(kind, [a], [b], [1], 1.0, max_iters=1, tuning=tuning)[2][0]["placement"]


def _last_n_with(kind, placement, lo, hi, tuning=_lib.TUNE_LATENCY):
    """largest n in [lo, hi) with `placement`; lo has it, hi does not (placements follow n monotonically: LDS room)"""
    assert _placement(kind, lo, tuning) == placement and _placement(kind, hi, tuning) != placement, (kind, placement, lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _placement(kind, mid, tuning) == placement:
            lo = mid
        else:
            hi = mid
    return lo


_lds = {}


def _lds_limit(kind, variant):
    """largest n at which a request for points + pool in LDS is honoured by this variant (bisected once per process)"""
    if (kind, variant) not in _lds:
        _lds[kind, variant] = _last_n_with(kind, 1, 512, 8192, tune(variant, 1))
    return _lds[kind, variant]


@pytest.mark.parametrize("kind", ["F", "H"])
@pytest.mark.parametrize("edge", [(1, 2), (2, 0)], ids=["points_leave_lds", "pool_leaves_lds"])
def test_both_sides_of_a_placement_limit(oracle_port, kind, edge):
    """512 threads, no placement override: the largest n with points + pool in LDS and n + 1 (pool only), the largest n with the pool in
    LDS and n + 1 (workspace).  The limit is found by bisection with one-sample launches, not written down here."""
    before, after = edge
    n_edge = _last_n_with(kind, before, 512, 8192) if before == 1 else _last_n_with(kind, before, 8192, 131072)
    print(f"{kind}: placement {before} up to n = {n_edge}")
    for n, want in ((n_edge, before), (n_edge + 1, after)):
        if kind == "F":
            p1, p2, _, _ = syn.two_view_fundamental(n, 0.35, 0.1, seed=8000 + before, plane_fraction=0.5)
            ref = oracle_port.find_fundamental(p1, p2, 0.5, 0.9999, es.EDGE_BUDGET, seed=77)
        else:
            p1, p2, _, _ = syn.homography_pairs(n, 0.35, 0.5, seed=8100 + before)
            ref = oracle_port.find_homography(p1, p2, 1.0, 0.999, es.EDGE_BUDGET, seed=77)
        assert ref[2]["I"] > 0.2 * n and ref[2]["lo_runs"] >= 1, ref[2]
        M, m, st = _run(kind, [p1], [p2], [77], 0.5 if kind == "F" else 1.0, max_iters=es.EDGE_BUDGET, tuning=_lib.TUNE_LATENCY)
        assert st[0]["threads"] == 512 and st[0]["placement"] == want, (kind, n, want, st[0])
        _compare(kind, M[0], m[0], st[0], ref, (kind, n, want))


# ---- 3. other coordinate frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", es.FRAME_NAMES)
@pytest.mark.parametrize("kind", ["F", "H"])
def test_drivers_in_other_coordinate_frames(oracle_port, kind, frame):
    """three scenes (n = 257 and 1000; one plane-dominated F scene, one scene with LAF rows), every metric, three workgroup sizes: the
    restatement on the same transformed input decides"""
    n_scenes = len(es.FRAME_F_SCENES if kind == "F" else es.FRAME_H_SCENES)
    cases = [es.frame_case(kind, j, frame) for j in range(n_scenes)]
    for et in (es.F_METRICS if kind == "F" else es.H_METRICS):
        for lc in sorted({c[4] for c in cases}):                      # a launch shares its row width and LAF coefficient
            js = [j for j in range(n_scenes) if cases[j][4] == lc]
            for variant in VARIANTS:
                M, m, st = _run(kind, [cases[j][0] for j in js], [cases[j][1] for j in js], [cases[j][3] for j in js], cases[js[0]][2], et, lc,
                                tuning=VARIANT[variant])
                for k, j in enumerate(js):
                    assert st[k]["threads"] == variant
                    _compare(kind, M[k], m[k], st[k], es.oracle_frame(oracle_port, kind, j, frame, et), (kind, frame, j, et, variant))


def _frame_models(fitted, seed):
    """models of a frame: the fitted one, rescaled by 1e+-12 and negated, perturbed copies, random ones"""
    rng = np.random.default_rng(seed); f = np.asarray(fitted, float).ravel()
    models = [f * s for s in (1.0, 1e-12, 1e12, -3.0)]
    models += [f + rng.normal(scale=10.0 ** -k, size=9) * np.abs(f) for k in range(1, 9) for _ in range(4)]       # entry-wise: the entries span many decades
    models += [f + rng.normal(scale=10.0 ** -k, size=9) * np.abs(f).max() for k in range(1, 9) for _ in range(2)]
    models += [rng.normal(size=9) for _ in range(40)] + [rng.normal(size=9) * np.abs(f) / np.abs(f).max() for _ in range(20)]
    return np.ascontiguousarray(np.array(models))


@pytest.mark.parametrize("frame", es.FRAME_NAMES)
def test_fundamental_screens_are_supersets_in_every_frame(frame):
    truth = _f_truth(0); tested = 0
    for n, seed in ((257, 11), (1000, 12)):
        p1, p2, _, _ = syn.two_view_fundamental(n, 0.5, 0.3, seed=seed)
        q1, q2, _ = es.to_frame(frame, p1, p2, 1.0)
        models = _frame_models(es.f_in_frame(frame, truth), seed)
        for kind in (0, 1):
            for px in (0.5, 2.0):
                th = (px * es.frame(frame)["th"]) ** 2
                c1, c2 = _screen_f(q1, q2, models, kind, th)
                _, _, R = _score(q1, q2, models, kind, th)
                exact = (R < th * 9 / 4).sum(axis=1)
                assert (c2 >= exact).all(), (frame, n, kind, px, int(np.argmax(exact.astype(np.int64) - c2)))
                assert (c1 >= exact).all(), (frame, n, kind, px, int(np.argmax(exact.astype(np.int64) - c1)))
                assert exact[0] > 0.3 * n, (frame, n, kind, px, exact[:4])      # the fitted model's band is hit
                tested += int((exact > 0).sum())
    assert tested > 50


@pytest.mark.parametrize("frame", es.FRAME_NAMES)
def test_homography_screen_is_a_superset_in_every_frame(frame):
    for n, seed in ((257, 21), (1000, 22)):
        p1, p2, _, _ = syn.homography_pairs(n, 0.5, 0.5, seed=seed)
        q1, q2, _ = es.to_frame(frame, p1, p2, 1.0, "H")
        models = _frame_models(es.h_raw_in_frame(frame, syn.H_1_6), seed)
        for px in (1.0, 3.0):
            th = (px * es.frame(frame, "H")["th"]) ** 2
            cnt, cand = _screen_h(q1, q2, models, th)
            _, _, R = _score(q1, q2, models, 10, th)
            assert np.array_equal(cnt, cand.sum(axis=1)), (frame, n, px)
            miss = (R < th * 9 / 4) & (cand == 0)
            assert not miss.any(), (frame, n, px, np.argwhere(miss)[:5].tolist())
            assert (R[0] < th * 9 / 4).sum() > 0.3 * n, (frame, n, px)
