"""GPU: the guided stage (mi_guided.hip) at its edges — candidate lists that are exactly full, query / train counts around the
16-query workgroups, 64-row steps and 1024-row LDS chunks, every residual kind with Hamming and the mutual search, thresholds of 0
and exactly at a residual, models scaled by huge and tiny factors, NaN / inf in keypoints and models, [n, 6] keypoint rows,
sub-batch calls of the C entry points with offsets[0] > 0, and a seeded random sweep.  The device must equal the restatement of
tests/guided_ref.py bit for bit and satisfy the float64 conditions of tests/matcher_ref.py under the oracle's gate.

Observed run time of this file on one MI355X: 6 s for its 68 tests (the numpy oracle's n1 x n2 residual matrices are most of it)."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, tensor_api
from tests import guided_ref as gr, matcher_ref as mr
from tests.test_gpu_guided import SIZES, _batch, _run, _scene, _t

pytestmark = pytest.mark.gpu

I3 = np.eye(3)
F_SAME_Y = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])             # x2^T F x1 = y1 - y2: the band of a query is its own image row


def _name(model, et):
    return gr.ERROR_NAMES[model][et]


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _check(P, got, model, et, px, M, K1, K2, D1, D2, norm, ratio, mutual, exact=True):
    """every pair of a batch against the oracle (bit for bit) and, with the oracle's gate, against the exact distances"""
    passed = 0
    for p in range(len(D1)):
        oi, od, om = gr.oracle(P, model, et, px, M[p], K1[p], K2[p], D1[p], D2[p], norm, ratio, mutual)
        gm, gi, gd = got[p]
        assert np.array_equal(gi, oi), (p, np.flatnonzero((gi != oi).any(1))[:5])
        assert np.array_equal(_bits(gd), _bits(od)), p
        assert np.array_equal(gm, om), p
        assert ((gi >= -1) & (gi < max(len(D2[p]), 1))).all(), p
        if exact:
            mr.check_knn2_against_exact(gi, gd, D1[p], D2[p], norm, gate=gr.gate_matrix(P, model, et, px, M[p], K1[p], K2[p]))
        passed += int((gi[:, 0] >= 0).sum())
    return passed


# ---- exact candidate counts ------------------------------------------------------------------------------------------------
def _trace(g):
    """mg_guided_kernel's list of one query from its gate row: per 64-row step the rows that pass join the list; at 64 or more the
    first 64 are flushed and the rest move down.  Returns (largest occupancy, carries after each flush, steps that flushed)."""
    cnt = peak = 0; carries = []; steps = []
    for s in range(0, len(g), 64):
        cnt += int(g[s:s + 64].sum()); peak = max(peak, cnt)
        if cnt >= 64:
            cnt -= 64; carries.append(cnt); steps.append(s // 64)
    return peak, carries, steps


def _R(*spans):
    return [i for lo, hi in spans for i in range(lo, hi)]


# name -> (gated train rows of query 0, what the placement must produce: (m, largest occupancy or None, predicate on (carries, flush steps)))
_PLACE = {
    "m0": ([], (0, 0, lambda c, s: not c)),
    "m1": ([70], (1, 1, lambda c, s: not c)),
    "m2_first_and_third_chunk": ([5, 2100], (2, 2, lambda c, s: not c)),
    "m63_one_step": (_R((0, 63)), (63, 63, lambda c, s: not c)),
    "m64_full_step": (_R((64, 128)), (64, 64, lambda c, s: c == [0])),
    "m64_63_plus_1": (_R((0, 63), (64, 65)), (64, 64, lambda c, s: c == [0] and s == [1])),
    "m65_63_plus_2": (_R((0, 63), (64, 66)), (65, 65, lambda c, s: c == [1])),
    "m127_63_then_64": (_R((0, 63), (64, 128)), (127, 127, lambda c, s: c == [63])),
    "m128": (_R((0, 63), (64, 129)), (128, 127, lambda c, s: c == [63, 0])),
    "m129": (_R((0, 63), (64, 130)), (129, 127, lambda c, s: c == [63, 1])),
    "m191_carry_63_twice": (_R((0, 63), (64, 192)), (191, 127, lambda c, s: c == [63, 63])),
    "m200_scattered": (_R((3, 40), (100, 190), (1000, 1060), (2150, 2163)), (200, None, lambda c, s: len(c) == 3)),
    "m128_flush_in_last_step_of_chunk": (_R((896, 959), (960, 1024), (1024, 1025)), (128, 127, lambda c, s: c == [63, 0] and s[0] == 15)),
    "m70_third_chunk_only": (_R((2048, 2118)), (70, 64, lambda c, s: c == [0] and s == [32])),
}
_N2 = 2200                                                            # three LDS chunks: 1024 + 1024 + 152 rows


def _placed_pair(model, rows, seed, dim, same_desc):
    rng = np.random.default_rng(seed)
    n1 = 6
    k1 = np.c_[1000.0 * (np.arange(n1) + 1), 500.0 + 10 * np.arange(n1)]
    k2 = np.c_[-1e5 - 10.0 * np.arange(_N2), -1e5 - 10.0 * np.arange(_N2)]        # far from every query, in x and in y
    k2[rows] = k1[0]
    if model == "F":
        k2[rows, 0] = rng.uniform(-50, 50, len(rows))                 # anywhere on the query's row
    free = rng.permutation(np.setdiff1d(np.arange(_N2), rows))
    k2[free[:3]] = k1[1]; k2[free[3]] = k1[2]                         # the other queries: three candidates, one, none
    d1 = rng.normal(size=(n1, dim)).astype(np.float32); d2 = rng.normal(size=(_N2, dim)).astype(np.float32)
    if same_desc:
        d2[rows] = d2[7]                                              # every candidate at the same distance: ties through the butterfly
    return k1, k2, d1, d2


@pytest.mark.parametrize("model", ["H", "F"])
@pytest.mark.parametrize("same_desc", [False, True], ids=["distinct", "ties"])
def test_exact_candidate_counts(oracle_port, model, same_desc):
    """m = 0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 200 candidates at chosen train rows: 63 pending + a full 64-row step (127 in
    the list), a carry of 63 after a flush, a flush in the last step before the 1024-row chunk boundary, candidates in the third
    chunk only; with one shared descriptor every candidate ties.  The occupancy of each placement is computed from the oracle's gate
    and asserted before the device is compared."""
    M1 = I3 if model == "H" else F_SAME_Y                             # the identity is its own driver form inv(H)^T
    names = list(_PLACE)
    K1, K2, D1, D2 = [], [], [], []
    for i, nm in enumerate(names):
        k1, k2, d1, d2 = _placed_pair(model, _PLACE[nm][0], 40 + i, 33, same_desc)
        K1.append(k1); K2.append(k2); D1.append(d1); D2.append(d2)
    M = np.stack([M1] * len(names))
    peaks = []
    for i, nm in enumerate(names):
        rows, (m, peak, pred) = _PLACE[nm]
        gate = gr.gate_matrix(oracle_port, model, 0, 1.0, M[i], K1[i], K2[i])
        assert list(np.flatnonzero(gate[0])) == rows and len(rows) == m, nm
        assert list(gate[1:4].sum(1)) == [3, 1, 0], nm
        pk, carries, steps = _trace(gate[0])
        assert (peak is None or pk == peak) and pred(carries, steps), (nm, pk, carries, steps)
        peaks.append(pk)
    assert max(peaks) == 127                                          # MG_LIST - 1: the list was as full as it can get
    for mutual in (False, True):
        got = _run(K1, K2, D1, D2, M, model, ratio=0.9, mutual=mutual, px_th=1.0, error_type="sampson")
        _check(oracle_port, got, model, 0, 1.0, M, K1, K2, D1, D2, "l2", 0.9, mutual)
        if same_desc:
            for i, nm in enumerate(names):
                rows = _PLACE[nm][0]
                assert list(got[i][1][0]) == (sorted(rows) + [-1, -1])[:2], nm      # the two lowest rows win every tie


# ---- query and train counts around MG_Q = 16, the 64-row step and the 1024-row chunk ----
_EDGE_SIZES = [(n1, n2) for n1 in (15, 16, 17, 33) for n2 in (63, 64, 65, 1023, 1024, 1025, 2049)]


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model,et,norm,dim", [("F", 0, "l2", 65), ("H", 0, "hamming", 36), ("H", 2, "l2", 33)])
def test_query_and_train_edges(oracle_port, model, et, norm, dim, mutual):
    px = 12.0 if et == 2 else 6.0
    K1, K2, D1, D2, M = [], [], [], [], []
    for i, (n1, n2) in enumerate(_EDGE_SIZES):
        k1, k2, d1, d2, Md = _scene(model, n1, n2, 500 + i, dim, norm)
        K1.append(k1); K2.append(k2); D1.append(d1); D2.append(d2); M.append(Md)
    M = np.stack(M)
    got = _run(K1, K2, D1, D2, M, model, ratio=0.9, mutual=mutual, px_th=px, error_type=_name(model, et))
    assert _check(oracle_port, got, model, et, px, M, K1, K2, D1, D2, norm, 0.9, mutual) > 100


# ---- every residual kind with the mutual search on Hamming and on 128 floats ----
@pytest.mark.parametrize("norm,dim", [("hamming", 32), ("l2", 128)])
@pytest.mark.parametrize("model,et", gr.KINDS)
def test_every_kind_mutual(oracle_port, model, et, norm, dim):
    px = 12.0 if (model == "H" and et in (2, 4)) else 6.0
    K1, K2, D1, D2, M = _batch(model, norm, dim, seed=20 + et)
    got = _run(K1, K2, D1, D2, M, model, ratio=0.9, mutual=True, px_th=px, error_type=_name(model, et))
    assert _check(oracle_port, got, model, et, px, M, K1, K2, D1, D2, norm, 0.9, True) > 200


# ---- threshold edges ----
def _one_row_scene(x1, x2, seed=1):
    """17 queries, 70 train rows; query 0 sits at x1, train row 40 at x2, everything else is far from everything"""
    rng = np.random.default_rng(seed)
    k1 = np.c_[3000.0 + 500 * np.arange(17), 7000.0 + 300 * np.arange(17)]; k1[0] = x1
    k2 = np.c_[-9000.0 - 400 * np.arange(70), -20000.0 - 700 * np.arange(70)]; k2[40] = x2
    return k1, k2, rng.normal(size=(17, 20)).astype(np.float32), rng.normal(size=(70, 20)).astype(np.float32)


def _accepts(P, model, et, px, M1, scene):
    k1, k2, d1, d2 = scene
    got = _run([k1], [k2], [d1], [d2], M1[None], model, ratio=0.9, px_th=px, error_type=_name(model, et))
    _check(P, got, model, et, px, M1[None], [k1], [k2], [d1], [d2], "l2", 0.9, False)
    assert got[0][1][0, 0] in (40, -1) and got[0][1][0, 1] == -1
    return got[0][1][0, 0] == 40


@pytest.mark.parametrize("model,et", gr.KINDS)
def test_threshold_zero(oracle_port, model, et):
    """px_th = 0 (screen = 0): a row exactly on the model has residual 0 and `<=` accepts it; one ulp off is rejected.  Which rows
    have a residual of exactly 0 is the oracle's word (the symmetric-sum kinds add 1e-10 to their denominators)."""
    M1 = I3 if model == "H" else F_SAME_Y
    x1 = np.array([100.0, 200.0])
    on = _one_row_scene(x1, x1)
    r_on = gr.resid(oracle_port, model, et, M1, on[0][:1], on[1][40:41])[0, 0]
    if (model, et) in (("F", 0), ("F", 1), ("H", 0), ("H", 1), ("H", 2)):
        assert r_on == 0.0                                            # the case is constructed
    assert _accepts(oracle_port, model, et, 0.0, M1, on) == bool(r_on <= 0.0)
    off = _one_row_scene(x1, np.nextafter(x1, np.inf))
    r_off = gr.resid(oracle_port, model, et, M1, off[0][:1], off[1][40:41])[0, 0]
    assert r_off > 0.0
    assert not _accepts(oracle_port, model, et, 0.0, M1, off)


def _px_reaching(model, et, r):
    """the smallest px_th whose threshold reaches r (th = px or fl(px * px)), and whether that threshold equals r exactly"""
    px = r if (model == "H" and et in (2, 4)) else np.sqrt(r)
    while gr.th(model, et, px) < r:
        px = np.nextafter(px, np.inf)
    while gr.th(model, et, np.nextafter(px, 0)) >= r:
        px = np.nextafter(px, 0)
    return float(px), bool(gr.th(model, et, px) == r)


_F_Y2 = np.array([[0.0, 0, 0], [0, 0, -1], [0, 0, 0]])                # x2^T F x1 = -y2, denominator 0 + 0 + 0 + 1: Sampson = y2^2


@pytest.mark.parametrize("model,et,M1,x2,r_want,exact_want", [
    ("H", 0, I3, (103.0, 204.0), None, None), ("H", 1, I3, (103.0, 204.0), 25.0, True), ("H", 2, I3, (103.0, 204.0), 5.0, True),
    ("H", 3, I3, (103.0, 204.0), None, None), ("H", 4, I3, (103.0, 204.0), None, True),
    ("F", 0, _F_Y2, (103.0, 5.0), 25.0, True), ("F", 0, F_SAME_Y, (103.0, 204.0), 8.0, None), ("F", 1, F_SAME_Y, (103.0, 204.0), 32.0, None)],
    ids=["H0", "H1", "H2", "H3", "H4", "F0_exact", "F0", "F1"])
def test_residual_exactly_at_the_threshold(oracle_port, model, et, M1, x2, r_want, exact_want):
    """x2 = x1 + (3, 4) under the identity: the one-way squared transfer error is exactly 25.  The threshold comes from the oracle's
    own residual r: the row is accepted at the smallest px_th whose threshold reaches r — equal to r where r is representable as a
    threshold (asserted for the constructed cases: H symm_sq_max 25, symm_max 5, symm_sum, and a rank-one F whose Sampson error is
    y2^2 = 25) — and rejected one ulp of px_th below."""
    x1 = np.array([100.0, 200.0])
    sc = _one_row_scene(x1, np.array(x2))
    r = gr.resid(oracle_port, model, et, M1, sc[0][:1], sc[1][40:41])[0, 0]
    assert np.isfinite(r) and r > 0 and (r_want is None or r == r_want), r
    px, exact = _px_reaching(model, et, r)
    assert exact_want is None or exact == exact_want, (r, px)
    assert _accepts(oracle_port, model, et, px, M1, sc)
    assert not _accepts(oracle_port, model, et, float(np.nextafter(px, 0)), M1, sc)


# ---- scaled models: the screens must not reject what the exact residual accepts ----
@pytest.mark.parametrize("model,et", gr.KINDS)
def test_scaled_models(oracle_port, model, et):
    px = 12.0 if (model == "H" and et in (2, 4)) else 6.0
    K1, K2, D1, D2, M = _batch(model, "l2", 37, seed=30 + et)
    base = None
    for scale in (1.0, -1.0, 1e-30, 1e30, 1e-150, 1e150):
        got = _run(K1, K2, D1, D2, M * scale, model, ratio=0.9, mutual=True, px_th=px, error_type=_name(model, et))
        passed = _check(oracle_port, got, model, et, px, M * scale, K1, K2, D1, D2, "l2", 0.9, True)
        if scale == 1.0:
            base = passed
            assert base > 200
        elif scale == -1.0:
            assert passed == base                                     # every residual is even in the model's sign


# ---- NaN and inf in keypoints and models ----
@pytest.mark.parametrize("model,et", [("F", 0), ("F", 1), ("H", 0), ("H", 3)])
def test_non_finite_keypoints_and_models(oracle_port, model, et):
    px = 6.0
    K1, K2, D1, D2, M = _batch(model, "l2", 37, seed=50 + et)
    kw = dict(ratio=0.9, mutual=True, px_th=px, error_type=_name(model, et))
    clean = _run(K1, K2, D1, D2, M, model, **kw)
    K1 = [k.copy() for k in K1]; K2 = [k.copy() for k in K2]; M = M.copy()
    # pairs (SIZES): 6 = (64, 64), 7 = (65, 200), 9 = (250, 320), 10 = (40, 2100); 8 = (300, 280) carries the zero model
    K1[6][10, 0] = np.nan; K2[6][63, 1] = np.inf; K2[6][0, 0] = -np.inf
    K1[9][249] = np.nan; K2[9][100, 0] = np.nan
    M[7, 1, 1] = np.nan; M[10, 2, 0] = np.inf
    M[2] = np.nan                                                     # (70, 1): a model of nine NaN
    touched = {2, 6, 7, 9, 10}
    got = _run(K1, K2, D1, D2, M, model, **kw)
    _check(oracle_port, got, model, et, px, M, K1, K2, D1, D2, "l2", 0.9, True)
    for p in range(len(SIZES)):
        if p not in touched:
            assert all(np.array_equal(u, v) for u, v in zip(got[p], clean[p])), p
    assert (got[2][1] == -1).all()                                    # NaN residuals fail
    assert (got[6][1][10] == -1).all() and (got[9][1][249] == -1).all() and not np.isin(got[9][1], [100]).any()
    all_nan = _run(K1, K2, D1, D2, np.full_like(M, np.nan), model, **kw)
    for m, i, d in all_nan:
        assert (m == -1).all() and (i == -1).all() and np.isposinf(d).all()


# ---- [n, 6] keypoint rows, and sub-batches whose offsets do not start at 0 ----
def _p(x, t):
    return x.ctypes.data_as(C.POINTER(t))


@pytest.mark.parametrize("model,et,norm,dim", [("F", 0, "l2", 37), ("H", 1, "hamming", 32)])
def test_kp_dim_6_and_offsets_above_zero(oracle_port, model, et, norm, dim):
    import torch
    px = 6.0; code = 0 if norm == "l2" else 1
    K1, K2, D1, D2, M = _batch(model, norm, dim, seed=60 + et)
    rng = np.random.default_rng(5)
    K1 = [np.c_[k, rng.normal(size=(len(k), 4))] for k in K1]; K2 = [np.c_[k, rng.normal(size=(len(k), 4))] for k in K2]
    kw = dict(ratio=0.9, mutual=True, px_th=px, error_type=_name(model, et))
    got = _run(K1, K2, D1, D2, M, model, **kw)                         # [n, 6] rows through the tensor API
    two = _run([k[:, :2] for k in K1], [k[:, :2] for k in K2], D1, D2, M, model, **kw)
    for p in range(len(SIZES)):
        assert all(np.array_equal(u, v) for u, v in zip(got[p], two[p])), p
    assert _check(oracle_port, got, model, et, px, M, [k[:, :2] for k in K1], [k[:, :2] for k in K2], D1, D2, norm, 0.9, True) > 200
    full_m = np.concatenate([g[0] for g in got]); full_i = np.concatenate([g[1] for g in got]); full_d = np.concatenate([g[2] for g in got])
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    o1 = np.zeros(len(c1) + 1, np.int64); o1[1:] = np.cumsum(c1); o2 = np.zeros(len(c2) + 1, np.int64); o2[1:] = np.cumsum(c2)
    A, B = np.ascontiguousarray(np.concatenate(D1)), np.ascontiguousarray(np.concatenate(D2))
    X1, X2 = np.ascontiguousarray(np.concatenate(K1)), np.ascontiguousarray(np.concatenate(K2))
    lo, hi = 4, 10                                                    # pairs 4 .. 9 of SIZES: both first offsets are above 0
    s1 = np.ascontiguousarray(o1[lo:hi + 1]); s2 = np.ascontiguousarray(o2[lo:hi + 1]); Ms = np.ascontiguousarray(M[lo:hi].reshape(-1, 9))
    assert s1[0] > 0 and s2[0] > 0
    a, b = int(s1[0]), int(s1[-1])
    assert b < len(A)                                                 # rows behind the sub-batch exist too
    mp = _lib.MatchParams(code, dim, 0.9, True); gp = _lib.GuideParams(model == "H", et, px)
    L = _lib.lib()

    def same(idx, dist, match):
        assert (idx[:a] == -7).all() and (idx[b:] == -7).all() and (dist[:a] == -7).all() and (dist[b:] == -7).all()      # rows outside: untouched
        assert np.array_equal(idx[a:b], full_i[a:b]) and np.array_equal(_bits(dist[a:b]), _bits(full_d[a:b]))
        if match is not None:
            assert (match[:a] == -7).all() and (match[b:] == -7).all() and np.array_equal(match[a:b], full_m[a:b])

    # host pointers, kp_dim = 6
    idx = np.full((len(A), 2), -7, np.int32); dist = np.full((len(A), 2), -7, np.float32); match = np.full(len(A), -7, np.int32)
    cnt = np.zeros(hi - lo, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_batch(C.byref(mp), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), _p(s1, C.c_int64),
                     _p(s2, C.c_int64), _lib.dptr(X1), _lib.dptr(X2), 6, hi - lo, _lib.dptr(Ms), C.byref(gp), 0, _p(idx, C.c_int32),
                     _p(dist, C.c_float), _p(match, C.c_int32), _p(cnt, C.c_int32)))
    same(idx, dist, match)
    assert list(cnt) == [int((got[p][0] >= 0).sum()) for p in range(lo, hi)]
    # device pointers: the guided 2-NN + decision, the guided 2-NN alone, the unguided batched 2-NN
    dA, dB, dX1, dX2, dM = _t(A), _t(B), _t(X1), _t(X2), _t(Ms)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    di = torch.full((len(A), 2), -7, dtype=torch.int32, device=dA.device); dd = torch.full((len(A), 2), -7.0, dtype=torch.float32, device=dA.device)
    dm = torch.full((len(A),), -7, dtype=torch.int32, device=dA.device)
    hc = np.zeros(hi - lo, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_batch_dev(C.byref(mp), dA.data_ptr(), dB.data_ptr(), _p(s1, C.c_int64), _p(s2, C.c_int64), dX1.data_ptr(),
                     dX2.data_ptr(), 6, hi - lo, dM.data_ptr(), C.byref(gp), 0, st, di.data_ptr(), dd.data_ptr(), dm.data_ptr(), None, _p(hc, C.c_int32)))
    same(di.cpu().numpy(), dd.cpu().numpy(), dm.cpu().numpy())
    assert list(hc) == list(cnt)
    di.fill_(-7); dd.fill_(-7.0)
    _lib.check_match(L.mi_degensac_match_guided_knn2_batch_dev(code, dA.data_ptr(), dB.data_ptr(), _p(s1, C.c_int64), _p(s2, C.c_int64), hi - lo, dim,
                     dX1.data_ptr(), dX2.data_ptr(), 6, dM.data_ptr(), C.byref(gp), 0, st, di.data_ptr(), dd.data_ptr()))
    torch.cuda.synchronize()
    same(di.cpu().numpy(), dd.cpu().numpy(), None)
    ui, ud = tensor_api.knn_match_batch_tensors(dA, dB, c1, c2)
    di.fill_(-7); dd.fill_(-7.0)
    _lib.check_match(L.mi_degensac_match_knn2_batch_dev(code, dA.data_ptr(), dB.data_ptr(), _p(s1, C.c_int64), _p(s2, C.c_int64), hi - lo, dim, 0, st,
                     di.data_ptr(), dd.data_ptr()))
    torch.cuda.synchronize()
    gi, gd = di.cpu().numpy(), dd.cpu().numpy()
    assert (gi[:a] == -7).all() and (gi[b:] == -7).all() and (gd[:a] == -7).all() and (gd[b:] == -7).all()
    assert np.array_equal(gi[a:b], ui.cpu().numpy()[a:b]) and np.array_equal(_bits(gd[a:b]), _bits(ud.cpu().numpy()[a:b]))


# ---- a seeded sweep over sizes, widths, norms, kinds, mutual, px_th and zero-model positions ----
@pytest.mark.parametrize("seed", [101, 202, 303, 404, 505, 606, 707, 808, 909, 1010, 1111, 1212, 1313, 1414, 1515, 1616])
def test_seeded_sweep(oracle_port, seed):
    rng = np.random.default_rng(seed)
    model, et = gr.KINDS[rng.integers(len(gr.KINDS))]
    norm = "hamming" if rng.random() < 0.3 else "l2"
    dim = int(rng.choice([4, 32, 68])) if norm == "hamming" else int(rng.choice([1, 5, 33, 64, 65, 130]))
    mutual = bool(rng.random() < 0.5)
    px = 0.0 if rng.random() < 0.15 else float(np.exp(rng.uniform(np.log(0.1), np.log(50.0))))
    K = int(rng.integers(3, 7))
    K1, K2, D1, D2, M = [], [], [], [], []
    for i in range(K):
        n1 = int(rng.choice([0, 1, 15, 17, 40, 90])) if rng.random() < 0.5 else int(rng.integers(0, 91))
        n2 = int(rng.integers(0, 2101)) if rng.random() < 0.2 else int(rng.integers(0, 401))
        k1, k2, d1, d2, Md = _scene(model, n1, n2, seed * 10 + i, dim, norm)
        if rng.random() < 0.25:
            Md = np.zeros((3, 3))
        K1.append(k1); K2.append(k2); D1.append(d1); D2.append(d2); M.append(Md)
    M = np.stack(M)
    got = _run(K1, K2, D1, D2, M, model, ratio=0.9, mutual=mutual, px_th=px, error_type=_name(model, et))
    _check(oracle_port, got, model, et, px, M, K1, K2, D1, D2, norm, 0.9, mutual)
