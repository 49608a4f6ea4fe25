"""GPU: the FGINN second neighbour over a pair list on image stores (mi_fginn.h on per-entry records; tensor_api.knn_match_fginn_pairs_tensors,
match_and_verify_fginn_pairs_tensors, matcher.match_and_verify_fginn_pairs, include/mi_degensac.h mi_degensac_match_*fginn*_pairs*).
Equality only.  Every result is compared (a) with the restatement of tests/fginn_ref.py per list entry on store slices, followed by its
keep, and (b) with knn_match_fginn_batch_tensors / match_and_verify_batch_tensors(fginn_th=) on the expansion of tests/pairs_ref.py with
the same seeds: idx equal, dist equal by bits.  A needy query has two rows, its output row and its descriptor row in store 1; the lists
here make them differ in both directions."""
import ctypes as C
import functools

import numpy as np
import pytest

import pydegensac_amd as pd
from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher, synthetic as syn, tensor_api
from tests import fginn_ref as fr, matcher_ref as mr, pairs_ref as pr

pytestmark = pytest.mark.gpu

NORMS = list(fr.NORMS)
CODE = {"l2": 0, "hamming": 1, "l2_u8": 4}
DET = [c for c in range(16) if c not in (12, 13)]      # every stats column but the two device clock readings
R = 10.0


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _w(norm):
    return 33 if norm == "l2" else 36


def _cat(xs, like):
    return np.concatenate(xs) if len(xs) else like[:0]


class Stores:
    """descriptor images of store 1, descriptor and keypoint images of store 2; one=True: store 1 IS store 2 (the same tensor twice)"""

    def __init__(self, D1, D2, K2, one=False):
        self.D1, self.D2, self.K2, self.one = D1, D2, K2, one
        self.c1 = [len(x) for x in D1]; self.c2 = [len(x) for x in D2]
        self.d1 = np.concatenate(D1); self.d2 = np.concatenate(D2); self.k2 = np.concatenate(K2)

    @classmethod
    def single(cls, D, Kp):
        return cls(D, D, Kp, True)


def _run(S, pairs, r, norm):
    a = _t(S.d1); b = a if S.one else _t(S.d2)
    idx, dist, po = tensor_api.knn_match_fginn_pairs_tensors(a, b, _t(S.k2), S.c1, S.c2, pairs, r, norm)
    return idx, dist, po


def _check(S, pairs, r, norm, got=None):
    """the pair-list call against (a) the restatement per entry and its keep and (b) the batched call on the expansion; returns the needy
    count of every entry, from the restatement"""
    import torch
    idx, dist, po = got or _run(S, pairs, r, norm)
    (e1,), (e2, ek2), c1, c2, want_po = pr.expand((S.d1,), S.c1, (S.d2, S.k2), S.c2, pairs)
    assert isinstance(po, np.ndarray) and po.dtype == np.int64 and np.array_equal(po, want_po)
    bi, bd = tensor_api.knn_match_fginn_batch_tensors(_t(e1), _t(e2), _t(ek2), c1, c2, r, norm)                  # (b)
    keep = tensor_api.match_filter_tensors(idx, dist, 0.9).cpu().numpy().astype(bool)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy()
    assert idx.shape == (po[-1], 2) and dist.shape == (po[-1], 2)
    assert np.array_equal(idx, bi.cpu().numpy()) and np.array_equal(_bits(dist), _bits(bd.cpu().numpy()))
    needy = []
    for p, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2)):                                                 # (a)
        oi, od, nd, _ = fr.fginn(S.D1[i], S.D2[j], S.K2[j][:, :2], r, norm)
        gi, gd = idx[po[p]:po[p + 1]], dist[po[p]:po[p + 1]]
        bad = (gi != oi).any(1) if gi.shape == oi.shape else None
        assert np.array_equal(gi, oi), (p, i, j, np.flatnonzero(bad)[:5], gi[bad][:3], oi[bad][:3])
        assert np.array_equal(_bits(gd), _bits(od)), (p, i, j, np.flatnonzero((_bits(gd) != _bits(od)).any(1))[:5])
        assert np.array_equal(keep[po[p]:po[p + 1]], fr.keep(oi, od, 0.9)), (p, i, j)
        needy.append(int(nd.sum()))
    return needy


def _grid(n, seed=0):
    g = np.arange(n) + 37 * seed
    return np.c_[100.0 * (g % 37), 100.0 * (g // 37)].astype(np.float64)


def _two_stores(scenes):
    """store 1 image s = the queries of scene s, store 2 image s = its train rows and keypoints: entry (s, s) is the scene as
    fginn_ref.twin_scene made it, entry (s, s') meets unrelated rows (a twinned nearest row still has its twin next to it)"""
    return Stores([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes])


def _one_store(scenes):
    """ONE store: image 2 s = the queries of scene s (keypoints on a grid, never read as train keypoints of a designed entry), image
    2 s + 1 = its train rows: entry (2 s, 2 s + 1) is the scene; (2 s + 1, 2 s + 1) is a self pair whose twinned rows are all needy"""
    D, Kp = [], []
    for k, (a, b, kp2) in enumerate(scenes):
        D += [a, b]; Kp += [_grid(len(a), k + 1), kp2]
    return Stores.single(D, Kp)


# ---- row counts, empty runs ------------------------------------------------------------------------------------------------------
Q_ROWS = [0, 0, 1, 63, 0, 0, 64, 65, 129, 0, 0]
T_ROWS = [0, 0, 1, 2, 63, 0, 0, 64, 65, 129, 0]


@pytest.mark.parametrize("norm", NORMS)
def test_row_counts_and_runs_of_empty_images(norm):
    """query images of 0 / 1 / 63 / 64 / 65 / 129 rows against train images of 0 / 1 / 2 / 63 / 64 / 65 / 129 rows, every combination, with
    runs of empty query and empty train images at the start, in the middle and at the end of their stores.  The queries are the first
    rows of one twin scene, whose train image (129 rows, 40 of them twins) is the last non-empty one: those entries have min(n1, 40) needy
    queries (more at 129, whose last queries are unrelated rows); the other train images carry twins of their own."""
    w = _w(norm)
    a, b, kp2 = fr.twin_scene(100, 129, 129, w, norm, 40)
    D1 = [a[:n].copy() for n in Q_ROWS]
    D2, K2 = [], []
    for k, n in enumerate(T_ROWS):
        _, bb, kk = (a, b, kp2) if n == 129 else fr.twin_scene(101 + k, 5, n, w, norm, min(5, n // 2))
        D2.append(bb); K2.append(kk)
    S = Stores(D1, D2, K2)
    pairs = [(i, j) for i in range(len(Q_ROWS)) for j in range(len(T_ROWS))]
    needy = _check(S, pairs, R, norm)
    at = {(i, j): needy[p] for p, (i, j) in enumerate(pairs)}
    for i, n in enumerate(Q_ROWS):                  # queries 0 .. 39 meet a twinned row, 40 .. 88 a single one, the rest are unrelated rows
        assert at[i, 9] == min(n, 40) if n <= 65 else at[i, 9] >= 40, (i, n, at[i, 9])
    assert all(at[i, j] == 0 for i in range(len(Q_ROWS)) for j in (0, 1, 2, 5, 6, 10))       # fewer than two train rows: nothing to rescan


# ---- needy counts ----------------------------------------------------------------------------------------------------------------
NEEDY = [0, 1, 63, 64, 65]


@pytest.mark.parametrize("norm", NORMS)
def test_needy_counts_around_the_tile_in_both_row_orders(norm):
    """entries with exactly 0 / 1 / 63 / 64 / 65 needy queries over ONE store, listed so that the first entry queries the LAST query image
    (query base > output base) and later entries query image 0 (query base < output base)"""
    scenes = [fr.twin_scene(20 + i, 130, 200, _w(norm), norm, m) for i, m in enumerate(NEEDY)]
    S = _one_store(scenes)
    order = [4, 2, 0, 3, 1, 0]
    pairs = [(2 * s, 2 * s + 1) for s in order]
    o1 = pr.offsets(S.c1); po = pr.offsets([S.c1[i] for i, _ in pairs])
    assert o1[pairs[0][0]] > po[0] and o1[pairs[2][0]] < po[2] and o1[pairs[5][0]] < po[5]
    assert _check(S, pairs, R, norm) == [NEEDY[s] for s in order]


@pytest.mark.parametrize("norm", NORMS)
def test_needy_counts_over_two_stores(norm):
    scenes = [fr.twin_scene(20 + i, 130, 200, _w(norm), norm, m) for i, m in enumerate(NEEDY)]
    S = _two_stores(scenes)
    pairs = [(s, s) for s in (3, 4, 0, 2, 1)] + [(0, 4), (4, 2)]
    needy = _check(S, pairs, R, norm)
    assert needy[:5] == [64, 65, 0, 63, 1]


# ---- the lists the single row number hid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_self_pairs_repeats_both_orders_and_a_shared_train_image(norm):
    """one store of twinned images.  Self pairs: the anchor is the query's own row at distance 0 and its twin the second neighbour, so
    both rows of every twin pair are needy; the same (i, j) twice; (i, j) next to (j, i); image 1 as the train image of four entries"""
    w = _w(norm)
    sizes = [(70, 12), (131, 30), (65, 9), (20, 4)]
    D, Kp = [], []
    for k, (n, m) in enumerate(sizes):
        _, b, kp2 = fr.twin_scene(40 + k, n, n, w, norm, m)
        D.append(b); Kp.append(kp2)
    D[0][20:30] = fr._near(np.random.default_rng(1), D[1][:10], norm, True)        # image 0 sees ten twinned rows of image 1
    S = Stores.single(D, Kp)
    pairs = [(3, 3), (1, 1), (0, 1), (1, 0), (2, 1), (0, 1), (3, 1), (0, 0), (2, 3)]
    needy = _check(S, pairs, R, norm)
    assert needy[0] == 2 * 4 and needy[1] == 2 * 30 and needy[7] == 2 * 12                         # self pairs
    assert needy[2] >= 10 and needy[2] == needy[5]                                                 # the repeat
    idx = _run(S, pairs, R, norm)[0].cpu().numpy()
    po = pr.offsets([S.c1[i] for i, _ in pairs])
    own = idx[po[1]:po[2]]
    assert (own[:, 0] == np.arange(131)).all() and (own[:30, 1] != np.arange(101, 131)).all()      # the twin is not the second neighbour


# ---- widths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,width", [("l2", w) for w in (1, 64, 65)] + [("hamming", w) for w in (4, 256, 260)]
                         + [("l2_u8", w) for w in (4, 64, 68, 128, 132, 256)])
def test_widths(norm, width):
    """1 / 64 / 65 words for the three norms, and the uint8 L2 width classes of the dense instances (<= 64, <= 128, <= 256 bytes)"""
    scenes = [fr.twin_scene(30 + i, n1, n2, width, norm, m) for i, (n1, n2, m) in enumerate([(7, 30, 3), (70, 130, 20), (66, 65, 9)])]
    needy = _check(_one_store(scenes), [(4, 5), (0, 1), (5, 5), (2, 3), (0, 3)], R, norm)
    assert sum(needy) > 0


# ---- the train split ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_a_list_that_takes_the_train_split_and_one_that_does_not(norm):
    scenes = [fr.twin_scene(50 + i, n1, n2, 8, norm, m) for i, (n1, n2, m) in enumerate([(8, 70, 4), (129, 200, 65), (65, 300, 30)])]
    S = _two_stores(scenes)
    few = [(1, 1), (2, 0), (0, 2), (1, 2), (2, 2)]
    k1 = [S.c1[i] for i, _ in few]; k2 = [S.c2[j] for _, j in few]
    assert mr.batch_split(k1, k2, _cus())[1] > 1
    needy = _check(S, few, R, norm)
    assert needy[0] == 65 and needy[4] == 30
    rng = np.random.default_rng(7)
    many = np.c_[rng.integers(1, 3, 600), rng.integers(0, 3, 600)]
    many[:3] = [(2, 2), (1, 1), (1, 1)]
    k1 = [S.c1[i] for i, _ in many]; k2 = [S.c2[j] for _, j in many]
    assert sum((c + 63) // 64 for c in k1) >= 2 * _cus() and mr.batch_split(k1, k2, _cus())[1] == 1
    needy = _check(S, many, R, norm)
    assert needy[:3] == [30, 65, 65]


# ---- placed distances: train row t at distance level[t] from every query -------------------------------------------------------------
def _levels(norm, lv, n1=1):
    lv = np.asarray(lv)
    if norm == "l2":
        b = np.zeros((len(lv), 3), np.float32); b[:, 0] = lv
        return np.zeros((n1, 3), np.float32), b
    b = (np.arange(8)[None, :] < lv[:, None]).astype(np.uint8)
    return np.zeros((n1, 8), np.uint8), b


def _tie_pair(norm, n2, rows, n1=2):
    """row 0 nearest, row 1 its twin (inside the radius), the two `rows` tie as the nearest competing rows, the rest farther"""
    lv = np.full(n2, 5); lv[0] = 0; lv[1] = 1; lv[list(rows)] = 2
    a, b = _levels(norm, lv, n1)
    kp2 = np.c_[100.0 * (1 + np.arange(n2)), np.zeros(n2)]; kp2[1] = kp2[0] + [1.0, 0.0]
    return a, b, kp2


@pytest.mark.parametrize("norm", NORMS)
def test_ties_across_a_tile_and_a_split_boundary(norm):
    """equal distances on both sides of the 64-row tile boundary and of the split boundary (rows t_chunk - 1 and t_chunk of an entry whose
    train image is split, the last split short), the entries listed against the store order: the lower index wins"""
    scenes = [_tie_pair(norm, 70, (63, 64), 3), _tie_pair(norm, 20000, (0, 1)), _tie_pair(norm, 70, (64, 69), 3)]
    pairs = [(2, 2), (1, 1), (0, 0), (1, 1)]
    t_chunk, splits = mr.batch_split([3, 2, 3, 2], [70, 20000, 70, 20000], _cus())
    rows = mr.split_rows(20000, t_chunk, splits)
    assert splits > 1 and 1 <= rows[-1] <= 63
    scenes[1] = _tie_pair(norm, 20000, (t_chunk - 1, t_chunk))
    S = _two_stores(scenes)
    got = _run(S, pairs, R, norm)
    assert _check(S, pairs, R, norm, got) == [3, 2, 3, 2]
    idx = got[0].cpu().numpy(); po = got[2]
    assert [list(idx[po[p]]) for p in range(4)] == [[0, 64], [0, t_chunk - 1], [0, 63], [0, t_chunk - 1]]


@pytest.mark.parametrize("norm", NORMS)
def test_radius_edge_on_integer_keypoints(norm):
    a, b = _levels(norm, [0, 1, 2, 3])
    kp2 = np.array([[0.0, 0], [3, 4], [100, 100], [0.5, 0]])
    a0, b0 = _levels(norm, [3, 2, 1, 0], 2)
    S = Stores([a0, a], [b0, b], [_grid(4), kp2])
    for r, second in ((5.0, 1), (np.nextafter(5.0, 6.0), 2), (0.0, 1), (4.0, 1)):
        got = _run(S, [(0, 0), (1, 1), (0, 1)], r, norm)
        _check(S, [(0, 0), (1, 1), (0, 1)], r, norm, got)
        idx = got[0].cpu().numpy()
        assert list(idx[2]) == [0, second] and list(idx[3]) == [0, second], r


@pytest.mark.parametrize("norm", NORMS)
def test_radius_zero_equals_the_plain_pair_list_2nn(norm):
    import torch
    scenes = [fr.twin_scene(60 + i, n1, n2, _w(norm), norm, m) for i, (n1, n2, m) in enumerate([(7, 30, 3), (70, 130, 20), (0, 2, 0), (65, 1, 0)])]
    S = _one_store(scenes)
    pairs = [(6, 7), (3, 3), (2, 3), (0, 1), (4, 5), (1, 6), (2, 5), (3, 2)]
    got = _run(S, pairs, 0.0, norm)
    a = _t(S.d1)
    pi, pdist, ppo = tensor_api.knn_match_pairs_tensors(a, a, S.c1, S.c2, pairs, norm)
    assert torch.equal(got[0], pi) and torch.equal(got[1].view(torch.int32), pdist.view(torch.int32)) and np.array_equal(got[2], ppo)
    assert _check(S, pairs, 0.0, norm, got) == [0] * len(pairs)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_keypoints(norm, bad):
    lv = np.array([0, 1, 2, 3, 4] + [6] * 70)
    a, b = _levels(norm, lv, 2)
    n2 = len(lv)
    base = np.c_[100.0 * np.arange(n2), 50.0 + np.zeros(n2)]; base[1] = base[0] + [1, 0]
    ka = base.copy(); ka[0, 0] = bad                                  # the anchor
    kc = base.copy(); kc[2, 1] = bad; kc[3] = bad                     # competing rows
    kb = base.copy(); kb[0] = bad; kb[2] = bad                        # both sides: inf - inf is NaN
    S = Stores([a], [b, b, b], [ka, kc, kb])
    pairs = [(0, 2), (0, 0), (0, 1), (0, 0)]
    got = _run(S, pairs, R, norm)
    _check(S, pairs, R, norm, got)
    idx = got[0].cpu().numpy()
    if np.isnan(bad):
        assert list(idx[2]) == [0, -1] and list(idx[4]) == [0, 4] and list(idx[6]) == [0, -1]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_descriptor_rows(bad):
    scenes = [fr.twin_scene(70 + i, n1, n2, 33, "l2", m) for i, (n1, n2, m) in enumerate([(7, 30, 3), (70, 130, 20)])]
    scenes[1][1][3, 5] = bad; scenes[1][1][120:, 0] = bad                           # a twinned train row and half of the twins
    scenes[1][0][9, 2] = bad
    needy = _check(_one_store(scenes), [(2, 3), (3, 3), (0, 1), (0, 3), (3, 1)], R, "l2")
    assert needy[0] > 0


@pytest.mark.parametrize("norm", NORMS)
def test_six_column_keypoints(norm):
    scenes = [fr.twin_scene(80 + i, n1, n2, _w(norm), norm, m) for i, (n1, n2, m) in enumerate([(7, 30, 3), (70, 130, 20)])]
    S = _one_store(scenes)
    rng = np.random.default_rng(2)
    S6 = Stores.single(S.D1, [np.c_[k, rng.normal(size=(len(k), 4))] for k in S.K2])
    assert S6.k2.shape[1] == 6
    assert _check(S6, [(2, 3), (0, 1), (3, 3)], R, norm)[:2] == [20, 3]


@pytest.mark.parametrize("norm", NORMS)
def test_second_stream_gives_the_same_bits(norm):
    import torch
    scenes = [fr.twin_scene(90 + i, n1, n2, _w(norm), norm, m) for i, (n1, n2, m) in enumerate([(7, 30, 3), (130, 200, 65), (5, 70, 2)])]
    S = _one_store(scenes)
    pairs = [(4, 5), (2, 3), (0, 1), (3, 3)]
    ref = _run(S, pairs, R, norm)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())
    a = _t(S.d1); k = _t(S.k2)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = tensor_api.knn_match_fginn_pairs_tensors(a, a, k, S.c1, S.c2, pairs, R, norm)
    s.synchronize()
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1].view(torch.int32), got[1].view(torch.int32))


# ---- the C entry points: stores that do not start at row 0 ----------------------------------------------------------------------------
def _p(x, t):
    return x.ctypes.data_as(C.POINTER(t))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kd", [2, 6])
def test_stores_whose_first_offset_is_above_zero(norm, kd):
    """rows in front of the first image, descriptors and keypoints alike, are never read (they hold NaN keypoints and other descriptors);
    mi_degensac_match_fginn_knn2_pairs_dev and the two match-and-verify forms against the calls on the stores cut to their images"""
    import torch
    w = _w(norm)
    scenes = [fr.twin_scene(110 + i, n1, n2, w, norm, m) for i, (n1, n2, m) in enumerate([(70, 130, 20), (7, 30, 3)])]
    S = _two_stores(scenes)
    rng = np.random.default_rng(3)
    k1 = np.c_[_grid(S.d1.shape[0]), rng.normal(size=(S.d1.shape[0], kd - 2))]
    k2 = np.c_[S.k2, rng.normal(size=(S.k2.shape[0], kd - 2))]
    pairs = [(1, 0), (0, 0), (1, 1), (0, 1)]
    prs = np.ascontiguousarray(pairs, np.int32); K = len(pairs)
    want_i, want_d, po = tensor_api.knn_match_fginn_pairs_tensors(_t(S.d1), _t(S.d2), _t(k2), S.c1, S.c2, pairs, R, norm)
    j1 = fr._rows(rng, 5, w, norm); j2 = fr._rows(rng, 12, w, norm)
    A = np.concatenate([j1, S.d1]); B = np.concatenate([j2, S.d2, j1])
    KA = np.concatenate([np.full((5, kd), np.nan), k1]); KB = np.concatenate([np.full((12, kd), np.nan), k2, np.full((5, kd), np.nan)])
    o1 = pr.offsets(S.c1) + 5; o2 = pr.offsets(S.c2) + 12
    n = int(po[-1])
    a, b, ka, kb = _t(A), _t(B), _t(KA), _t(KB)
    idx = torch.full((n, 2), -7, dtype=torch.int32, device=_dev()); dist = torch.full((n, 2), -7.0, dtype=torch.float32, device=_dev())
    L = _lib.lib(); st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mi_degensac_match_fginn_knn2_pairs_dev(CODE[norm], a.data_ptr(), b.data_ptr(), _p(o1, C.c_int64), 2, _p(o2, C.c_int64), 2, _p(prs, C.c_int32),
                                                  K, w, kb.data_ptr(), kd, R, 0, st, idx.data_ptr(), dist.data_ptr())
    assert rc == 0, L.mi_degensac_match_last_error()
    torch.cuda.synchronize()
    assert torch.equal(idx, want_i) and torch.equal(dist.view(torch.int32), want_d.view(torch.int32))
    # match and verify: the device form and the host-pointer form on the offset stores against the tensor call on the cut stores
    seeds = np.array([5, 6, 7, 8], np.uint32)
    kw = dict(model="H", max_iters=500, seeds=seeds, norm=norm, mutual=True)
    M, match, inl, stt, cnt, _ = tensor_api.match_and_verify_fginn_pairs_tensors(_t(k1), _t(k2), _t(S.d1), _t(S.d2), S.c1, S.c2, pairs, R, **kw)
    mp = _lib.MatchParams(CODE[norm], w, 0.9, True, R); prm = matcher.estimator_params("H", max_iters=500)
    dM = torch.zeros((K, 9), dtype=torch.float64, device=_dev()); dm = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    di = torch.full((n,), 7, dtype=torch.uint8, device=_dev()); ds = torch.zeros((K, 16), dtype=torch.int32, device=_dev())
    dseed = _t(seeds.view(np.int32)); hc = np.zeros(K, np.int32)
    rc = L.mi_degensac_match_verify_fginn_pairs_dev(1, C.byref(mp), a.data_ptr(), b.data_ptr(), _p(o1, C.c_int64), 2, _p(o2, C.c_int64), 2, ka.data_ptr(),
                                                    kb.data_ptr(), kd, _p(prs, C.c_int32), K, C.byref(prm), dseed.data_ptr(), 0, st, dM.data_ptr(),
                                                    dm.data_ptr(), di.data_ptr(), ds.data_ptr(), _p(hc, C.c_int32))
    assert rc == 0, L.mi_degensac_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dm, match) and torch.equal(di.bool(), inl) and np.array_equal(hc, cnt) and torch.equal(ds[:, DET], stt[:, DET])
    hM = np.zeros((K, 9)); hm = np.full(n, -7, np.int32); hi = np.full(n, 7, np.uint8); hs = np.zeros((K, 16), np.int32); hc2 = np.zeros(K, np.int32)
    rc = L.mi_degensac_match_verify_fginn_pairs(1, C.byref(mp), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), _p(o1, C.c_int64), 2,
                                                _p(o2, C.c_int64), 2, _p(KA, C.c_double), _p(KB, C.c_double), kd, _p(prs, C.c_int32), K, C.byref(prm),
                                                _p(seeds, C.c_uint32), 0, _p(hM, C.c_double), _p(hm, C.c_int32), _p(hi, C.c_uint8), _p(hs, C.c_int32),
                                                _p(hc2, C.c_int32))
    assert rc == 0, L.mi_degensac_last_error()
    assert np.array_equal(hm, match.cpu().numpy()) and np.array_equal(hi.astype(bool), inl.cpu().numpy()) and np.array_equal(hc2, cnt)
    assert np.array_equal(hM, dM.cpu().numpy()) and cnt.sum() > 0


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _collection(model):
    """The three views of tests/test_gpu_match_pairs._scene plus its 3-row image, every third keypoint of each view twinned: one more
    row 1.5 px away with a near-equal descriptor, the rows of an image shuffled.  Returns (xy [N, 2], k6 [N, 6], desc [N, 64], counts)."""
    from tests.test_gpu_match_pairs import _scene
    xy, _, _, desc, counts = _scene(model)
    rng = np.random.default_rng(23)
    o = pr.offsets(counts)
    X, D = [], []
    for i, n in enumerate(counts):
        x, d = xy[o[i]:o[i + 1]], desc[o[i]:o[i + 1]]
        tw = np.arange(0, n, 3) if n > 3 else np.zeros(0, np.int64)
        x = np.r_[x, x[tw] + [1.5, 0.0]]; d = np.r_[d, d[tw] + 0.002 * rng.normal(size=(len(tw), 64)).astype(np.float32)]
        perm = rng.permutation(len(x))
        X.append(x[perm]); D.append(d[perm])
    xy = np.concatenate(X); desc = np.concatenate(D)
    k6 = np.c_[xy, rng.normal(size=(len(xy), 4))]
    return xy, k6, desc, [len(x) for x in X]


SCENE_PAIRS = [(2, 1), (1, 0), (0, 1), (3, 0), (0, 0), (1, 0), (1, 2)]
SEEDS = [11, 4000000000, 7, 9, 123456, 4000000000, 3]


def _tentatives_by_the_restatement(xy, desc, counts, pairs, r, mutual):
    """(a): match of every entry from fginn_ref.fginn, its keep and, with mutual, the plain reverse nearest neighbour"""
    o = pr.offsets(counts); out = []
    for i, j in pairs:
        a, b = desc[o[i]:o[i + 1]], desc[o[j]:o[j + 1]]
        oi, od, _, _ = fr.fginn(a, b, xy[o[j]:o[j + 1]], r, "l2")
        keep = fr.keep(oi, od, 0.9)
        if mutual:
            back = mo.top2(fr.dmat(b, a, "l2"))[0][:, 0]
            keep &= back[np.clip(oi[:, 0], 0, None)] == np.arange(len(a))
        out.append(np.where(keep, oi[:, 0], -1))
    return np.concatenate(out)


def _verify_both(kps, desc, counts, pairs, r, **kw):
    import torch
    tk, td = _t(kps), _t(desc)
    got = tensor_api.match_and_verify_fginn_pairs_tensors(tk, tk, td, td, counts, counts, pairs, r, **kw)
    (ek1, ed1), (ek2, ed2), c1, c2, po = pr.expand((kps, desc), counts, (kps, desc), counts, pairs)
    want = tensor_api.match_and_verify_batch_tensors(_t(ek1), _t(ek2), _t(ed1), _t(ed2), c1, c2, fginn_th=r, **kw)
    torch.cuda.synchronize()
    M, match, inl, st, cnt, gpo = got
    assert np.array_equal(gpo, po) and gpo.dtype == np.int64
    assert torch.equal(M.contiguous().view(torch.int64), want[0].contiguous().view(torch.int64))      # the models' bits
    assert torch.equal(match, want[1]) and torch.equal(inl, want[2])
    assert torch.equal(st[:, DET], want[3][:, DET])
    assert isinstance(cnt, np.ndarray) and np.array_equal(cnt, want[4])
    return got


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model", ["F", "H"])
def test_pipeline_equals_the_batched_call_and_the_restatement(model, mutual):
    import torch
    xy, k6, desc, counts = _collection(model)
    kw = dict(model=model, mutual=mutual, max_iters=2000, seeds=SEEDS)
    M, match, inl, st, cnt, po = _verify_both(xy, desc, counts, SCENE_PAIRS, R, **kw)
    match = match.cpu().numpy()
    assert np.array_equal(match, _tentatives_by_the_restatement(xy, desc, counts, SCENE_PAIRS, R, mutual))
    assert [int((match[po[p]:po[p + 1]] >= 0).sum()) for p in range(len(SCENE_PAIRS))] == list(cnt)
    tk, td = _t(xy), _t(desc)
    plain = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, **kw)
    need = 8 if model == "F" else 4
    assert cnt[3] < need and not M[3].any()                                                           # the short entry
    assert all(cnt[p] > plain[4][p] + 10 for p in (0, 1, 2, 6)) and all(M[p].any() for p in (0, 1, 2, 6))      # the rule changes the tentatives
    assert torch.equal(M[1], M[5]) and np.array_equal(match[po[1]:po[2]], match[po[5]:po[6]])         # the repeat has the same seed
    # [n, 6] keypoint rows give the same matches (only x, y are read by the rule)
    got6 = _verify_both(k6, desc, counts, SCENE_PAIRS, R, **kw)
    assert np.array_equal(got6[1].cpu().numpy(), match)


def test_numpy_entry_point_with_one_and_two_stores():
    xy, k6, desc, counts = _collection("F")
    o = pr.offsets(counts)
    kl = [xy[o[i]:o[i + 1]] for i in range(4)]; dl = [desc[o[i]:o[i + 1]] for i in range(4)]
    tk, td = _t(xy), _t(desc)
    for mutual in (False, True):
        kw = dict(model="F", mutual=mutual, max_iters=2000, seeds=SEEDS)
        M, match, inl, st, cnt, po = tensor_api.match_and_verify_fginn_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, R, **kw)
        match = match.cpu().numpy(); inl = inl.cpu().numpy(); st = st.cpu().numpy()
        for second in (dict(), dict(kps2_list=kl, desc2_list=dl)):
            Mh, mh, ih = matcher.match_and_verify_fginn_pairs(kl, dl, SCENE_PAIRS, R, **second, **kw)
            sth = pd.last_stats()
            assert np.array_equal(M.cpu().numpy(), Mh)
            for p in range(len(SCENE_PAIRS)):
                assert np.array_equal(match[po[p]:po[p + 1]], mh[p]) and np.array_equal(inl[po[p]:po[p + 1]], ih[p]), p
                assert [sth[p][k] for k in ("samples", "lo_runs", "I")] == list(st[p, [0, 1, 3]]) and sth[p]["tentatives"] == cnt[p], p
    # two different stores: the train images come from a database of images 1 and 2
    pairs2 = [(0, 0), (2, 1), (3, 0), (1, 1)]
    M, match, inl, st, cnt, po = tensor_api.match_and_verify_fginn_pairs_tensors(tk, _t(xy[o[1]:o[3]]), td, _t(desc[o[1]:o[3]]), counts, counts[1:3], pairs2,
                                                                                 R, model="F", max_iters=2000, seeds=SEEDS[:4])
    Mh, mh, ih = matcher.match_and_verify_fginn_pairs(kl, dl, pairs2, R, model="F", max_iters=2000, seeds=SEEDS[:4], kps2_list=kl[1:3], desc2_list=dl[1:3])
    assert np.array_equal(M.cpu().numpy(), Mh) and Mh[0].any()
    match = match.cpu().numpy(); inl = inl.cpu().numpy()
    for p in range(4):
        assert np.array_equal(match[po[p]:po[p + 1]], mh[p]) and np.array_equal(inl[po[p]:po[p + 1]], ih[p]), p


def test_match_and_verify_on_a_second_stream():
    import torch
    xy, k6, desc, counts = _collection("F")
    kw = dict(model="F", mutual=True, max_iters=2000, seeds=SEEDS)
    tk, td = _t(xy), _t(desc)
    want = tensor_api.match_and_verify_fginn_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, R, **kw)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(s):
        got = tensor_api.match_and_verify_fginn_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, R, **kw)
    assert np.array_equal(got[4], want[4])                                                            # host values, before any wait here
    s.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and torch.equal(got[3][:, DET], want[3][:, DET])


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model", ["F", "H"])
def test_chain_into_guided_matching(model, mutual):
    """match_and_verify_fginn_pairs_tensors, then guided_match_pairs_tensors on the models it returned, equals
    match_and_verify_batch_tensors(fginn_th=, guided=True) on the expansion with the same seeds"""
    import torch
    xy, k6, desc, counts = _collection(model)
    tk, td = _t(xy), _t(desc)
    kw = dict(model=model, mutual=mutual, max_iters=2000, seeds=SEEDS)
    Mu, match, inl, stats, cnt, po = tensor_api.match_and_verify_fginn_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, R, **kw)
    gm, gi, gd, gpo = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, Mu, model=model, mutual=mutual)
    (ek1, ed1), (ek2, ed2), c1, c2, want_po = pr.expand((xy, desc), counts, (xy, desc), counts, SCENE_PAIRS)
    want = tensor_api.match_and_verify_batch_tensors(_t(ek1), _t(ek2), _t(ed1), _t(ed2), c1, c2, guided=True, fginn_th=R, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(gpo, want_po) and np.array_equal(po, want_po)
    assert torch.equal(Mu.contiguous().view(torch.int64), want[0].contiguous().view(torch.int64))
    assert torch.equal(match, want[1]) and torch.equal(gm, want[5])
    gm = gm.cpu().numpy()
    for p in (0, 1, 2, 6):
        assert (gm[po[p]:po[p + 1]] >= 0).sum() >= 20, p
