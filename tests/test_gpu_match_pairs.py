"""GPU: the pair-list calls (include/mi_degensac.h mi_degensac_match_*_pairs*): descriptors and keypoints stored once per image, a
list of (i, j) image indices.  Equality only: every case compares the pair-list call with the batched call on the expansion of
tests/pairs_ref.py (pair p's rows copied out of the stores), bit for bit.  Both run one kernel under two row tables, so those cases check
the tables; the kernel itself is anchored against the dense single-pair kernel and the numpy oracle, entry by entry."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher, synthetic as syn, tensor_api
from tests import matcher_ref as mr, pairs_ref as pr

pytestmark = pytest.mark.gpu

# every stats column but the two device clock readings (ticks_best, ticks_total), which differ between any two runs of one call
DET = [c for c in range(16) if c not in (12, 13)]
# image sizes: output and store bases that are no multiples of 64, partly filled query tiles, train sets shorter than one tile and
# longer than two, an empty image; image 7 takes part in no pair
SIZES = [0, 1, 2, 63, 64, 65, 129, 10]
# descending order, (i, j) with (j, i), a self pair, a repeated pair, the empty image as query side and as train side
PAIRS = [(6, 5), (5, 6), (4, 4), (6, 5), (3, 1), (2, 6), (0, 6), (6, 0), (1, 2), (5, 3), (6, 6), (0, 0)]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _descs(seed, n, dim, norm):
    """n descriptor rows of `dim` elements: a third of the rows are noisy copies of other rows of the store, rows 70 and 75 exact
    duplicates of rows 3 and 5 (ties across images)"""
    rng = np.random.default_rng([seed, n, dim])
    src = rng.integers(0, max(n, 1), n)
    if norm == "l2":
        d = rng.normal(size=(n, dim)).astype(np.float32)
        c = d[src] + 0.05 * rng.normal(size=(n, dim)).astype(np.float32)
    else:
        d = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        c = d[src] ^ (rng.random((n, dim)) < 0.03).astype(np.uint8)
    take = rng.random(n) < 0.33
    d[take] = c[take]
    if n > 80:
        d[70] = d[3]; d[75] = d[5]
    return d


def _bits(t):
    import torch
    return t.view(torch.int32)


def _knn_both(d1, c1, d2, c2, pairs, norm):
    """(pair-list result, batched result on the expansion, pair_offsets): device tensors"""
    import torch
    a = _t(d1); b = a if d2 is d1 else _t(d2)                            # one store: the same tensor on both sides
    idx, dist, po = tensor_api.knn_match_pairs_tensors(a, b, c1, c2, pairs, norm)
    (e1,), (e2,), k1, k2, want_po = pr.expand((d1,), c1, (d2,), c2, pairs)
    ridx, rdist = tensor_api.knn_match_batch_tensors(_t(e1), _t(e2), k1, k2, norm)
    torch.cuda.synchronize()
    assert isinstance(po, np.ndarray) and po.dtype == np.int64 and np.array_equal(po, want_po)
    assert idx.shape == ridx.shape and dist.shape == rdist.shape
    assert torch.equal(idx, ridx) and torch.equal(_bits(dist), _bits(rdist))
    return idx, dist, (k1, k2)


# 1 word, one full chunk of 64 words, a chunk and one word; uint8 L2 at 4 / 128 / 256 bytes = the NS 2 / 4 / 8 instances
WIDTHS = [("l2", 1), ("l2", 64), ("l2", 65), ("hamming", 4), ("hamming", 256), ("hamming", 260), ("l2_u8", 4), ("l2_u8", 128), ("l2_u8", 256)]


@pytest.mark.parametrize("norm,dim", WIDTHS)
def test_knn2_equals_the_batched_call_on_the_expansion(norm, dim):
    d = _descs(1, sum(SIZES), dim, norm)
    idx, dist, (k1, k2) = _knn_both(d, SIZES, d, SIZES, PAIRS, norm)
    t_chunk, splits = mr.batch_split(list(k1), list(k2), _cus())
    assert splits > 1                                                    # few pairs: the train split is taken
    idx = idx.cpu().numpy()
    po = pr.offsets(k1)
    for p, (i, j) in enumerate(PAIRS):                                   # indices are local to image j; -1 exactly where it is too small
        blk = idx[po[p]:po[p + 1]]
        assert blk.shape[0] == SIZES[i] and (blk < max(SIZES[j], 1)).all()
        assert ((blk[:, 0] == -1) == (SIZES[j] < 1)).all() and ((blk[:, 1] == -1) == (SIZES[j] < 2)).all()
    self_pair = idx[po[2]:po[3]]                                         # (4, 4): every row finds itself (or an exact duplicate before it)
    assert (self_pair[:, 0] >= 0).all() and (self_pair[:, 0] <= np.arange(SIZES[4])).all()


@pytest.mark.parametrize("norm,dim", [("l2", 8), ("hamming", 8), ("l2_u8", 8)])
def test_knn2_many_pairs_take_no_train_split(norm, dim):
    sizes = [129, 65, 200]
    rng = np.random.default_rng(7)
    pairs = rng.integers(0, 3, (300, 2))
    d = _descs(2, sum(sizes), dim, norm)
    _, _, (k1, k2) = _knn_both(d, sizes, d, sizes, pairs, norm)
    assert sum((c + 63) // 64 for c in k1) >= 2 * _cus()
    assert mr.batch_split(list(k1), list(k2), _cus())[1] == 1            # the tiles cover the CUs twice: one split


def _entries_equal_dense_kernel_and_oracle(d, sizes, pairs, entries, norm):
    """list entries `entries` of the pair-list 2-NN over the one store d against knn_match_tensors (the dense single-pair kernel) and the
    numpy oracle on the entry's two images: idx equal, dist equal by bits"""
    import torch
    a = _t(d)
    idx, dist, po = tensor_api.knn_match_pairs_tensors(a, a, sizes, sizes, pairs, norm)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy().view(np.uint32)
    o = pr.offsets(sizes)
    for p in entries:
        i, j = pairs[p]
        q, t = d[o[i]:o[i + 1]], d[o[j]:o[j + 1]]
        gi, gd = idx[po[p]:po[p + 1]], dist[po[p]:po[p + 1]]
        assert gi.shape == (sizes[i], 2)
        di, dd = tensor_api.knn_match_tensors(_t(q), _t(t), norm)
        assert np.array_equal(gi, di.cpu().numpy()) and np.array_equal(gd, dd.cpu().numpy().view(np.uint32)), (p, i, j)
        oi, od = mo.knn2(q, t, "l2" if norm == "l2_u8" else norm)       # uint8 rows under L2: the float32 path on the same values
        assert np.array_equal(gi, oi) and np.array_equal(gd, od.view(np.uint32)), (p, i, j)


ANCHOR_WIDTHS = [("l2", 65), ("hamming", 8), ("l2_u8", 128)]


@pytest.mark.parametrize("norm,dim", ANCHOR_WIDTHS)
def test_knn2_split_list_equals_the_dense_kernel_and_the_oracle(norm, dim):
    k1 = [SIZES[i] for i, _ in PAIRS]; k2 = [SIZES[j] for _, j in PAIRS]
    assert mr.batch_split(k1, k2, _cus())[1] > 1                         # the train split is taken
    _entries_equal_dense_kernel_and_oracle(_descs(11, sum(SIZES), dim, norm), SIZES, PAIRS, range(len(PAIRS)), norm)


@pytest.mark.parametrize("norm,dim", ANCHOR_WIDTHS)
def test_knn2_unsplit_list_equals_the_dense_kernel_and_the_oracle(norm, dim):
    sizes = [129, 65, 200]
    pairs = np.random.default_rng(7).integers(0, 3, (300, 2))            # the list of test_knn2_many_pairs_take_no_train_split
    k1 = [sizes[i] for i, _ in pairs]; k2 = [sizes[j] for _, j in pairs]
    assert mr.batch_split(k1, k2, _cus())[1] == 1
    sample = np.random.default_rng(8).choice(len(pairs), 20, replace=False)
    _entries_equal_dense_kernel_and_oracle(_descs(12, sum(sizes), dim, norm), sizes, pairs, sample, norm)


@pytest.mark.parametrize("norm,dim", [("l2", 33), ("hamming", 32), ("l2_u8", 32)])
def test_knn2_single_pair_and_two_stores(norm, dim):
    c1 = [70, 0, 5]; c2 = [3, 131]
    d1 = _descs(3, sum(c1), dim, norm); d2 = _descs(4, sum(c2), dim, norm)
    d2[3:3 + 70:2] = d1[0:70:2]                                          # true matches between the stores
    _knn_both(d1, c1, d2, c2, [(0, 1)], norm)                            # K = 1
    _knn_both(d1, c1, d2, c2, [(2, 1), (0, 0), (1, 1), (0, 1), (2, 0), (0, 1)], norm)
    _knn_both(d2, c2, d1, c1, [(1, 0), (1, 1), (0, 2)], norm)            # the stores the other way round


@pytest.mark.parametrize("norm,dim", [("l2", 65), ("hamming", 8), ("l2_u8", 128)])
def test_knn2_stores_whose_first_offset_is_above_zero(norm, dim):
    """the C ABI takes store offsets that do not start at 0: rows in front of the first image are never read"""
    import torch
    code = {"l2": 0, "hamming": 1, "l2_u8": 4}[norm]
    d = _descs(5, sum(SIZES), dim, norm)
    want_idx, want_dist, _ = tensor_api.knn_match_pairs_tensors(_t(d), _t(d), SIZES, SIZES, PAIRS, norm)
    junk1 = _descs(6, 5, dim, norm); junk2 = _descs(7, 12, dim, norm)
    a = _t(np.concatenate([junk1, d])); b = _t(np.concatenate([junk2, d, junk1]))
    o1 = pr.offsets(SIZES) + 5; o2 = pr.offsets(SIZES) + 12
    prs = np.ascontiguousarray(PAIRS, np.int32)
    n = want_idx.shape[0]
    idx = torch.full((n, 2), -7, dtype=torch.int32, device=_dev()); dist = torch.full((n, 2), -7.0, dtype=torch.float32, device=_dev())
    lp = C.POINTER(C.c_int64)
    rc = _lib.lib().mi_degensac_match_knn2_pairs_dev(code, a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), len(SIZES), o2.ctypes.data_as(lp),
                                                     len(SIZES), prs.ctypes.data_as(C.POINTER(C.c_int32)), len(prs), dim, 0,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream), idx.data_ptr(), dist.data_ptr())
    assert rc == 0, _lib.lib().mi_degensac_match_last_error()
    torch.cuda.synchronize()
    assert torch.equal(idx, want_idx) and torch.equal(_bits(dist), _bits(want_dist))


# ---- decisions and the pipeline ----
@functools.lru_cache(maxsize=None)
def _scene(model):
    """Three images of about 150 keypoints that see one scene (image 1 = the second view of image 0, image 2 = image 1 under a similarity,
    so every pair of them has a model of either kind) and image 3 with 3 rows (below 4 tentatives).  Returns (xy [N, 2] float64, k4 [N, 4]
    float32, k6 [N, 6] float64, desc [N, 64] float32, counts)."""
    rng = np.random.default_rng(17)
    n = 150
    if model == "F":
        p1, p2, lab, _ = syn.two_view_fundamental(n, 0.6, 0.1, seed=21)
    else:
        p1, p2, lab, _ = syn.homography_pairs(n, 0.6, 0.5, seed=22)
    d0 = rng.normal(size=(n, 64)).astype(np.float32)

    def view(pts, perm, keep):
        d = d0 + 0.15 * rng.normal(size=d0.shape).astype(np.float32)
        d[~lab] = rng.normal(size=((~lab).sum(), 64)).astype(np.float32)
        return pts[perm][:keep], d[perm][:keep]
    c, s = np.cos(0.2), np.sin(0.2)
    p3 = 1.1 * p2 @ np.array([[c, s], [-s, c]]) + np.array([30.0, -12.0])
    imgs = [(p1, d0), view(p2, rng.permutation(n), 146), view(p3, rng.permutation(n), 139), view(p1, np.arange(n), 3)]
    xy = np.concatenate([x for x, _ in imgs]); desc = np.concatenate([d for _, d in imgs])
    N = len(xy)
    k4 = np.c_[xy, rng.uniform(2, 9, N), rng.uniform(0, 360, N)].astype(np.float32)
    a = np.radians(k4[:, 3].astype(np.float64)); sz = k4[:, 2].astype(np.float64)
    k6 = np.c_[k4[:, :2].astype(np.float64), sz * np.cos(a), sz * np.sin(a), -sz * np.sin(a), sz * np.cos(a)]
    return xy, k4, k6, desc, [len(x) for x, _ in imgs]


# both orders, the self pair, a repeat, the short pair (3 query rows) next to eligible ones
SCENE_PAIRS = [(0, 1), (1, 0), (1, 2), (3, 0), (0, 0), (0, 1)]
SEEDS = [11, 4000000000, 7, 9, 123456, 11]


def _verify_both(kps, desc, counts, pairs, **kw):
    import torch
    tk, td = _t(kps), _t(desc)
    got = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, counts, counts, pairs, **kw)
    (ek1, ed1), (ek2, ed2), c1, c2, po = pr.expand((kps, desc), counts, (kps, desc), counts, pairs)
    want = tensor_api.match_and_verify_batch_tensors(_t(ek1), _t(ek2), _t(ed1), _t(ed2), c1, c2, **kw)
    torch.cuda.synchronize()
    M, match, inl, st, cnt, gpo = got
    assert np.array_equal(gpo, po) and gpo.dtype == np.int64
    assert torch.equal(M.contiguous().view(torch.int64), want[0].contiguous().view(torch.int64))      # the models' bits
    assert torch.equal(match, want[1]) and torch.equal(inl, want[2])
    assert torch.equal(st[:, DET], want[3][:, DET])
    assert isinstance(cnt, np.ndarray) and np.array_equal(cnt, want[4])
    return got


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("form", ["xy", "laf6", "kpts4"])
@pytest.mark.parametrize("model", ["F", "H"])
def test_match_and_verify_equals_the_batched_call_on_the_expansion(model, form, mutual):
    xy, k4, k6, desc, counts = _scene(model)
    kps = {"xy": xy, "laf6": k6, "kpts4": k4}[form]
    M, match, inl, st, cnt, po = _verify_both(kps, desc, counts, SCENE_PAIRS, model=model, mutual=mutual, max_iters=2000, seeds=SEEDS)
    need = 8 if model == "F" else 4
    M = M.cpu().numpy(); inl = inl.cpu().numpy(); match = match.cpu().numpy(); st = st.cpu().numpy()
    assert cnt[3] < need and not M[3].any() and not st[3].any() and not inl[po[3]:po[4]].any()      # the short pair
    for p in (0, 1, 2):                                                                               # eligible, with a model and inliers
        assert cnt[p] >= 40 and M[p].any() and inl[po[p]:po[p + 1]].sum() >= need and st[p, 0] > 0, (p, cnt)
    assert cnt[4] == counts[0] and (match[po[4]:po[5]] == np.arange(counts[0])).all()               # the self pair: every row matches itself
    assert np.array_equal(M[0], M[5]) and np.array_equal(match[po[0]:po[1]], match[po[5]:po[6]])     # the repeat has the same seed
    for p in range(len(SCENE_PAIRS)):
        assert cnt[p] == (match[po[p]:po[p + 1]] >= 0).sum()


@pytest.mark.parametrize("norm", ["hamming", "l2_u8"])
def test_decisions_on_uint8_rows_with_and_without_mutual(norm):
    """the ratio test and the mutual check on the tiling store: the self pairs and the both-orders pairs are where the back block's
    bases can go wrong; default seeds (parallel.pair_seeds(0, K) in both calls)"""
    d = _descs(8, sum(SIZES), 32, norm)
    rng = np.random.default_rng(9)
    kps = rng.uniform(0, 500, (sum(SIZES), 2))
    kept = 0
    for mutual in (False, True):
        got = _verify_both(kps, d, SIZES, PAIRS, model="H", mutual=mutual, max_iters=500, norm=norm)
        kept += int(got[4].sum())
    assert kept > 0


def test_numpy_entry_point_equals_the_tensor_one():
    import pydegensac_amd as pd
    xy, k4, k6, desc, counts = _scene("F")
    o = pr.offsets(counts)
    kl = [xy[o[i]:o[i + 1]] for i in range(4)]; dl = [desc[o[i]:o[i + 1]] for i in range(4)]
    for mutual in (False, True):
        kw = dict(model="F", mutual=mutual, max_iters=2000, seeds=SEEDS)
        M, match, inl, st, cnt, po = tensor_api.match_and_verify_pairs_tensors(_t(xy), _t(xy), _t(desc), _t(desc), counts, counts, SCENE_PAIRS, **kw)
        Mh, mh, ih = matcher.match_and_verify_pairs(kl, dl, SCENE_PAIRS, **kw)
        sth = pd.last_stats()
        assert np.array_equal(M.cpu().numpy(), Mh)
        match = match.cpu().numpy(); inl = inl.cpu().numpy(); st = st.cpu().numpy()
        for p in range(len(SCENE_PAIRS)):
            assert np.array_equal(match[po[p]:po[p + 1]], mh[p]) and np.array_equal(inl[po[p]:po[p + 1]], ih[p]), p
            assert [sth[p][k] for k in ("samples", "lo_runs", "I")] == list(st[p, [0, 1, 3]]) and sth[p]["tentatives"] == cnt[p], p
    # two stores: the database images given as a second pair of lists
    pairs2 = [(0, 0), (2, 1), (3, 0), (1, 1)]
    M, match, inl, st, cnt, po = tensor_api.match_and_verify_pairs_tensors(_t(xy), _t(xy[o[1]:o[3]]), _t(desc), _t(desc[o[1]:o[3]]), counts, counts[1:3],
                                                                           pairs2, model="F", max_iters=2000, seeds=SEEDS[:4])
    Mh, mh, ih = matcher.match_and_verify_pairs(kl, dl, pairs2, model="F", max_iters=2000, seeds=SEEDS[:4], kps2_list=kl[1:3], desc2_list=dl[1:3])
    assert np.array_equal(M.cpu().numpy(), Mh) and Mh[0].any()
    match = match.cpu().numpy(); inl = inl.cpu().numpy()
    for p in range(4):
        assert np.array_equal(match[po[p]:po[p + 1]], mh[p]) and np.array_equal(inl[po[p]:po[p + 1]], ih[p]), p


def _stats_rows(dicts):
    """last_stats() back to the stats columns (column 15 with its flag bits)"""
    rows = np.array([[d[k] for k in _lib.STAT_NAMES] for d in dicts])
    rows[:, 15] += np.array([d["set_aside"] << 8 | d["streamed"] << 9 | d["discarded"] << 10 | d["rerun"] << 11 for d in dicts])
    return rows


@pytest.mark.parametrize("mutual", [False, True])
def test_host_forms_with_both_sides_naming_one_store(mutual):
    """the host-pointer forms share their staging: the ragged batch uploads both sides whatever they are, the list uploads a store named
    twice only once.  Both equal the tensor forms: models, match, inlier and every stats column but the clock readings."""
    import pydegensac_amd as pd
    xy, k4, k6, desc, counts = _scene("F")
    o = pr.offsets(counts)
    kl = [xy[o[i]:o[i + 1]] for i in range(4)]; dl = [desc[o[i]:o[i + 1]] for i in range(4)]
    kw = dict(model="F", mutual=mutual, max_iters=2000)
    tk, td = _t(xy), _t(desc)

    def same(host, stats, M, match, inl, st, po):
        assert np.array_equal(M.cpu().numpy(), host[0])
        match = match.cpu().numpy(); inl = inl.cpu().numpy()
        for p in range(len(po) - 1):
            assert np.array_equal(match[po[p]:po[p + 1]], host[1][p]) and np.array_equal(inl[po[p]:po[p + 1]], host[2][p]), p
        assert np.array_equal(_stats_rows(stats)[:, DET], st.cpu().numpy()[:, DET])

    # the ragged batch: pair p = (image p, image p), one list object on both sides
    M, match, inl, st, cnt = tensor_api.match_and_verify_batch_tensors(tk, tk, td, td, counts, counts, seeds=SEEDS[:4], **kw)
    host = matcher.match_and_verify_batch(kl, kl, dl, dl, seeds=SEEDS[:4], **kw)
    same(host, pd.last_stats(), M, match, inl, st, o)
    assert list(cnt) == counts                                           # every row matches itself
    # the list: one store, then the same store given again as the second one
    M, match, inl, st, cnt, po = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, seeds=SEEDS, **kw)
    for second in (dict(), dict(kps2_list=kl, desc2_list=dl)):
        host = matcher.match_and_verify_pairs(kl, dl, SCENE_PAIRS, seeds=SEEDS, **second, **kw)
        same(host, pd.last_stats(), M, match, inl, st, po)


def test_non_default_stream_and_one_synchronisation():
    """on a side stream the outputs are valid after ONE stream.synchronize() (the call enqueues everything after its read of the counts),
    and the tentative counts come back as host values"""
    import torch
    xy, k4, k6, desc, counts = _scene("F")
    kw = dict(model="F", mutual=True, max_iters=2000, seeds=SEEDS)
    tk, td = _t(xy), _t(desc)
    want = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, **kw)
    widx, wdist, _ = tensor_api.knn_match_pairs_tensors(td, td, counts, counts, SCENE_PAIRS)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(s):
        got = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, **kw)
        idx, dist, _ = tensor_api.knn_match_pairs_tensors(td, td, counts, counts, SCENE_PAIRS)
    assert isinstance(got[4], np.ndarray) and got[4].dtype == np.int64 and np.array_equal(got[4], want[4])     # host values, before any wait here
    s.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert torch.equal(got[3][:, DET], want[3][:, DET])
    assert torch.equal(idx, widx) and torch.equal(_bits(dist), _bits(wdist))
    po = got[5]; match = got[1].cpu().numpy()
    assert [int((match[po[p]:po[p + 1]] >= 0).sum()) for p in range(len(SCENE_PAIRS))] == list(got[4])
