"""GPU: the dense matcher (mi_matcher.hip) at the edges of its tiling — descriptor widths that cross the 64-word LDS chunk unevenly,
row counts on both sides of the 64-row tiles, train splits that are short or empty, ties across tile / split / chunk edges — and the
non-finite rule.  Every case runs three paths (matcher.knn_match, tensor_api.knn_match_batch_tensors with the pair as the middle
one of three so that its offsets are not zero, matcher.match_snn with mutual off and on), asserts bit equality with
oracle/matcher_np.py, and — independently of that restatement — the float64 conditions of tests/matcher_ref.py."""
import numpy as np
import pytest

from oracle import matcher_np as mo
from pydegensac_amd import matcher, tensor_api
from tests import matcher_ref as mr

pytestmark = pytest.mark.gpu


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _pad4(x):
    return np.pad(x, ((0, 0), (0, (-x.shape[1]) % 4))) if x.dtype == np.uint8 else x


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _batched(a, b, family, left, right, seed=11):
    """knn_match_batch_tensors on (left pair, this pair, right pair): this pair's rows, and the neighbours checked on the way"""
    dim = a.shape[1]
    la, lb = mr.descs(seed, left[0], left[1], dim, family); ra, rb = mr.descs(seed + 1, right[0], right[1], dim, family)
    A = _pad4(np.concatenate([la, a, ra])); B = _pad4(np.concatenate([lb, b, rb]))
    c1 = [len(la), len(a), len(ra)]; c2 = [len(lb), len(b), len(rb)]
    idx, dist = tensor_api.knn_match_batch_tensors(_t(A), _t(B), c1, c2)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    norm = "hamming" if a.dtype == np.uint8 else "l2"
    o = np.concatenate([[0], np.cumsum(c1)])
    for p, (x, y) in enumerate([(la, lb), (a, b), (ra, rb)]):
        ri, rd = mo.knn2(x, y, norm)
        assert np.array_equal(idx[o[p]:o[p + 1]], ri), ("batched path, pair", p)
        assert np.array_equal(_bits(dist[o[p]:o[p + 1]]), _bits(rd)), ("batched path, pair", p)
    return idx[o[1]:o[2]], dist[o[1]:o[2]]


def _three_paths(a, b, family, left=mr.LEFT, right=mr.RIGHT, exact=True):
    norm = "hamming" if family == "hamming" else "l2"
    ri, rd = mo.knn2(a, b, norm)
    idx, dist = matcher.knn_match(a, b, norm)
    assert np.array_equal(idx, ri), ("single-pair path", np.flatnonzero((idx != ri).any(1))[:5])
    assert np.array_equal(_bits(dist), _bits(rd)), "single-pair path"
    bi, bd = _batched(a, b, family, left, right)
    assert np.array_equal(bi, idx) and np.array_equal(_bits(bd), _bits(dist)), "the two paths split the train set differently and must agree"
    for mutual in (False, True):
        q, t, d = matcher.match_snn(a, b, 0.9, mutual, norm)
        rq, rt, rdd = mo.match_snn(a, b, 0.9, mutual, norm)
        assert np.array_equal(q, rq) and np.array_equal(t, rt) and np.array_equal(_bits(d), _bits(rdd)), ("match_snn", mutual)
    if exact:
        mr.check_knn2_against_exact(idx, dist, a, b, norm)
        mr.check_knn2_against_exact(bi, bd, a, b, norm)
    return idx, dist


# ---- widths: a partly filled chunk after a full one (65, 100, 129, 200), more than two chunks (256, 512), one to three words ----
@pytest.mark.parametrize("family", mr.L2_FAMILIES)
@pytest.mark.parametrize("dim", mr.L2_DIMS)
def test_width_sweep_l2(dim, family):
    a, b = mr.descs(1, *mr.WIDTH_SHAPE, dim, family)
    chunks, last = -(-dim // 64), dim - 64 * ((dim - 1) // 64)       # LDS chunks of 64 words, words in the last one
    if dim in (65, 100, 129, 200):
        assert chunks >= 2 and last < 64                              # a partly filled chunk after a full one
    if dim in (256, 512):
        assert chunks > 2 and last == 64
    _three_paths(a, b, family)


@pytest.mark.parametrize("dim", [1, 3, 65, 129, 512])
def test_width_sweep_l2_subnormal_squares_bit_exact_only(dim):
    """1e-20 scale: every fp32 square is subnormal or zero.  The relative bound g does not hold once terms underflow, so only the
    bit-exact comparison with numpy runs: it fails if the kernel flushes denormals where numpy does not."""
    a, b = mr.descs(1, *mr.WIDTH_SHAPE, dim, "subnormal")
    with np.errstate(under="ignore"):
        sq = (a[:, None, :1] - b[None, :, :1]) ** 2
    assert (sq < np.finfo(np.float32).tiny).all() and (sq > 0).any()           # the family is what it claims
    _three_paths(a, b, "subnormal", exact=False)


@pytest.mark.parametrize("nbytes", mr.HAMMING_BYTES)
def test_width_sweep_hamming_and_padding(nbytes):
    """bytes -> words: 1..4 bytes one word, 252 / 256 bytes 63 / 64 words (one chunk), 260 a second chunk with one word, 512 two
    chunks.  matcher._prep pads rows to whole 32-bit words with zero bytes on both sides, which adds no differing bit: the distances
    equal the exact popcount of the unpadded rows (check_knn2_against_exact), padded by the caller or by the package."""
    a, b = mr.descs(2, *mr.WIDTH_SHAPE, nbytes, "hamming")
    idx, dist = _three_paths(a, b, "hamming")
    pi, pd = matcher.knn_match(_pad4(a), _pad4(b), "hamming")
    assert np.array_equal(pi, idx) and np.array_equal(pd, dist)
    wide = (-nbytes) % 4 + 4                                          # more zero words than needed change nothing either
    pi, pd = matcher.knn_match(np.pad(a, ((0, 0), (0, wide))), np.pad(b, ((0, 0), (0, wide))), "hamming")
    assert np.array_equal(pi, idx) and np.array_equal(pd, dist)


# ---- rows on both sides of the 64-row tiles, at a width with a partial second chunk ----
@pytest.mark.parametrize("n2", mr.ROW_N2)
@pytest.mark.parametrize("n1", mr.ROW_N1)
def test_row_sweep_l2(n1, n2):
    for family in mr.L2_FAMILIES:
        a, b = mr.descs(3, n1, n2, mr.ROW_L2_DIM, family)
        _three_paths(a, b, family)


@pytest.mark.parametrize("n2", mr.ROW_N2)
@pytest.mark.parametrize("n1", mr.ROW_N1)
def test_row_sweep_hamming(n1, n2):
    a, b = mr.descs(4, n1, n2, mr.ROW_HAMMING_BYTES, "hamming")
    _three_paths(a, b, "hamming")


# ---- train splits ----
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", mr.SPLIT_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_train_splits(case):
    """one split, several full splits, a last split of 1..63 rows, a split without rows (batched path only: the single-pair rule
    sizes the split count from the pair's own rows) — the case of every shape is computed from the restated launch rule with the
    device's CU count and asserted, and the two paths, which split differently, must agree with the oracle and with each other"""
    n1, n2, dim, (left, right), want_single, want_batch = case
    cus = _cus()
    t_chunk, splits = mr.single_split(n1, n2, cus)
    assert mr.split_case(mr.split_rows(n2, t_chunk, splits)) == want_single, (cus, t_chunk, splits)
    t_chunk, splits = mr.batch_split([left[0], n1, right[0]], [left[1], n2, right[1]], cus)
    assert mr.split_case(mr.split_rows(n2, t_chunk, splits)) == want_batch, (cus, t_chunk, splits)
    a, b = mr.descs(5, n1, n2, dim, "normal")
    _three_paths(a, b, "normal", left, right)


# ---- ties ----
_TIE_N2 = 1100            # with 70 queries: 18 splits of 64 rows (single-pair path), so 63 | 64 is a tile AND a split boundary
_TIES = [(0, 63, 64, 65, _TIE_N2 - 1), (63, 64), (64, 65), (65, _TIE_N2 - 1), (0, _TIE_N2 - 1), (63, _TIE_N2 - 1), (127, 128), (1023, 1024),
         (1087, 1088, _TIE_N2 - 1)]


@pytest.mark.parametrize("family,dim", [("normal", 129), ("hamming", 260)])
@pytest.mark.parametrize("rows", _TIES, ids=lambda r: "-".join(map(str, r)))
def test_ties_across_tile_split_and_chunk_edges_go_to_the_lower_index(rows, family, dim):
    n1 = 70
    t_chunk, splits = mr.single_split(n1, _TIE_N2, _cus())
    cuts = {s * t_chunk for s in range(1, splits)}
    if rows in ((63, 64), (127, 128), (1023, 1024), (1087, 1088, _TIE_N2 - 1)):
        assert rows[1] in cuts, (t_chunk, splits)                     # the duplicates straddle a split boundary of the single-pair path
    bt, bs = mr.batch_split([mr.LEFT[0], n1, mr.RIGHT[0]], [mr.LEFT[1], _TIE_N2, mr.RIGHT[1]], _cus())
    a, b = mr.descs(9, n1, _TIE_N2, dim, family)
    norm = "hamming" if family == "hamming" else "l2"
    v = b[200].copy()
    for r in rows:
        b[r] = v
    a[10] = v                                                         # a query equal to the duplicates
    a[11] = v; a[11, dim - 1] = a[11, dim - 1] + 1 if norm == "l2" else a[11, dim - 1] ^ 1   # and one at the same distance from all
    b[200] = b[201]                                                   # the source row itself is no further copy
    idx, dist = _three_paths(a, b, family)
    lo = sorted(rows)[:2]
    assert list(idx[10]) == lo and list(idx[11]) == lo, (idx[10], idx[11], t_chunk, splits, bt, bs)
    assert dist[10, 0] == 0 and dist[10, 1] == 0 and dist[11, 0] == dist[11, 1] > 0
    back, _ = matcher.knn_match(b, a, norm)                           # the transposed search: queries 10 and 11 tie for no train row,
    assert (back[list(rows), 0] == 10).all()                          # every duplicate's nearest query is 10 (distance 0)


# ---- non-finite descriptor distances: one rule for the dense single-pair, the batched and the guided path ----
def test_non_finite_distances_are_not_neighbours_in_any_path():
    """include/mi_degensac.h: a train row whose distance to the query is NaN or +inf — NaN or +-inf in a descriptor row, or finite rows
    whose squared distance overflows fp32 (one component 3e19 apart) — is not a neighbour: it takes no slot in idx, a query left with
    fewer than two finite distances gets -1 / inf, and such a slot never passes the ratio test."""
    n1, n2, dim = 70, 300, 65
    a, b = mr.descs(10, n1, n2, dim, "normal")
    bad_rows = [0, 63, 64, 130, n2 - 1]
    b[0, 64] = np.nan; b[63, 0] = np.inf; b[64, 17] = -np.inf; b[130, 64] = 3e19; b[n2 - 1, 1] = np.nan
    a[5, 3] = np.nan; a[6, 64] = np.inf; a[7, 0] = -3e19                # queries with no finite distance at all
    a[8, 64] = 3e19                                                   # finite against row 130 only (difference 0 in that word)
    ri, rd = mo.knn2(a, b, "l2")
    assert (ri[[5, 6, 7]] == -1).all() and list(ri[8]) == [130, -1] and np.isfinite(rd[8, 0]) and np.isposinf(rd[8, 1])
    ok = np.setdiff1d(np.arange(n1), [5, 6, 7, 8])
    assert not np.isin(ri[ok], bad_rows).any() and (ri[ok] >= 0).all()
    idx, dist = _three_paths(a, b, "normal", exact=False)             # single-pair, batched, match_snn with and without mutual
    finite_rows = ~np.isin(np.arange(n2), bad_rows)                   # for these queries the rule acts like a gate on the finite rows
    mr.check_knn2_against_exact(idx[ok], dist[ok], a[ok], b, "l2", gate=np.tile(finite_rows, (len(ok), 1)))
    # the guided path with a gate that passes every row: the same answer
    rng = np.random.default_rng(3)
    k1 = rng.uniform(0, 500, (n1, 2)); k2 = rng.uniform(0, 500, (n2, 2))
    M = rng.normal(size=(1, 3, 3))
    match, gi, gd = tensor_api.guided_match_batch_tensors(_t(k1), _t(k2), _t(a), _t(b), [n1], [n2], _t(M), model="F", px_th=1e100,
                                                          ratio=0.9, driver_form=True)
    assert np.array_equal(gi.cpu().numpy(), idx) and np.array_equal(_bits(gd.cpu().numpy()), _bits(dist))
    match = match.cpu().numpy()
    assert (match[[5, 6, 7]] == -1).all() and match[8] == 130          # one finite candidate: the guided decision lets it pass
    # the transposed search: the non-finite train rows as queries find nothing
    back, bd = matcher.knn_match(b, a, "l2")
    assert (back[[0, 63, 64, n2 - 1]] == -1).all() and np.isposinf(bd[[0, 63, 64, n2 - 1]]).all() and list(back[130]) == [8, -1]
