"""TEST INFRASTRUCTURE ONLY: a float64 reference of the matcher stage that knows nothing about the kernels' accumulation order,
and the descriptor families the shape tests share (plain numpy, no fixtures).

oracle/matcher_np.py restates the device's own fp32 arithmetic, so a mistake made in both passes every bit-exact test.  The check
here needs no such restatement: it holds for any kernel that sums the dim squared differences in fp32 in SOME order and takes one
correctly rounded sqrtf, and it fails for one that drops a word, a train row or a chunk.

The L2 bound, g = (dim + 2) * 2**-24 with u = 2**-24 the fp32 unit roundoff: a_k - b_k carries one rounding (1 + d1), its square a
second (the term is s_k (1 + d)^3 with s_k the exact square), and a sum of dim non-negative terms in any order adds at most dim - 1
more factors (1 + d) to every term.  So the fp32 sum S' obeys |S' - S| <= ((1 + u)^(dim + 2) - 1) S, and sqrtf — which halves a
relative error and adds one rounding of its own — leaves |dist - D| <= g D to first order with about a factor of two to spare.
Ranking by distances that are each within g of the truth can prefer a row whose exact distance is larger by at most
(1 + g) / (1 - g).  The bound is derived, not measured; no other tolerance appears in the tests that use it.  It assumes that no
square underflows: the "subnormal" family below (1e-20 scale, squares below the smallest normal fp32) is for bit-exact
comparisons only and never reaches check_knn2_against_exact."""
import numpy as np

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def g_bound(dim):
    return (dim + 2) * 2.0 ** -24


def dist64(a, b, norm):
    """the exact distance matrix [n1, n2]: L2 = float64 of the float32 inputs (differences, squares and a pairwise sum in float64:
    error of a few 2**-53, eight orders below the bound), Hamming = the integer popcount of the differing bits"""
    a = np.asarray(a); b = np.asarray(b)
    n1, n2 = a.shape[0], b.shape[0]
    if norm == "l2":
        assert a.dtype == np.float32 and b.dtype == np.float32
        a = a.astype(np.float64); b = b.astype(np.float64)
        D = np.zeros((n1, n2))
    else:
        assert a.dtype == np.uint8 and b.dtype == np.uint8
        D = np.zeros((n1, n2), np.int64)
    step = max(1, (1 << 22) // max(1, n2 * a.shape[1]))              # query rows per block: bounded temporary
    for r in range(0, n1, step):
        if norm == "l2":
            d = a[r:r + step, None, :] - b[None, :, :]
            D[r:r + step] = np.sqrt(np.sum(d * d, axis=2))
        else:
            D[r:r + step] = _POP8[np.bitwise_xor(a[r:r + step, None, :], b[None, :, :])].sum(axis=2, dtype=np.int64)
    return D


def check_knn2_against_exact(idx, dist, a, b, norm, gate=None):
    """Assert, for EVERY query, that (idx, dist) [n1, 2] is a correct 2-NN of a in b under the exact distances.  gate (bool [n1, n2],
    optional) restricts the candidates of each query to its gated rows (the guided form)."""
    idx = np.asarray(idx); dist = np.asarray(dist)
    a = np.asarray(a); b = np.asarray(b)
    n1, n2 = a.shape[0], b.shape[0]
    assert idx.shape == (n1, 2) and dist.shape == (n1, 2), (idx.shape, dist.shape)
    if n1 == 0:
        return
    g_ok = np.ones((n1, n2), bool) if gate is None else np.asarray(gate, bool)
    assert g_ok.shape == (n1, n2)
    cand = g_ok.sum(axis=1)                                          # candidates per query
    # indices: in range, distinct, -1 exactly where the query has fewer than k + 1 candidates; inf distance with -1
    for k in range(2):
        miss = cand <= k
        assert np.array_equal(idx[:, k] == -1, miss), ("-1 where a candidate exists, or an index where none does", k,
                                                       np.flatnonzero((idx[:, k] == -1) != miss)[:5])
        assert ((idx[:, k] >= -1) & (idx[:, k] < max(n2, 1))).all(), ("index out of range", k)
        assert np.isposinf(dist[miss, k]).all(), ("a missing neighbour must carry dist = inf", k)
    two = cand >= 2
    assert (idx[two, 0] != idx[two, 1]).all(), "the two neighbours of a query must be distinct rows"
    if n2 == 0:
        return
    D = dist64(a, b, norm)
    r = np.arange(n1)
    for k in range(2):
        have = np.flatnonzero(cand > k)
        assert g_ok[have, idx[have, k]].all(), ("a neighbour outside the gate", k)
    if norm == "l2":
        g = g_bound(a.shape[1])
        Dm = np.where(g_ok, D, np.inf)
        srt = np.sort(Dm, axis=1)[:, :2]                             # the exact smallest and second-smallest candidate distance
        for k in range(min(2, n2)):
            have = np.flatnonzero(cand > k)
            De = D[have, idx[have, k]]
            lim = srt[have, k] * (1 + g) / (1 - g)
            assert (De <= lim).all(), ("neighbour %d is farther than the exact one allows" % k, have[De > lim][:5],
                                       (De / np.maximum(srt[have, k], 1e-300)).max())
            err = np.abs(dist[have, k].astype(np.float64) - De)
            assert (err <= g * De).all(), ("distance %d off the exact one by more than g" % k, have[err > g * De][:5], (err / np.maximum(De, 1e-300)).max() / g)
        assert (dist[two, 0] <= dist[two, 1]).all(), "nearest first"
    else:
        big = np.int64(1) << 40
        Dm = np.where(g_ok, D, big)
        order = np.argsort(Dm, axis=1, kind="stable")[:, :2]         # lexicographic minimum of (distance, index)
        for k in range(min(2, n2)):
            have = np.flatnonzero(cand > k)
            assert np.array_equal(idx[have, k], order[have, k]), ("Hamming neighbour %d is not the (distance, index) minimum" % k,
                                                                  have[idx[have, k] != order[have, k]][:5])
            assert np.array_equal(dist[have, k].astype(np.int64), D[have, idx[have, k]]), ("Hamming distance %d is not the popcount" % k)
            assert np.array_equal(dist[have, k], np.floor(dist[have, k]))


# ---- descriptor families and shapes shared by test_matcher_ref_cpu.py (the oracle alone) and test_gpu_matcher_shapes.py ----
L2_DIMS = [1, 2, 3, 63, 64, 65, 100, 127, 129, 192, 200, 256, 512]
HAMMING_BYTES = [1, 3, 4, 5, 64, 252, 256, 260, 512]
WIDTH_SHAPE = (130, 200)
ROW_N1 = [1, 63, 64, 65, 127, 128, 129]
ROW_N2 = [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1025]
ROW_L2_DIM, ROW_HAMMING_BYTES = 65, 260
L2_FAMILIES = ["normal", "sift", "tiny"]              # checked against float64; "subnormal" is bit-exact only (see the module docstring)


def descs(seed, n1, n2, dim, family):
    """(a [n1, dim], b [n2, dim]) of one family: half the queries are noisy copies of train rows (true matches), query 0 is an exact copy of
    the LAST train row (a kernel that loses row n2 - 1 is seen at every width), train rows 3, 5, 7 are exact duplicates (ties) and the last query
    equals them.  family: "normal" (unit normal), "sift" (unnormalised 0..255 floats: large dynamic range), "tiny" (1e-12 scale: tiny
    but normal squares), "subnormal" (1e-20 scale: fp32 squares underflow), "hamming" (uint8 bytes)."""
    rng = np.random.default_rng([seed, n1, n2, dim])
    m = min(n1, n2) // 2
    pick = rng.permutation(n2)[:m]
    if family == "hamming":
        b = rng.integers(0, 256, size=(n2, dim), dtype=np.uint8); a = rng.integers(0, 256, size=(n1, dim), dtype=np.uint8)
        a[:m] = b[pick] ^ (rng.random((m, dim)) < 0.03).astype(np.uint8)
        if n1 and n2:
            a[0] = b[n2 - 1]
    else:
        if family == "sift":
            b = rng.integers(0, 256, size=(n2, dim)).astype(np.float32); a = rng.integers(0, 256, size=(n1, dim)).astype(np.float32)
            noise = np.rint(3.0 * rng.normal(size=(n1, dim))).astype(np.float32)
        else:
            s = np.float32({"normal": 1.0, "tiny": 1e-12, "subnormal": 1e-20}[family])
            b = rng.normal(size=(n2, dim)).astype(np.float32) * s; a = rng.normal(size=(n1, dim)).astype(np.float32) * s
            noise = 0.05 * rng.normal(size=(n1, dim)).astype(np.float32) * s
        a[:m] = b[pick] + noise[:m]
        if n1 and n2:
            a[0] = b[n2 - 1]
    if n2 > 8:
        b[5] = b[3]; b[7] = b[3]
        if n1 > 1:
            a[n1 - 1] = b[3]
    return a, b


# ---- the launch code's train-split rule (mi_matcher.hip: mi_degensac_match_knn2_dev and mt_batch_knn2), restated -----------------
def _chunk(qtiles, max_n2, cus, batched):
    ttiles = (max_n2 + 63) // 64 if max_n2 > 0 else 1
    splits = 1 if (batched and qtiles >= 2 * cus) else (2 * cus + qtiles - 1) // qtiles
    splits = max(1, min(splits, ttiles, 256))
    t_chunk = ((ttiles + splits - 1) // splits) * 64
    return t_chunk, ((max_n2 + t_chunk - 1) // t_chunk if max_n2 > 0 else 1)


def single_split(n1, n2, cus=256):
    """(t_chunk, splits) of the single-pair path: every split owns at least one row"""
    return _chunk((n1 + 63) // 64, n2, cus, False)


def batch_split(counts1, counts2, cus=256):
    """(t_chunk, splits) of the batched path: one chunk for the batch, from its tile count and its LARGEST train set, so a pair
    with a smaller train set has splits without rows"""
    return _chunk(sum((c + 63) // 64 for c in counts1), max(counts2) if len(counts2) else 0, cus, True)


def split_rows(n2, t_chunk, splits):
    """train rows of every split of a pair with n2 rows"""
    return [max(0, min(n2, (s + 1) * t_chunk) - s * t_chunk) for s in range(splits)]


# the batched tests place the pair under test between these two (n1, n2) pairs, so that its offsets are not zero
LEFT, RIGHT = (7, 300), (5, 70)
# (n1, n2, dim, (left, right) neighbours of the batched call, case of the single-pair path, case of the batched path) on 256 CUs.
# Cases: "one" = one split; "full" = several splits, all full; "short" = the last split holds 1..63 rows (fewer than one tile);
# "part" = several splits, the last one shorter than t_chunk by whole tiles or more than a tile; "empty" = a split without rows.
SPLIT_CASES = [
    (130, 64, 65, (LEFT, RIGHT), "one", "empty"),          # batched: 300 train rows of the left pair make 5 splits, this pair fills one
    (130, 1024, 65, (LEFT, RIGHT), "full", "full"),        # 16 splits of 64 rows in both paths
    (130, 1025, 65, (LEFT, RIGHT), "short", "short"),      # 17 splits, the last with 1 row
    (130, 1087, 65, (LEFT, RIGHT), "short", "short"),      # 17 splits, the last with 63 rows
    (130, 65, 65, ((7, 1025), (5, 1025)), "short", "empty"),   # batched: 17 splits of 64 from the neighbours, this pair: 64, 1, then 15 empty
    (130, 25541, 33, (LEFT, RIGHT), "short", "part"),      # t_chunk = 192 (3 tiles): 134 splits, the last with 5 rows; batched: 100 of 256, last 197
    (32768, 200, 8, ((7, 130), (5, 70)), "one", "one"),    # 512 query tiles cover the CUs twice: one split over 200 rows (4 tiles)
]


def split_case(rows):
    """the case name of a pair from the rows of its splits"""
    if len(rows) == 1:
        return "one"
    if min(rows) == 0:
        return "empty"
    if 1 <= rows[-1] <= 63:
        return "short"
    return "full" if len(set(rows)) == 1 else "part"
