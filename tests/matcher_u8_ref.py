"""TEST INFRASTRUCTURE ONLY: the uint8 L2 matcher (norm "l2_u8", include/mi_degensac.h MI_DEGENSAC_NORM_L2_U8) restated in int64
numpy, and the input families its CPU and GPU tests share.

    S[i, j] = sum_k (a[i, k] - b[j, k])^2 in int64,  dist = sqrt(float32(S)),  neighbours by stable argsort of S (ties: lower index)

For dim <= 256, S <= 256 * 255^2 = 16 646 400 < 2^24, so float32(S) is exact and every partial sum of the float32 oracle
(oracle/matcher_np.py dist_matrix(..., "l2"), which casts to float32 and accumulates in ascending k) is an exact integer too: the
two must agree bit for bit.  tests/test_matcher_u8l2_cpu.py asserts that on every family below, so that the GPU tests may compare
the device with the existing oracle alone.  `bug` builds the two deliberately wrong restatements that comparison has to reject."""
import numpy as np

ROWS = (0, 1, 2, 63, 64, 65, 127, 129, 1000)
DIMS = (4, 8, 60, 64, 68, 128, 132, 252, 256)
UNPADDED_DIMS = (5, 130)
FAMILIES = ("uniform", "sift", "extremes")


def sq_dist(a, b, bug=None):
    """int64 [n1, n2] squared distances.  bug = "signed": bytes read as int8 without the +128 offset (what a matrix-core kernel
    computes when it forgets x ^ 0x80); bug = "drop_word": the second 32-bit word of every row (bytes 4..7) is left out."""
    a = np.asarray(a); b = np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8
    if bug == "signed":
        x = a.view(np.int8).astype(np.int64); y = b.view(np.int8).astype(np.int64)
    else:
        x = a.astype(np.int64); y = b.astype(np.int64)
    if bug == "drop_word":
        keep = np.ones(a.shape[1], bool); keep[4:8] = False
        x = x[:, keep]; y = y[:, keep]
    # |x|^2 + |y|^2 - 2 x.y in int64: exact, whatever the order
    return (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * (x @ y.T)


def knn2(a, b, bug=None):
    """(idx [n1, 2] int32, dist [n1, 2] float32) with -1 / inf where b has fewer than two rows"""
    S = sq_dist(a, b, bug)
    n1, n2 = S.shape
    idx = np.full((n1, 2), -1, np.int32); dist = np.full((n1, 2), np.inf, np.float32)
    order = np.argsort(S, axis=1, kind="stable")[:, :2]
    r = np.arange(n1)
    for k in range(order.shape[1]):
        idx[:, k] = order[:, k]; dist[:, k] = np.sqrt(S[r, order[:, k]].astype(np.float32))
    return idx, dist


def same_bits(got, want):
    """idx equal and dist equal as bit patterns"""
    gi, gd = got; wi, wd = want
    return bool(np.array_equal(np.asarray(gi), wi) and
                np.array_equal(np.ascontiguousarray(gd, np.float32).view(np.uint32), np.ascontiguousarray(wd, np.float32).view(np.uint32)))


def descs(family, n1, n2, dim, seed):
    """uniform:  independent random bytes (asymmetric: catches k-map and row / column errors), half the queries near a train row
    sift:     SIFT-like rows (many zeros and small values, a few entries at the 255 clip), built from few prototypes so that whole
              rows repeat on both sides: heavy ties, where the lower train index must win
    extremes: rows of all 0 and all 255 mixed with random rows (S reaches dim * 255^2)"""
    rng = np.random.default_rng([seed, n1, n2, dim, FAMILIES.index(family)])
    if family == "uniform":
        a = rng.integers(0, 256, (n1, dim), dtype=np.uint8); b = rng.integers(0, 256, (n2, dim), dtype=np.uint8)
        m = min(n1, n2) // 2
        if m:
            near = b[rng.permutation(n2)[:m]].astype(np.int64) + rng.integers(-6, 7, (m, dim))
            a[:m] = np.clip(near, 0, 255).astype(np.uint8)
        return a, b
    if family == "sift":
        proto = np.minimum(rng.exponential(18.0, (12, dim)) * (rng.random((12, dim)) < 0.6), 255).astype(np.uint8)
        proto[:, ::17] = 255
        a = proto[rng.integers(0, 12, n1)].copy(); b = proto[rng.integers(0, 12, n2)].copy()
        flip = rng.random(b.shape) < 0.01
        b[flip] = (b[flip].astype(np.int64) + 1).clip(0, 255).astype(np.uint8)
        if n2 > 8:
            b[5] = b[3]; b[7] = b[3]
        return a, b
    a = rng.integers(0, 256, (n1, dim), dtype=np.uint8); b = rng.integers(0, 256, (n2, dim), dtype=np.uint8)
    a[0::3] = 0; a[1::3] = 255; b[0::4] = 255; b[1::4] = 0
    return a, b


def shapes():
    """(n1, n2, dim) triples in which every row count of ROWS appears on either side and every dim of DIMS appears, the 1000-row
    sides with the dims 128 and 256; the full product would mostly repeat the same tiles"""
    out = []
    for i, n1 in enumerate(ROWS):
        for j in (0, 4):
            n2 = ROWS[(i + 3 + j) % len(ROWS)]
            out.append((n1, n2, DIMS[(2 * i + j) % len(DIMS)]))
    out += [(1000, 1000, 128), (129, 1000, 256), (1000, 127, 256), (65, 65, 4), (64, 129, 252), (2, 2, 256)]
    return out
