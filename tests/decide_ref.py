"""TEST INFRASTRUCTURE ONLY (CPU, numpy): the decision rule of include/mi_degensac.h (MI_DEGENSAC_DECIDE_*) restated on 2-NN results, once
for the unguided form and once for the guided form, and a designed scene on the integer codes of tests/verify_ref.py in which every
query STATES under which rules it is kept and why (tests/test_decide_cpu.py, tests/test_gpu_decide.py).

The arithmetic is the kernel's: the product ratio * dist[1] in float32, the ratio tests strict (<), the distance threshold not (<=)."""
import numpy as np

from oracle import matcher_np as mo
from tests import verify_ref as vr

NO_RATIO, BACK_RATIO, MAX_DIST = 1, 2, 4


def decide(idx, dist, ratio=0.9, back=None, bdist=None, flags=0, max_dist=0.0):
    """keep [n1] bool of the UNGUIDED form.  idx / dist [n1, 2]: the forward 2-NN; back / bdist [n2, 2]: the reverse one (back = None: no
    mutual check).  A missing slot 1 fails either ratio test."""
    idx = np.asarray(idx); dist = np.asarray(dist, np.float32); r = np.float32(ratio)
    j = idx[:, 0]
    keep = j >= 0
    if not flags & NO_RATIO:
        keep &= (idx[:, 1] >= 0) & (dist[:, 0] < r * dist[:, 1])
    if flags & MAX_DIST:
        keep &= dist[:, 0] <= np.float32(max_dist)
    if back is not None and len(back) == 0:
        return np.zeros(len(idx), bool)                                  # no train row: nothing to be mutual with
    if back is not None:
        jj = np.clip(j, 0, None)
        keep &= np.asarray(back)[jj, 0] == np.arange(len(idx))
        if flags & BACK_RATIO:
            bd = np.asarray(bdist, np.float32)
            keep &= (np.asarray(back)[jj, 1] >= 0) & (bd[jj, 0] < r * bd[jj, 1])
    else:
        assert not flags & BACK_RATIO, "BACK_RATIO reads the reverse search of the mutual check"
    return keep


def decide_guided(idx, dist, ratio=0.9, back=None, bdist=None, flags=0, max_dist=0.0):
    """keep [n1] bool of the GUIDED form: a missing slot 1 has dist = inf and passes either ratio test, because nothing competes"""
    idx = np.asarray(idx); dist = np.asarray(dist, np.float32); r = np.float32(ratio)
    j = idx[:, 0]
    keep = j >= 0
    if not flags & NO_RATIO:
        keep &= dist[:, 0] < r * dist[:, 1]
    if flags & MAX_DIST:
        keep &= dist[:, 0] <= np.float32(max_dist)
    if back is not None and len(back) == 0:
        return np.zeros(len(idx), bool)                                  # no train row: nothing to be mutual with
    if back is not None:
        jj = np.clip(j, 0, None)
        keep &= np.asarray(back)[jj, 0] == np.arange(len(idx))
        if flags & BACK_RATIO:
            bd = np.asarray(bdist, np.float32)
            keep &= bd[jj, 0] < r * bd[jj, 1]
    else:
        assert not flags & BACK_RATIO, "BACK_RATIO reads the reverse search of the mutual check"
    return keep


def rule_flags(ratio, mutual, max_dist):
    """(flags, ratio as a number, mutual as a bool, max_dist as a number) of the Python keywords ratio / mutual / max_dist"""
    f = (NO_RATIO if ratio is None else 0) | (BACK_RATIO if mutual == "ratio" else 0) | (MAX_DIST if max_dist is not None else 0)
    return f, 1.0 if ratio is None else ratio, bool(mutual), 0.0 if max_dist is None else max_dist


def tentatives(d1, d2, ratio=0.9, mutual=False, max_dist=None, norm="l2"):
    """(query rows ascending, train rows) of one pair under the keywords' rule, from the oracle's 2-NN in both directions"""
    n = "l2" if norm == "l2_u8" else norm
    idx, dist = mo.knn2(d1, d2, n)
    flags, r, mu, md = rule_flags(ratio, mutual, max_dist)
    back = bdist = None
    if mu:
        back, bdist = mo.knn2(d2, d1, n)
        if len(d2) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
    q = np.flatnonzero(decide(idx, dist, r, back, bdist, flags, md))
    return q.astype(np.int64), idx[q, 0].astype(np.int64)


def pair_ref(port, model, k1, k2, d1, d2, seed, ratio=0.9, mutual=False, max_dist=None, norm="l2"):
    """verify_ref.pair_ref under a rule: the restatement's tentatives, then the estimator of verify_ref on them"""
    q, t = tentatives(d1, d2, ratio, mutual, max_dist, norm)
    est = vr.estimate(port, model, k1[q], k2[t], seed) if len(q) >= vr.MIN_PTS[model] else None
    if est is not None and not np.asarray(est[0]).any():                # no model found: the calls return a zero model and, as they document
        est = (est[0], np.zeros(len(q), bool), est[2])                   # ("inlier of the pair's model"), no inliers; the estimator's raw mask is not kept
    return vr.result(model, len(d1), q, t, est)


# ---- the designed scene -------------------------------------------------------------------------------------------------------------
# ids with pairwise Hamming distance >= 2 (an id and its parity bit): two different codes are >= 4 sqrt(2) apart under L2 and >= 16 bits
# under Hamming, "far" against the distances 0 / 1 / 2 the scene decides on
def _id(k):
    return (k << 1) | (bin(k).count("1") & 1)


RATIO = 0.5
# query row -> why.  Train rows are shuffled; t(x) = the train row made for query x.
ROWS = {
    0: "exact: t holds its code (d0 = 0), every other train row is far",
    1: "near1: t holds its code + 1 in component 12 (d0 = 1 = the max_dist edge)",
    2: "near2: t holds its code + 2 in component 12 (d0 = 2)",
    3: "tie0: the train set holds its code twice (d0 = d1 = 0): the ratio test drops it, NO_RATIO keeps it at the lower row",
    4: "edge: code + 1 (component 12) and code + 2 (component 13), d0 = 1, d1 = 2: 1 < 0.5 * 2 is false, NO_RATIO keeps it",
    5: "back edge: its t = code + 1 (component 12); query 6 lies at 2 from that t, so bd0 = 1, bd1 = 2: BACK_RATIO at 0.5 drops it",
    6: "the second query of row 5's t (code + 1 in 12 and + 2 in 13): forward d0 = 2 passes, the mutual check fails",
    7: "exact, like 0 (a second plainly kept row, behind the special ones)",
    8: "reverse tie: rows 8 and 9 are the same code, t its exact copy: bd0 = bd1 = 0, mutual keeps 8, BACK_RATIO drops it",
    9: "reverse tie: the higher of the two equal queries, dropped by the mutual check",
}
N1 = len(ROWS)
# the stated kept sets: (ratio, mutual, max_dist) -> query rows
KEPT = {
    (RATIO, False, None): [0, 1, 2, 5, 6, 7, 8, 9],
    (RATIO, True, None): [0, 1, 2, 5, 7, 8],
    (RATIO, "ratio", None): [0, 1, 2, 7],
    (0.6, "ratio", None): [0, 1, 2, 4, 5, 7],                            # 1 < 0.6 * 2 holds: both edges (rows 4 and 5) are edges of ratio 0.5 only
    (None, False, None): list(range(N1)),
    (None, True, None): [0, 1, 2, 3, 4, 5, 7, 8],
    (None, True, 2.0): [0, 1, 2, 3, 4, 5, 7, 8],                        # at or above every d0: nothing changes
    (None, True, 1.0): [0, 1, 3, 4, 5, 7, 8],                           # d0 == max_dist is kept, near2 goes
    (None, True, float(np.nextafter(np.float32(1.0), np.float32(0.0)))): [0, 3, 7, 8],
    (None, True, 0.0): [0, 3, 7, 8],                                    # only duplicated rows
    (RATIO, False, 1.0): [0, 1, 5, 7, 8, 9],
    (RATIO, "ratio", 0.0): [0, 7],
}


def scene(norm="l2", fillers=4, seed=0):
    """dict(d1 [N1, 16], d2, n1, n2, norm, train_of [N1] = the stated nearest train row); descriptors float32 for "l2", else uint8"""
    assert norm in vr.NORMS
    rng = np.random.default_rng([7, seed])
    ids = iter(_id(k) for k in range(1, 1 << 10))
    code = lambda: vr._codes([next(ids)], norm)[0]
    b = lambda c, comp, d: vr._bump(c, comp, d, norm)
    q = [None] * N1; t = []; owner = []

    def add(row, c):
        t.append(c); owner.append(row)
    for r in (0, 7):
        q[r] = code(); add(r, q[r].copy())
    q[1] = code(); add(1, b(q[1], 12, 1))
    q[2] = code(); add(2, b(q[2], 12, 2))
    q[3] = code(); add(3, q[3].copy()); add(-1, q[3].copy())
    q[4] = code(); add(4, b(q[4], 12, 1)); add(-1, b(q[4], 13, 2))
    q[5] = code(); add(5, b(q[5], 12, 1)); q[6] = b(b(q[5], 12, 1), 13, 2)
    q[8] = code(); q[9] = q[8].copy(); add(8, q[8].copy())
    for _ in range(fillers):
        add(-1, code())
    d1 = np.array(q, np.uint8); d2 = np.array(t, np.uint8); owner = np.array(owner)
    perm = rng.permutation(len(d2)); d2 = d2[perm]; owner = owner[perm]
    train_of = np.full(N1, -1, np.int64)
    for r in range(N1):
        w = np.flatnonzero(owner == r)
        if len(w):
            train_of[r] = w[0]
    train_of[6] = train_of[5]; train_of[9] = train_of[8]
    train_of[3] = np.flatnonzero((d2 == d1[3]).all(1)).min()            # the lower of the two equal rows
    cast = (lambda a: a.astype(np.float32)) if norm == "l2" else (lambda a: a)
    return dict(d1=np.ascontiguousarray(cast(d1)), d2=np.ascontiguousarray(cast(d2)), n1=N1, n2=len(d2), norm=norm, train_of=train_of)


# ---- the same decisions at other row widths ---------------------------------------------------------------------------------------------
def widened(sc, dim):
    """the designed scene with its rows padded with zeros to `dim` components (dim >= 16): no distance changes, so KEPT holds as stated"""
    assert dim >= sc["d1"].shape[1]
    pad = lambda a: np.ascontiguousarray(np.pad(a, ((0, 0), (0, dim - a.shape[1]))))                                # noqa: E731
    return dict(sc, d1=pad(sc["d1"]), d2=pad(sc["d2"]))


# One 32-bit word per row: a row is the code of ONE number v in 0 .. 32, a float [v] under "l2", the bytes [v, 0, 0, 0] under "l2_u8" and v
# one-bits in unary under "hamming", so that the distance of two rows is |a - b| under every norm.
SCALAR_Q = [0, 11, 12, 22, 31]
SCALAR_T = [0, 10, 20, 31]
# forward (d0, d1): q0 (0, 10), q1 (1, 9), q2 (2, 8), q3 (2, 9), q4 (0, 11).  reverse: t0 -> q0 (0), q1 (11); t1 -> q1 (1), q2 (2): the strict
# edge 1 < 0.5 * 2 of BACK_RATIO; t2 -> q3 (2), q2 (8); t3 -> q4 (0), q3 (9).  q2 is nobody's nearest query.
SCALAR_KEPT = {
    (None, True, None): [0, 1, 3, 4],
    (None, True, 1.0): [0, 1, 4],                                       # d0 == max_dist is kept, the rows at 2 go
    (RATIO, "ratio", None): [0, 3, 4],                                  # q1 falls at the reverse edge
    (0.6, "ratio", None): [0, 1, 3, 4],
    (RATIO, False, 1.0): [0, 1, 4],
    (RATIO, False, None): [0, 1, 2, 3, 4],
}
SCALAR_TRAIN_OF = np.array([0, 1, 1, 2, 3])


def scalar_scene(norm):
    def rows(vals):
        v = np.asarray(vals, np.int64)
        if norm == "l2":
            return np.ascontiguousarray(v[:, None].astype(np.float32))
        if norm == "l2_u8":
            out = np.zeros((len(v), 4), np.uint8); out[:, 0] = v
            return out
        bits = ((1 << v) - 1).astype(np.uint64)                          # v one-bits
        return np.ascontiguousarray(bits.astype("<u4").view(np.uint8).reshape(len(v), 4))
    assert norm in vr.NORMS and max(SCALAR_Q + SCALAR_T) < 32
    return dict(d1=rows(SCALAR_Q), d2=rows(SCALAR_T), n1=len(SCALAR_Q), n2=len(SCALAR_T), norm=norm, train_of=SCALAR_TRAIN_OF)
