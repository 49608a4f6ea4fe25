"""TEST INFRASTRUCTURE ONLY (never imported by pydegensac_amd/): numpy restatement of the matcher stage the reference's
example runs through OpenCV (examples/simple-example.py:46-53: BFMatcher().knnMatch(descs1, descs2, k=2) and the ratio
test `m.distance < 0.9 * n.distance`).  OpenCV (cv2, absent from this image) is the third-party dependency; its
brute-force matcher returns, per query, the train rows in ascending distance, distance = NORM_L2 of the float32
difference (NORM_HAMMING for uint8), first-found on ties.  Stated here with one fixed arithmetic so that the GPU
kernel can be compared bit for bit: fp32 squared differences accumulated over the dimension in ascending order."""
import numpy as np


def dist_matrix(desc1, desc2, norm="l2"):
    a = np.asarray(desc1); b = np.asarray(desc2)
    if norm == "l2":
        a = a.astype(np.float32); b = b.astype(np.float32)
        acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
        for k in range(a.shape[1]):                              # ascending k, one rounding per operation
            d = (a[:, k, None] - b[None, :, k]).astype(np.float32)
            acc = (acc + (d * d).astype(np.float32)).astype(np.float32)
        return np.sqrt(acc).astype(np.float32)
    x = np.bitwise_xor(a[:, None, :], b[None, :, :])
    return np.unpackbits(x, axis=2).sum(axis=2).astype(np.float32)


def top2(D, ok=None):
    """The two smallest entries of every row of D in (distance, index) order, among the columns where ok (bool, optional) holds.
    The non-finite rule of include/mi_degensac.h: a train row whose distance to the query is NaN or +inf (NaN / inf in a descriptor
    row, or an fp32 overflow of the squared sum) is not a neighbour — it takes no slot, and a query with fewer than two finite
    candidates gets idx = -1 / dist = inf, exactly as with fewer than two train rows."""
    n1, n2 = D.shape
    idx = np.full((n1, 2), -1, np.int32); dist = np.full((n1, 2), np.inf, np.float32)
    if n2 == 0:
        return idx, dist
    fin = np.isfinite(D) if ok is None else (np.isfinite(D) & ok)
    Dm = np.where(fin, D, np.float32(np.inf))
    order = np.argsort(Dm, axis=1, kind="stable")[:, :2]         # stable: the lower index wins a tie
    r = np.arange(n1)
    for k in range(order.shape[1]):
        is_nb = fin[r, order[:, k]]
        idx[:, k] = np.where(is_nb, order[:, k], -1); dist[:, k] = np.where(is_nb, Dm[r, order[:, k]], np.inf)
    return idx, dist


def knn2(desc1, desc2, norm="l2"):
    with np.errstate(invalid="ignore", over="ignore"):
        D = dist_matrix(desc1, desc2, norm)
    return top2(D)


def match_snn(desc1, desc2, ratio=0.9, mutual=False, norm="l2"):
    idx, dist = knn2(desc1, desc2, norm)
    keep = (idx[:, 1] >= 0) & (dist[:, 0] < np.float32(ratio) * dist[:, 1])
    if mutual:
        back, _ = knn2(desc2, desc1, norm)
        keep &= back[np.clip(idx[:, 0], 0, None), 0] == np.arange(len(idx))
    q = np.flatnonzero(keep)
    return q, idx[q, 0].astype(np.int64), dist[q, 0]
