"""TEST INFRASTRUCTURE ONLY: the FGINN second neighbour (include/mi_degensac.h mi_degensac_match_fginn_knn2_batch_dev) restated on
oracle/matcher_np.py's distance matrix and top2, and the scenes the CPU and GPU tests share.

    slot 0 = top2(D)[:, 0];  ok[q, t] = t != i0[q] and dx*dx + dy*dy >= r*r  (float64, dx = x2[t] - x2[i0[q]]; NaN compares false)
    slot 1 = top2(D, ok)[:, 0];  needy[q] = the plain second neighbour exists and does not compete (what the device rescans)."""
import numpy as np

from oracle import matcher_np as mo

NORMS = ("l2", "hamming", "l2_u8")


def dmat(a, b, norm):
    """the matcher's distance matrix: l2_u8 is L2 on the uint8 values (exact, so equal to the float32 accumulation)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return mo.dist_matrix(a, b, "hamming" if norm == "hamming" else "l2")


def ok_mask(i0, kp2, r):
    kp2 = np.asarray(kp2, np.float64); n2 = kp2.shape[0]
    an = np.clip(i0, 0, None)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = kp2[None, :, 0] - kp2[an, 0][:, None]; dy = kp2[None, :, 1] - kp2[an, 1][:, None]
        ok = dx * dx + dy * dy >= np.float64(r) * np.float64(r)
    ok &= np.arange(n2)[None, :] != i0[:, None]
    ok[i0 < 0] = False
    return ok


def fginn(a, b, kp2, r, norm):
    """(idx [n1, 2] int32, dist [n1, 2] float32, needy [n1] bool, ok [n1, n2] bool) of one pair"""
    D = dmat(a, b, norm)
    pi, pd = mo.top2(D)
    n1, n2 = D.shape
    idx = pi.copy(); dist = pd.copy()
    if n2 == 0:
        return idx, dist, np.zeros(n1, bool), np.zeros((n1, 0), bool)
    ok = ok_mask(pi[:, 0], kp2, r)
    si, sd = mo.top2(D, ok)
    idx[:, 1] = si[:, 0]; dist[:, 1] = sd[:, 0]
    needy = (pi[:, 1] >= 0) & ~ok[np.arange(n1), np.clip(pi[:, 1], 0, None)]
    return idx, dist, needy, ok


def keep(idx, dist, ratio):
    return (idx[:, 1] >= 0) & (dist[:, 0] < np.float32(ratio) * dist[:, 1])


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _rows(rng, n, width, norm):
    """width = float32 words (l2) or bytes (hamming, l2_u8)"""
    if norm == "l2":
        return rng.normal(size=(n, width)).astype(np.float32)
    return rng.integers(0, 256, size=(n, width), dtype=np.uint8)


def _near(rng, rows, norm, big):
    """copies of rows: big = a query's view of its train row (0.05 sigma noise / one bit changed in 24 bytes), else a twin's
    near-equal descriptor (0.002 sigma / one bit in one byte)"""
    if norm == "l2":
        return rows + ((0.05 if big else 0.002) * rng.normal(size=rows.shape)).astype(np.float32)
    out = rows.copy()
    for i in range(out.shape[0]):
        c = rng.permutation(out.shape[1])[:min(24 if big else 1, out.shape[1])]
        out[i, c] = out[i, c] ^ 1
    return out


def twin_scene(seed, n1, n2, width, norm, n_needy, spacing=100.0, twin_px=1.5):
    """Query i (i < m = min(n1, n2 - n_needy)) is a noisy copy of train row i.  The first n_needy train rows have a TWIN: one more train
    row, appended after the first n2 - n_needy, with a near-equal descriptor and a keypoint twin_px away.  Every other keypoint sits
    on a grid `spacing` apart.  Returns (a, b, kp2)."""
    rng = np.random.default_rng([seed, n1, n2, width, n_needy])
    base = n2 - n_needy
    assert 0 <= n_needy <= min(n1, base)
    b = _rows(rng, n2, width, norm); a = _rows(rng, n1, width, norm)
    m = min(n1, base)
    a[:m] = _near(rng, b[:m], norm, True)
    b[base:] = _near(rng, b[:n_needy], norm, False)
    g = np.arange(n2)
    kp2 = np.c_[spacing * (g % 37), spacing * (g // 37)].astype(np.float64)
    kp2[base:] = kp2[:n_needy] + np.array([twin_px, 0.0])
    return a, b, kp2
