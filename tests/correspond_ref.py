"""TEST INFRASTRUCTURE ONLY: the numpy restatement of the correspondence export (include/mi_degensac.h mi_degensac_correspondences_*)
that test_correspond_cpu.py pins on hand-written tables and test_gpu_correspond.py compares the device with.  Selection, order, offsets,
total, the capacity cut and local / store rows are index arithmetic; the residuals come from the CPU oracle's own metric functions
(oracle/dg_oracle.c through oracle.port) on u = [x1, y1, 1, x2, y2, 1], the way tests/guided_ref.resid calls them."""
import numpy as np


def offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def identity_pairs(K):
    return np.stack([np.arange(K), np.arange(K)], axis=1).astype(np.int64)


def layout(counts1, counts2, pairs):
    """(o1, o2, pairs [K, 2], out [K + 1]): the stores' offsets and the first output row of every entry"""
    o1, o2 = offsets(counts1), offsets(counts2)
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = np.concatenate([[0], np.cumsum(np.diff(o1)[pr[:, 0]])]).astype(np.int64)
    return o1, o2, pr, out


def select(match, keep, counts1, counts2, pairs):
    """(sel [N] bool, entry_of_row [N], q [N] = the row's index in its query image)"""
    o1, o2, pr, out = layout(counts1, counts2, pairs)
    N = int(out[-1])
    match = np.asarray(match)
    assert match.shape == (N,)
    ent = np.repeat(np.arange(len(pr)), np.diff(out))
    q = np.arange(N) - out[ent]
    nt = np.diff(o2)[pr[ent, 1]]
    sel = (match >= 0) & (match < nt)
    if keep is not None:
        sel &= np.asarray(keep).astype(np.uint8) != 0
    return sel, ent, q


def export(match, counts1, counts2, pairs, keep=None, store_rows=False, capacity=None, kps1=None, kps2=None):
    """dict(rows [n, 2] int32, entry [n] int32, pts [n, 4] or None, corr_offsets [K + 1] int64, total) with n = min(total, capacity): the
    WRITTEN prefix of the per-correspondence arrays (what lies beyond it is not the call's to touch)"""
    o1, o2, pr, out = layout(counts1, counts2, pairs)
    sel, ent, q = select(match, keep, counts1, counts2, pairs)
    r = np.flatnonzero(sel)                                            # row order = list order, query order inside an entry
    e = ent[r]
    m = np.asarray(match)[r].astype(np.int64)
    s1, s2 = o1[pr[e, 0]] + q[r], o2[pr[e, 1]] + m                     # rows of the stores
    rows = np.stack([s1, s2] if store_rows else [q[r], m], axis=1).astype(np.int32).reshape(-1, 2)
    csum = np.concatenate([[0], np.cumsum(sel)]).astype(np.int64)
    corr_offsets = csum[out]                                           # the selected rows before the entry's first row; empty entries repeat
    total = int(csum[-1])
    n = total if capacity is None else min(total, int(capacity))
    pts = None
    if kps1 is not None:
        pts = np.concatenate([np.asarray(kps1)[s1, :2], np.asarray(kps2)[s2, :2]], axis=1).astype(np.float64).reshape(-1, 4)[:n]
    return dict(rows=rows[:n], entry=e[:n].astype(np.int32), pts=pts, corr_offsets=corr_offsets, total=total)


def resid(P, model, et, Md, entry, pts):
    """the estimator's residual of every exported correspondence under ITS entry's model (driver form, Md [K, 9] or [K, 3, 3]): the oracle's
    dg_oracle_FDs / dg_oracle_FDsSym / dg_oracle_HDS_full, one call per entry that owns correspondences"""
    Md = np.ascontiguousarray(Md, np.float64).reshape(-1, 9)
    pts = np.asarray(pts, np.float64).reshape(-1, 4)
    d = np.full(len(pts), np.nan)
    L = P.lib(); dp = P.dp
    for p in np.unique(entry):
        ix = np.flatnonzero(entry == p)
        u = np.ones((len(ix), 6)); u[:, 0:2] = pts[ix, 0:2]; u[:, 3:5] = pts[ix, 2:4]
        u = np.ascontiguousarray(u); out = np.zeros(len(ix)); m = Md[p].copy()
        with np.errstate(all="ignore"):
            if model == "F":
                (L.dg_oracle_FDs if et == 0 else L.dg_oracle_FDsSym)(dp(u), dp(m), dp(out), len(ix))
            else:
                L.dg_oracle_HDS_full(et, dp(u), dp(m), dp(out), len(ix))
        d[ix] = out
    return d


def same_bits_or_nan(got, want):
    """bit for bit where the oracle's value is not NaN, NaN where it is NaN"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all() and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)))
