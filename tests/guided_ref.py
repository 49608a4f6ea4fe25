"""TEST INFRASTRUCTURE ONLY: the restatement of guided matching that test_gpu_guided.py and test_gpu_guided_edges.py compare the
device with.  Every (query, train) residual comes from the CPU oracle's own metric functions (oracle/dg_oracle.c through
oracle.port), is gated with `<=`, and the gated rows are ranked by the matcher's numpy distances (oracle/matcher_np.py)."""
import numpy as np

from oracle import matcher_np as mo

KINDS = [("F", 0), ("F", 1), ("H", 0), ("H", 1), ("H", 2), ("H", 3), ("H", 4)]
ERROR_NAMES = {"F": ["sampson", "symm_epipolar"], "H": ["sampson", "symm_sq_max", "symm_max", "symm_sq_sum", "symm_sum"]}


def th(model, et, px):
    return px if (model == "H" and et in (2, 4)) else px * px


def resid(P, model, et, Md, x1, x2):
    """r(M; x1_q, y1_q, x2_t, y2_t) for every (q, t) of a pair, [n1, n2], from the oracle's metrics on u = [x1, y1, 1, x2, y2, 1]"""
    n1, n2 = len(x1), len(x2)
    u = np.ones((n1 * n2, 6)); u[:, 0:2] = np.repeat(x1[:, :2], n2, 0); u[:, 3:5] = np.tile(x2[:, :2], (n1, 1))
    d = np.zeros(n1 * n2); m = np.ascontiguousarray(Md, np.float64).ravel().copy(); L = P.lib(); dp = P.dp
    if model == "F":
        (L.dg_oracle_FDs if et == 0 else L.dg_oracle_FDsSym)(dp(u), dp(m), dp(d), n1 * n2)
    else:
        L.dg_oracle_HDS_full(et, dp(u), dp(m), dp(d), n1 * n2)
    return d.reshape(n1, n2)


def gated_knn2(gate, D):
    """the two nearest gated rows per query in (distance, index) order; a gated row whose distance is NaN or inf is no neighbour
    (the non-finite rule of matcher_np.top2)"""
    return mo.top2(D, gate)


def gate_matrix(P, model, et, px, Md, k1, k2):
    n1, n2 = len(k1), len(k2)
    if n1 and n2 and np.any(Md):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return resid(P, model, et, Md, k1, k2) <= th(model, et, px)          # NaN fails
    return np.zeros((n1, n2), bool)


def oracle(P, model, et, px, Md, k1, k2, d1, d2, norm, ratio, mutual):
    n1, n2 = len(d1), len(d2)
    gate = gate_matrix(P, model, et, px, Md, k1, k2)
    with np.errstate(invalid="ignore", over="ignore"):
        D = mo.dist_matrix(d1, d2, norm) if n1 and n2 else np.zeros((n1, n2), np.float32)
    idx, dist = gated_knn2(gate, D)
    keep = (idx[:, 0] >= 0) & (dist[:, 0] < np.float32(ratio) * dist[:, 1])
    if mutual:
        back, _ = gated_knn2(gate.T, D.T)
        keep &= back[np.clip(idx[:, 0], 0, None), 0] == np.arange(n1) if n2 else keep
    return idx, dist, np.where(keep, idx[:, 0], -1).astype(np.int32)
