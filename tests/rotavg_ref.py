"""The rule of rotation averaging (include/mi_degensac.h mi_degensac_rotation_average_dev) restated in numpy float64: one IEEE operation
per written operator, in the header's order, the sums in the order of G = mi_degensac_rotation_average_tile(0) lanes and their butterfly.
Every elementwise numpy operation below is one IEEE operation per element (numpy contracts nothing), so running the rule over all
half-edges at once changes no bit; what is NOT used (an other end that is not set, an opposed half-edge) is replaced by +0.0 before the
sums, which equals skipping it: an accumulator that starts as +0.0 never becomes -0.0.
`broken` names one of three deliberately wrong variants that tests/test_rotavg_cpu.py must reject."""
import math

import numpy as np

from pydegensac_amd import _lib

KNOWN, OK, UNREACHED, ISOLATED = range(4)
CONVERGED, MAX_SWEEPS, NO_ROOT = range(3)
Q_MIN = 2.0 ** -10


def group():
    return _lib.rotavg_group()


def used_edges(pairs, R_rel, n, weight=None, edge_keep=None):
    """the header's five conditions -> bool [K]"""
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    K = len(pr)
    i, j = pr[:, 0], pr[:, 1]
    u = (i >= 0) & (i < n) & (j >= 0) & (j < n) & (i != j)
    if edge_keep is not None:
        u &= np.asarray(edge_keep).astype(np.uint8) != 0
    with np.errstate(all="ignore"):
        if weight is not None:
            w = np.asarray(weight, np.float64)
            u &= (w > 0.0) & np.isfinite(w)
        r = np.asarray(R_rel, np.float64).reshape(K, 9)
        s = r[:, 0] * r[:, 0]
        for k in range(1, 9):
            s = s + r[:, k] * r[:, k]
        u &= np.abs(s - 3.0) <= 1e-6
    return u


def mul(A, B, tr=False):
    """P = A B (A^T B where tr) on rows of nine: P[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]"""
    A, B = np.broadcast_arrays(A, B)
    P = np.empty(A.shape)
    for i in range(3):
        x0 = np.where(tr, A[..., i], A[..., 3 * i]); x1 = np.where(tr, A[..., 3 + i], A[..., 3 * i + 1]); x2 = np.where(tr, A[..., 6 + i], A[..., 3 * i + 2])
        for j in range(3):
            P[..., 3 * i + j] = (x0 * B[..., j] + x1 * B[..., 3 + j]) + x2 * B[..., 6 + j]
    return P


def mul_bt(P, R):
    """Q = P R^T: Q[i][j] = (P[i][0] R[j][0] + P[i][1] R[j][1]) + P[i][2] R[j][2]"""
    Q = np.empty(P.shape)
    for i in range(3):
        for j in range(3):
            Q[..., 3 * i + j] = (P[..., 3 * i] * R[..., 3 * j] + P[..., 3 * i + 1] * R[..., 3 * j + 1]) + P[..., 3 * i + 2] * R[..., 3 * j + 2]
    return Q


def cayley(a0, a1, a2):
    """Ca(a) on rows of nine, as the header writes it out"""
    b0 = a0 + a0; b1 = a1 + a1; b2 = a2 + a2
    aa = (a0 * a0 + a1 * a1) + a2 * a2; p = 1.0 - aa; d = 1.0 + aa
    return np.stack([(p + b0 * a0) / d, (b0 * a1 - b2) / d, (b0 * a2 + b1) / d, (b1 * a0 + b2) / d, (p + b1 * a1) / d, (b1 * a2 - b0) / d,
                     (b2 * a0 - b1) / d, (b2 * a1 + b0) / d, (p + b2 * a2) / d], -1)


def lane_sum(T, G):
    """T [n, rounds * G] in position order -> the group's sum [n]: lane l adds its positions in ascending order from +0.0, then the butterfly"""
    n = T.shape[0]
    T = T.reshape(n, -1, G)
    acc = np.zeros((n, G))
    for r in range(T.shape[1]):
        acc = acc + T[:, r, :]
    lanes = np.arange(G)
    m = G // 2
    while m >= 1:
        acc = acc + acc[:, lanes ^ m]
        m //= 2
    assert (acc == acc[:, :1]).all() or np.isnan(acc).any()           # every lane holds the same bits
    return acc[:, 0]


def average(pairs, R_rel, n, weight=None, edge_keep=None, R0=None, known=None, root=0, sweeps=200, damping=0.5, robust_deg=5.0, tol=1e-9, G=None,
            broken=None, trace=None):
    """-> (R [n, 3, 3], info [n, 4] int32, step [n], summary [4] int64, edge_cos [K]); trace: a list that takes R after every sweep that ran"""
    G = group() if G is None else G
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    K = len(pr)
    Rr = np.asarray(R_rel, np.float64).reshape(K, 9)
    wt = np.ones(K) if weight is None else np.asarray(weight, np.float64)
    used = used_edges(pr, Rr, n, weight, edge_keep)
    # the half-edges of the used edges, grouped by camera, ascending in h inside a camera
    h = np.arange(2 * K)[np.repeat(used, 2)]
    cam = pr[h >> 1, h & 1] if len(h) else np.zeros(0, np.int64)
    order = np.argsort(cam, kind="stable")
    h = h[order]; hc = cam[order]; he = h >> 1; hs = h & 1
    ho = pr[he, 1 - hs] if len(h) else np.zeros(0, np.int64)
    hw = wt[he]
    H = len(h)
    off = np.searchsorted(hc, np.arange(n + 1))
    deg = np.diff(off)
    rounds = max(1, -(-int(deg.max() if n else 0) // G))
    slot = np.full((n, rounds * G), H, np.int64)                       # H = the padding element
    for c in range(n):
        slot[c, :deg[c]] = np.arange(off[c], off[c + 1])
    kn = (np.arange(n) == root) if known is None else (np.asarray(known).astype(np.uint8) != 0)
    R = np.zeros((n, 9))
    if known is None:
        R[root] = np.eye(3).ravel()
    else:
        R[kn] = np.asarray(R0, np.float64).reshape(n, 9)[kn]
    setsw = np.where(kn, 0, -1).astype(np.int64)
    step = np.full(n, np.nan); opp = np.zeros(n, np.int64)
    tol2 = tol * tol
    s2 = None
    if robust_deg is not None:
        sg = math.tan(robust_deg * (3.141592653589793 / 360.0)); s2 = sg * sg
    damp = 1.0 if broken == "no_damping" else damping

    def sweep(s, R, setsw, step, sel):
        """the new state of the cameras in sel (bool [n]) from the state (R, setsw, step); the others are copied"""
        with np.errstate(all="ignore"):
            oset = setsw[ho] >= 0
            tr = (hs == 1) if broken == "transpose" else (hs == 0)
            P = mul(Rr[he], R[ho], tr)
            Rn = R.copy(); sn = setsw.copy(); stn = step.copy(); on = np.zeros(n, np.int64)
            chg = False
            # not set: the heaviest half-edge whose other end is set, ties to the lowest position
            start = sel & ~kn & (setsw < 0)
            wpad = np.append(np.where(oset, hw, -np.inf), -np.inf)[slot]
            bp = np.argmax(wpad, axis=1)
            has = start & (wpad[np.arange(n), bp] > -np.inf)
            if has.any():
                Rn[has] = P[slot[has, bp[has]]]; sn[has] = s; chg = True
            # set and not known
            move = sel & ~kn & (setsw >= 0)
            Q = mul_bt(P, R[hc])
            q = 1.0 + ((Q[:, 0] + Q[:, 4]) + Q[:, 8])
            good = oset & (q > Q_MIN)
            w0 = (Q[:, 7] - Q[:, 5]) / q; w1 = (Q[:, 2] - Q[:, 6]) / q; w2 = (Q[:, 3] - Q[:, 1]) / q
            f = hw
            if s2 is not None:
                m = (w0 * w0 + w1 * w1) + w2 * w2; g = s2 / (s2 + m)
                f = f * (g * g)
            terms = [f, f * w0, f * w1, f * w2]
            S, W0, W1, W2 = [lane_sum(np.append(np.where(good, t, 0.0), 0.0)[slot], G) for t in terms]
            on[move] = np.append((oset & ~good).astype(np.int64), 0)[slot].sum(1)[move]
            upd = move & (S > 0.0)
            u0 = W0 / S; u1 = W1 / S; u2 = W2 / S
            st = (u0 * u0 + u1 * u1) + u2 * u2
            N = mul(cayley(damp * u0, damp * u1, damp * u2), R)
            Rn[upd] = N[upd]; stn[upd] = st[upd]
            chg = chg or bool((st[upd] > tol2).any())
        return Rn, sn, stn, on, chg

    every = np.ones(n, bool)
    changed = [True]; last = 0
    for s in range(1, sweeps + 1):
        if not changed[s - 1]:
            break
        last = s
        if broken == "gauss_seidel":
            chg = False; on = np.zeros(n, np.int64)
            for c in range(n):
                R, setsw, step, o1, c1 = sweep(s, R, setsw, step, np.arange(n) == c)
                on[c] = o1[c]; chg = chg or c1
            opp = on
        else:
            R, setsw, step, opp, chg = sweep(s, R, setsw, step, every)
        changed.append(chg)
        if trace is not None:
            trace.append(R.reshape(n, 3, 3).copy())
    isset = setsw >= 0
    info = np.zeros((n, 4), np.int32)
    info[:, 0] = deg; info[:, 1] = setsw; info[:, 2] = opp
    info[:, 3] = np.where(kn, KNOWN, np.where(isset, OK, np.where(deg > 0, UNREACHED, ISOLATED)))
    still = changed[last]
    summary = np.array([0 if last == 0 else last - (0 if still else 1), int(isset.sum()), int(used.sum()),
                        NO_ROOT if not kn.any() else MAX_SWEEPS if still else CONVERGED], np.int64)
    cosv = np.full(K, np.nan)
    with np.errstate(all="ignore"):
        i = np.clip(pr[:, 0], 0, n - 1); j = np.clip(pr[:, 1], 0, n - 1)
        T = mul(Rr, R[i]); B = R[j]
        d = [(T[:, 3 * k] * B[:, 3 * k] + T[:, 3 * k + 1] * B[:, 3 * k + 1]) + T[:, 3 * k + 2] * B[:, 3 * k + 2] for k in range(3)]
        c = (((d[0] + d[1]) + d[2]) - 1.0) / 2.0
    ok = used & isset[i] & isset[j]
    cosv[ok] = c[ok]
    return R.reshape(n, 3, 3), info, step, summary, cosv


# ---- scenes ----
def rot(axis, deg):
    """a rotation matrix by Rodrigues' formula (the scenes' generator, not the rule)"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = math.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(t) * Kx + (1 - math.cos(t)) * (Kx @ Kx)


def random_rotations(n, rng, max_deg=180.0):
    return np.stack([rot(rng.normal(size=3), rng.uniform(-max_deg, max_deg)) for _ in range(n)])


def relative(Rg, pairs, rng=None, noise_deg=0.0):
    """R_rel[k] = N_k R_j R_i^T with a random rotation N_k of noise_deg (standard deviation of the angle)"""
    pr = np.asarray(pairs).reshape(-1, 2)
    out = np.empty((len(pr), 3, 3))
    for k, (i, j) in enumerate(pr):
        out[k] = Rg[j] @ Rg[i].T
        if noise_deg:
            out[k] = rot(rng.normal(size=3), rng.normal() * noise_deg) @ out[k]
    return out


def angle_deg(A, B):
    """the angle between rotations [.., 3, 3] in degrees"""
    c = (np.einsum("...ij,...ij->...", A, B) - 1.0) / 2.0
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def gauge_errors(R, Rg, ref=0):
    """the angle in degrees between R[c] and Rg[c] after the gauge is aligned at camera ref: R[c] ~ Rg[c] Rg[ref]^T R[ref]"""
    G = Rg[ref].T @ R[ref]
    return angle_deg(R, Rg @ G)
