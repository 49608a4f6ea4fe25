"""The relative pose on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_lists*) restated in numpy, in three parts.

decompose: the header's rule from F and two cameras to the four candidates, one numpy float64 operation per written operator in the header's
order (numpy contracts nothing; + - * / and sqrt are correctly rounded on both sides), so the device's candidates can be demanded bit for
bit.  Its Jacobi rule (jacobi) is the one that tests/pose_h_ref.py decomposes the calibrated homography with.

from_candidates: the per-row rule and the counts GIVEN the four candidates of every entry, in the header's operation order.  Every line
below is one numpy ufunc on float64 (arrays over the rows of an entry: an elementwise ufunc is the scalar IEEE operation per element,
numpy contracts nothing), every sum of three terms is (first + second) + third, so the results can be demanded bit for bit.

candidates_svd: an independent decomposition of E = K2^T F K1 with numpy.linalg.svd (Hartley & Zisserman 9.6.2), in no particular order
and with none of the header's operation orders: the device's four candidates are compared with it as a set, to 1e-9.  A Jacobi rule
that sweeps its column pairs in another order passes that comparison and fails the bitwise one (broken="order").

The scenes of test_gpu_pose.py live here (gpu_scenes) so that test_pose_cpu.py can state their margin without a device."""
import functools

import numpy as np

from pydegensac_amd import synthetic as syn

OK, BAD_MODEL, BAD_CAMERA, TRUNCATED, EMPTY = range(5)
TOL = 1e-9                                                             # the project's model tolerance
SWEEPS = 6
f8 = np.float64


def cos_min(deg):
    return float(np.cos(np.deg2rad(float(deg))))


def kmat(c):
    return np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]])


def f_from_pose(R, t, cam1, cam2):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return np.linalg.inv(kmat(cam2)).T @ tx @ R @ np.linalg.inv(kmat(cam1))


def relative(poses, i, j):
    """(R, t / |t|) of X_j = R X_i + t for two cameras of synthetic.collection_cameras"""
    (Ri, ti), (Rj, tj) = poses[i], poses[j]
    R = Rj @ Ri.T; t = tj - R @ ti
    return R, t / np.linalg.norm(t)


# ---- part 0: the decomposition, operation for operation ----
def _det(M):
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6])


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def jacobi(A, sort=True, broken=None):
    """the one-sided Jacobi rule of the pose calls on nine float64 -> (sigma [3], v [3][3] columns, b [3][3] columns), sorted descending.
    broken="order": the column pairs of a sweep as (0 1) (1 2) (0 2), which converges as well and rounds differently."""
    v = [[f8(1), f8(0), f8(0)], [f8(0), f8(1), f8(0)], [f8(0), f8(0), f8(1)]]
    b = [[A[0], A[3], A[6]], [A[1], A[4], A[7]], [A[2], A[5], A[8]]]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for i, j in ((0, 1), (1, 2), (0, 2)) if broken == "order" else ((0, 1), (0, 2), (1, 2)):
                al, be, ga = _dot(b[i], b[i]), _dot(b[j], b[j]), _dot(b[i], b[j])
                if ga != 0:
                    z = (be - al) / (f8(2.0) * ga)
                    t = (f8(1.0) if z >= 0 else f8(-1.0)) / (abs(z) + np.sqrt(f8(1.0) + z * z))
                    c = f8(1.0) / np.sqrt(f8(1.0) + t * t); s = c * t
                    for k in range(3):
                        x, y, p, q = b[i][k], b[j][k], v[i][k], v[j][k]
                        b[i][k] = c * x - s * y; b[j][k] = s * x + c * y; v[i][k] = c * p - s * q; v[j][k] = s * p + c * q
        sg = [np.sqrt(_dot(x, x)) for x in b]
    if sort:
        for i, j in ((0, 1), (1, 2), (0, 1)):
            if sg[j] > sg[i]:
                sg[i], sg[j] = sg[j], sg[i]; v[i], v[j] = v[j], v[i]; b[i], b[j] = b[j], b[i]
    return sg, v, b


def decompose(F, cam1, cam2, broken=None):
    """The header's rule from F and two cameras (focal lengths finite and not zero) up to the candidates: dict(status = OK | BAD_MODEL,
    cand [4, 12], c2 [4, 3], rotated = whether any Jacobi rotation was applied, det = the determinants of Ra and Rb before their flip).
    BAD_MODEL leaves zeros.  broken: "order" goes to jacobi."""
    out = dict(status=BAD_MODEL, cand=np.zeros((4, 12)), c2=np.zeros((4, 3)), rotated=False, det=(f8(0), f8(0)))
    F = [f8(x) for x in np.asarray(F, np.float64).reshape(9)]
    fx1, fy1, cx1, cy1 = (f8(x) for x in cam1); fx2, fy2, cx2, cy2 = (f8(x) for x in cam2)
    with np.errstate(all="ignore"):
        G = [None] * 9; E = [None] * 9
        for i in range(3):
            G[3 * i] = F[3 * i] * fx1; G[3 * i + 1] = F[3 * i + 1] * fy1
            G[3 * i + 2] = (F[3 * i] * cx1 + F[3 * i + 1] * cy1) + F[3 * i + 2]
        for j in range(3):
            E[j] = fx2 * G[j]; E[3 + j] = fy2 * G[3 + j]
            E[6 + j] = (cx2 * G[j] + cy2 * G[3 + j]) + G[6 + j]
        m = f8(0.0)
        for x in E:
            if not np.isfinite(x):
                return out
            if abs(x) > m:
                m = abs(x)
        if not m > 0:
            return out
        A = [x / m for x in E]
        sg, v, b = jacobi(A, broken=broken)
        cols = [[A[i], A[3 + i], A[6 + i]] for i in range(3)]          # (columns that are orthogonal as given stay as they are: ga == 0 throughout)
        out["rotated"] = any(_dot(cols[i], cols[j]) != 0 for i, j in ((0, 1), (0, 2), (1, 2)))
        if not sg[1] > 0:
            return out
        u1 = [b[0][r] / sg[0] for r in range(3)]; u2 = [b[1][r] / sg[1] for r in range(3)]
        t = _cross(u1, u2)
        nrm = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        t = [x / nrm for x in t]
        Ra = [(u2[r] * v[0][c] - u1[r] * v[1][c]) + t[r] * v[2][c] for r in range(3) for c in range(3)]
        Rb = [(u1[r] * v[1][c] - u2[r] * v[0][c]) + t[r] * v[2][c] for r in range(3) for c in range(3)]
        out["det"] = (_det(Ra), _det(Rb))
        if out["det"][0] < 0:
            Ra = [-x for x in Ra]
        if out["det"][1] < 0:
            Rb = [-x for x in Rb]
        if not (np.isfinite(t).all() and np.isfinite(Ra).all() and np.isfinite(Rb).all()):
            return out
        for q in range(4):
            Rm = Ra if q < 2 else Rb; sgn = f8(-1.0) if q & 1 else f8(1.0)
            tq = [sgn * x for x in t]
            out["cand"][q, :9] = Rm; out["cand"][q, 9:] = tq
            out["c2"][q] = [-((Rm[j] * tq[0] + Rm[3 + j] * tq[1]) + Rm[6 + j] * tq[2]) for j in range(3)]
    out["status"] = OK
    return out


def decompose_scene(sc, broken=None):
    """decompose on every entry of a scene -> list of its dicts; None where the entry's range or cameras are refused (the device writes
    zeros there as it does for BAD_MODEL)"""
    out = []
    for p in range(len(sc["off"]) - 1):
        i1, i2 = (2 * p, 2 * p + 1) if sc["idx"] is None else (int(sc["idx"][p, 0]), int(sc["idx"][p, 1]))
        st = entry_status(sc["F"][p], sc["cams"], i1, i2, int(sc["off"][p]), int(sc["off"][p + 1]), len(sc["pts"]))
        out.append(None if st in (TRUNCATED, BAD_CAMERA) else decompose(sc["F"][p], sc["cams"][i1], sc["cams"][i2], broken))
    return out


# ---- part 2: the independent decomposition ----
def candidates_svd(F, cam1, cam2, broken=None):
    """[4, 12] = (R row-major, t) x 4 of E = K2^T F K1; None where E is zero, not finite or of rank < 2"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    if broken == "Ft":
        F = F.T
    if broken == "swap":
        cam1, cam2 = cam2, cam1
    with np.errstate(all="ignore"):
        E = kmat(cam2).T @ F @ kmat(cam1)
    if not np.isfinite(E).all() or not E.any():
        return None
    E = E / np.abs(E).max()
    U, s, Vt = np.linalg.svd(E)
    if not s[1] > 0:
        return None
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    out = []
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            out.append(np.concatenate([R.ravel(), t]))
    return np.array(out)


def same_set(a, b, tol=TOL):
    """the two lists of four candidates hold the same four, each entry to tol (rotations and unit vectors: absolute = relative)"""
    a = np.asarray(a).reshape(4, 12); b = np.asarray(b).reshape(4, 12); left = list(range(4))
    for x in a:
        d = [np.abs(x - b[k]).max() for k in left]
        k = int(np.argmin(d))
        if not d[k] <= tol:
            return False
        left.pop(k)
    return True


# ---- part 1: the rule given candidates ----
def entry_status(F, cams, i1, i2, b, e, cap):
    """the statuses that precede the decomposition, in the header's order of precedence (BAD_MODEL here: E zero or not finite only)"""
    if not 0 <= b <= e <= cap:
        return TRUNCATED
    n = len(cams)
    if not (0 <= i1 < n and 0 <= i2 < n):
        return BAD_CAMERA
    f = np.array([cams[i1][0], cams[i1][1], cams[i2][0], cams[i2][1]])
    if not np.isfinite(f).all() or (f == 0).any():
        return BAD_CAMERA
    with np.errstate(all="ignore"):
        E = kmat(cams[i2]).T @ np.asarray(F, np.float64).reshape(3, 3) @ kmat(cams[i1])
    if not np.isfinite(E).all() or not E.any():
        return BAD_MODEL
    return OK


def rows_rule(cand, cam1, cam2, rows):
    """one candidate (12) on the rows [n, 4] of an entry: (lambda1, lambda2, cosang, X [n, 3], den), one ufunc per IEEE operation"""
    R = np.asarray(cand[:9], np.float64).reshape(3, 3); t = np.asarray(cand[9:], np.float64)
    f8 = np.float64
    c2 = [-((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2]) for j in range(3)]
    x1, y1, x2, y2 = (np.ascontiguousarray(rows[:, k], f8) for k in range(4))
    with np.errstate(all="ignore"):
        d1x = (x1 - f8(cam1[2])) / f8(cam1[0]); d1y = (y1 - f8(cam1[3])) / f8(cam1[1])
        d2x = (x2 - f8(cam2[2])) / f8(cam2[0]); d2y = (y2 - f8(cam2[3])) / f8(cam2[1])
        r2 = [(R[0, j] * d2x + R[1, j] * d2y) + R[2, j] for j in range(3)]
        a = (d1x * d1x + d1y * d1y) + f8(1.0)
        b = (d1x * r2[0] + d1y * r2[1]) + r2[2]
        c = (r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]
        d = (d1x * c2[0] + d1y * c2[1]) + c2[2]
        e = (r2[0] * c2[0] + r2[1] * c2[1]) + r2[2] * c2[2]
        den = a * c - b * b
        l1 = (c * d - b * e) / den
        l2 = (b * d - a * e) / den
        cosang = b / np.sqrt(a * c)
        X = np.stack([f8(0.5) * ((l1 * d1x + c2[0]) + l2 * r2[0]), f8(0.5) * ((l1 * d1y + c2[1]) + l2 * r2[1]),
                      f8(0.5) * ((l1 + c2[2]) + l2 * r2[2])], 1)
    return l1, l2, cosang, X, den


def from_candidates(sc, cands, broken=None):
    """The whole call on a scene given cands [K, 4, 12] (the device's own, or candidates_svd's; an entry whose candidates are None or not
    finite is BAD_MODEL).  Returns dict(pose [K, 12], front [cap] uint8, info [K, 5], X, depth, cosang, cand_front [K, 4])."""
    pts, off, cams = sc["pts"], sc["off"], sc["cams"]
    K = len(off) - 1; cap = len(pts); cm = cos_min(sc["deg"]) if "cos_min" not in sc else sc["cos_min"]
    out = dict(pose=np.zeros((K, 12)), front=np.zeros(cap, np.uint8), info=np.zeros((K, 5), np.int32), X=np.full((cap, 3), np.nan),
               depth=np.full((cap, 2), np.nan), cosang=np.full(cap, np.nan), cand_front=np.zeros((K, 4), np.int32))
    for p in range(K):
        b, e = int(off[p]), int(off[p + 1])
        i1, i2 = (2 * p, 2 * p + 1) if sc["idx"] is None else (int(sc["idx"][p, 0]), int(sc["idx"][p, 1]))
        st = entry_status(sc["F"][p], cams, i1, i2, b, e, cap)
        if st == OK and (cands[p] is None or not np.isfinite(np.asarray(cands[p], np.float64)).all() or not np.asarray(cands[p]).any()):
            st = BAD_MODEL
        if st == OK:
            use = np.ones(e - b, bool) if sc["keep"] is None else sc["keep"][b:e] != 0
            if not use.any():
                st = EMPTY
        if st != OK:
            out["info"][p, 4] = st
            continue
        rows = pts[b:e]
        res = [rows_rule(cands[p][q], cams[i1], cams[i2], rows) for q in range(4)]
        with np.errstate(invalid="ignore"):
            fr = [use & ((r[0] >= 0) & (r[1] >= 0) if broken == "ge" else (r[0] > 0) & (r[1] > 0)) for r in res]
        cnt = [int(f.sum()) for f in fr]
        q = int(np.argmax(cnt))                                        # the first of the largest
        l1, l2, cs, X, _ = res[q]
        with np.errstate(invalid="ignore"):
            wide = fr[q] & (cs <= cm)
        out["pose"][p] = cands[p][q]
        out["cand_front"][p] = cnt
        out["info"][p] = [int(use.sum()), cnt[q], max(c for k, c in enumerate(cnt) if k != q), int(wide.sum()), OK]
        idx = b + np.flatnonzero(use)
        out["front"][idx] = fr[q][use]
        out["X"][idx] = X[use]; out["depth"][idx, 0] = l1[use]; out["depth"][idx, 1] = l2[use]; out["cosang"][idx] = cs[use]
    return out


def svd_candidates_of(sc, broken=None):
    K = len(sc["off"]) - 1; out = []
    for p in range(K):
        i1, i2 = (2 * p, 2 * p + 1) if sc["idx"] is None else (int(sc["idx"][p, 0]), int(sc["idx"][p, 1]))
        n = len(sc["cams"])
        ok = 0 <= i1 < n and 0 <= i2 < n and entry_status(sc["F"][p], sc["cams"], i1, i2, 0, 0, 0) == OK
        out.append(candidates_svd(sc["F"][p], sc["cams"][i1], sc["cams"][i2], broken) if ok else None)
    return out


def reference(sc, broken=None):
    """both parts together: the rule on numpy's own candidates (no device anywhere)"""
    return from_candidates(sc, svd_candidates_of(sc, "Ft" if broken == "Ft" else "swap" if broken == "swap" else None),
                           "ge" if broken == "ge" else None)


def rot_err_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra).reshape(3, 3) @ np.asarray(Rb).reshape(3, 3).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def dir_err_deg(ta, tb):
    c = float(np.dot(ta, tb) / (np.linalg.norm(ta) * np.linalg.norm(tb)))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


# ---- scenes ----
M_CAMS = 8


def cam_of(i, varied=True):
    """intrinsics of image i: every image its own, so that swapped or shifted camera rows show"""
    return np.array([800.0 + 10 * i, 790.0 + 7 * i, 500.0 + 3 * i, 375.0 - 2 * i]) if varied else \
        np.array([syn.FOCAL, syn.FOCAL, syn.IMG_W / 2, syn.IMG_H / 2])


def pair_rows(n, i, j, seed, sigma=0.0, outliers=0.0, varied=True):
    """n rows of the pair (i, j) of collection_cameras(M_CAMS): projections of a random cloud (noise sigma px), a share `outliers` of them
    with a random x2, y2.  Returns (rows [n, 4], F, R, t, cam_i, cam_j)."""
    rng = np.random.default_rng([seed, i, j, n])
    _, poses = syn.collection_cameras(M_CAMS)
    ci, cj = cam_of(i, varied), cam_of(j, varied)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 8, n)], 1)
    p1 = syn._project(kmat(ci), *poses[i], X) + rng.normal(0, sigma, (n, 2)) if n else np.zeros((0, 2))
    p2 = syn._project(kmat(cj), *poses[j], X) + rng.normal(0, sigma, (n, 2)) if n else np.zeros((0, 2))
    bad = rng.random(n) < outliers
    p2[bad] = np.stack([rng.uniform(0, 1000, int(bad.sum())), rng.uniform(0, 750, int(bad.sum()))], 1)
    R, t = relative(poses, i, j)
    return np.ascontiguousarray(np.concatenate([p1, p2], 1)), f_from_pose(R, t, ci, cj), R, t, ci, cj


# Rank-2 matrices, scaled to a largest entry of 1, that are no essential matrices (sigma2 / sigma1 = 0.062, 0.050, 0.127) and on which the
# reference's 3 x 3 routine of the DEGENSAC branch (csrc/dg_mat3.h dg_svd3_right) returns a V with max |V^T V - I| = 0.18, 0.014, 0.19:
# found by a search over random rank-2 matrices with that routine compiled for the host (tests/mat3_host.cpp).  A decomposition that
# starts from that V gives candidates that are no rotations; test_pose_cpu.py checks the property, test_gpu_pose.py the device.
NONORTH_F = [[float.fromhex(x) for x in row] for row in (
    ('0x1.1104b0f61c2d8p-4', '0x1.e10e775d12682p-4', '0x1.906f7306f84dbp-4', '-0x1.4ed533a850422p-1', '-0x1.0000000000000p+0',
     '-0x1.a6274ec477b93p-2', '-0x1.02457a2db9d9fp-4', '-0x1.ddcc1f0c64fcfp-4', '-0x1.cc6aae1935f8dp-4'),
    ('-0x1.2d4af06a147d4p-7', '-0x1.988723601dc3ap-8', '0x1.479ccd7cb386fp-4', '-0x1.3d5cbb1308e42p-4', '0x1.0f42126807371p-3',
     '-0x1.7021731378f29p-4', '0x1.272d333357164p-1', '-0x1.0000000000000p+0', '0x1.74fe02148a53fp-1'),
    ('0x1.d85f2f60c3116p-1', '0x1.025ec4eef9f6bp-3', '-0x1.0000000000000p+0', '-0x1.a9c571b8a0925p-2', '0x1.a1741dbdcc9edp-4',
     '0x1.4d7102abcd7bdp-1', '0x1.78eb50b89b8b4p-5', '-0x1.35822e34e55afp-5', '-0x1.b053c41329b01p-4'))]

PAIRS = [(0, 7), (1, 2), (6, 3), (2, 5), (7, 0), (3, 4), (0, 4), (5, 1)]
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


def _scene(entries, deg, by_index=False, keep=None, lead=0, tail=0):
    """entries: list of (rows, F, cam1 | image i, cam2 | image j).  by_index: the cameras are rows of one table of M_CAMS images."""
    off = np.concatenate([[lead], lead + np.cumsum([len(r[0]) for r in entries])]).astype(np.int64)
    pts = np.full((int(off[-1]) + tail, 4), 123.0)                     # rows that no entry owns are finite and plausible
    for (rows, *_), b in zip(entries, off):
        pts[b:b + len(rows)] = rows
    F = np.array([np.asarray(r[1], np.float64).reshape(9) for r in entries]).reshape(len(entries), 9)
    if by_index:
        cams = np.array([cam_of(i) for i in range(M_CAMS)]); idx = np.array([[r[2], r[3]] for r in entries], np.int32).reshape(-1, 2)
    else:
        cams = np.array([c for r in entries for c in (r[2], r[3])]).reshape(-1, 4); idx = None
    return dict(pts=pts, off=off, F=F, cams=cams, idx=idx, keep=keep, deg=deg)


def _entry(n, k, seed, by_index=False, **kw):
    i, j = PAIRS[k % len(PAIRS)]
    rows, F, R, t, ci, cj = pair_rows(n, i, j, seed, **kw)
    return (rows, F, i, j) if by_index else (rows, F, ci, cj)


@functools.lru_cache(maxsize=None)
def gpu_scenes():
    S = {}
    # entry lengths at the edges of a wave, of a load of the workgroup and of a step; noise and outliers, so that front and wide vary
    S["lengths"] = _scene([_entry(n, k, 11, sigma=0.3, outliers=0.2) for k, n in enumerate(LENGTHS)], 4.0, lead=3, tail=5)
    S["lengths_exact"] = _scene([_entry(n, k + 3, 12) for k, n in enumerate(LENGTHS)], 1.5)
    # keep: the last (partly filled) wave only, one row per wave, all zero; empty entries first, last and between; cameras by index
    ents = [_entry(0, 0, 13, True), _entry(1100, 1, 13, True, sigma=0.2), _entry(0, 2, 13, True), _entry(700, 3, 13, True, sigma=0.2),
            _entry(90, 4, 13, True), _entry(0, 5, 13, True)]
    sc = _scene(ents, 4.0, by_index=True)
    keep = np.zeros(len(sc["pts"]), np.uint8)
    b = int(sc["off"][1]); keep[b + 1088:b + 1100] = 1
    b = int(sc["off"][3]); keep[b + 3:b + 700:64] = 1
    sc["keep"] = keep
    S["keep"] = sc
    # 300 entries (past the grid cap) on one table of cameras: image 0 is in 112 of them
    S["many"] = _scene([_entry(9 + k % 7, k, 14, True, sigma=0.1) for k in range(300)], 2.0, by_index=True)
    # a non-zero first offset, a range across cap, one beyond it, a decreasing pair
    sc = _scene([_entry(30, 1, 15, sigma=0.1), _entry(40, 2, 15, sigma=0.1)], 2.0, lead=10, tail=20)
    e0, e1 = sc["F"].copy(), sc["cams"].copy()
    sc["off"] = np.array([10, 40, 120, 130, 40, 80], np.int64)          # entries: ok | across | beyond | decreasing | ok (the rows of entry 1)
    sc["F"] = np.array([e0[0], e0[1], e0[1], e0[1], e0[1]]); sc["cams"] = np.concatenate([e1[0:2], e1[2:4], e1[2:4], e1[2:4], e1[2:4]])
    S["offsets"] = sc
    # models: zero, one NaN, one inf, x 1e150, x 1e-150, as they are
    ents = [_entry(40, k, 16, sigma=0.1) for k in range(6)]
    sc = _scene(ents, 2.0)
    sc["F"][0] = 0.0; sc["F"][1, 4] = np.nan; sc["F"][2, 0] = np.inf; sc["F"][3] *= 1e150; sc["F"][4] *= 1e-150
    S["models"] = sc
    # cameras: fx = 0, fy NaN, fx inf (of camera 2), an index below and one beyond the table, and one that is fine
    sc = _scene([_entry(20, k, 17, True, sigma=0.1) for k in range(6)], 2.0, by_index=True)
    sc["cams"] = np.concatenate([sc["cams"], [[0.0, 790, 500, 375], [800, np.nan, 500, 375], [np.inf, 790, 500, 375]]])
    sc["idx"][0, 0] = 8; sc["idx"][1, 0] = 9; sc["idx"][2, 1] = 10; sc["idx"][3, 0] = -1; sc["idx"][4, 1] = 11
    S["cameras"] = sc
    # rows that are not finite, and one that is huge, among good ones
    sc = _scene([_entry(100, 2, 18, sigma=0.1), _entry(300, 5, 18, sigma=0.1)], 2.0)
    sc["pts"][5, 0] = np.nan; sc["pts"][17, 3] = np.inf; sc["pts"][64, 1] = -np.inf; sc["pts"][99] = 1e300; sc["pts"][100 + 256, 2] = np.nan
    S["bad_rows"] = sc
    # models as an estimator returns them: no essential matrix under the cameras (sigma1 != sigma2, rank 3 by a hair), sigma1 ~ sigma2
    rng = np.random.default_rng(20)
    sc = _scene([_entry(60, k, 20, sigma=0.2) for k in range(8)], 2.0)
    sc["F"] = sc["F"] * (1.0 + 2e-3 * rng.normal(size=sc["F"].shape))
    S["noisy_models"] = sc
    # rank-2 models that are no essential matrices, on which the reference's 3 x 3 routine returns a V that is not orthogonal; identity
    # cameras (F is E), six rows each in normalised coordinates: what a wrong pair of an exhaustive list looks like
    rng = np.random.default_rng(21)
    one = np.array([1.0, 1.0, 0.0, 0.0])
    S["nonessential"] = _scene([(rng.uniform(-0.5, 0.5, (6, 4)), F, one, one) for F in NONORTH_F], 1.5)
    S["exact"] = exact_scene()
    return S


def exact_scene():
    """identity cameras, R = I, t = (1, 0, 0): F = E = [t]x holds 0 and +-1 only.  Row 0 has x1 = x2 = 0 (d = e = 0: lambda1 = lambda2 = 0
    under every candidate), row 1 has the same point in both images (d1 == r2 under R = I: den = 0), the rest are points in front."""
    rng = np.random.default_rng(19)
    X = np.stack([rng.uniform(-2, 2, 30), rng.uniform(-1.5, 1.5, 30), rng.uniform(4, 8, 30)], 1)
    rows = np.stack([X[:, 0] / X[:, 2], X[:, 1] / X[:, 2], (X[:, 0] + 1.0) / X[:, 2], X[:, 1] / X[:, 2]], 1)
    rows[0] = [0.0, 0.25, 0.0, -0.5]
    rows[1] = [0.125, 0.25, 0.125, 0.25]
    F = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    one = np.array([1.0, 1.0, 0.0, 0.0])
    sc = _scene([(rows, F, one, one)], 1.5)
    sc["fragile"] = True                                             # counts hang on exact zeros: only the device's own candidates state them
    return sc


EDGES = ("rank2", "equal_sigma", "diagonal", "negative_det", "tiny", "huge", "rank1")


@functools.lru_cache(maxsize=None)
def edge_scene():
    """The edges of the decomposition, one entry and one row each, identity cameras (E is F to the bit) but for the two scaled models:
    an exact rank-2 E of small integers (largest entry 8: A = E / m is exact); sigma1 == sigma2 exactly, E = [t]x R of integers from a
    rational rotation; a diagonal E, whose columns are orthogonal as given (ga == 0 skips every rotation); the second one with a column
    halved, whose sigma sort exchanges columns of V an odd number of times, so that Ra has determinant -1 before its flip; a pose's F under
    two real cameras times 1e-150 and times 1e150; a rank-1 E whose columns are b, b / 2, b / 4 (the first rotation of pair (0 1) has z =
    -3 / 4, t = -1 / 2, s = -c / 2 exactly, so s b + c (b / 2) is 0 to the bit, and so on: sigma2 == 0), BAD_MODEL with zeros.
    test_pose_cpu.py asserts each of these properties on the restatement."""
    rng = np.random.default_rng(23)
    one = np.array([1.0, 1.0, 0.0, 0.0])
    Rq = np.array([[1.0, -4, 8], [8, 4, 1], [-4, 7, 4]]); Rq = Rq * np.sign(np.linalg.det(Rq))          # 9 x a rotation
    tx = np.array([[0.0, -2, 2], [2, 0, -1], [-2, 1, 0]])                                                # [t]x of t = (1, 2, 2)
    _, F, _, _, ci, cj = pair_rows(1, 6, 3, 23)
    models = dict(rank2=(np.array([[1.0, 2, 4], [2, -1, 4], [3, 1, 8]]), one, one), equal_sigma=(tx @ Rq, one, one),
                  diagonal=(np.diag([1.0, 1.0, 0.0]), one, one), negative_det=((tx @ Rq) * np.array([0.5, 1.0, 1.0]), one, one),
                  tiny=(F * 1e-150, ci, cj), huge=(F * 1e150, ci, cj), rank1=(np.outer([1.0, 2, 4], [1.0, 0.5, 0.25]), one, one))
    return _scene([(rng.uniform(-0.5, 0.5, (1, 4)), *models[k]) for k in EDGES], 1.5)
