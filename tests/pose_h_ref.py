"""The relative pose from a homography on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_h_lists*) restated in
numpy, in three parts.

decompose: the header's rule from H and two cameras to the candidates, one numpy float64 operation per written operator in the header's
order (numpy contracts nothing; + - * / and sqrt are correctly rounded on both sides), so the device's candidates can be demanded bit
for bit.

from_candidates: the per-row rule and the counts GIVEN the candidates and normals of every entry; the ray / midpoint / lambda / cosang
part is tests/pose_ref.py rows_rule itself, the plane-side test and the pure rotation are added here.

candidates_svd: an independent decomposition through numpy.linalg.svd with Faugeras & Lustman's closed form (the device uses the
construction of Ma, Soatto, Kosecka & Sastry from V alone), in no particular order: compared with the device's four as a set, to 1e-9.

The scenes of test_gpu_pose_h.py live here (gpu_scenes) so that test_pose_h_cpu.py can state their margin without a device."""
import functools

import numpy as np

from tests import pose_ref as R

OK, BAD_MODEL, BAD_CAMERA, TRUNCATED, EMPTY, ROTATION = range(6)
TOL = R.TOL
ROT_EPS = 1e-3
f8 = np.float64
jacobi, _det, _dot, _cross = R.jacobi, R._det, R._dot, R._cross          # one restatement of the Jacobi rule for both calls


def h_from_pose(Rm, t, n, d, cam1, cam2):
    """H = K2 (R + t n^T / d) K1^-1 of the plane n . X = d in the frame of camera 1 (x2 ~ H x1)"""
    return R.kmat(cam2) @ (np.asarray(Rm) + np.outer(t, n) / d) @ np.linalg.inv(R.kmat(cam1))


def normalised_g(H, cam1, cam2):
    """step 1 of the rule: (A = G / m as nine float64, status)"""
    H = [f8(x) for x in np.asarray(H, np.float64).reshape(9)]
    fx1, fy1, cx1, cy1 = (f8(x) for x in cam1); fx2, fy2, cx2, cy2 = (f8(x) for x in cam2)
    with np.errstate(all="ignore"):
        A = [None] * 9
        for i in range(3):
            A[3 * i] = H[3 * i] * fx1; A[3 * i + 1] = H[3 * i + 1] * fy1
            A[3 * i + 2] = (H[3 * i] * cx1 + H[3 * i + 1] * cy1) + H[3 * i + 2]
        G = [None] * 9
        for j in range(3):
            G[j] = (A[j] - cx2 * A[6 + j]) / fx2; G[3 + j] = (A[3 + j] - cy2 * A[6 + j]) / fy2; G[6 + j] = A[6 + j]
        m = f8(0.0)
        for x in G:
            if not np.isfinite(x):
                return None, BAD_MODEL
            if abs(x) > m:
                m = abs(x)
        if not m > 0:
            return None, BAD_MODEL
        return [x / m for x in G], OK


def decompose(H, cam1, cam2, rotation_eps=ROT_EPS, broken=None):
    """The header's rule up to the candidates: dict(status = OK | ROTATION | BAD_MODEL, cand [4, 12], normal [4, 3], tod [4], G [3, 3] =
    the normalised matrix of step 3).  broken: "unsorted" leaves sigma in column order, "unnormalised" keeps t = t / d."""
    out = dict(status=BAD_MODEL, cand=np.zeros((4, 12)), normal=np.zeros((4, 3)), tod=np.zeros(4), G=np.zeros((3, 3)))
    A, st = normalised_g(H, cam1, cam2)
    if st != OK:
        return out
    sg, v, b = jacobi(A, sort=broken != "unsorted")
    if not sg[2] > 0 or not min(sg) > 0:
        return out
    with np.errstate(all="ignore"):
        sign = f8(-1.0) if _det(A) < 0 else f8(1.0)
        Gn = [sign * (x / sg[1]) for x in A]
        out["G"] = np.array(Gn).reshape(3, 3)
        if sg[0] - sg[2] <= f8(rotation_eps) * sg[1]:
            u = [[b[i][r] / sg[i] for r in range(3)] for i in range(3)]
            Rm = [(u[0][r] * v[0][c] + u[1][r] * v[1][c]) + u[2][r] * v[2][c] for r in range(3) for c in range(3)]
            if _det(Rm) < 0:
                Rm = [-x for x in Rm]
            if not np.isfinite(Rm).all():
                return out
            out["cand"][0, :9] = Rm; out["status"] = ROTATION
            return out
        s1 = sg[0] / sg[1]; s3 = sg[2] / sg[1]
        h = [[sign * (b[i][r] / sg[1]) for r in range(3)] for i in range(3)]
        p = np.sqrt((f8(1.0) - s3) * (f8(1.0) + s3)); q = np.sqrt((s1 - f8(1.0)) * (s1 + f8(1.0))); w = np.sqrt((s1 - s3) * (s1 + s3))
        for k in range(2):
            if k == 0:
                a = [(p * v[0][c] + q * v[2][c]) / w for c in range(3)]; g = [(p * h[0][r] + q * h[2][r]) / w for r in range(3)]
            else:
                a = [(p * v[0][c] - q * v[2][c]) / w for c in range(3)]; g = [(p * h[0][r] - q * h[2][r]) / w for r in range(3)]
            n = _cross(v[1], a); rn = _cross(h[1], g)
            Rm = [(h[1][r] * v[1][c] + g[r] * a[c]) + rn[r] * n[c] for r in range(3) for c in range(3)]
            T = [((Gn[3 * r] * n[0] + Gn[3 * r + 1] * n[1]) + Gn[3 * r + 2] * n[2]) - rn[r] for r in range(3)]
            tod = np.sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2])
            t = T if broken == "unnormalised" else [x / tod for x in T]
            for sgn, slot in ((f8(1.0), k), (f8(-1.0), k + 2)):
                out["cand"][slot, :9] = Rm; out["cand"][slot, 9:] = [sgn * x for x in t]
                out["normal"][slot] = [sgn * x for x in n]; out["tod"][slot] = tod
    if not (np.isfinite(out["cand"]).all() and np.isfinite(out["normal"]).all() and np.isfinite(out["tod"]).all()):
        return dict(status=BAD_MODEL, cand=np.zeros((4, 12)), normal=np.zeros((4, 3)), tod=np.zeros(4), G=out["G"])
    out["status"] = OK
    return out


# ---- the independent decomposition ----
def candidates_svd(H, cam1, cam2, rotation_eps=ROT_EPS):
    """(status, cand [4, 12], normal [4, 3], t / d [4, 3]) of G = K2^-1 H K1 by numpy's SVD and Faugeras & Lustman's closed form for three
    distinct singular values (which also covers two equal ones); a pure rotation gives one candidate"""
    with np.errstate(all="ignore"):
        G = np.linalg.inv(R.kmat(cam2)) @ np.asarray(H, np.float64).reshape(3, 3) @ R.kmat(cam1)
    if not np.isfinite(G).all() or not G.any():
        return BAD_MODEL, None, None, None
    G = G / np.abs(G).max()
    U, d, Vt = np.linalg.svd(G)
    if not d[2] > 0:
        return BAD_MODEL, None, None, None
    G = G / d[1] * (1.0 if np.linalg.det(G) > 0 else -1.0)
    U, d, Vt = np.linalg.svd(G); V = Vt.T
    s = np.linalg.det(U) * np.linalg.det(V)                           # +1: det G > 0
    if d[0] - d[2] <= rotation_eps:
        Rm = U @ Vt
        return ROTATION, np.concatenate([(Rm * np.sign(np.linalg.det(Rm))).ravel(), np.zeros(3)])[None].repeat(4, 0), None, None
    x1 = np.sqrt((d[0] ** 2 - d[1] ** 2) / (d[0] ** 2 - d[2] ** 2)); x3 = np.sqrt((d[1] ** 2 - d[2] ** 2) / (d[0] ** 2 - d[2] ** 2))
    sin = np.sqrt((d[0] ** 2 - d[1] ** 2) * (d[1] ** 2 - d[2] ** 2)) / ((d[0] + d[2]) * d[1])
    cos = (d[1] ** 2 + d[0] * d[2]) / ((d[0] + d[2]) * d[1])
    cand, nor, tds = [], [], []
    for e1 in (1.0, -1.0):
        for e3 in (1.0, -1.0):
            sn = e1 * e3 * sin
            Rp = np.array([[cos, 0, -sn], [0, 1, 0], [sn, 0, cos]])
            tp = (d[0] - d[2]) * np.array([e1 * x1, 0, -e3 * x3]); npr = np.array([e1 * x1, 0, e3 * x3])
            Rm = s * U @ Rp @ Vt; t = U @ tp; n = V @ npr
            cand.append(np.concatenate([Rm.ravel(), t / np.linalg.norm(t)])); nor.append(n); tds.append(t)
    return OK, np.array(cand), np.array(nor), np.array(tds)


def same_set(cand, normal, ref_cand, ref_normal, tol=TOL):
    """the two lists of four (R, t, n) hold the same four, each number to tol"""
    a = np.concatenate([np.asarray(cand).reshape(4, 12), np.asarray(normal).reshape(4, 3)], 1)
    b = np.concatenate([np.asarray(ref_cand).reshape(4, 12), np.asarray(ref_normal).reshape(4, 3)], 1)
    left = list(range(4))
    for x in a:
        d = [np.abs(x - b[k]).max() for k in left]
        k = int(np.argmin(d))
        if not d[k] <= tol:
            return False
        left.pop(k)
    return True


# ---- the rule given candidates ----
def entry_status(H, cams, i1, i2, b, e, cap, rotation_eps=ROT_EPS):
    """the status of an entry before its rows are looked at, in the header's order of precedence, and its decomposition (or None)"""
    if not 0 <= b <= e <= cap:
        return TRUNCATED, None
    n = len(cams)
    if not (0 <= i1 < n and 0 <= i2 < n):
        return BAD_CAMERA, None
    f = np.array([cams[i1][0], cams[i1][1], cams[i2][0], cams[i2][1]])
    if not np.isfinite(f).all() or (f == 0).any():
        return BAD_CAMERA, None
    dec = decompose(H, cams[i1], cams[i2], rotation_eps)
    return dec["status"], dec


def cam_rows(sc, p):
    return (2 * p, 2 * p + 1) if sc["idx"] is None else (int(sc["idx"][p, 0]), int(sc["idx"][p, 1]))


def from_candidates(sc, cands=None, normals=None, broken=None):
    """The whole call on a scene.  cands [K, 4, 12] and normals [K, 4, 3]: the device's own; None: the restatement's (decompose).  The
    status of an entry before its rows is always the restatement's.  broken: "no_side" drops the plane-side test, "unsorted" and
    "unnormalised" go to decompose.  Returns dict(pose, front, info, normal, t_over_d, X, depth, cosang, cand, cand_normal, cand_front)."""
    pts, off, cams = sc["pts"], sc["off"], sc["cams"]
    K = len(off) - 1; cap = len(pts); cm = sc["cos_min"] if "cos_min" in sc else R.cos_min(sc["deg"]); eps = sc.get("rotation_eps", ROT_EPS)
    out = dict(pose=np.zeros((K, 12)), front=np.zeros(cap, np.uint8), info=np.zeros((K, 5), np.int32), normal=np.zeros((K, 3)),
               t_over_d=np.zeros(K), X=np.full((cap, 3), np.nan), depth=np.full((cap, 2), np.nan), cosang=np.full(cap, np.nan),
               cand=np.zeros((K, 4, 12)), cand_normal=np.zeros((K, 4, 3)), cand_front=np.zeros((K, 4), np.int32))
    for p in range(K):
        b, e = int(off[p]), int(off[p + 1])
        i1, i2 = cam_rows(sc, p)
        st, dec = entry_status(sc["H"][p], cams, i1, i2, b, e, cap, eps)
        if broken in ("unsorted", "unnormalised") and dec is not None:
            dec = decompose(sc["H"][p], cams[i1], cams[i2], eps, broken); st = dec["status"]
        if st not in (OK, ROTATION):
            out["info"][p, 4] = st
            continue
        cd = dec["cand"] if cands is None else np.asarray(cands[p], np.float64).reshape(4, 12)
        nr = dec["normal"] if normals is None else np.asarray(normals[p], np.float64).reshape(4, 3)
        out["cand"][p] = cd; out["cand_normal"][p] = nr
        use = np.ones(e - b, bool) if sc["keep"] is None else sc["keep"][b:e] != 0
        if not use.any():
            out["info"][p, 4] = EMPTY
            continue
        rows = pts[b:e]; c1, c2 = cams[i1], cams[i2]
        idx = b + np.flatnonzero(use)
        with np.errstate(all="ignore"):
            d1x = (rows[:, 0] - f8(c1[2])) / f8(c1[0]); d1y = (rows[:, 1] - f8(c1[3])) / f8(c1[1])
            if st == ROTATION:
                Rm = cd[0]
                fr = use & ((Rm[6] * d1x + Rm[7] * d1y) + Rm[8] > 0)
                cs = R.rows_rule(cd[0], c1, c2, rows)[2]
                out["pose"][p] = cd[0]; out["cand_front"][p, 0] = int(fr.sum())
                out["info"][p] = [int(use.sum()), int(fr.sum()), 0, 0, ROTATION]
                out["front"][idx] = fr[use]; out["cosang"][idx] = cs[use]
                continue
            res = [R.rows_rule(cd[q], c1, c2, rows) for q in range(4)]
            side = [(nr[q][0] * d1x + nr[q][1] * d1y) + nr[q][2] > 0 for q in range(4)]
            fr = [use & (r[0] > 0) & (r[1] > 0) & (True if broken == "no_side" else s) for r, s in zip(res, side)]
            cnt = [int(f.sum()) for f in fr]
            q = int(np.argmax(cnt))
            l1, l2, cs, X, _ = res[q]
            wide = fr[q] & (cs <= cm)
        out["pose"][p] = cd[q]; out["normal"][p] = nr[q]; out["t_over_d"][p] = dec["tod"][q]
        out["cand_front"][p] = cnt
        out["info"][p] = [int(use.sum()), cnt[q], max(c for k, c in enumerate(cnt) if k != q), int(wide.sum()), OK]
        out["front"][idx] = fr[q][use]
        out["X"][idx] = X[use]; out["depth"][idx, 0] = l1[use]; out["depth"][idx, 1] = l2[use]; out["cosang"][idx] = cs[use]
    return out


# ---- scenes ----
def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def planar_rows(n, Rm, t, nrm, d, c1, c2, seed, sigma=0.0, outliers=0.0):
    """n rows of points on the plane nrm . X = d (camera 1's frame) seen by camera 1 at the origin and camera 2 at X2 = Rm X + t"""
    rng = np.random.default_rng([seed, n])
    x = np.stack([rng.uniform(-0.45, 0.45, n), rng.uniform(-0.35, 0.35, n), np.ones(n)], 1)
    i = np.arange(n); odd = i % 2 == 1; c = (i // 2 + i // 64) % 4          # every other row near a corner of the field, all four in turn
    x[odd, 0] = np.where(c[odd] & 1, 0.45, -0.45) * rng.uniform(0.9, 1.0, int(odd.sum()))
    x[odd, 1] = np.where(c[odd] & 2, 0.35, -0.35) * rng.uniform(0.9, 1.0, int(odd.sum()))
    X = x * (d / (x @ nrm))[:, None]
    Y = X @ np.asarray(Rm).T + t
    p1 = np.stack([c1[0] * x[:, 0] + c1[2], c1[1] * x[:, 1] + c1[3]], 1) + rng.normal(0, sigma, (n, 2))
    p2 = np.stack([c2[0] * Y[:, 0] / Y[:, 2] + c2[2], c2[1] * Y[:, 1] / Y[:, 2] + c2[3]], 1) + rng.normal(0, sigma, (n, 2))
    bad = rng.random(n) < outliers
    p2[bad] = np.stack([rng.uniform(0, 1000, int(bad.sum())), rng.uniform(0, 750, int(bad.sum()))], 1)
    return np.ascontiguousarray(np.concatenate([p1, p2], 1))


def rotation_rows(n, Rm, c1, c2, seed, sigma=0.0):
    rng = np.random.default_rng([seed, n, 1])
    x = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.3, 0.3, n), np.ones(n)], 1)
    Y = x @ np.asarray(Rm).T
    p1 = np.stack([c1[0] * x[:, 0] + c1[2], c1[1] * x[:, 1] + c1[3]], 1) + rng.normal(0, sigma, (n, 2))
    p2 = np.stack([c2[0] * Y[:, 0] / Y[:, 2] + c2[2], c2[1] * Y[:, 1] / Y[:, 2] + c2[3]], 1) + rng.normal(0, sigma, (n, 2))
    return np.ascontiguousarray(np.concatenate([p1, p2], 1))


# The generator's poses.  A homography leaves two poses that pass every test on rows with n . d1 > 0 under both normals, so a scene tells
# them apart only where the other solution's plane cuts the field of view: these poses (sideways baselines, found by a search over a coarse
# grid) have the other normal within 0.1 of perpendicular to the optical axis and every corner of the field at least 0.08 off its plane.
POSES = [
    (rot([-0.8, -0.7, 0.4], 6.0), np.array([0.8, -0.4, 0.0]), np.array([0.2, -0.5, 1.0]), 6.5),
    (rot([-0.7, 0.3, -0.4], 12.0), np.array([-0.5, -1.2, 0.1]), np.array([-0.2, -0.3, 1.0]), 6.5),
    (rot([0.7, -0.1, -0.1], -13.0), np.array([-0.5, -1.3, 0.2]), np.array([-0.1, 0.7, 1.0]), 6.5),
    (rot([-0.7, 1.0, 0.3], -10.0), np.array([0.7, 0.1, 0.1]), np.array([-0.7, 0.6, 1.0]), 3.0),
    (rot([0.6, -1.0, -1.0], -16.0), np.array([-1.3, -1.3, 0.2]), np.array([0.4, 0.2, 1.0]), 6.5),
    (rot([-0.7, 0.7, 0.7], 2.0), np.array([0.3, -0.6, 0.0]), np.array([0.5, -0.1, 1.0]), 7.0),
]
ROTS = [rot([0.1, 1.0, 0.0], 25.0), rot([1.0, 0.2, 0.3], -10.0), rot([0.2, -0.3, 1.0], 30.0)]


def pose_of(k):
    Rm, t, n, d = POSES[k % len(POSES)]
    return Rm, t, n / np.linalg.norm(n), d


def planar_entry(n, k, seed, by_index=False, **kw):
    """entry k: pose k of POSES under the cameras of pair k of pose_ref.PAIRS -> (rows, H, cam1 | i, cam2 | j)"""
    i, j = R.PAIRS[k % len(R.PAIRS)]
    c1, c2 = R.cam_of(i), R.cam_of(j)
    Rm, t, nrm, d = pose_of(k)
    rows = planar_rows(n, Rm, t, nrm, d, c1, c2, seed, **kw)
    H = h_from_pose(Rm, t, nrm, d, c1, c2)
    return (rows, H, i, j) if by_index else (rows, H, c1, c2)


def rotation_entry(n, k, seed, by_index=False, **kw):
    i, j = R.PAIRS[k % len(R.PAIRS)]
    c1, c2 = R.cam_of(i), R.cam_of(j)
    Rm = ROTS[k % len(ROTS)]
    H = R.kmat(c2) @ Rm @ np.linalg.inv(R.kmat(c1))
    rows = rotation_rows(n, Rm, c1, c2, seed, **kw)
    return (rows, H, i, j) if by_index else (rows, H, c1, c2)


def truth(k, rotation=False):
    """(R, t / |t|, n, |t| / d) of entry k"""
    if rotation:
        return ROTS[k % len(ROTS)], np.zeros(3), np.zeros(3), 0.0
    Rm, t, nrm, d = pose_of(k)
    return Rm, t / np.linalg.norm(t), nrm, float(np.linalg.norm(t) / d)


def _scene(entries, deg, **kw):
    sc = R._scene(entries, deg, **kw)
    sc["H"] = sc.pop("F")
    return sc


LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


def near_rotation_h(ratio, c1, c2):
    """a homography whose sigma1 - sigma3 is `ratio` times sigma2 to a part in 1e6: R + t n^T with a short t that is neither parallel nor
    perpendicular to R n (three distinct singular values), its length found by three secant steps on numpy's singular values"""
    Rm = ROTS[0]; n = np.array([0.0, 0.0, 1.0]); u = Rm @ np.array([0.6, 0.0, 0.8])
    mag = ratio
    for _ in range(3):
        d = np.linalg.svd(Rm + mag * np.outer(u, n), compute_uv=False)
        if d[0] > d[2]:
            mag = mag * ratio / ((d[0] - d[2]) / d[1])
    return R.kmat(c2) @ (Rm + mag * np.outer(u, n)) @ np.linalg.inv(R.kmat(c1)), Rm, mag * u


@functools.lru_cache(maxsize=None)
def gpu_scenes():
    S = {}
    # entry lengths at the edges of a wave, of a load of the workgroup and of a step; noise and outliers, so that front and wide vary
    S["lengths"] = _scene([planar_entry(n, k, 31, sigma=0.3, outliers=0.2) for k, n in enumerate(LENGTHS)], 2.0, lead=3, tail=5)
    S["lengths_exact"] = _scene([planar_entry(n, k + 2, 32) for k, n in enumerate(LENGTHS)], 1.5)
    # keep: the last (partly filled) wave only, one row per wave, all zero; empty entries first, last and between; cameras by index
    ents = [planar_entry(0, 0, 33, True), planar_entry(1100, 1, 33, True, sigma=0.2), planar_entry(0, 2, 33, True),
            planar_entry(700, 3, 33, True, sigma=0.2), planar_entry(90, 4, 33, True), rotation_entry(70, 5, 33, True), planar_entry(0, 5, 33, True)]
    sc = _scene(ents, 2.0, by_index=True)
    keep = np.zeros(len(sc["pts"]), np.uint8)
    b = int(sc["off"][1]); keep[b + 1088:b + 1100] = 1
    b = int(sc["off"][3]); keep[b + 3:b + 700:64] = 1
    b = int(sc["off"][5]); keep[b + 64:b + 70] = 1
    sc["keep"] = keep
    S["keep"] = sc
    # 300 entries (past the grid cap) on one table of cameras, every seventh a pure rotation
    S["many"] = _scene([(rotation_entry if k % 7 == 3 else planar_entry)(9 + k % 7, k, 34, True, sigma=0.1) for k in range(300)], 1.0, by_index=True)
    # a non-zero first offset, a range across cap, one beyond it, a decreasing pair
    sc = _scene([planar_entry(30, 1, 35, sigma=0.1), planar_entry(40, 2, 35, sigma=0.1)], 1.0, lead=10, tail=20)
    e0, e1 = sc["H"].copy(), sc["cams"].copy()
    sc["off"] = np.array([10, 40, 120, 130, 40, 80], np.int64)          # entries: ok | across | beyond | decreasing | ok (the rows of entry 1)
    sc["H"] = np.array([e0[0], e0[1], e0[1], e0[1], e0[1]]); sc["cams"] = np.concatenate([e1[0:2], e1[2:4], e1[2:4], e1[2:4], e1[2:4]])
    S["offsets"] = sc
    # models: zero, one NaN, one inf, x 1e150, x 1e-150, rank 2 exactly, rank 2 to rounding, a reflection (det < 0 as given)
    sc = _scene([planar_entry(40, k, 36, sigma=0.1) for k in range(8)], 1.0)
    sc["H"][0] = 0.0; sc["H"][1, 4] = np.nan; sc["H"][2, 0] = np.inf; sc["H"][3] *= 1e150; sc["H"][4] *= 1e-150
    Hm = sc["H"][6].reshape(3, 3).copy(); Hm[2] = 0.5 * Hm[0] - 2.0 * Hm[1]; sc["H"][6] = Hm.ravel()
    sc["H"][7] *= -1.0
    sc["H"][5].reshape(3, 3)[:, 0] = 0.0                               # rank 2 with a column of zeros: sigma3 is exactly 0
    S["models"] = sc
    # cameras: fx = 0, fy NaN, fx inf (of camera 2), an index below and one beyond the table, and one that is fine
    sc = _scene([planar_entry(20, k, 37, True, sigma=0.1) for k in range(6)], 1.0, by_index=True)
    sc["cams"] = np.concatenate([sc["cams"], [[0.0, 790, 500, 375], [800, np.nan, 500, 375], [np.inf, 790, 500, 375]]])
    sc["idx"][0, 0] = 8; sc["idx"][1, 0] = 9; sc["idx"][2, 1] = 10; sc["idx"][3, 0] = -1; sc["idx"][4, 1] = 11
    S["cameras"] = sc
    # rows that are not finite, and one that is huge, among good ones
    sc = _scene([planar_entry(100, 2, 38, sigma=0.1), planar_entry(300, 5, 38, sigma=0.1)], 1.0)
    sc["pts"][5, 0] = np.nan; sc["pts"][17, 3] = np.inf; sc["pts"][64, 1] = -np.inf; sc["pts"][99] = 1e300; sc["pts"][100 + 256, 2] = np.nan
    S["bad_rows"] = sc
    # models as an estimator returns them
    rng = np.random.default_rng(40)
    sc = _scene([planar_entry(60, k, 40, sigma=0.2) for k in range(8)], 1.0)
    sc["H"] = sc["H"] * (1.0 + 1e-4 * rng.normal(size=sc["H"].shape))
    S["noisy_models"] = sc
    # pure rotations, exact and as an estimator returns them, and a model just on either side of rotation_eps
    ents = [rotation_entry(50, k, 41, sigma=0.1) for k in range(4)]
    c1, c2 = R.cam_of(0), R.cam_of(7)
    Hn, Rm, _ = near_rotation_h(0.5e-3, c1, c2)
    ents.append((rotation_rows(50, Rm, c1, c2, 41), Hn, c1, c2))
    # just beyond rotation_eps: a baseline of a thousandth of the plane's distance, 7 rows of that plane (nothing tells its two solutions apart)
    Hn, Rm, t = near_rotation_h(2e-3, c1, c2)
    ents.append((planar_rows(7, Rm, t, np.array([0.0, 0.0, 1.0]), 1.0, c1, c2, 41), Hn, c1, c2))
    sc = _scene(ents, 1.0)
    sc["H"][2:4] = sc["H"][2:4] * (1.0 + 1e-5 * rng.normal(size=sc["H"][2:4].shape))
    S["rotations"] = sc
    # a plane seen from behind: the rows are where the generator's plane is not (x1 mirrored through the principal point of a plane whose
    # points then lie behind camera 1), so no candidate has them all in front
    sc = _scene([planar_entry(40, 1, 42), planar_entry(40, 2, 42)], 1.0)
    sc["pts"][:40, 2:] = 2 * np.array([R.cam_of(2)[2], R.cam_of(2)[3]]) - sc["pts"][:40, 2:]
    S["behind"] = sc
    return S
