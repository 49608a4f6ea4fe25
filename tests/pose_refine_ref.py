"""The refinement of relative poses on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_refine_lists*) restated in
numpy float64, in the header's operation order: every line is one numpy ufunc per written IEEE operation (arrays over the rows of an entry,
numpy.float64 scalars in the 5 x 5 solve; numpy contracts nothing), a sum of three terms is (a + b) + c, and the 21 sums of a pass are
added per thread (rows i == tau mod 256 in ascending i), per wave (lane l takes v[l] + v[l + m] for m = 32 .. 1) and per workgroup
(((w0 + w1) + w2) + w3) as the kernel adds them.  So the device's outputs can be demanded bit for bit.

`broken` selects one of the wrong rules that test_pose_refine_cpu.py must reject: "nodenom" (the derivative of the denominator dropped
from J), "left" (the generators of a left-multiplied rotation C R with the right-multiplied retraction), "tree" (the wave's sum taken
lane after lane).

The scenes of test_gpu_pose_refine.py live here (gpu_scenes) so that test_pose_refine_cpu.py can look at them without a device."""
import functools

import numpy as np

from tests import pose_ref as P

CONVERGED, STALLED, MAX_TRIALS, SHORT, NOT_FINITE, BAD_POSE, BAD_CAMERA, TRUNCATED = range(8)
f8 = np.float64
T = 256


def cross_mat(x, R):
    """[x]x R: column j is cross(x, column j of R)"""
    X = np.empty((3, 3))
    for j in range(3):
        X[0, j] = x[1] * R[2, j] - x[2] * R[1, j]
        X[1, j] = x[2] * R[0, j] - x[0] * R[2, j]
        X[2, j] = x[0] * R[1, j] - x[1] * R[0, j]
    return X


def model(R, t, broken=None):
    """(Ms [6, 3, 3] = E, G_0 .. G_4; u; v) at the pose (R, t)"""
    with np.errstate(all="ignore"):
        E = cross_mat(t, R)
        m = np.abs(t)
        ax = (2 if m[2] < m[1] else 1) if m[1] < m[0] else (2 if m[2] < m[0] else 0)
        z = f8(0.0)
        c = [np.array([z, -t[2], t[1]]), np.array([t[2], z, -t[0]]), np.array([-t[1], t[0], z])][ax]
        nc = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        u = np.array([c[0] / nc, c[1] / nc, c[2] / nc])
        v = np.array([t[1] * u[2] - t[2] * u[1], t[2] * u[0] - t[0] * u[2], t[0] * u[1] - t[1] * u[0]])
        Ms = np.zeros((6, 3, 3))
        Ms[0] = E
        if broken == "left":                                          # d/dw of [t]x C(w) R: not what the retraction R C(w) does
            for k in range(3):
                ek = np.zeros(3); ek[k] = 1.0
                Ms[1 + k] = cross_mat(t, cross_mat(ek, R))
        else:
            Ms[1, :, 1] = E[:, 2]; Ms[1, :, 2] = -E[:, 1]
            Ms[2, :, 0] = -E[:, 2]; Ms[2, :, 2] = E[:, 0]
            Ms[3, :, 0] = E[:, 1]; Ms[3, :, 1] = -E[:, 0]
        Ms[4] = cross_mat(u, R)
        Ms[5] = cross_mat(v, R)
    return Ms, u, v


def rays(rows, cam1, cam2):
    x1, y1, x2, y2 = (np.ascontiguousarray(rows[:, k], f8) for k in range(4))
    with np.errstate(all="ignore"):
        return ((x1 - f8(cam1[2])) / f8(cam1[0]), (y1 - f8(cam1[3])) / f8(cam1[1]),
                (x2 - f8(cam2[2])) / f8(cam2[0]), (y2 - f8(cam2[3])) / f8(cam2[1]))


def epi(Ms, cam1, cam2, d):
    """epi of every matrix of Ms [m, 3, 3] on every row: (n, a0, a1, b0, b1), each [m, rows]"""
    d1x, d1y, d2x, d2y = d
    M = lambda i, j: Ms[:, i, j][:, None]                              # noqa: E731
    with np.errstate(all="ignore"):
        A0 = (M(0, 0) * d1x + M(0, 1) * d1y) + M(0, 2)
        A1 = (M(1, 0) * d1x + M(1, 1) * d1y) + M(1, 2)
        A2 = (M(2, 0) * d1x + M(2, 1) * d1y) + M(2, 2)
        B0 = (M(0, 0) * d2x + M(1, 0) * d2y) + M(2, 0)
        B1 = (M(0, 1) * d2x + M(1, 1) * d2y) + M(2, 1)
        n = (d2x * A0 + d2y * A1) + A2
        return n, A0 / f8(cam2[0]), A1 / f8(cam2[1]), B0 / f8(cam1[0]), B1 / f8(cam1[1])


def row_terms(Ms, cam1, cam2, d, broken=None):
    """(r [rows], J [5, rows]) under E = Ms[0] and the generators Ms[1:]"""
    n, a0, a1, b0, b1 = epi(Ms, cam1, cam2, d)
    with np.errstate(all="ignore"):
        e = [x[0] for x in (n, a0, a1, b0, b1)]
        s = ((e[1] * e[1] + e[2] * e[2]) + e[3] * e[3]) + e[4] * e[4]
        q = np.sqrt(s)
        r = e[0] / q
        if len(Ms) == 1:
            return r, None
        h = ((e[1] * a0[1:] + e[2] * a1[1:]) + e[3] * b0[1:]) + e[4] * b1[1:]
        J = n[1:] / q if broken == "nodenom" else n[1:] / q - (e[0] * h) / (s * q)
    return r, J


def sums(r, J, use, broken=None):
    """the 21 sums in the kernel's order of addition"""
    n = len(r)
    with np.errstate(all="ignore"):
        terms = [r * r] + [J[k] * r for k in range(5)] + [J[k] * J[l] for k in range(5) for l in range(k, 5)]
        Tm = np.stack(terms) if n else np.zeros((21, 0))
        acc = np.zeros((21, T))
        tau = np.arange(T)
        for base in range(0, n, T):
            i = base + tau; j = np.minimum(i, n - 1)
            ok = (i < n) & use[j]
            acc = np.where(ok, acc + Tm[:, j], acc)                    # a row that is not used adds nothing
        v = acc.reshape(21, 4, 64).copy()
        if broken == "tree":
            w = np.zeros((21, 4))
            for lane in range(64):
                w = w + v[:, :, lane]
        else:
            m = 32
            while m >= 1:
                v[:, :, :m] = v[:, :, :m] + v[:, :, m:2 * m]
                m //= 2
            w = v[:, :, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


A_AT = {(k, l): 6 + 5 * k - k * (k - 1) // 2 + (l - k) for k in range(5) for l in range(k, 5)}


def solve(S, lam):
    """delta of (A + lambda diag A) delta = -g by the header's unpivoted Cholesky; None when a pivot is not > 0"""
    A = lambda k, l: S[A_AT[(min(k, l), max(k, l))]]                    # noqa: E731
    L = np.zeros((5, 5))
    with np.errstate(all="ignore"):
        for j in range(5):
            x = A(j, j) + lam * A(j, j)
            for k in range(j):
                x = x - L[j, k] * L[j, k]
            if not x > 0:
                return None
            L[j, j] = np.sqrt(x)
            for i in range(j + 1, 5):
                z = A(j, i)
                for k in range(j):
                    z = z - L[i, k] * L[j, k]
                L[i, j] = z / L[j, j]
        y = np.zeros(5); dl = np.zeros(5)
        for i in range(5):
            x = -S[1 + i]
            for k in range(i):
                x = x - L[i, k] * y[k]
            y[i] = x / L[i, i]
        for i in range(4, -1, -1):
            x = y[i]
            for k in range(i + 1, 5):
                x = x - L[k, i] * dl[k]
            dl[i] = x / L[i, i]
    return dl


def retract(R, t, u, v, dl):
    """(R C(w), (t + delta3 u + delta4 v) / |.|) with the Cayley rotation of w = delta[0 .. 2]"""
    with np.errstate(all="ignore"):
        w = dl[:3]; a = f8(0.5) * w
        aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]; p = f8(1.0) - aa; d = f8(1.0) + aa
        C = np.array([[(p + w[0] * a[0]) / d, (w[0] * a[1] - w[2]) / d, (w[0] * a[2] + w[1]) / d],
                      [(w[1] * a[0] + w[2]) / d, (p + w[1] * a[1]) / d, (w[1] * a[2] - w[0]) / d],
                      [(w[2] * a[0] - w[1]) / d, (w[2] * a[1] + w[0]) / d, (p + w[2] * a[2]) / d]])
        Rn = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                Rn[i, j] = (R[i, 0] * C[0, j] + R[i, 1] * C[1, j]) + R[i, 2] * C[2, j]
        z = np.array([(t[j] + dl[3] * u[j]) + dl[4] * v[j] for j in range(3)])
        nz = np.sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2])
        return Rn, np.array([z[0] / nz, z[1] / nz, z[2] / nz])


def f_of(R, t, cam1, cam2):
    """K2^-T [t]x R K1^-1 in the header's order"""
    with np.errstate(all="ignore"):
        E = cross_mat(t, R); H = np.empty((3, 3)); F = np.empty((3, 3))
        for i in range(3):
            H[i, 0] = E[i, 0] / f8(cam1[0]); H[i, 1] = E[i, 1] / f8(cam1[1])
            H[i, 2] = (E[i, 2] - H[i, 0] * f8(cam1[2])) - H[i, 1] * f8(cam1[3])
        for j in range(3):
            F[0, j] = H[0, j] / f8(cam2[0]); F[1, j] = H[1, j] / f8(cam2[1])
            F[2, j] = (H[2, j] - F[0, j] * f8(cam2[2])) - F[1, j] * f8(cam2[3])
    return F


def refine_entry(rows, use, pose, cam1, cam2, max_trials=20, ftol=1e-12, broken=None, trace=None):
    """One entry whose range and cameras are in order.  Returns dict(pose [12], cost [2], info [4], resid [rows], F [9]); trace (a list)
    receives the 21 sums of the current pose after every pass that was accepted, the start included."""
    pose = np.asarray(pose, f8); n = len(rows)
    nan = f8(np.nan)
    out = dict(pose=pose.copy(), cost=np.array([nan, nan]), info=np.zeros(4, np.int32), resid=np.full(n, np.nan), F=np.zeros(9))
    R = pose[:9].reshape(3, 3).copy(); t = pose[9:].copy()
    with np.errstate(all="ignore"):
        tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    if not np.isfinite(pose).all() or not tt > 0:
        out["pose"][:] = 0.0; out["info"][3] = BAD_POSE
        return out
    d = rays(rows, cam1, cam2)
    used = int(use.sum())
    Ms, u, v = model(R, t, broken)
    S = sums(*row_terms(Ms, cam1, cam2, d, broken), use, broken) if n else np.zeros(21)
    out["info"][0] = used
    out["F"] = f_of(R, t, cam1, cam2).ravel()
    if used < 5:
        out["info"][3] = SHORT
        return out
    if not np.isfinite(S[0]):
        out["info"][3] = NOT_FINITE
        return out
    if trace is not None:
        trace.append(S.copy())
    lam = f8(1e-3); cost0 = S[0]; trials = accepted = 0
    with np.errstate(all="ignore"):
        while True:
            if trials >= max_trials:
                status = MAX_TRIALS
                break
            trials += 1
            dl = solve(S, lam)
            better = False
            if dl is not None:
                Rn, tn = retract(R, t, u, v, dl)
                Mn, un, vn = model(Rn, tn, broken)
                Sn = sums(*row_terms(Mn, cam1, cam2, d, broken), use, broken)
                better = bool(Sn[0] < S[0])
            if better:
                cost = S[0]
                R, t, u, v, S = Rn, tn, un, vn, Sn
                accepted += 1
                lam = np.maximum(lam / f8(10.0), f8(1e-12))
                if trace is not None:
                    trace.append(S.copy())
                if (cost - S[0]) <= f8(ftol) * cost:
                    status = CONVERGED
                    break
            else:
                lam = f8(10.0) * lam
                if lam > 1e12:
                    status = STALLED
                    break
    out["pose"] = np.concatenate([R.ravel(), t]); out["cost"] = np.array([cost0, S[0]]); out["info"][:] = [used, trials, accepted, status]
    r, _ = row_terms(model(R, t)[0][:1], cam1, cam2, d)
    out["resid"][use] = r[use]
    out["F"] = f_of(R, t, cam1, cam2).ravel()
    return out


def reference(sc, max_trials=20, ftol=1e-12, broken=None, pose=None):
    """the whole call on a scene (pts, off, cams, idx, keep, pose): dict(pose [K, 12], cost [K, 2], info [K, 4], resid [cap], F [K, 9])"""
    pts, off, cams = sc["pts"], sc["off"], sc["cams"]
    pose = sc["pose"] if pose is None else pose
    K = len(off) - 1; cap = len(pts)
    out = dict(pose=np.array(pose, f8).reshape(K, 12).copy(), cost=np.full((K, 2), np.nan), info=np.zeros((K, 4), np.int32), resid=np.full(cap, np.nan),
               F=np.zeros((K, 9)))
    for p in range(K):
        b, e = int(off[p]), int(off[p + 1])
        if not 0 <= b <= e <= cap:
            out["info"][p, 3] = TRUNCATED
            continue
        i1, i2 = (2 * p, 2 * p + 1) if sc["idx"] is None else (int(sc["idx"][p, 0]), int(sc["idx"][p, 1]))
        if not (0 <= i1 < len(cams) and 0 <= i2 < len(cams)):
            out["info"][p, 3] = BAD_CAMERA
            continue
        f = np.array([cams[i1][0], cams[i1][1], cams[i2][0], cams[i2][1]])
        if not np.isfinite(f).all() or (f == 0).any():
            out["info"][p, 3] = BAD_CAMERA
            continue
        use = np.ones(e - b, bool) if sc["keep"] is None else sc["keep"][b:e] != 0
        one = refine_entry(pts[b:e], use, out["pose"][p], cams[i1], cams[i2], max_trials, ftol, broken)
        out["pose"][p] = one["pose"]; out["cost"][p] = one["cost"]; out["info"][p] = one["info"]; out["F"][p] = one["F"]
        if one["info"][3] <= MAX_TRIALS:
            out["resid"][b:e] = one["resid"]
    return out


# ---- independent of the restatement ----
def sampson_cost(R, t, cam1, cam2, rows, use=None):
    """sum of squared Sampson distances of F = K2^-T [t]x R K1^-1 in pixels: the textbook formula on numpy's own inverse"""
    F = P.f_from_pose(np.asarray(R).reshape(3, 3), np.asarray(t), cam1, cam2)
    x1 = np.concatenate([rows[:, :2], np.ones((len(rows), 1))], 1); x2 = np.concatenate([rows[:, 2:], np.ones((len(rows), 1))], 1)
    l2 = x1 @ F.T; l1 = x2 @ F
    r2 = np.einsum("ni,ni->n", x2, l2) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)
    return float(r2.sum() if use is None else r2[use].sum())


def perturbed(Rg, tg, seed, deg=3.0):
    """a start pose a few degrees from (Rg, tg): a random rotation on the right, a random tangent step on t"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3); w *= np.tan(np.deg2rad(deg) / 2.0) / np.linalg.norm(w)          # Cayley parameter of a rotation by deg
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    C = np.linalg.solve(np.eye(3) - Wx, np.eye(3) + Wx)
    s = rng.normal(size=3); s -= tg * (s @ tg); s *= np.tan(np.deg2rad(deg)) / np.linalg.norm(s)
    t = tg + s
    return np.concatenate([(Rg @ C).ravel(), t / np.linalg.norm(t)])


# ---- scenes ----
LENGTHS = [0, 1, 4, 5, 6, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]


def _entry(n, k, seed, by_index=False, deg=2.0, **kw):
    i, j = P.PAIRS[k % len(P.PAIRS)]
    rows, F, Rg, tg, ci, cj = P.pair_rows(n, i, j, seed, **kw)
    return ((rows, F, i, j) if by_index else (rows, F, ci, cj)), perturbed(Rg, tg, [seed, k], deg)


def _scene(pairs, **kw):
    sc = P._scene([e for e, _ in pairs], 1.5, **kw)
    sc["pose"] = np.array([q for _, q in pairs]).reshape(len(pairs), 12)
    del sc["F"], sc["deg"]
    return sc


@functools.lru_cache(maxsize=None)
def gpu_scenes():
    S = {}
    # entry lengths at the edges of the rule (4, 5, 6), of a wave, of a load of the workgroup and of a step; a non-zero first offset and
    # rows behind the last entry that no entry owns
    S["lengths"] = _scene([_entry(n, k, 41, sigma=0.3) for k, n in enumerate(LENGTHS)], lead=3, tail=5)
    # keep: the last (partly filled) wave only, one row per wave, exactly 5 of 300, all zero; empty entries first, last and between
    ents = [_entry(0, 0, 43, True), _entry(1100, 1, 43, True, sigma=0.2), _entry(0, 2, 43, True), _entry(700, 3, 43, True, sigma=0.2),
            _entry(300, 4, 43, True, sigma=0.2), _entry(90, 5, 43, True), _entry(0, 6, 43, True)]
    sc = _scene(ents, by_index=True)
    keep = np.zeros(len(sc["pts"]), np.uint8)
    b = int(sc["off"][1]); keep[b + 1088:b + 1100] = 1
    b = int(sc["off"][3]); keep[b + 3:b + 700:64] = 1
    b = int(sc["off"][4]); keep[[b + 2, b + 70, b + 131, b + 255, b + 299]] = 1
    sc["keep"] = keep
    S["keep"] = sc
    # 300 entries (past the grid cap) on one table of cameras
    S["many"] = _scene([_entry(9 + k % 7, k, 44, True, sigma=0.1) for k in range(300)], by_index=True)
    # a non-zero first offset, a range across cap, one beyond it, a decreasing pair
    sc = _scene([_entry(30, 1, 45, sigma=0.1), _entry(40, 2, 45, sigma=0.1)], lead=10, tail=20)
    sc["off"] = np.array([10, 40, 120, 130, 40, 80], np.int64)          # entries: ok | across | beyond | decreasing | ok (the rows of entry 1)
    sc["pose"] = sc["pose"][[0, 1, 1, 1, 1]].copy(); sc["cams"] = np.concatenate([sc["cams"][0:2]] + [sc["cams"][2:4]] * 4)
    sc["pose"][2, 3] = np.nan                                         # TRUNCATED comes before BAD_POSE: copied through as it is
    S["offsets"] = sc
    # start poses: zero, one NaN, one inf, x 1e150, x 1e-150 (the whole pose), t alone x 1e150 and x 1e-150, t of length 1e-170, as it is
    sc = _scene([_entry(40, k, 46, sigma=0.1) for k in range(9)])
    q = sc["pose"]
    q[0] = 0.0; q[1, 4] = np.nan; q[2, 10] = np.inf; q[3] *= 1e150; q[4] *= 1e-150; q[5, 9:] *= 1e150; q[6, 9:] *= 1e-150; q[7, 9:] *= 1e-170
    S["poses"] = sc
    # cameras: fx = 0, fy NaN, fx inf (of camera 2), an index below and one beyond the table, and one that is fine
    sc = _scene([_entry(20, k, 47, True, sigma=0.1) for k in range(6)], by_index=True)
    sc["cams"] = np.concatenate([sc["cams"], [[0.0, 790, 500, 375], [800, np.nan, 500, 375], [np.inf, 790, 500, 375]]])
    sc["idx"][0, 0] = 8; sc["idx"][1, 0] = 9; sc["idx"][2, 1] = 10; sc["idx"][3, 0] = -1; sc["idx"][4, 1] = 11
    S["cameras"] = sc
    # rows that are not finite among good ones (NOT_FINITE), the same rows kept out by keep (a run), and a huge row
    sc = _scene([_entry(100, 2, 48, sigma=0.1), _entry(300, 5, 48, sigma=0.1), _entry(100, 2, 48, sigma=0.1), _entry(80, 3, 48, sigma=0.1)])
    sc["pts"][5, 0] = np.nan; sc["pts"][100 + 256, 2] = np.inf; sc["pts"][400 + 5, 0] = np.nan; sc["pts"][500 + 7] = 1e300
    sc["keep"] = np.ones(len(sc["pts"]), np.uint8); sc["keep"][400 + 5] = 0
    S["bad_rows"] = sc
    # two views from one centre: t is not observable
    S["rotation"] = rotation_scene()
    return S


def rotation_scene():
    rng = np.random.default_rng(49)
    a = 0.3; Rg = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    cam = P.cam_of(0, False); X = np.stack([rng.uniform(-2, 2, 60), rng.uniform(-1.5, 1.5, 60), rng.uniform(4, 8, 60)], 1)
    from pydegensac_amd import synthetic as syn
    rows = np.concatenate([syn._project(P.kmat(cam), np.eye(3), np.zeros(3), X), syn._project(P.kmat(cam), Rg, np.zeros(3), X)], 1)
    rows = rows + rng.normal(0, 0.3, rows.shape)
    sc = P._scene([(rows, np.eye(3), cam, cam)], 1.5)
    sc["pose"] = perturbed(Rg, np.array([0.6, 0.0, 0.8]), 50, 1.0).reshape(1, 12)
    del sc["F"], sc["deg"]
    return sc
