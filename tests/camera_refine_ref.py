"""The rule of mi_degensac_camera_refine_tracks* (include/mi_degensac.h) restated in numpy: float64, one IEEE operation per written
operator (numpy's elementwise + - * / sqrt contract nothing), the sums in the header's order (256 threads, the wave tree, the four
waves).  The device is held to this bit for bit (tests/test_gpu_camera_refine.py); tests/test_camera_refine_cpu.py checks the
restatement itself against independent numpy.  Also the catalogue of scenes both test files share.
A scene is a dict: off [T + 1], obs [M], img [M], nt (None or the device word), kps [rows, 2], cams [n, 4], poses [n, 12], X [T, 3],
keep (None or uint8 [M]), refine (None or uint8 [n])."""
import functools

import numpy as np

CONVERGED, STALLED, MAX_TRIALS, FIXED, BEHIND, NOT_FINITE, SHORT, BAD_POSE, BAD_CAMERA = range(9)
DBL_MAX = np.finfo(np.float64).max
NS = 28
F = np.float64


def _finite(x):
    return np.abs(x) <= DBL_MAX


def table(sc, broken=None):
    """the image-major table of the header: (img_offsets [n + 1] int64, img_obs [M] int32, track_of [M]); an index out of range is never
    used as one"""
    off = sc["off"]; T = len(off) - 1; M = len(sc["obs"]); n = len(sc["cams"]); rows = len(sc["kps"])
    nt = T if sc.get("nt") is None else min(max(int(sc["nt"]), 0), T)
    key = np.full(M, n, np.int64); track_of = np.full(M, -1, np.int64)
    X = sc["X"]; keep = sc.get("keep")
    for k in range(nt):
        b, e = int(off[k]), int(off[k + 1])
        if not (0 <= b <= e <= M) or e == b:
            continue
        p = np.arange(b, e)
        track_of[p] = k
        m = sc["img"][p].astype(np.int64); r = sc["obs"][p].astype(np.int64)
        u = (m >= 0) & (m < n) & (r >= 0) & (r < rows) & bool(_finite(X[k]).all())
        if keep is not None:
            u = u & (keep[p] != 0)
        rr = np.where(u, r, 0)
        if rows:
            u = u & _finite(sc["kps"][rr, 0]) & _finite(sc["kps"][rr, 1])
        key[p] = np.where(u, m, n)
    order = np.argsort(key, kind="stable")
    if broken == "unstable":                                           # descending positions inside an image
        order = np.lexsort((-np.arange(M), key))
    sk = key[order]
    io = np.searchsorted(sk, np.arange(n + 1), side="left").astype(np.int64)
    img_obs = np.where(sk < n, order, -1).astype(np.int32)
    return io, img_obs, track_of


def tree_sum(terms, used):
    """the header's order: terms [L, K] with L a multiple of 256, used [L]; thread tau adds its used terms in ascending i from +0.0, the
    wave tree v[l] + v[l + m] for m = 32 .. 1, then ((w0 + w1) + w2) + w3.  Returns [K]."""
    L, K = terms.shape
    t = terms.reshape(L // 256, 256, K); u = used.reshape(L // 256, 256)
    acc = np.zeros((256, K))
    for s in range(L // 256):
        acc = np.where(u[s][:, None], acc + t[s], acc)
    w = acc.reshape(4, 64, K).copy()
    m = 32
    while m >= 1:
        w[:, :m] = w[:, :m] + w[:, m:2 * m]
        m //= 2
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def project(o, pose, cam):
    """P [3], Zc, u, v, rx, ry of the observations o (x, y, X0, X1, X2: arrays) under the pose [12] and the camera [4]"""
    R = pose[:9]; t = pose[9:]; fx, fy, cx, cy = cam
    X0, X1, X2 = o["X0"], o["X1"], o["X2"]
    P = [(R[3 * i] * X0 + R[3 * i + 1] * X1) + R[3 * i + 2] * X2 for i in range(3)]
    xc = P[0] + t[0]; yc = P[1] + t[1]; zc = P[2] + t[2]
    u = xc / zc; v = yc / zc
    rx = (fx * u + cx) - o["x"]; ry = (fy * v + cy) - o["y"]
    return P, zc, u, v, rx, ry


def jacobian(o, pose, cam):
    """rx, ry, Zc, Jx [6], Jy [6]"""
    fx, fy = cam[0], cam[1]
    P, zc, u, v, rx, ry = project(o, pose, cam)
    ax = fx / zc; ex = (fx * u) / zc; ay = fy / zc; ey = (fy * v) / zc
    zero = np.zeros_like(ax)
    jx = [-(ex * P[1]), ax * P[2] + ex * P[0], -(ax * P[1]), ax, zero, -ex]
    jy = [-(ay * P[2] + ey * P[1]), ey * P[0], ay * P[0], zero, ay, -ey]
    return rx, ry, zc, jx, jy


def one_pass(o, pose, cam):
    """the 28 sums and `behind` of a pass"""
    rx, ry, zc, jx, jy = jacobian(o, pose, cam)
    t = [rx * rx + ry * ry]
    for k in range(6):
        t.append(jx[k] * rx + jy[k] * ry)
    for k in range(6):
        for l in range(k, 6):
            t.append(jx[k] * jx[l] + jy[k] * jy[l])
    s = tree_sum(np.stack(t, -1), o["used"])
    return s, int((o["used"] & ~(zc > 0.0)).sum())


def cayley(w):
    a = [F(0.5) * w[i] for i in range(3)]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]; p = F(1.0) - aa; d = F(1.0) + aa
    return [(p + w[0] * a[0]) / d, (w[0] * a[1] - w[2]) / d, (w[0] * a[2] + w[1]) / d,
            (w[1] * a[0] + w[2]) / d, (p + w[1] * a[1]) / d, (w[1] * a[2] - w[0]) / d,
            (w[2] * a[0] - w[1]) / d, (w[2] * a[1] + w[0]) / d, (p + w[2] * a[2]) / d]


def update(pose, dl, broken=None):
    """R' = C(w) R, t' = t + tau"""
    C = cayley(dl[:3]); R = pose[:9]
    out = np.empty(12)
    for i in range(3):
        for j in range(3):
            if broken == "right":
                out[3 * i + j] = (R[3 * i] * C[j] + R[3 * i + 1] * C[3 + j]) + R[3 * i + 2] * C[6 + j]
            else:
                out[3 * i + j] = (C[3 * i] * R[j] + C[3 * i + 1] * R[3 + j]) + C[3 * i + 2] * R[6 + j]
    for j in range(3):
        out[9 + j] = pose[9 + j] + dl[3 + j]
    return out


def solve(s, lam):
    """delta of the trial from the sums s at lambda; None when a pivot is not > 0"""
    g = s[1:7]; A = s[7:]
    at = lambda k, l: A[6 * k - k * (k - 1) // 2 + (l - k)]           # noqa: E731
    L = [[None] * 6 for _ in range(6)]
    ok = True
    for j in range(6):
        x = at(j, j) + lam * at(j, j)
        for k in range(j):
            x = x - L[j][k] * L[j][k]
        ok = ok and bool(x > 0.0)
        L[j][j] = np.sqrt(x)
        for i in range(j + 1, 6):
            z = at(j, i)
            for k in range(j):
                z = z - L[i][k] * L[j][k]
            L[i][j] = z / L[j][j]
    if not ok:
        return None
    y = [None] * 6; dl = [None] * 6
    for i in range(6):
        x = -g[i]
        for k in range(i):
            x = x - L[i][k] * y[k]
        y[i] = x / L[i][i]
    for i in range(5, -1, -1):
        x = y[i]
        for k in range(i + 1, 6):
            x = x - L[k][i] * dl[k]
        dl[i] = x / L[i][i]
    return dl


def image_obs(sc, pos, track_of):
    """the used observations of one image at the positions pos, padded to a multiple of 256"""
    n = len(pos); L = max((n + 255) // 256 * 256, 256)
    z = lambda a: np.concatenate([a, np.zeros(L - n)])                 # noqa: E731
    r = sc["obs"][pos]; k = track_of[pos]
    return dict(x=z(sc["kps"][r, 0]), y=z(sc["kps"][r, 1]), X0=z(sc["X"][k, 0]), X1=z(sc["X"][k, 1]), X2=z(sc["X"][k, 2]), used=np.arange(L) < n)


def refine_image(o, n, pose, cam, may_move, max_trials=20, ftol=1e-12, broken=None, trace=None):
    """one image: (pose [12], cost0, cost1, trials, accepted, status, scored); trace: a list that takes `behind` of every accepted trial"""
    nan = F(np.nan)
    if not (_finite(cam[0]) and _finite(cam[1]) and cam[0] != 0.0 and cam[1] != 0.0):
        return pose, nan, nan, 0, 0, BAD_CAMERA, False
    if not _finite(pose).all():
        return pose, nan, nan, 0, 0, BAD_POSE, False
    if n < 3:
        return pose, nan, nan, 0, 0, SHORT, False
    s, behind = one_pass(o, pose, cam)
    if not _finite(s[0]):
        return pose, nan, nan, 0, 0, NOT_FINITE, False
    if behind:
        return pose, s[0], s[0], 0, 0, BEHIND, False
    if not may_move:
        return pose.copy(), s[0], s[0], 0, 0, FIXED, True
    cost0 = s[0]; lam = F(1e-3); trials = 0; accepted = 0; cur = pose.copy()
    while True:
        if trials >= max_trials:
            status = MAX_TRIALS
            break
        trials += 1
        dl = solve(s, lam)
        ok = dl is not None
        if ok:
            tri = update(cur, dl, broken)
            s2, behind = one_pass(o, tri, cam)
            ok = bool(s2[0] < s[0]) and (behind == 0 or broken == "no_zc")
        if ok:
            cost = s[0]
            cur = tri; s = s2; accepted += 1
            if trace is not None:
                trace.append(behind)
            lam = max(lam / F(10.0), F(1e-12))
            if (cost - s2[0]) <= F(ftol) * cost:
                status = CONVERGED
                break
        else:
            lam = F(10.0) * lam
            if lam > 1e12:
                status = STALLED
                break
    return cur, cost0, s[0], trials, accepted, status, True


def reference(sc, max_trials=20, ftol=1e-12, broken=None, trace=None):
    """every output of the call on the scene, whole, fills included: dict poses [n, 12], cost [n, 2], info [n, 4], err [M], io [n + 1], iobs [M]"""
    n = len(sc["cams"]); M = len(sc["obs"])
    io, iobs, track_of = table(sc, broken)
    poses = np.array(sc["poses"], np.float64).reshape(n, 12).copy(); cost = np.full((n, 2), np.nan); info = np.zeros((n, 4), np.int32)
    err = np.full(M, np.nan)
    refine = sc.get("refine")
    with np.errstate(all="ignore"):
        for m in range(n):
            pos = iobs[io[m]:io[m + 1]].astype(np.int64); cnt = len(pos)
            o = image_obs(sc, pos, track_of) if cnt else None
            pose, c0, c1, trials, acc, status, scored = refine_image(o, cnt, poses[m].copy(), sc["cams"][m], refine is None or refine[m] != 0,
                                                                     max_trials, ftol, broken, trace)
            poses[m] = pose; cost[m] = (c0, c1); info[m] = (cnt, trials, acc, status)
            if scored:
                _, _, _, _, rx, ry = project(o, pose, sc["cams"][m])
                err[pos] = np.sqrt(rx * rx + ry * ry)[:cnt]
    return dict(poses=poses, cost=cost, info=info, err=err, io=io, iobs=iobs)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def rodrigues(v):
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(v) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def cameras(n, seed=0):
    """n pinhole cameras (f = 800, principal point (500, 400)) that all see the box x in [-2, 2], y in [-1.5, 1.5], z in [4, 8] in front:
    centres within 1.5 of the origin in x, rotations of a few degrees.  Returns (cams [n, 4], poses [n, 12])."""
    rng = np.random.default_rng(1000 + seed)
    cams = np.tile([800.0, 800.0, 500.0, 400.0], (n, 1))
    poses = np.empty((n, 12))
    for i in range(n):
        c = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)])
        R = rodrigues(rng.uniform(-0.08, 0.08, 3))
        poses[i] = np.concatenate([R.ravel(), -R @ c])
    return cams, poses


def perturb(poses, rot=0.01, trans=0.02, seed=0):
    """every pose with a rotation of `rot` radians about a random axis on the left and a translation offset of length `trans`"""
    rng = np.random.default_rng(2000 + seed)
    out = poses.copy()
    for i in range(len(poses)):
        a = rng.normal(size=3); a *= rot / np.linalg.norm(a)
        d = rng.normal(size=3); d *= trans / np.linalg.norm(d)
        out[i, :9] = (rodrigues(a) @ poses[i, :9].reshape(3, 3)).ravel(); out[i, 9:] = poses[i, 9:] + d
    return out


def proj(cams, poses, i, X):
    R = poses[i, :9].reshape(3, 3); Xc = X @ R.T + poses[i, 9:]
    return np.stack([cams[i, 0] * Xc[..., 0] / Xc[..., 2] + cams[i, 2], cams[i, 1] * Xc[..., 1] / Xc[..., 2] + cams[i, 3]], -1)


def make_scene(counts, seed=0, sigma=0.5, first=0, tail=0, T=None, rot=0.01, trans=0.02):
    """image m of len(counts) images observes counts[m] distinct tracks, drawn at random from T tracks (default: the largest count plus
    7); the tables are track-major as the tracks call writes them (inside a track ascending image), every observation has a store row of
    its own (the rows are permuted).  first: positions before the first track; tail: positions behind the last, filled with -1.  The
    poses are the generator's, perturbed; the generator's are in "truth", the points X are the generator's."""
    rng = np.random.default_rng(seed)
    n = len(counts); T = (max(counts) if n else 0) + 7 if T is None else T
    cams, truth = cameras(n, seed)
    X = np.stack([rng.uniform(-2, 2, T), rng.uniform(-1.5, 1.5, T), rng.uniform(4, 8, T)], 1)
    sees = np.zeros((T, n), bool)
    for m, c in enumerate(counts):
        sees[rng.choice(T, c, replace=False), m] = True
    lens = sees.sum(1); Mo = int(lens.sum())
    off = np.concatenate([[first], first + np.cumsum(lens)]).astype(np.int64)
    M = first + Mo + tail
    obs = np.full(M, -1, np.int32); img = np.full(M, -1, np.int32)
    kk, mm = np.nonzero(sees)                                          # track-major, ascending image inside a track
    rows = rng.permutation(Mo + 5)[:Mo].astype(np.int32)
    obs[first:first + Mo] = rows; img[first:first + Mo] = mm
    kps = rng.uniform(0, 1000, (Mo + 5, 2))
    for m in range(n):
        sel = mm == m
        kps[rows[sel]] = proj(cams, truth, m, X[kk[sel]]) + (rng.normal(0, sigma, (int(sel.sum()), 2)) if sigma else 0.0)
    return dict(off=off, obs=obs, img=img, nt=None, kps=np.ascontiguousarray(kps), cams=cams, poses=perturb(truth, rot, trans, seed), X=X, keep=None,
                refine=None, truth=truth)


def _copy(sc):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}


def positions_of(sc, m):
    """the positions of image m in the tables, ascending"""
    return np.flatnonzero(sc["img"] == m)


def mask_scene(seed=3):
    """images of 256, 256 and 300 observations of which only the last 64 (in the image's order), one per 64 and exactly 3 stay used: by
    turns through obs_keep, a row behind the store and a keypoint that is NaN"""
    sc = _copy(make_scene([256, 256, 300, 40], seed=seed, T=320))
    sc["keep"] = np.ones(len(sc["obs"]), np.uint8)
    rules = [lambda i: i >= 192, lambda i: i % 64 == 5, lambda i: i in (7, 150, 299)]
    turn = 0
    for m, rule in enumerate(rules):
        for i, p in enumerate(positions_of(sc, m)):
            if rule(i):
                continue
            turn += 1
            if turn % 3 == 0: sc["keep"][p] = 0                        # noqa: E701
            elif turn % 3 == 1: sc["obs"][p] = len(sc["kps"]) + turn % 4          # noqa: E701
            else: sc["kps"][sc["obs"][p], turn % 2] = np.nan          # noqa: E701
    return sc


def edge_scene(seed=4):
    """the table's edges: tracks with a decreasing pair of offsets, a pair beyond M and a negative one (their positions belong to nobody),
    NaN and inf rows of X, images and rows out of range, keypoints that are not finite, two keypoints of one image in one track"""
    sc = _copy(make_scene([30, 25, 20, 35], seed=seed, T=40, tail=6))
    off = sc["off"]; M = len(sc["obs"])
    # four tracks that own nothing between tracks 9 and 10: beyond M, decreasing, negative (no position is owned twice)
    sc["off"] = np.concatenate([off[:11], [M + 2, M + 1, -3], off[10:]]).astype(np.int64)
    sc["X"] = np.concatenate([sc["X"][:10], np.ones((4, 3)), sc["X"][10:]])
    sc["X"][3] = np.nan; sc["X"][5, 1] = np.inf; sc["X"][7, 2] = -np.inf
    sc["img"][2] = 4; sc["img"][9] = -1; sc["img"][14] = np.iinfo(np.int32).max; sc["img"][15] = np.iinfo(np.int32).min
    sc["obs"][20] = len(sc["kps"]); sc["obs"][21] = -1; sc["obs"][22] = np.iinfo(np.int32).max
    sc["kps"][sc["obs"][30], 0] = np.inf; sc["kps"][sc["obs"][31], 1] = np.nan; sc["kps"][sc["obs"][32], 0] = -np.inf
    k = next(k for k in range(25, len(sc["off"]) - 1) if sc["off"][k + 1] - sc["off"][k] >= 2)
    b = int(sc["off"][k]); sc["img"][b + 1] = sc["img"][b]            # two keypoints of one image in one track
    return sc


def pose_scene(seed=5):
    """poses and cameras that are not usable, each on an image of 20 observations: zeros, NaN, inf, 1e150 and 1e-150 in R and in t, fx = 0,
    fy = inf, fx = NaN, a NaN principal point (which is only a cost that is not finite)"""
    sc = _copy(make_scene([20] * 14, seed=seed, T=60))
    P = sc["poses"]
    P[0] = 0.0; P[1, 4] = np.nan; P[2, 10] = np.inf; P[3, 0] = 1e150; P[4, 11] = 1e150; P[5, :9] *= 1e-150; P[6, 9:] = 1e-150
    P[7, 2] = -np.inf; P[8, :9] *= 1e150
    sc["cams"][9, 0] = 0.0; sc["cams"][10, 1] = np.inf; sc["cams"][11, 0] = np.nan; sc["cams"][12, 2] = np.nan
    return sc


def hand_scene():
    """every status on numbers written by hand.  f = 100, principal point 0, R = I unless said; the points lie at z = 4 (a power of two,
    so that u, v and the keypoints are exact).
    image 0 BAD_CAMERA (fx = 0); 1 BAD_POSE (a NaN in t); 2 SHORT (two observations); 3 NOT_FINITE (t[2] = -4: Zc = 0 exactly); 4 BEHIND
    (t[2] = -20); 5 FIXED (refine = 0), with a residual; 6 STALLED: the keypoints are the exact projections, the cost is 0 and no cost is
    < 0, so every trial is rejected until lambda passes 1e12; 7 CONVERGED from t = (0.05, -0.02, 0.1) on keypoints with a fixed pattern of offsets below a pixel; 8 MAX_TRIALS with max_trials = 2,
    the same start as 7 under a rotation."""
    pts = np.array([[1.0, 2, 4], [-1, 1, 4], [2, -1, 4], [-2, -2, 4], [0.5, 0.25, 4], [1.5, -0.5, 8], [-0.5, 1.5, 8], [0.25, -1.25, 2]])
    T = len(pts); n = 9
    cams = np.tile([100.0, 100.0, 0.0, 0.0], (n, 1)); cams[0, 0] = 0.0
    I = np.eye(3).ravel()
    poses = np.tile(np.concatenate([I, [0.0, 0, 0]]), (n, 1))
    poses[1, 10] = np.nan; poses[3, 11] = -4.0; poses[4, 11] = -20.0
    poses[7, 9:] = [0.05, -0.02, 0.1]
    poses[8, :9] = rodrigues([0.01, -0.02, 0.015]).ravel(); poses[8, 9:] = [0.05, -0.02, 0.1]
    exact = np.stack([100.0 * pts[:, 0] / pts[:, 2], 100.0 * pts[:, 1] / pts[:, 2]], 1)
    kps = []; obs = []; img = []; off = [0]
    per_image = {0: range(T), 1: range(T), 2: (0, 1), 3: range(5), 4: range(T), 5: range(T), 6: range(T), 7: range(T), 8: range(T)}
    for k in range(T):                                                 # track-major: track k, its images ascending
        for m in range(n):
            if k in per_image[m]:
                obs.append(len(kps)); img.append(m)
                noise = [0.37 * ((7 * k) % 5 - 2), 0.21 * ((3 * k) % 7 - 3)] if m in (7, 8) else [0.5, -0.25] if m == 5 else [0.0, 0.0]
                kps.append(exact[k] + noise)
        off.append(len(obs))
    refine = np.ones(n, np.uint8); refine[5] = 0
    return dict(off=np.array(off, np.int64), obs=np.array(obs, np.int32), img=np.array(img, np.int32), nt=None, kps=np.array(kps, np.float64), cams=cams,
                poses=poses, X=pts.copy(), keep=None, refine=refine)


def near_scene(seed=78):
    """points barely in front of cameras that start too close to them: Gauss-Newton steps overshoot, and some trial poses that lower the
    cost put an observation behind the camera.  Such a trial is rejected (found by a search over seeds for a scene on which accepting it
    changes the result)."""
    rng = np.random.default_rng(seed)
    sc = _copy(make_scene([8] * 6, seed=seed, sigma=0.0, T=12, rot=0.0, trans=0.0))
    sc["X"][:, 2] = rng.uniform(0.4, 1.2, len(sc["X"])); sc["X"][:, :2] *= 0.2
    sc["poses"] = sc["truth"].copy()
    _, _, tof = table(sc)
    for p in range(len(sc["obs"])):
        if sc["img"][p] >= 0:
            sc["kps"][sc["obs"][p]] = proj(sc["cams"], sc["truth"], sc["img"][p], sc["X"][tof[p]])
    sc["poses"][:, 11] -= rng.uniform(0.2, 0.38, 6)
    sc["poses"][:, 9:11] += rng.normal(0, 0.1, (6, 2))
    return sc


COUNTS = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]
EMPTY = [0, 0, 50, 0, 0, 0, 40, 30, 0, 20, 0, 0]


@functools.lru_cache(maxsize=None)
def gpu_scenes():
    """the catalogue of tests/test_gpu_camera_refine.py (and of the CPU tests that walk it), built once and never written to"""
    S = {}
    S["counts"] = make_scene(COUNTS, seed=1, first=3, tail=5)
    S["masks"] = mask_scene()
    S["empty"] = make_scene(EMPTY, seed=2, tail=4)
    rng = np.random.default_rng(6)
    S["many"] = make_scene(rng.integers(3, 41, 300).tolist(), seed=7, T=600, tail=9, sigma=0.3)
    S["edges"] = edge_scene()
    S["poses"] = pose_scene()
    S["hand"] = hand_scene()
    sc = _copy(make_scene([60, 50, 40, 70, 45], seed=8, T=90, sigma=0.0))
    S["exact"] = sc
    S["near"] = near_scene()
    return S


CONVERGING = ("counts", "empty")                                      # every image with at least 4 observations is meant to converge
