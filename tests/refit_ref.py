"""TEST INFRASTRUCTURE ONLY: the restatement of the refit (include/mi_degensac.h mi_degensac_refit_lists*) as a loop over the CPU oracle's
own functions (oracle/dg_oracle.c through oracle.port): residuals by dg_oracle_FDs / dg_oracle_FDsSym / dg_oracle_HDS_full on
u = [x1, y1, 1, x2, y2, 1], the member list by dg_oracle_inlidxs, the fit by dg_oracle_u2f / dg_oracle_u2h.  test_refit_cpu.py pins it on
hand-written lists and shows that three broken variants fail there; test_gpu_refit.py compares the device with it.  It also holds the scenes
and the margin every scene must have for "mask bit for bit" to be a fair demand.  The member scenes (member_scene, MEMBER_STORES) fix the
member COUNT of an entry, which is what the solvers switch on; plain_fit is the numpy solution the oracle's fits are held against."""
import ctypes as C

import numpy as np

from pydegensac_amd import synthetic as syn

FIXED, MAX_FITS, SHORT, BAD_FIT, WORSE, TRUNCATED = range(6)
F_TYPES = {"sampson": 0, "symm_epipolar": 1}
H_TYPES = {"sampson": 0, "symm_sq_max": 1, "symm_max": 2, "symm_sq_sum": 3, "symm_sum": 4}
DEFAULT_PX = {"F": 0.5, "H": 1.0}
MARGIN = 1e-6


def threshold(model, et, px_th=None):
    px = DEFAULT_PX[model] if px_th is None else px_th
    return px if (model == "H" and et in (2, 4)) else px * px


def _u(rows):
    u = np.ones((len(rows), 6)); u[:, 0:2] = rows[:, 0:2]; u[:, 3:5] = rows[:, 2:4]
    return np.ascontiguousarray(u)


def resid(P, model, et, M, rows):
    """the oracle's residual of every row [n, 4] under the driver-form model M (9 numbers)"""
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    d = np.zeros(len(rows))
    if len(rows) == 0:
        return d
    u = _u(rows); m = np.ascontiguousarray(np.asarray(M, np.float64).ravel().copy()); L = P.lib()
    with np.errstate(all="ignore"):
        if model == "F":
            (L.dg_oracle_FDs if et == 0 else L.dg_oracle_FDsSym)(P.dp(u), P.dp(m), P.dp(d), len(rows))
        else:
            L.dg_oracle_HDS_full(et, P.dp(u), P.dp(m), P.dp(d), len(rows))
    return d


def model_ok(M):
    M = np.asarray(M, np.float64).ravel()
    return bool(np.isfinite(M).all() and (M != 0).any())


def members(P, model, et, M, rows, th, strict=False):
    """(ids int32 in row order, residuals): resid <= th through dg_oracle_inlidxs (a NaN is not a member); a zero or non-finite model has none.
    strict=True is the broken `<`."""
    d = resid(P, model, et, M, rows)
    if not model_ok(M) or len(d) == 0:
        return np.zeros(0, np.int32), d
    if strict:
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(d < th).astype(np.int32), d
    lst = np.zeros(len(d), np.int32)
    S = P.lib().dg_oracle_inlidxs(P.dp(np.ascontiguousarray(d)), len(d), C.c_double(th), P.ip(lst))
    return lst[:S.I].copy(), d


def fit(P, model, rows, ids):
    u = _u(np.asarray(rows, np.float64).reshape(-1, 4)); ids = np.ascontiguousarray(ids, np.int32); M = np.zeros(9)
    with np.errstate(all="ignore"):
        (P.lib().dg_oracle_u2f if model == "F" else P.lib().dg_oracle_u2h)(P.dp(u), P.ip(ids), len(ids), P.dp(M))
    return M


def refit_entry(P, model, et, M0, rows, th, max_fits=4, broken=None):
    """The rule on one entry.  Returns (best [9], ids of its members, (n0, members, fits, status), visited = every model whose members were
    taken).  broken: None, or "lt" (`<` for `<=`), "smaller" (accepts a fit that loses members), "allrows" (fits on all rows)."""
    minn = 8 if model == "F" else 4
    best = np.asarray(M0, np.float64).ravel().copy()
    I, _ = members(P, model, et, best, rows, th, broken == "lt")
    n0 = len(I); fits = 0; status = MAX_FITS; visited = [best.copy()]
    for _ in range(max_fits):
        if len(I) < minn:
            status = SHORT; break
        M = fit(P, model, rows, np.arange(len(rows), dtype=np.int32) if broken == "allrows" else I); fits += 1
        if not np.isfinite(M).all():
            status = BAD_FIT; break
        I2, _ = members(P, model, et, M, rows, th, broken == "lt"); visited.append(M.copy())
        if len(I2) < len(I) and broken != "smaller":
            status = WORSE; break
        same = np.array_equal(I2, I)
        best = M; I = I2
        if same:
            status = FIXED; break
    return best, I, (n0, len(I), fits, status), visited


def refit(P, pts, off, models, model="F", et=0, px_th=None, max_fits=4, broken=None):
    """The whole call on numpy arrays: pts [cap, 4], off [K + 1], models [K, 9] or [K, 3, 3] in driver form.  Returns dict(models [K, 9],
    inlier [cap] uint8, info [K, 4] int32, visited = per entry the models whose members were taken)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 4); off = np.asarray(off, np.int64); M = np.asarray(models, np.float64).reshape(-1, 9)
    K = len(off) - 1; cap = len(pts); th = threshold(model, et, px_th)
    out = M.copy(); inl = np.zeros(cap, np.uint8); info = np.zeros((K, 4), np.int32); visited = []
    for p in range(K):
        b, e = int(off[p]), int(off[p + 1])
        if not (0 <= b <= e <= cap):
            info[p] = (0, 0, 0, TRUNCATED); visited.append([]); continue
        best, I, inf, vis = refit_entry(P, model, et, M[p], pts[b:e], th, max_fits, broken)
        out[p] = best; inl[b + I] = 1; info[p] = inf; visited.append(vis)
    return dict(models=out, inlier=inl, info=info, visited=visited)


def min_margin(P, scene, ref):
    """the smallest |resid - th| / th over every row of every entry under every model the restatement visited (inf without rows)"""
    pts, off = scene["pts"], scene["off"]; th = threshold(scene["model"], scene["et"], scene.get("px_th")); m = np.inf
    for p, vis in enumerate(ref["visited"]):
        for M in vis:
            d = resid(P, scene["model"], scene["et"], M, pts[off[p]:off[p + 1]])
            d = d[np.isfinite(d)]
            if len(d):
                m = min(m, float(np.abs(d - th).min()) / th)
    return m


def rel_fro(a, b):
    """relative Frobenius distance of two models of one entry"""
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return 0.0 if np.array_equal(a, b, equal_nan=True) else np.inf
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
HC = np.linalg.inv(syn.H_1_6).T                                       # the driver's form of the generator's homography


def _rows(model, n, seed, ratio=0.7, sigma=None):
    """n rows x1 y1 x2 y2 of a two-view scene with outliers and the driver-form ground truth"""
    if model == "F":
        p1, p2, lab, F = syn.two_view_fundamental(max(n, 1), ratio, 0.1 if sigma is None else sigma, seed=seed)
        M = (F / np.linalg.norm(F)).ravel()
    else:
        p1, p2, lab, _ = syn.homography_pairs(max(n, 1), ratio, 0.3 if sigma is None else sigma, seed=seed)
        M = (HC / np.linalg.norm(HC)).ravel()
    return np.ascontiguousarray(np.concatenate([p1[:n, :2], p2[:n, :2]], axis=1)), lab[:n], M


def start_model(P, model, rows, lab, seed, take=24):
    """a start model that is good but not at its fixed point: the oracle's fit on the first `take` labelled inliers"""
    ids = np.flatnonzero(lab)[:take].astype(np.int32)
    if len(ids) < (8 if model == "F" else 4):
        return None
    return fit(P, model, rows, ids)


def lengths_scene(P, model, et, lengths, seed, o0=0, tail=0, px_th=None):
    """one entry per length (0 = an empty entry), start models from start_model (the ground truth where an entry is too short for one);
    o0 unowned rows in front, `tail` behind"""
    rng = np.random.default_rng(seed)
    chunks = [rng.uniform(0, 500, (o0, 4))]; off = [o0]; models = []
    for k, n in enumerate(lengths):
        rows, lab, gt = _rows(model, n, seed * 1000 + k)
        M = start_model(P, model, rows, lab, seed) if n else None
        models.append(gt if M is None else M)
        chunks.append(rows.reshape(-1, 4)); off.append(off[-1] + n)
    chunks.append(rng.uniform(0, 500, (tail, 4)))
    return dict(model=model, et=et, px_th=px_th, pts=np.ascontiguousarray(np.concatenate(chunks)), off=np.asarray(off, np.int64),
                models=np.ascontiguousarray(np.array(models)).reshape(len(lengths), 9))


H_LENGTHS = [0, 3, 4, 5, 10, 11, 12, 13, 16, 17, 63, 64, 65, 0, 0, 255, 256, 257, 1023, 1024, 1025, 2049, 0]
F_LENGTHS = [0, 0, 7, 8, 9, 16, 17, 63, 64, 65, 0, 255, 256, 257, 1023, 1024, 1025, 2049, 0]


def sparse_scene(P, model, et, n, where, seed):
    """one entry of n rows whose only rows near the model are those at `where`: noise-free rows of the ground truth; every other row is
    drawn again until its residual under the ground truth is beyond 1000 th; the start model is the ground truth"""
    good, _, gt = _rows(model, max(len(where), 16), seed, ratio=1.0, sigma=0.0)
    rng = np.random.default_rng(seed + 7)
    out = rng.uniform(0, 700, (n, 4)); th = threshold(model, et)
    keep = np.zeros(n, bool); keep[list(where)] = True
    while True:
        with np.errstate(invalid="ignore"):
            bad = ~keep & ~(resid(P, model, et, gt, out) > 1000 * th)
        if not bad.any():
            break
        out[bad] = rng.uniform(0, 700, (int(bad.sum()), 4))
    out[list(where)] = good[:len(where)]
    return dict(model=model, et=et, px_th=None, pts=np.ascontiguousarray(out), off=np.asarray([0, n], np.int64), models=gt.reshape(1, 9).copy())


# ---- scenes fixed by member count: the unit entry of the non-minimal fits -------------------------------------------------------------
# x' = s x + t per image, the same scale in both; px_th scales with s.  "shifted" is the large-coordinate frame of
# test_gpu_units.test_screening_counts_are_supersets_of_the_exact_band, "normalised" is centred on the F generator's image and scaled by 1e-3
MEMBER_FRAMES = {
    "shifted":    dict(s=37.0, t1=(5000.0, 5000.0), t2=(-9000.0, -9000.0)),
    "normalised": dict(s=1e-3, t1=(-syn.IMG_W / 2 * 1e-3, -syn.IMG_H / 2 * 1e-3), t2=(-syn.IMG_W / 2 * 1e-3, -syn.IMG_H / 2 * 1e-3)),
    "large":      dict(s=1e4, t1=(0.0, 0.0), t2=(0.0, 0.0)),
}
MEMBER_SIGMA = 0.05
F_COUNTS = (8, 9, 15, 16, 17, 18, 23, 24, 25, 63, 64, 65, 255, 256, 257, 511, 512, 513)
H_COUNTS = (4, 5, 11, 12, 13, 14, 19, 20, 21, 63, 64, 65, 255, 256, 257, 513)
FRAME_COUNTS = {"F": (16, 17, 64, 257), "H": (12, 13, 64, 257)}
SWITCH_COUNTS = {"F": (16, 17), "H": (12, 13)}                         # the last count of the small solver and the first of the big one
POSITION_M = {"F": 24, "H": 13}


def model_in_frame(model, M, fr):
    """the driver-form model of the same geometry after x1' = T1 x1, x2' = T2 x2 (F: x2' F x1 = 0; H_c: x1 ~ H_c' x2), unit Frobenius norm"""
    T1, T2 = (np.array([[fr["s"], 0, t[0]], [0, fr["s"], t[1]], [0, 0, 1.0]]) for t in (fr["t1"], fr["t2"]))
    M = np.asarray(M, np.float64).reshape(3, 3)
    Mf = np.linalg.inv(T2).T @ M @ (np.linalg.inv(T1) if model == "F" else T1.T)
    return (Mf / np.linalg.norm(Mf)).ravel()


def member_scene(P, model, et, m, seed, sigma=MEMBER_SIGMA, where=None, frame=None, n=None, distinct=None):
    """one entry of n rows whose members under the ground truth are exactly the m rows at `where`, in the style of sparse_scene: the members
    are NOISY rows of the ground truth (sigma px: the fit is a least-squares problem, not an exact null space), every other row is drawn
    again until its residual under the ground truth is beyond 1000 th; the start model is the ground truth.  where=None: m sorted random
    positions in n = 2 m + 37 rows, so that the gather is never a contiguous copy.  distinct=d: the members are d distinct rows repeated
    in turn (a rank-deficient set).  frame: a name of MEMBER_FRAMES; the scene is built in the pixel frame and then mapped, px_th and the
    start model with it.  The dict also holds where (int32, sorted) and m."""
    rng = np.random.default_rng([seed, 7])
    if where is None:
        n = 2 * m + 37 if n is None else n
        where = np.sort(rng.choice(n, m, replace=False))
    where = np.asarray(sorted(where), np.int32)
    assert len(where) == m and len(set(where.tolist())) == m and n is not None and where[-1] < n
    good, _, gt = _rows(model, max(m, 16), seed, ratio=1.0, sigma=sigma)
    if distinct:
        good = good[np.arange(m) % distinct]
    out = rng.uniform(0, 700, (n, 4)); th = threshold(model, et)
    keep = np.zeros(n, bool); keep[where] = True
    while True:
        with np.errstate(all="ignore"):
            bad = ~keep & ~(resid(P, model, et, gt, out) > 1000 * th)
        if not bad.any():
            break
        out[bad] = rng.uniform(0, 700, (int(bad.sum()), 4))
    out[where] = good[:m]
    px = None
    if frame is not None:
        fr = MEMBER_FRAMES[frame]
        out[:, 0:2] = out[:, 0:2] * fr["s"] + np.asarray(fr["t1"]); out[:, 2:4] = out[:, 2:4] * fr["s"] + np.asarray(fr["t2"])
        gt = model_in_frame(model, gt, fr); px = DEFAULT_PX[model] * fr["s"]
    return dict(model=model, et=et, px_th=px, pts=np.ascontiguousarray(out), off=np.asarray([0, n], np.int64), models=gt.reshape(1, 9).copy(),
                where=[where], m=[m])


def concat_scenes(scenes, order=None, stride=1):
    """the entries of one-entry scenes of one model kind, error type and threshold behind each other in one store, in `order` (default: as
    given); stride = s puts s - 1 empty entries between two of them, so that with s = the grid of the kernel one workgroup takes them all,
    one after the other.  where / m are per entry (None / 0 for an empty one)"""
    order = list(range(len(scenes))) if order is None else list(order)
    a = scenes[0]
    assert all((s["model"], s["et"], s["px_th"]) == (a["model"], a["et"], a["px_th"]) and len(s["off"]) == 2 for s in scenes)
    off = [0]; models = []; where = []; m = []
    for k, q in enumerate(order):
        s = scenes[q]
        off.append(off[-1] + len(s["pts"])); models.append(s["models"][0]); where.append(s["where"][0]); m.append(s["m"][0])
        if k + 1 < len(order):
            for _ in range(stride - 1):
                off.append(off[-1]); models.append(s["models"][0]); where.append(None); m.append(0)
    return dict(model=a["model"], et=a["et"], px_th=a["px_th"], pts=np.ascontiguousarray(np.concatenate([scenes[q]["pts"] for q in order])),
                off=np.asarray(off, np.int64), models=np.ascontiguousarray(np.array(models)).reshape(-1, 9), where=where, m=m)


# The data seeds that were picked, not taken as they came: F on 8 noisy members (the exact null vector of 8 rows made singular is no longer
# exact: at most seeds a member is lost, the entry ends WORSE and the fitted model is not the output) and the rank-deficient F sets (the
# same, with a null space of six or three dimensions).  At these the restatement ends FIXED with a margin of 0.9 or more.
_PICKED = {("F", 0, 8, 0): 33, ("F", 0, 9, 5): 74, ("F", 0, 20, 5): 8}


def _seed(model, et, m, extra=0):
    return 1000000 * _PICKED.get((model, et, m, extra), 0) + 100000 * (1 if model == "F" else 2) + 10000 * et + 10 * m + extra


def count_entries(P, model, et, counts):
    """one member scene per count; the 4-row H scene from noise-free rows (the 4-point fit on noisy rows loses members: the entry would
    end WORSE and the fitted model would not be the output)"""
    return [member_scene(P, model, et, m, _seed(model, et, m), 0.0 if (model == "H" and m == 4) else MEMBER_SIGMA) for m in counts]


def position_entries(P, model):
    """m members at the edges of the scoring pass (1024 rows per step, 256 per load, 64 per wave): all in rows >= 1024 of 1100 rows (the
    second step); rows 0, 1023, 1024 and n - 1 among them; all inside the last, partly filled wave (rows 640 .. 699) of the last load of
    700 rows"""
    m = POSITION_M[model]; rng = np.random.default_rng(m)
    late = 1024 + rng.choice(76, m, replace=False)
    edges = np.concatenate([[0, 1023, 1024, 1099], rng.choice(np.arange(1, 1023), m - 4, replace=False)])
    wave = 640 + rng.choice(60, m, replace=False)
    return [member_scene(P, model, 0, m, _seed(model, 0, m, k + 1), where=w, n=n) for k, (w, n) in enumerate(((late, 1100), (edges, 1100), (wave, 700)))]


RANKDEF = ((9, 3), (20, 6))                                           # (members, distinct rows among them)


def rankdef_entries(P, model):
    """member sets that do not determine the model: three distinct rows three times each, six distinct rows in 20 (for H six rows do
    determine it: there the set is only repeated)"""
    return [member_scene(P, model, 0, m, _seed(model, 0, m, 5), distinct=d) for m, d in RANKDEF]


def frame_entries(P, model, frame):
    return [member_scene(P, model, 0, m, _seed(model, 0, m, 7), frame=frame) for m in FRAME_COUNTS[model]]


# name of the store -> builder of its one-entry scenes (one model kind, error type and threshold per store: one call each)
MEMBER_STORES = {
    "F_members_0": lambda P: count_entries(P, "F", 0, F_COUNTS) + position_entries(P, "F"),
    "F_members_1": lambda P: count_entries(P, "F", 1, SWITCH_COUNTS["F"]),
    "H_members_0": lambda P: count_entries(P, "H", 0, H_COUNTS) + position_entries(P, "H"),
    **{f"H_members_{et}": (lambda P, et=et: count_entries(P, "H", et, SWITCH_COUNTS["H"])) for et in (1, 2, 3, 4)},
    **{f"{k}_frame_{fr}": (lambda P, k=k, fr=fr: frame_entries(P, k, fr)) for k in "FH" for fr in MEMBER_FRAMES},
    "F_rankdef": lambda P: rankdef_entries(P, "F"),
    "H_rankdef": lambda P: rankdef_entries(P, "H"),
}
_ENTRIES = {}


def member_entries(P, name):
    """the one-entry scenes of a member store, built once"""
    if name not in _ENTRIES:
        _ENTRIES[name] = MEMBER_STORES[name](P)
    return _ENTRIES[name]


def plain_fit(model, rows):
    """TEST REFERENCE, independent of the oracle: the least-squares model of the rows [m, 4] in float64 numpy.  Hartley normalisation per
    image (centroid to the origin, mean distance sqrt 2), the m x 9 (F) or 2 m x 9 (H, DLT) design matrix, its last right singular vector
    by np.linalg.svd, for F the smallest singular value of the 3 x 3 zeroed by a second SVD, then the normalisation undone.  Where the
    reference's solver works on raw coordinates (F on 8 rows, H on 4: the system has an exact null vector) there is no normalisation.
    Returns (model [9] in driver form, the design matrix)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 4); m = len(rows)
    raw = m <= (8 if model == "F" else 4)
    T = []
    for c in (rows[:, 0:2], rows[:, 2:4]):
        if raw:
            T.append(np.eye(3)); continue
        mu = c.mean(axis=0); s = np.sqrt(2.0) / np.hypot(*(c - mu).T).mean()
        T.append(np.array([[s, 0, -s * mu[0]], [0, s, -s * mu[1]], [0, 0, 1.0]]))
    a = np.c_[rows[:, 0:2], np.ones(m)] @ T[0].T; b = np.c_[rows[:, 2:4], np.ones(m)] @ T[1].T
    if model == "F":
        Z = (b[:, :, None] * a[:, None, :]).reshape(m, 9)             # b' F a = 0
        Fn = np.linalg.svd(Z)[2][-1].reshape(3, 3)
        U, S, Vt = np.linalg.svd(Fn); S[2] = 0.0
        return (T[1].T @ (U * S) @ Vt @ T[0]).ravel(), Z
    Z = np.zeros((2 * m, 9))                                           # a ~ M' b: rows (b, 0, -a0 b) and (0, b, -a1 b) on M[3 j + l]
    for j in range(3):
        Z[0::2, 3 * j] = b[:, j]; Z[0::2, 3 * j + 2] = -a[:, 0] * b[:, j]
        Z[1::2, 3 * j + 1] = b[:, j]; Z[1::2, 3 * j + 2] = -a[:, 1] * b[:, j]
    Mn = np.linalg.svd(Z)[2][-1].reshape(3, 3)
    return (T[1].T @ Mn @ np.linalg.inv(T[0]).T).ravel(), Z


def aligned_rel_fro(a, b):
    """relative Frobenius distance of two models up to scale and sign: both to unit norm, the nearer of a - b and a + b"""
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    a = a / np.linalg.norm(a); b = b / np.linalg.norm(b)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


def gap_bound(Z):
    """eps |N|_2 / (l8 - l9) of N = Z' Z: the first-order change of N's last eigenvector under a relative perturbation eps of N"""
    lam = np.linalg.eigvalsh(Z.T @ Z)
    return float(np.finfo(float).eps * lam[-1] / (lam[1] - lam[0]))


def many_scene(P, model, et, K, seed):
    """K short entries (10 .. 40 rows) behind each other: more entries than the grid has workgroups"""
    rng = np.random.default_rng(seed)
    return lengths_scene(P, model, et, [int(x) for x in rng.integers(10, 41, K)], seed)


def offsets_scene(P, model="F", et=0, seed=11):
    """entries that are no ranges of the list: cap = 100 rows, entry 2 crosses cap, entry 3 starts beyond it, entry 4 is a decreasing pair;
    entries 0, 1 and 5 are whole and do not overlap"""
    sc = lengths_scene(P, model, et, [20, 30, 10, 40], seed)
    sc["off"] = np.asarray([0, 20, 50, 110, 130, 60, 100], np.int64)
    rng = np.random.default_rng(seed)
    sc["models"] = np.ascontiguousarray(np.concatenate([sc["models"][:2], rng.normal(size=(3, 9)), sc["models"][3:4]]))
    return sc


def models_scene(P, model, et, seed=13, n=100):
    """six entries of n rows: start models zero, with a NaN, scaled by 1e150 and 1e-150, with an inf, and a good one"""
    sc = lengths_scene(P, model, et, [n] * 6, seed)
    M = sc["models"]
    M[0] = 0.0; M[1, 4] = np.nan; M[2] *= 1e150; M[3] *= 1e-150; M[4, 0] = np.inf
    return sc


def bad_rows_scene(P, model, et, seed=17):
    """rows that are not finite inside entries that otherwise refit"""
    sc = lengths_scene(P, model, et, [40, 300, 70], seed)
    pts = sc["pts"]
    pts[3, 0] = np.nan; pts[50, 2] = np.inf; pts[51] = np.nan; pts[339, 3] = -np.inf; pts[345, 1] = np.nan
    return sc


_SCENES = {}


def gpu_scenes(P):
    """every scene test_gpu_refit.py uses, by name (built once): test_refit_cpu.py asserts the margin on each of them"""
    if _SCENES:
        return _SCENES
    S = _SCENES
    S["F_len_0"] = lengths_scene(P, "F", 0, F_LENGTHS, 3, o0=5, tail=9)
    S["F_len_1"] = lengths_scene(P, "F", 1, F_LENGTHS, 4, o0=1, tail=3)
    S["H_len_0"] = lengths_scene(P, "H", 0, H_LENGTHS, 5, o0=7, tail=2)
    for et in (1, 2, 3, 4):
        S[f"H_len_{et}"] = lengths_scene(P, "H", et, [0, 4, 5, 12, 13, 65, 0, 257, 1025], 50 + et, o0=3, tail=1)
    S["F_px2"] = lengths_scene(P, "F", 0, [9, 64, 300], 21, px_th=2.0)
    S["F_8_per_wave"] = sparse_scene(P, "F", 0, 600, [64 * k + 3 for k in range(8)], 31)
    S["F_8_last_wave"] = sparse_scene(P, "F", 0, 300, list(range(290, 298)), 32)
    S["F_7_of_300"] = sparse_scene(P, "F", 0, 300, [1, 60, 64, 127, 128, 255, 299], 33)
    S["H_4_per_wave"] = sparse_scene(P, "H", 0, 250, [3, 67, 131, 195], 34)
    S["H_4_last_wave"] = sparse_scene(P, "H", 0, 200, [193, 194, 195, 196], 35)
    S["H_3_of_200"] = sparse_scene(P, "H", 0, 200, [0, 100, 199], 36)
    S["F_many"] = many_scene(P, "F", 0, 300, 41)
    S["H_many"] = many_scene(P, "H", 0, 300, 42)
    S["F_offsets"] = offsets_scene(P, "F", 0)
    S["H_offsets"] = offsets_scene(P, "H", 0)
    S["F_models"] = models_scene(P, "F", 0)
    S["H_models"] = models_scene(P, "H", 0)
    S["H_models_3"] = models_scene(P, "H", 3)
    S["F_bad_rows"] = bad_rows_scene(P, "F", 0)
    S["H_bad_rows"] = bad_rows_scene(P, "H", 0)
    for name in MEMBER_STORES:
        S[name] = concat_scenes(member_entries(P, name))
    return S


_REFS = {}


def reference(P, name, max_fits=4):
    """the restatement's result on a scene of gpu_scenes, computed once and shared"""
    key = (name, max_fits)
    if key not in _REFS:
        sc = gpu_scenes(P)[name]
        _REFS[key] = refit(P, sc["pts"], sc["off"], sc["models"], sc["model"], sc["et"], sc["px_th"], max_fits)
    return _REFS[key]
