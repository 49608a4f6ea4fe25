"""TEST INFRASTRUCTURE ONLY: the restatement of the refit (include/mi_degensac.h mi_degensac_refit_lists*) as a loop over the CPU oracle's
own functions (oracle/dg_oracle.c through oracle.port): residuals by dg_oracle_FDs / dg_oracle_FDsSym / dg_oracle_HDS_full on
u = [x1, y1, 1, x2, y2, 1], the member list by dg_oracle_inlidxs, the fit by dg_oracle_u2f / dg_oracle_u2h.  test_refit_cpu.py pins it on
hand-written lists and shows that three broken variants fail there; test_gpu_refit.py compares the device with it.  It also holds the scenes
and the margin every scene must have for "mask bit for bit" to be a fair demand."""
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
    return S


_REFS = {}


def reference(P, name, max_fits=4):
    """the restatement's result on a scene of gpu_scenes, computed once and shared"""
    key = (name, max_fits)
    if key not in _REFS:
        sc = gpu_scenes(P)[name]
        _REFS[key] = refit(P, sc["pts"], sc["off"], sc["models"], sc["model"], sc["et"], sc["px_th"], max_fits)
    return _REFS[key]
