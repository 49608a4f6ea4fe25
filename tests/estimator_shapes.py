"""TEST INFRASTRUCTURE ONLY: the input families of tests/test_estimator_shapes_cpu.py and tests/test_gpu_estimator_shapes.py.  No GPU here.

Two families.  (1) Row counts on both sides of every boundary of the F / H kernels' tiling: the wave tile of 64 x DG_PU = 256 points
(dg_score_tiles.h), the workgroup pass step of 512 / 1024 / 2048 rows of the 128- / 256- / 512-thread variants and the cooperative
slices that are rounded up to it (dg_f_coop.h).  (2) Coordinate frames other than the pixel frame of pydegensac_amd/synthetic.py: an
affine map per image applied to x, y (and to the LAF columns), the threshold scaled with it.

Everything is generated from fixed seeds.  The restatement's results are computed once per process and shared (oracle_f / oracle_h)."""
import numpy as np

from pydegensac_amd import synthetic as syn

E = (8, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
LAF_NS = (257, 513, 1025)
SCREEN_F_MODELS = (1, 63, 64, 65, 128, 129)          # 64 models per wave in mi_degensac_screen_counts
SCREEN_H_MODELS = (1, 3, 4, 5, 7, 8, 9)              # four per sweep in mi_degensac_screen_counts_h
SAMPLER_NS = {7: (8, 9, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097), 4: (4, 5, 63, 64, 65, 4096, 4097)}
SAMPLER_ITERS = 300                                   # 2100 / 1200 swaps: the pool of 4 ... 65 rows is rewritten many times over
COOP_CASES = ((128, 513), (128, 1025), (256, 1025), (512, 2049))      # (threads, n): one and two pass steps + 1 row
COOP_HELPERS = (1, 3, 7)

F_CALL = dict(px_th=0.5, conf=0.9999, max_iters=3000)
H_CALL = dict(px_th=1.0, conf=0.999, max_iters=3000)
LAF_COEF = {"F": 1.0, "H": 3.0}
EDGE_BUDGET = 300                                     # samples of the runs at the placement limit (n of a few thousand .. 30 000)
H_KEYS = ("samples", "lo_runs", "rejected", "I", "models", "best_sample")
F_KEYS = H_KEYS + ("degen", "Ih", "full_passes", "ex_passes")

_F_RATIOS = (0.45, 0.6, 0.35, 0.75)
_H_RATIOS = (0.5, 0.35, 0.7, 0.25)
_F_LAF_SEED = {257: 3357, 513: 3613, 1025: 9125}


def f_scene(n, laf=False):
    """The F scene of row count n: (pts1, pts2, seed).  Inlier ratios 0.35 ... 0.75 (0.9 on 8 rows); every third count plane-dominated."""
    if laf:
        # half of the inliers carry a random frame in image 2 and the others a noisy one; data seeds at which the restatement turns a
        # candidate down on the LAF check (tests/test_estimator_shapes_cpu.py asserts it)
        p1, p2, _, _ = syn.two_view_fundamental(n, 0.5, 0.1, seed=_F_LAF_SEED[n], laf=True, laf_bad=0.5, laf_sigma=0.5)
        return p1, p2, 41 + n
    i = E.index(n)
    ir = 0.9 if n < 16 else _F_RATIOS[i % 4]
    pf = (0.7, 0.85)[(i // 3) % 2] if i % 3 == 1 else 0.0
    p1, p2, _, _ = syn.two_view_fundamental(n, ir, 0.1, seed=3100 + n, plane_fraction=pf)
    return p1, p2, 41 + n


def h_scene(n, laf=False):
    i = E.index(n)
    ir = 0.75 if n < 16 else _H_RATIOS[i % 4]
    p1, p2, _, _ = syn.homography_pairs(n, ir, 0.5, seed=4100 + n, laf=laf)
    return p1, p2, 57 + n


def coop_scenes(n):
    """Four F pairs of n rows for one cooperative launch (ordinary and plane-dominated): (A, B, seeds)."""
    A, B = [], []
    for j, (ir, pf) in enumerate([(0.4, 0.0), (0.5, 0.7), (0.3, 0.0), (0.6, 0.9)]):
        p1, p2, _, _ = syn.two_view_fundamental(n, ir, 0.1, seed=5100 + 10 * n + j, plane_fraction=pf); A.append(p1); B.append(p2)
    return A, B, [7000 + n + j for j in range(4)]          # (shape, seed) is the key of test_gpu_variants' oracle cache: no seed of that file


def far_outlier_scene(n, seed, min_px=5.0):
    """Noise-free inliers of a two-view geometry and outliers that lie at least min_px from their epipolar lines in both images:
    (pts1, pts2, is_inlier, F_gt).  With a tiny threshold the 9/4 th band of F_gt holds the inliers and nothing else, by a wide margin."""
    p1, p2, lab, F = syn.two_view_fundamental(n, 0.5, 0.0, seed=seed)
    rng = np.random.default_rng([seed, 77])
    for _ in range(64):
        x1 = np.c_[p1, np.ones(n)]; x2 = np.c_[p2, np.ones(n)]
        l2 = x1 @ F.T; l1 = x2 @ F; r = np.abs((x2 * l2).sum(1))
        d = np.minimum(r / np.hypot(l2[:, 0], l2[:, 1]), r / np.hypot(l1[:, 0], l1[:, 1]))
        near = ~lab & (d < min_px)
        if not near.any():
            return p1, p2, lab, F
        k = int(near.sum())
        p2[near] = np.stack([rng.uniform(0, syn.IMG_W, k), rng.uniform(0, syn.IMG_H, k)], 1)
    raise AssertionError("could not move the outliers off the epipolar lines")


# ---- coordinate frames ---------------------------------------------------------------------------------------------------------------
CX, CY, FOCAL = syn.IMG_W / 2, syn.IMG_H / 2, syn.FOCAL
# image k: q = s_k * p + t_k per axis; th = the factor of the threshold (the scale; for the anisotropic frame the larger one, so that
# every inlier of the pixel frame stays inside the band).  This table is the one place that lists the frames.
# "H": what the homography scenes take instead.  The restatement alone loses the homography once IMAGE 2 lies 2000 or more from the
# origin (I = 115 / 305 / 433 at a shift of 0 and of +-1000, 7 / 8 / 13 at +2000, 4 ... 10 at 1e4 ... 1e6; a shift of image 1 alone
# costs nothing up to 1e6): the 4-point fit and the least squares of the reference work on raw coordinates.  A comparison on "no
# model" would be vacuous, so the homography's offset frame keeps 1e6 in image 1 and 1e3 in image 2, and its anisotropic frame shifts
# image 2 by -5e3 instead of -5e4 (tests/test_estimator_shapes_cpu.py: at least 80 % of the pixel frame's inliers in every frame).
FRAMES = {
    "identity":    dict(s1=(1.0, 1.0), t1=(0.0, 0.0), s2=(1.0, 1.0), t2=(0.0, 0.0), th=1.0),
    "centred":     dict(s1=(1.0, 1.0), t1=(-CX, -CY), s2=(1.0, 1.0), t2=(-CX, -CY), th=1.0),
    "normalised":  dict(s1=(1 / FOCAL, 1 / FOCAL), t1=(-CX / FOCAL, -CY / FOCAL), s2=(1 / FOCAL, 1 / FOCAL), t2=(-CX / FOCAL, -CY / FOCAL), th=1 / FOCAL),
    "x40":         dict(s1=(40.0, 40.0), t1=(0.0, 0.0), s2=(40.0, 40.0), t2=(0.0, 0.0), th=40.0),
    "offset":      dict(s1=(1.0, 1.0), t1=(1e6, 1e6), s2=(1.0, 1.0), t2=(1e6, 1e6), th=1.0, H=dict(t2=(1e3, 1e3))),
    "anisotropic": dict(s1=(8.0, 1.0), t1=(0.0, 0.0), s2=(8.0, 1.0), t2=(-5e4, -5e4), th=8.0, H=dict(t2=(-5e3, -5e3))),
}
FRAME_NAMES = tuple(FRAMES)


def _map(p, s, t, inverse=False):
    q = np.array(p, dtype=np.float64, copy=True)
    if inverse:
        q[:, 0] = (q[:, 0] - t[0]) / s[0]; q[:, 1] = (q[:, 1] - t[1]) / s[1]
    else:
        q[:, 0] = q[:, 0] * s[0] + t[0]; q[:, 1] = q[:, 1] * s[1] + t[1]
    if q.shape[1] == 6:
        # the LAF columns are offsets: (x + a11, y + a21) and (x + a12, y + a22) are points of the image (bindings.cpp:337-409)
        k = (1 / s[0], 1 / s[1]) if inverse else s
        q[:, 2] *= k[0]; q[:, 3] *= k[0]; q[:, 4] *= k[1]; q[:, 5] *= k[1]
    return np.ascontiguousarray(q)


def frame(name, kind="F"):
    f = dict(FRAMES[name]); f.update(f.pop("H", {}) if kind == "H" else {})
    return f


def to_frame(name, p1, p2, th, kind="F"):
    f = frame(name, kind)
    return _map(p1, f["s1"], f["t1"]), _map(p2, f["s2"], f["t2"]), th * f["th"]


def from_frame(name, q1, q2, th, kind="F"):
    f = frame(name, kind)
    return _map(q1, f["s1"], f["t1"], True), _map(q2, f["s2"], f["t2"], True), th / f["th"]


def frame_matrices(name, kind="F"):
    f = frame(name, kind)
    T = [np.array([[s[0], 0, t[0]], [0, s[1], t[1]], [0, 0, 1.0]]) for s, t in ((f["s1"], f["t1"]), (f["s2"], f["t2"]))]
    return T[0], T[1]


def f_in_frame(name, F):
    """x2' F x1 = 0 in the pixel frame -> the same geometry in the frame"""
    T1, T2 = frame_matrices(name)
    return np.linalg.inv(T2).T @ F @ np.linalg.inv(T1)


def h_raw_in_frame(name, H):
    """x2 ~ H x1 in the pixel frame -> the drivers' raw model (inv(H).T flattened, image 2 -> image 1) in the frame"""
    T1, T2 = frame_matrices(name, "H")
    return np.linalg.inv(T2 @ H @ np.linalg.inv(T1)).T.ravel()


# (n, inlier ratio, plane fraction, LAF rows) / (n, inlier ratio, LAF rows): three scenes each, n = 257 and 1000
FRAME_F_SCENES = ((257, 0.5, 0.0, False), (1000, 0.45, 0.7, False), (1000, 0.35, 0.0, True))
FRAME_H_SCENES = ((257, 0.5, False), (1000, 0.35, False), (1000, 0.5, True))
F_METRICS = (0, 1)
H_METRICS = (0, 1, 2, 3, 4)


def frame_scene(kind, j):
    """Scene j of the frame family in the pixel frame: (pts1, pts2, seed, laf_coef)."""
    if kind == "F":
        n, ir, pf, laf = FRAME_F_SCENES[j]
        # (the LAF scene's data seed is one at which the restatement turns candidates down on the LAF check under both metrics)
        p1, p2, _, _ = syn.two_view_fundamental(n, ir, 0.1, seed=6502 if laf else 6100 + j, plane_fraction=pf, laf=laf, laf_bad=0.5, laf_sigma=0.5)
    else:
        n, ir, laf = FRAME_H_SCENES[j]
        p1, p2, _, _ = syn.homography_pairs(n, ir, 0.5, seed=6200 + j, laf=laf)
    return p1, p2, 91 + 7 * j, LAF_COEF[kind] if laf else 0.0


def frame_case(kind, j, frame):
    """Scene j mapped into a frame: (pts1, pts2, threshold, seed, laf_coef)."""
    p1, p2, seed, lc = frame_scene(kind, j)
    q1, q2, th = to_frame(frame, p1, p2, (F_CALL if kind == "F" else H_CALL)["px_th"], kind)
    return q1, q2, th, seed, lc


# ---- the restatement, once per process ---------------------------------------------------------------------------------------------------
_cache = {}


def oracle_f(port, key, p1, p2, seed, px_th=None, et=0, laf_coef=0.0, max_iters=None):
    if ("F", key) not in _cache:
        _cache["F", key] = port.find_fundamental(p1, p2, F_CALL["px_th"] if px_th is None else px_th, F_CALL["conf"],
                                                 F_CALL["max_iters"] if max_iters is None else max_iters, et, True, laf_coef, True, seed=seed)
    return _cache["F", key]


def oracle_h(port, key, p1, p2, seed, px_th=None, et=0, laf_coef=0.0, max_iters=None):
    if ("H", key) not in _cache:
        _cache["H", key] = port.find_homography(p1, p2, H_CALL["px_th"] if px_th is None else px_th, H_CALL["conf"],
                                                H_CALL["max_iters"] if max_iters is None else max_iters, et, True, laf_coef, seed=seed)
    return _cache["H", key]


def oracle_e(port, kind, n, laf=False):
    """The restatement on the E-family scene (kind, n, LAF rows)."""
    p1, p2, seed = (f_scene if kind == "F" else h_scene)(n, laf)
    return (oracle_f if kind == "F" else oracle_h)(port, ("E", n, laf), p1, p2, seed, laf_coef=LAF_COEF[kind] if laf else 0.0)


def oracle_frame(port, kind, j, frame, et):
    q1, q2, th, seed, lc = frame_case(kind, j, frame)
    return (oracle_f if kind == "F" else oracle_h)(port, ("frame", j, frame, et), q1, q2, seed, px_th=th, et=et, laf_coef=lc)


# ---- float64 restatement of the two superset predicates (what the GPU file asserts about the screens' counts) ------------------------------
def sampson_f(F, p1, p2):
    """plain float64 Sampson residuals r^2 / (|M' x2|^2 + |M x1|^2) over the first two rows, r = x2' M x1, M = model.reshape(3, 3)"""
    M = np.asarray(F, float).reshape(3, 3)
    x1 = np.c_[np.asarray(p1)[:, :2], np.ones(len(p1))]; x2 = np.c_[np.asarray(p2)[:, :2], np.ones(len(p2))]
    a = x2 @ M; b = x1 @ M.T                      # a = M' x2, b = M x1 (per point)
    r = (x1 * a).sum(1)
    return r * r / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


def superset_ok(counts, resid, th):
    """every screen count is at least the number of residuals inside the 9/4 th band"""
    return bool((np.asarray(counts, np.int64) >= (np.asarray(resid) < th * 9 / 4).sum(axis=1)).all())


def all_in_band_ok(counts, resid, th):
    """with every residual inside the band a count is exactly the number of rows: no row dropped, none counted twice"""
    resid = np.asarray(resid)
    assert (resid < th * 9 / 4).all(), "precondition: the threshold must put every row inside the band"
    return bool((np.asarray(counts, np.int64) == resid.shape[1]).all())
