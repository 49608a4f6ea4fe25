"""Tentative correspondences on the GPU: the matcher stage of the reference's example pipeline
(examples/simple-example.py:46-53) behind libmi_degensac.so (include/mi_degensac.h, mi_degensac_match*).

    bf = cv2.BFMatcher(); matches = bf.knnMatch(descs1, descs2, k=2)          ->  idx, dist = knn_match(descs1, descs2)
    tentatives = [m for m, n in matches if m.distance < 0.9 * n.distance]     ->  q, t, d = match_snn(descs1, descs2, 0.9)

float32 descriptors use the L2 norm (cv2.BFMatcher's default, what the example runs on AKAZE's KAZE descriptors), uint8
descriptors the Hamming norm.  norm="l2_u8" is the L2 norm on uint8 rows as they are (SIFT / RootSIFT x 512, quantised HardNet /
SOSNet / SuperPoint; dim <= 256): the squared distance is an exact integer below 2^24, formed on the int8 matrix cores, and idx / dist
are bit for bit those of norm="l2" on the same rows cast to float32.  No CPU path: without the HIP library / a gfx950 device every
call raises."""
import collections
import ctypes as C

import numpy as np

from . import _lib

NORM_L2, NORM_HAMMING, NORM_L2_U8 = 0, 1, 4
L2_U8_MAX_DIM = 256          # 256 * 255^2 < 2^24: the squared distance stays exact in fp32
_NORMS = {"l2": NORM_L2, "hamming": NORM_HAMMING, "l2_u8": NORM_L2_U8}


def _pad_words(a, b):
    """uint8 rows padded to whole 32-bit words; zero bytes on both sides add no differing bits and no squared difference"""
    pad = (-a.shape[1]) % 4
    if pad:
        a = np.pad(a, ((0, 0), (0, pad))); b = np.pad(b, ((0, 0), (0, pad)))
    return a, b


def _prep(desc1, desc2, norm):
    a = np.asarray(desc1); b = np.asarray(desc2)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or a.shape[1] == 0:
        raise ValueError("descriptors should be arrays [n1, dim] and [n2, dim] with the same dim")
    if norm is None:
        norm = "hamming" if a.dtype == np.uint8 and b.dtype == np.uint8 else "l2"
    if norm not in _NORMS:
        raise ValueError("norm should be 'l2', 'hamming' or 'l2_u8'")
    if norm == "l2":
        return NORM_L2, np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("the Hamming norm needs uint8 descriptors" if norm == "hamming" else "norm 'l2_u8' needs uint8 descriptors")
    if norm == "l2_u8" and a.shape[1] > L2_U8_MAX_DIM:
        raise ValueError(f"norm 'l2_u8' takes dim <= {L2_U8_MAX_DIM}: use float32 descriptors with norm 'l2' beyond that")
    a, b = _pad_words(a, b)
    return _NORMS[norm], np.ascontiguousarray(a), np.ascontiguousarray(b)


# ---- the argument checks' small parts: every text is the caller's, which check comes first is the caller's order ----
def _float(x, text):
    """float(x); raises ValueError(text) for what has no float value"""
    try:
        return float(x)
    except (TypeError, ValueError):
        raise ValueError(text)


def _number(x, text, lo=-np.inf, hi=np.inf):
    """a real number (not a bool) with lo <= x <= hi, as a float; NaN is outside every range; raises ValueError(text)"""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not lo <= float(x) <= hi:
        raise ValueError(text)
    return float(x)


def _integer(x, text, lo=None, hi=None):
    """an integer (not a bool) with lo <= x <= hi where a bound is given, as an int; raises ValueError(text)"""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or (lo is not None and x < lo) or (hi is not None and x > hi):
        raise ValueError(text)
    return int(x)


def _sd(x):
    """(shape, dtype) of an optional array or tensor, as the check_* functions take it"""
    return None if x is None else (tuple(x.shape), x.dtype)


def _rows_list(arrays, text):
    """one array per pair / image as a list of arrays, all 2-D with the dtype and width of entry 0, and at least one; raises
    ValueError(text)"""
    a = [np.asarray(x) for x in arrays]
    if len(a) == 0 or any(x.ndim != 2 or x.dtype != a[0].dtype or x.shape[1] != a[0].shape[1] for x in a):
        raise ValueError(text)
    return a


def _knn_out(n, with_match):
    """the 2-NN result arrays of n query rows with their fills: idx -1, dist inf, and with with_match match -1 (else None)"""
    return np.full((n, 2), -1, np.int32), np.full((n, 2), np.inf, np.float32), np.full(n, -1, np.int32) if with_match else None


# the decision rule of a matcher call (include/mi_degensac.h MI_DEGENSAC_DECIDE_*): ratio as a float (1.0 where it is not read), mutual as
# a bool, decide = the bit flags, max_dist as a float (0.0 where it is not read)
Rule = collections.namedtuple("Rule", "ratio mutual decide max_dist")


def check_rule(ratio, mutual=False, max_dist=None, fginn=False):
    """The shared check of ratio / mutual / max_dist of every matcher call -> Rule; raises ValueError.
    ratio: a finite number > 0, or None = no ratio test (a query is a tentative when it has a nearest neighbour; one train row is enough).
    mutual: False, True, or "ratio" = mutual nearest neighbours whose ratio test also holds at the train row's own reverse search.
    max_dist: None, or a finite number >= 0: also require dist[0] <= max_dist (the returned L2 distance, or Hamming bits).
    fginn: the call runs the FGINN second neighbour, which is defined for the forward ratio test only (max_dist goes with it)."""
    decide = 0
    if ratio is None:
        decide |= _lib.DECIDE_NO_RATIO; r = 1.0
    else:
        r = _float(ratio, "ratio should be a number, or None for no ratio test")
        if not np.isfinite(r) or r <= 0:
            raise ValueError("ratio should be finite and > 0")
    if isinstance(mutual, str):
        if mutual != "ratio":
            raise ValueError('mutual should be False, True or "ratio"')
        if ratio is None:
            raise ValueError('mutual="ratio" needs a ratio: ratio=None is no ratio test in either direction')
        decide |= _lib.DECIDE_BACK_RATIO
    md = 0.0
    if max_dist is not None:
        md = _float(max_dist, "max_dist should be a number")
        if not (np.isfinite(md) and md >= 0 and md <= float(np.finfo(np.float32).max)):
            raise ValueError("max_dist should be finite and >= 0")
        decide |= _lib.DECIDE_MAX_DIST
    if fginn and decide & (_lib.DECIDE_NO_RATIO | _lib.DECIDE_BACK_RATIO):
        raise ValueError('the FGINN second neighbour belongs to the forward ratio test: it goes with max_dist, not with ratio=None or mutual="ratio"')
    return Rule(r, bool(mutual), decide, md)


def _run(desc1, desc2, norm, ratio, mutual, want_keep, device, max_dist=None):
    rule = check_rule(ratio, mutual, max_dist)
    code, a, b = _prep(desc1, desc2, norm)
    n1, n2, dim = a.shape[0], b.shape[0], a.shape[1]
    idx, dist, _ = _knn_out(n1, False)
    keep = np.zeros(n1, np.uint8) if want_keep else None
    out = (_lib.ptr(idx), _lib.ptr(dist), _lib.ptr(keep) if want_keep else None)
    if rule.decide == 0:
        rc = _lib.lib().mi_degensac_match(code, a.ctypes.data_as(C.c_void_p), n1, b.ctypes.data_as(C.c_void_p), n2, dim, rule.ratio,
                                          int(rule.mutual), int(device), *out)
    else:
        mp = _lib.match_params(code, dim, rule)
        rc = _lib.lib().mi_degensac_match_ex(C.byref(mp), a.ctypes.data_as(C.c_void_p), n1, b.ctypes.data_as(C.c_void_p), n2, int(device), *out)
    _lib.check_match(rc)
    return idx, dist, keep


def knn_match(desc1, desc2, norm=None, device=0):
    """The two nearest rows of desc2 for every row of desc1 (cv2 `knnMatch(descs1, descs2, k=2)`): idx [n1, 2] (train
    indices, -1 where desc2 has fewer than two rows) and dist [n1, 2], nearest first, ties to the lower index."""
    idx, dist, _ = _run(desc1, desc2, norm, 1.0, False, False, device)
    return idx, dist


def match_snn(desc1, desc2, ratio=0.9, mutual=False, norm=None, device=0, *, max_dist=None):
    """Second-nearest-neighbour ratio test (`m.distance < ratio * n.distance`), optionally restricted to mutual nearest
    neighbours: (query indices, train indices, distances) of the tentative correspondences, in query order.
    ratio=None, mutual="ratio" and max_dist: the decision rule of check_rule (match_nn / match_mnn / match_smnn name its usual forms)."""
    idx, dist, keep = _run(desc1, desc2, norm, ratio, mutual, True, device, max_dist)
    sel = np.flatnonzero(keep)
    return sel.astype(np.int64), idx[sel, 0].astype(np.int64), dist[sel, 0]


def match_nn(desc1, desc2, max_dist=None, norm=None, device=0):
    """Nearest-neighbour matching, the rule of learned descriptors without a ratio test: every row of desc1 with a nearest row in desc2
    (one train row is enough), optionally only at distance <= max_dist.  Returns the triple of match_snn."""
    return match_snn(desc1, desc2, None, False, norm, device, max_dist=max_dist)


def match_mnn(desc1, desc2, max_dist=None, norm=None, device=0):
    """Mutual-nearest-neighbour matching: match_nn restricted to the pairs that are each other's nearest neighbour, optionally only at
    distance <= max_dist (SuperPoint / DISK / ALIKED style).  Returns the triple of match_snn."""
    return match_snn(desc1, desc2, None, True, norm, device, max_dist=max_dist)


def match_smnn(desc1, desc2, ratio=0.9, max_dist=None, norm=None, device=0):
    """Mutual nearest neighbours whose ratio test holds in BOTH directions: `d0 < ratio * d1` at the query and at its train row's own
    reverse search (a train row with a single query row has no second distance and is dropped), optionally only at distance <= max_dist.
    Returns the triple of match_snn."""
    if ratio is None:
        raise ValueError("match_smnn is the ratio test in both directions: ratio should be a number (match_mnn has none)")
    return match_snn(desc1, desc2, ratio, "ratio", norm, device, max_dist=max_dist)


def match_fginn(desc1, desc2, kps2, ratio=0.9, spatial_th=10.0, mutual=False, norm=None, device=0, *, max_dist=None):
    """match_snn with the FGINN ratio test (first geometrically inconsistent neighbour, Mishkin et al.): the second distance of
    `m.distance < ratio * n.distance` comes from the nearest row of desc2 whose keypoint (kps2 [n2, >= 2]: x, y, ...) lies at least
    spatial_th pixels from the nearest neighbour's keypoint, so that the twin keypoints a detector emits for one structure (a second
    orientation, a neighbouring scale) do not veto a correct match.  A query whose every other train row lies inside the radius is
    not kept; the mutual check is the plain one.  Returns (query indices, train indices, distances) in query order."""
    rule = check_rule(ratio, mutual, max_dist, fginn=True)
    code, a, b = _prep(desc1, desc2, norm)
    r = check_fginn_th(spatial_th, "spatial_th")
    k2 = np.asarray(kps2, np.float64)
    if k2.ndim != 2 or k2.shape[1] < 2 or k2.shape[0] != b.shape[0]:
        raise ValueError("kps2 should hold one keypoint row (x, y, ...) per row of desc2")
    k2 = np.ascontiguousarray(k2[:, :2])
    import torch
    from . import tensor_api
    if not torch.cuda.is_available():
        raise _lib.MiDegensacError("no HIP device: this library has no CPU path")
    dev = torch.device("cuda", int(device))
    name = {NORM_L2: "l2", NORM_HAMMING: "hamming", NORM_L2_U8: "l2_u8"}[code]
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    idx, dist = tensor_api.knn_match_fginn_batch_tensors(ta, tb, torch.from_numpy(k2).to(dev), [a.shape[0]], [b.shape[0]], r, name)
    back = tensor_api.knn_match_tensors(tb, ta, name)[0] if mutual and b.shape[0] > 0 else None
    keep = tensor_api.match_filter_tensors(idx, dist, ratio, back) if rule.decide == 0 else \
        tensor_api.match_decide_tensors(idx, dist, ratio, back, None, max_dist)
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy()
    sel = np.flatnonzero(keep.cpu().numpy())
    return sel.astype(np.int64), idx[sel, 0].astype(np.int64), dist[sel, 0]


def tentative_points(kps1, kps2, desc1, desc2, ratio=0.9, mutual=False, norm=None, device=0, *, max_dist=None):
    """Matched coordinates ready for findHomography / findFundamentalMatrix: kps are [n, >=2] arrays (x, y, ...); ratio / mutual /
    max_dist as for match_snn"""
    q, t, _ = match_snn(desc1, desc2, ratio, mutual, norm, device, max_dist=max_dist)
    a = np.asarray(kps1, np.float64); b = np.asarray(kps2, np.float64)
    return a[q], b[t]


def kpts_to_xyA(kpts, device=0):
    """utils.py:24-41 `convert_cv2_kpts_to_xyA` on the GPU for keypoints given as an array [n, 4] = (x, y, size, angle in
    degrees) (cv2.KeyPoint.pt / .size / .angle): the [n, 6] float64 rows (x, y, a11, a12, a21, a22) the estimators accept."""
    k = np.ascontiguousarray(kpts, np.float32)
    if k.ndim != 2 or k.shape[1] != 4:
        raise ValueError("keypoints should be an array [n, 4] = (x, y, size, angle)")
    out = np.zeros((k.shape[0], 6))
    _lib.check_match(_lib.lib().mi_degensac_kpts_to_xyA(_lib.ptr(k), k.shape[0], int(device), _lib.dptr(out)), value_error=False)
    return out


# ---- float descriptors -> the uint8 rows of norm="l2_u8" (include/mi_degensac.h mi_degensac_desc_quantize*) ----
QUANT_NONE, QUANT_L2, QUANT_L1ROOT = 0, 1, 2
_QUANT_NORMALIZE = {None: QUANT_NONE, "none": QUANT_NONE, "l2": QUANT_L2, "l1root": QUANT_L1ROOT}
# preset -> (normalize, scale, offset).  "sift" and "rootsift" are the x 512 bytes of the SIFT convention; "unit" puts a signed
# unit-norm learned descriptor (HardNet, SOSNet, SuperPoint) around 128: a common offset cancels in every difference
QUANT_PRESETS = {"sift": ("l2", 512.0, 0), "rootsift": ("l1root", 512.0, 0), "unit": ("l2", 256.0, 128)}


def quant_params(preset="rootsift", normalize=None, scale=None, offset=None):
    """preset and the keywords that override it -> (normalize code, scale, offset), checked; raises ValueError.  normalize: "none", "l2",
    "l1root" (or the codes 0, 1, 2); scale: finite and > 0; offset: an integer 0 .. 255."""
    if preset not in QUANT_PRESETS:
        raise ValueError(f"preset should be one of {', '.join(sorted(QUANT_PRESETS))}")
    nz, sc, of = QUANT_PRESETS[preset]
    if normalize is not None:
        nz = normalize
    if isinstance(nz, str) and nz in _QUANT_NORMALIZE:
        nz = _QUANT_NORMALIZE[nz]
    elif isinstance(nz, bool) or nz not in (QUANT_NONE, QUANT_L2, QUANT_L1ROOT):
        raise ValueError('normalize should be "none", "l2" or "l1root"')
    if scale is not None:
        sc = _float(scale, "scale should be a number")
    if not (np.isfinite(sc) and sc > 0):
        raise ValueError("scale should be finite and > 0")
    if offset is not None:
        of = _integer(offset, "offset should be an integer 0 .. 255", 0, 255)
    return int(nz), float(sc), of


def check_quantize_input(shape, dtype):
    """shape and dtype name of the float descriptors of the quantise calls (numpy or torch); raises ValueError"""
    if _dtype_name(dtype) != "float32":
        raise ValueError("descriptors to quantise should be float32")
    if len(shape) != 2 or not 1 <= shape[1] <= L2_U8_MAX_DIM:
        raise ValueError(f"descriptors to quantise should be [n, dim] with 1 <= dim <= {L2_U8_MAX_DIM}")


def quantize_descriptors(desc, preset="rootsift", *, normalize=None, scale=None, offset=None, device=0, return_clipped=False):
    """float32 descriptors [n, dim] (dim <= 256) -> the uint8 rows [n, dim] that norm="l2_u8" takes, computed on the GPU
    (include/mi_degensac.h mi_degensac_desc_quantize states the arithmetic: fp64, q = clamp(rint(scale * y) + offset, 0, 255) with y the
    row as it is, L2-normalised, or the signed square root of the L1-normalised row).  preset: a key of QUANT_PRESETS — "sift" (L2, 512, 0),
    "rootsift" (L1-root, 512, 0), "unit" (L2, 256, 128: signed learned descriptors); normalize / scale / offset override it.
    A row with a NaN or an infinity, or one that cannot be normalised (all zero), becomes the constant row `offset`.
    return_clipped=True adds clipped [n] int32: the columns of each row that left 0 .. 255 before the clamp, -1 for such a dead row.
    Distances: an "l2_u8" distance between quantised rows is about scale x the float distance of the normalised rows, so a max_dist
    meant in float units is multiplied by scale.  The pad to whole 32-bit words is trimmed here (the matcher calls pad again)."""
    a = np.asarray(desc)
    check_quantize_input(a.shape, a.dtype)
    nz, sc, of = quant_params(preset, normalize, scale, offset)
    a = np.ascontiguousarray(a)
    n, dim = a.shape
    out = np.zeros((n, (dim + 3) & ~3), np.uint8)
    clipped = np.zeros(n, np.int32) if return_clipped else None
    qp = _lib.QuantParams(nz, sc, of)
    _lib.check_match(_lib.lib().mi_degensac_desc_quantize(C.byref(qp), a.ctypes.data_as(C.c_void_p), n, dim, int(device),
                                                          out.ctypes.data_as(C.c_void_p),
                                                          clipped.ctypes.data_as(C.c_void_p) if return_clipped else None))
    out = np.ascontiguousarray(out[:, :dim])
    return (out, clipped) if return_clipped else out


# ---- many image pairs at once: descriptors + keypoints -> tentatives -> F / H (include/mi_degensac.h mi_degensac_match_verify_batch*) ----
_MODEL_DEFAULTS = {"F": (0.5, 0.9999, 100000), "H": (1.0, 0.999, 50000)}          # findFundamentalMatrix / findHomography


def _dtype_name(dt):
    s = str(dt)
    return s[6:] if s.startswith("torch.") else np.dtype(dt).name


def _check_sides(model, ratio, norm, d1_shape, d1_dtype, d2_shape, d2_dtype, k1_shape, k1_dtype, k2_shape, k2_dtype):
    """model, ratio, norm and the descriptor / keypoint arrays of the two sides, on shapes and dtype names -> (norm code, "xy" / "kpts")"""
    if model not in ("F", "H"):
        raise ValueError("model should be 'F' or 'H'")
    if ratio is not None:                       # None = no ratio test (check_rule)
        r = _float(ratio, "ratio should be a number")
        if not np.isfinite(r) or r <= 0:
            raise ValueError("ratio should be finite and > 0")
    if len(d1_shape) != 2 or len(d2_shape) != 2 or d1_shape[1] != d2_shape[1] or d1_shape[1] == 0:
        raise ValueError("descriptors should be [N1, dim] and [N2, dim] with the same dim")
    t1, t2 = _dtype_name(d1_dtype), _dtype_name(d2_dtype)
    if t1 != t2 or t1 not in ("float32", "uint8"):
        raise ValueError("descriptors should both be float32 (L2) or both uint8 (Hamming)")
    if norm is None:
        norm = "hamming" if t1 == "uint8" else "l2"
    if norm not in _NORMS:
        raise ValueError("norm should be 'l2', 'hamming' or 'l2_u8'")
    if norm == "hamming" and t1 != "uint8":
        raise ValueError("the Hamming norm needs uint8 descriptors")
    if norm == "l2" and t1 != "float32":
        raise ValueError("the L2 norm needs float32 descriptors (norm 'l2_u8' takes uint8 rows of dim <= 256 as they are)")
    if norm == "l2_u8" and t1 != "uint8":
        raise ValueError("norm 'l2_u8' needs uint8 descriptors")
    if norm == "l2_u8" and d1_shape[1] > L2_U8_MAX_DIM:
        raise ValueError(f"norm 'l2_u8' takes dim <= {L2_U8_MAX_DIM}: use float32 descriptors with norm 'l2' beyond that")
    kind = _kps_kind((k1_shape, k1_dtype), (k2_shape, k2_dtype))
    if k1_shape[0] != d1_shape[0] or k2_shape[0] != d2_shape[0]:
        raise ValueError("one keypoint row per descriptor row")
    return _NORMS[norm], kind


def _kps_kind(kps1, kps2):
    """the layout of the two sides' keypoints, each (shape, dtype): "xy" for float64 rows [n, 2] / [n, 6], "kpts" for float32 [n, 4];
    raises ValueError"""
    kinds = []
    for shp, dt in (kps1, kps2):
        name = _dtype_name(dt)
        if len(shp) == 2 and name == "float64" and shp[1] in (2, 6):
            kinds.append(("xy", shp[1]))
        elif len(shp) == 2 and name == "float32" and shp[1] == 4:
            kinds.append(("kpts", 4))
        else:
            raise ValueError("keypoints should be float64 [n, 2] / [n, 6] rows or float32 [n, 4] = (x, y, size, angle)")
    if kinds[0] != kinds[1]:
        raise ValueError("kps1 and kps2 should have the same layout")
    return kinds[0][0]


def _counts_to_offsets(counts, n_rows, per, side_by_side):
    """rows per pair / per image of the two sides, counts = (counts1, counts2) against n_rows = (rows1, rows2) -> [offsets1, offsets2],
    int64 [len + 1] each; raises ValueError.  side_by_side: every check on side 1 before any on side 2 (the pair-list calls), else every
    side under one check before the next check (the ragged calls): which text a call raises for two different defects is pinned."""
    checks = [(lambda c, n: c.ndim != 1, f"counts1 and counts2 should be 1-D with one entry per {per}"),
              (lambda c, n: c.size and not np.issubdtype(c.dtype, np.integer), "counts should be integers"),
              (lambda c, n: (c < 0).any(), "counts should be >= 0"),
              (lambda c, n: c.sum() != n, "counts do not add up to the number of descriptor rows")]
    sides = [(np.asarray(c), n) for c, n in zip(counts, n_rows)]
    if side_by_side:
        order = [(side, check) for side in sides for check in checks]
    else:
        order = [(side, check) for check in checks for side in sides]
    for (c, n), (bad, msg) in order:
        if bad(c, n):
            raise ValueError(msg)
    offs = []
    for c, _ in sides:
        o = np.zeros(len(c) + 1, np.int64); np.cumsum(c, out=o[1:]); offs.append(o)
    return offs


def _seeds_u32(seeds, K):
    """one seed per pair as contiguous uint32 [K] (any integer, taken modulo 2^32); None = parallel.pair_seeds(0, K); raises ValueError"""
    if seeds is None:
        from . import parallel
        seeds = parallel.pair_seeds(0, K)
    sd = np.asarray(seeds)
    if sd.shape != (K,):
        raise ValueError("one seed per pair")
    return np.ascontiguousarray(sd.astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)


def check_match_verify_args(model, ratio, norm, d1_shape, d1_dtype, d2_shape, d2_dtype, k1_shape, k1_dtype, k2_shape, k2_dtype, counts1, counts2,
                            fginn_th=None):
    """The argument checks of the batched match-and-verify calls, on shapes and dtype names only (numpy or torch).  Returns
    (norm code, "xy" for float64 rows [n, 2] / [n, 6] or "kpts" for float32 keypoints [n, 4], offsets1, offsets2); raises ValueError.
    fginn_th: None, or the FGINN radius (finite and >= 0)."""
    if fginn_th is not None:
        check_fginn_th(fginn_th)
    code, kind = _check_sides(model, ratio, norm, d1_shape, d1_dtype, d2_shape, d2_dtype, k1_shape, k1_dtype, k2_shape, k2_dtype)
    if np.ndim(counts1) == 1 and np.ndim(counts2) == 1 and len(counts1) != len(counts2):
        raise ValueError("counts1 and counts2 should be 1-D with one entry per pair")
    o1, o2 = _counts_to_offsets((counts1, counts2), (d1_shape[0], d2_shape[0]), "pair", False)
    return code, kind, o1, o2


def check_match_pairs_args(model, ratio, norm, d1_shape, d1_dtype, d2_shape, d2_dtype, k1_shape, k1_dtype, k2_shape, k2_dtype, counts1, counts2, pairs,
                           seeds=None, guided=False, fginn_th=None):
    """The argument checks of the pair-list calls (knn_match_pairs_tensors, match_and_verify_pairs[_tensors], guided_match_pairs[_tensors]),
    on shapes and dtype names (numpy or torch) and on the list itself.  counts1 [M1] / counts2 [M2] are the rows per image of the two
    stores, pairs an integer array [K, 2] with K >= 1 of (image of store 1, image of store 2); seeds None or one per list entry.  guided
    and fginn_th are refused: the calls that have them as arguments do not run those stages (guided matching over a list is a call of
    its own, guided_match_pairs[_tensors]).  Returns (norm code, "xy" / "kpts", offsets1 [M1 + 1], offsets2 [M2 + 1], pairs as
    contiguous int32 [K, 2], pair_offsets int64 [K + 1], seeds as uint32 [K] or None); raises ValueError."""
    if guided:
        raise ValueError("guided matching is not part of this pair-list call: pass the models it returns to guided_match_pairs / "
                         "guided_match_pairs_tensors")
    if fginn_th is not None:
        raise ValueError("fginn_th (the FGINN ratio test) is not part of the pair-list calls: use match_and_verify_batch, or "
                         "match_and_verify_fginn_pairs / match_and_verify_fginn_pairs_tensors over a pair list")
    code, kind = _check_sides(model, ratio, norm, d1_shape, d1_dtype, d2_shape, d2_dtype, k1_shape, k1_dtype, k2_shape, k2_dtype)
    offs = _counts_to_offsets((counts1, counts2), (d1_shape[0], d2_shape[0]), "image", True)
    pr, po = _check_pair_list(pairs, offs[0], offs[1])
    return code, kind, offs[0], offs[1], pr, po, None if seeds is None else _seeds_u32(seeds, len(pr))


def _check_pair_list(pairs, o1, o2):
    """a pair list over two stores with the image offsets o1 / o2 -> (pairs as contiguous int32 [K, 2], pair_offsets int64 [K + 1]);
    raises ValueError"""
    pr = np.asarray(pairs)
    if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
        raise ValueError("pairs should be an integer array [K, 2] of (image of store 1, image of store 2)")
    K = pr.shape[0]
    if K == 0:
        raise ValueError("at least one pair")
    m1, m2 = len(o1) - 1, len(o2) - 1
    if (pr < 0).any() or (pr[:, 0] >= m1).any() or (pr[:, 1] >= m2).any():
        raise ValueError(f"pairs hold an image index outside its store ({m1} and {m2} images)")
    pr = np.ascontiguousarray(pr, np.int32)
    po = np.zeros(K + 1, np.int64); np.cumsum(np.diff(o1)[pr[:, 0]], out=po[1:])
    if po[-1] > 0x3fffffff or np.diff(o2)[pr[:, 1]].sum() > 0x3fffffff:
        raise ValueError("too many rows in one pair list")
    return pr, po


# ---- a checked layout and the entry points' layout arguments: the order inside each family is the ABI (include/mi_degensac.h) ----
# pr None = the ragged batch (entry p = pair p, po = o1), else a pair list over image stores; K entries, n output rows
Layout = collections.namedtuple("Layout", "name o1 o2 pr po K n")


def layout(o1, o2, pr=None, po=None):
    if pr is None:
        return Layout("batch", o1, o2, None, o1, len(o1) - 1, int(o1[-1]))
    return Layout("pairs", o1, o2, pr, po, len(pr), int(po[-1]))


def _stores(L):
    return _lib.ptr(L.o1), len(L.o1) - 1, _lib.ptr(L.o2), len(L.o2) - 1


def knn_layout(L, dim):
    """mi_degensac_match_knn2_* / _fginn_knn2_*: the arguments between the descriptors and (FGINN: the keypoints,) the device"""
    return (_lib.ptr(L.o1), _lib.ptr(L.o2), L.K, dim) if L.pr is None else _stores(L) + (_lib.ptr(L.pr), L.K, dim)


def verify_layout(L, kp1, kp2, kp_dim):
    """mi_degensac_match_verify_* and _verify_fh_*: the arguments between the descriptors and the estimator's parameter block(s); kp1 /
    kp2 = the keypoint pointers as the entry point takes them"""
    return (_lib.ptr(L.o1), _lib.ptr(L.o2), kp1, kp2, kp_dim, L.K) if L.pr is None else _stores(L) + (kp1, kp2, kp_dim, _lib.ptr(L.pr), L.K)


def guided_layout(L, kp1, kp2, kp_dim):
    """mi_degensac_match_guided_*: the arguments between the descriptors and the models"""
    return (_lib.ptr(L.o1), _lib.ptr(L.o2), kp1, kp2, kp_dim, L.K) if L.pr is None else _stores(L) + (_lib.ptr(L.pr), L.K, kp1, kp2, kp_dim)


def exhaustive_pairs(n, ordered=False):
    """The pair list of a collection of n images matched exhaustively: every (i, j) with i < j in lexicographic order, [n (n - 1) / 2, 2],
    or with ordered=True every (i, j) with i != j, [n (n - 1), 2] (the ratio test is not symmetric).  int64."""
    n = int(n)
    if n < 0:
        raise ValueError("n should be >= 0")
    i, j = np.divmod(np.arange(n * n, dtype=np.int64), max(n, 1))
    sel = (i != j) if ordered else (i < j)
    return np.stack([i[sel], j[sel]], axis=1)


def check_fginn_th(fginn_th, name="fginn_th"):
    """the FGINN radius of the matcher calls: a finite number >= 0; raises ValueError"""
    r = _float(fginn_th, f"{name} should be a number")
    if not (np.isfinite(r) and r >= 0):
        raise ValueError(f"{name} should be finite and >= 0")
    return r


def guided_entry(layout, fginn_r):
    """the guided entry point of a layout ("batch_dev", "batch", "pairs_dev", "pairs"): fginn_r None = the plain call, a checked radius =
    the call that honours second_nn / spatial_th of its match params (FGINN inside the gate)"""
    return getattr(_lib.lib(), f"mi_degensac_match_guided_{'' if fginn_r is None else 'fginn_'}{layout}")


def estimator_params(model, px_th=None, conf=None, max_iters=None, laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True,
                     enable_degeneracy_check=True):
    """mi_degensac_params of findFundamentalMatrix / findHomography with their defaults where an argument is None"""
    from .api import _error_type, error_type_dict_fundamental, error_type_dict_homography
    d = _MODEL_DEFAULTS[model]
    et = _error_type(error_type_dict_fundamental if model == "F" else error_type_dict_homography, error_type)
    return _lib.make_params(d[0] if px_th is None else px_th, d[1] if conf is None else conf, d[2] if max_iters is None else max_iters, et,
                            symmetric_error_check, max(0.0, laf_consistensy_coef), enable_degeneracy_check if model == "F" else True)


def check_guided_fginn_th(guided, guided_fginn_th):
    """guided_fginn_th of the match-and-verify calls: None, or (only with guided=True) the checked radius; raises ValueError"""
    if guided_fginn_th is None:
        return None
    if not guided:
        raise ValueError("guided_fginn_th is the FGINN radius of the guided stage: pass guided=True with it (fginn_th is the radius of "
                         "the tentatives in front of the estimator)")
    return check_fginn_th(guided_fginn_th, "guided_fginn_th")


def check_guided_args(model, px_th, error_type, models_shape, models_dtype, K):
    """The guided stage's own argument checks, after check_match_verify_args (shapes and dtype names only, numpy or torch): models
    float64 [K, 3, 3], px_th >= 0 (None = the model's default), error_type one of the model's names.  Returns (px_th, error_type code);
    raises ValueError."""
    from .api import _error_type, error_type_dict_fundamental, error_type_dict_homography
    if model not in ("F", "H"):
        raise ValueError("model should be 'F' or 'H'")
    if tuple(models_shape) != (K, 3, 3):
        raise ValueError(f"models should be [K, 3, 3] = [{K}, 3, 3], one model per pair")
    if _dtype_name(models_dtype) != "float64":
        raise ValueError("models should be float64")
    px = _float(_MODEL_DEFAULTS[model][0] if px_th is None else px_th, "px_th should be a number")
    if not px >= 0:
        raise ValueError("px_th should be >= 0 (and not NaN)")
    et = _error_type(error_type_dict_fundamental if model == "F" else error_type_dict_homography, error_type)
    return px, et


def _h_driver_form(M):
    """user-facing H -> the driver's form H_c = inv(H)^T (utils.py:108 inverted); zero models stay zero"""
    out = np.zeros_like(M)
    for i in range(M.shape[0]):
        if np.abs(M[i]).sum() != 0:
            out[i] = np.linalg.inv(M[i]).T
    return out


def _h_user_form(M):
    """the driver's H_c -> the user-facing H = inv(H_c^T) (utils.py:108); zero models stay zero"""
    out = np.zeros_like(M)
    for i in range(M.shape[0]):
        if np.abs(M[i]).sum() != 0:
            out[i] = np.linalg.inv(M[i].T)
    return out


def _driver_models(M, model, driver_form, K):
    """the models of a call as the library takes them: contiguous float64 [K, 9], H in the driver's form"""
    return np.ascontiguousarray(M if (model == "F" or driver_form) else _h_driver_form(M), np.float64).reshape(K, 9)


def _set_last_stats(st, cnt):
    """the per-pair stats rows [K, 16] and tentative counts [K] of a match-and-verify call -> last_stats()"""
    from . import api
    stats = [_lib.stats_dict(s) for s in st]
    for d, c in zip(stats, cnt):
        d["tentatives"] = int(c)
    api._tls.stats = stats


def _stack_pairs(kps1_list, kps2_list, desc1_list, desc2_list, model, ratio, norm, device, fginn_th=None):
    """the per-pair lists of the batched calls -> (norm code, A, B, K1, K2, offsets1, offsets2): descriptors padded to whole 32-bit
    words for uint8 rows, keypoints as float64 [n, 2] / [n, 6] rows"""
    K = len(desc1_list)
    if not (len(kps1_list) == len(kps2_list) == len(desc2_list) == K):
        raise ValueError("kps1_list, kps2_list, desc1_list and desc2_list should hold one entry per pair")
    if K == 0:
        raise ValueError("at least one pair")
    a, b, k1, k2 = (_rows_list(lst, "every pair's arrays should be 2-D with the dtype and width of pair 0")
                    for lst in (desc1_list, desc2_list, kps1_list, kps2_list))
    c1 = [x.shape[0] for x in a]; c2 = [x.shape[0] for x in b]
    if [x.shape[0] for x in k1] != c1 or [x.shape[0] for x in k2] != c2:
        raise ValueError("one keypoint row per descriptor row")
    A = np.concatenate(a); B = np.concatenate(b); K1 = np.concatenate(k1); K2 = np.concatenate(k2)
    code, kind, o1, o2 = check_match_verify_args(model, ratio, norm, A.shape, A.dtype, B.shape, B.dtype, K1.shape, K1.dtype, K2.shape, K2.dtype,
                                                 np.asarray(c1, np.int64), np.asarray(c2, np.int64), fginn_th)
    return code, kind, A, B, K1, K2, o1, o2


def _finish_pairs(code, kind, A, B, K1, K2, device):
    if code != NORM_L2:
        A, B = _pad_words(A, B)
    A = np.ascontiguousarray(A); B = np.ascontiguousarray(B)
    if kind == "kpts":
        K1 = kpts_to_xyA(K1, device); K2 = kpts_to_xyA(K2, device)
    return A, B, np.ascontiguousarray(K1, np.float64), np.ascontiguousarray(K2, np.float64)


def _guided_host(L, code, A, B, K1, K2, Md, model, rule, px, et, device, fginn_r=None):
    """mi_degensac_match_guided_batch / _pairs (fginn_r, a checked radius: mi_degensac_match_guided_fginn_*) on prepared host arrays;
    L = the checked layout, Md = [K, 9] driver-form models.  Returns (match, idx, dist, counts)."""
    idx, dist, match = _knn_out(L.n, True)
    cnt = np.zeros(L.K, np.int32)
    mp = _lib.match_params(code, A.shape[1], rule, fginn_r); gp = _lib.GuideParams(model == "H", et, px)
    rc = guided_entry(L.name, fginn_r)(C.byref(mp), _lib.vptr(A), _lib.vptr(B), *guided_layout(L, _lib.dptr(K1), _lib.dptr(K2), K1.shape[1]),
                                       _lib.dptr(Md), C.byref(gp), int(device), _lib.ptr(idx), _lib.ptr(dist), _lib.ptr(match), _lib.ptr(cnt))
    _lib.check_match(rc)
    return match, idx, dist, cnt


def _guided_matches(L, match, dist):
    """per entry of L (query indices, train indices, distances) of the queries with a guided match, in query order"""
    out = []
    for p in range(L.K):
        m = match[L.po[p]:L.po[p + 1]]
        q = np.flatnonzero(m >= 0)
        out.append((q.astype(np.int64), m[q].astype(np.int64), dist[L.po[p]:L.po[p + 1]][q, 0]))
    return out


def guided_match_batch(kps1_list, kps2_list, desc1_list, desc2_list, models, model="F", ratio=0.9, mutual=False, px_th=None,
                       error_type="sampson", norm=None, driver_form=False, device=0, fginn_th=None, *, max_dist=None):
    """Guided matching of K image pairs in one call: per pair the 2-NN search restricted to the train keypoints that are inliers of
    the pair's model (models [K, 3, 3] float64: F, or the user-facing H that findHomography returns; driver_form=True takes them in the
    driver's form, H_c = inv(H)^T), with the estimator's residual for error_type and its threshold from px_th (None = the model's
    default, 0.5 for F, 1.0 for H).  The ratio test then keeps a query whose nearest gated row is closer than ratio times the second;
    a query with a single gated row passes (nothing competes with it).  A zero model gives its pair no matches.  Arrays as for
    match_and_verify_batch.  Returns per pair (query indices, train indices, distances) in query order, like match_snn.
    A gate that lets everything through (a huge px_th) is correct but slower than the unguided matcher.
    fginn_th: None = the second gated row decides; a number (pixels of kps2, finite and >= 0) takes the second distance from the nearest
    GATED row whose keypoint lies at least that far from the nearest gated row's (FGINN inside the gate), so a keypoint's own twin (a
    second orientation, a neighbouring scale), which lies inside the band too, no longer fails the ratio test.  A query whose only gated
    companions lie inside the radius is KEPT (dist1 = inf: nothing competes with it), unlike match_fginn, which needs a second row.
    ratio=None, mutual="ratio" and max_dist: the rule of check_rule; the reverse ratio test takes the guided form too (a train row with a
    single gated query row passes)."""
    rule = check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    code, kind, A, B, K1, K2, o1, o2 = _stack_pairs(kps1_list, kps2_list, desc1_list, desc2_list, model, ratio, norm, device)
    K = len(o1) - 1
    M = np.asarray(models)
    px, et = check_guided_args(model, px_th, error_type, M.shape, M.dtype, K)
    fr = None if fginn_th is None else check_fginn_th(fginn_th)
    A, B, K1, K2 = _finish_pairs(code, kind, A, B, K1, K2, device)
    L = layout(o1, o2)
    match, _, dist, _ = _guided_host(L, code, A, B, K1, K2, _driver_models(M, model, driver_form, K), model, rule, px, et, device, fr)
    return _guided_matches(L, match, dist)


def guided_match(kps1, kps2, desc1, desc2, M, model="F", ratio=0.9, mutual=False, px_th=None, error_type="sampson", norm=None,
                 driver_form=False, device=0, fginn_th=None, *, max_dist=None):
    """guided_match_batch for one pair: (query indices, train indices, distances) of the guided matches under model M [3, 3];
    fginn_th as there (FGINN inside the gate; a query whose only gated companions are its twins is kept)"""
    return guided_match_batch([kps1], [kps2], [desc1], [desc2], np.asarray(M)[None], model, ratio, mutual, px_th, error_type, norm,
                              driver_form, device, fginn_th, max_dist=max_dist)[0]


def match_and_verify_batch(kps1_list, kps2_list, desc1_list, desc2_list, model="F", ratio=0.9, mutual=False, px_th=None, conf=None,
                           max_iters=None, laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True,
                           enable_degeneracy_check=True, seeds=None, norm=None, device=0, guided=False, fginn_th=None, guided_fginn_th=None, *,
                           max_dist=None):
    """K image pairs from descriptors and keypoints to models in one call: per pair the 2-NN ratio test of match_snn (optionally
    mutual), then findFundamentalMatrix (model "F") or findHomography ("H") on its tentatives, all pairs in one launch.  kps are
    float64 [n, 2] / [n, 6] rows or float32 [n, 4] keypoints (x, y, size, angle -> LAF rows as kpts_to_xyA); descriptors float32
    (L2) or uint8 (Hamming, or L2 with norm="l2_u8" and dim <= 256; padded to whole 32-bit words here).
    A pair with fewer than 8 (F) / 4 (H) tentatives gets a zero model
    and no inliers.  seeds default to parallel.pair_seeds(0, K).  Returns (models [K, 3, 3], [match_p], [inlier_p]): match_p[i] =
    the train row of query i or -1, inlier_p[i] = query i is a tentative and an inlier; H is the user-facing inv(H_c^T).
    guided=True runs guided_match_batch after the estimator with the driver-form models it returned (no conversion), this call's
    px_th / error_type / ratio / mutual, and adds a fourth element [guided_p]: the guided match of every query or -1.
    fginn_th: None = the plain ratio test; a number switches it to the FGINN ratio test of match_fginn at that radius in pixels of
    kps2 (the guided stage keeps its own gate and decision).
    guided_fginn_th: None, or the radius of guided_match_batch(fginn_th=) for the guided stage; only with guided=True (ValueError else).
    ratio=None, mutual="ratio" and max_dist: the rule of check_rule, for the tentatives and (guided form) for the guided stage.
    last_stats() holds the per-pair statistics, with "tentatives"."""
    gfr = check_guided_fginn_th(guided, guided_fginn_th)
    rule = check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    if gfr is not None:
        check_rule(ratio, mutual, max_dist, fginn=True)
    code, kind, A, B, K1, K2, o1, o2 = _stack_pairs(kps1_list, kps2_list, desc1_list, desc2_list, model, ratio, norm, device, fginn_th)
    K = len(o1) - 1
    prm = estimator_params(model, px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check)
    A, B, K1, K2 = _finish_pairs(code, kind, A, B, K1, K2, device)
    sd = _seeds_u32(seeds, K)
    L = layout(o1, o2)
    # guide: the driver-form models as the library wrote them, before the inversion to the user-facing H
    guide = (lambda M: _guided_host(L, code, A, B, K1, K2, M, model, rule, prm.px_th, prm.error_type, device, gfr)[0]) if guided else None
    M, match, inl, gm = _verify_host(_lib.lib().mi_degensac_match_verify_batch, L, model, _lib.match_params(code, A.shape[1], rule, fginn_th),
                                     A, B, K1, K2, prm, sd, device, guide)
    res = (M, _cut(L, match), _cut(L, inl, bool))
    return res + (_cut(L, gm),) if guided else res


def _verify_out(K, n):
    """the outputs of one estimator over a layout with their fills: (model [K, 9], inlier [n] uint8, stats [K, 16])"""
    return np.zeros((K, 9)), np.zeros(n, np.uint8), np.zeros((K, 16), np.int32)


def _cut(L, x, dtype=None):
    """a per-row output as one array per entry of L"""
    return [x[L.po[p]:L.po[p + 1]] if dtype is None else x[L.po[p]:L.po[p + 1]].astype(dtype) for p in range(L.K)]


def _verify_host(entry, L, model, mp, A, B, K1, K2, prm, sd, device, guide=None):
    """a host-pointer single-model mi_degensac_match_verify_* call on prepared arrays, for both layouts; guide (nullable) gets the
    driver-form models [K, 9].  Returns (model [K, 3, 3] — H user-facing —, match [n], inlier [n] uint8, what guide returned)."""
    M, inl, st = _verify_out(L.K, L.n)
    match = np.full(L.n, -1, np.int32); cnt = np.zeros(L.K, np.int32)
    rc = entry(1 if model == "H" else 0, C.byref(mp), _lib.vptr(A), _lib.vptr(B), *verify_layout(L, _lib.dptr(K1), _lib.dptr(K2), K1.shape[1]),
               C.byref(prm), _lib.ptr(sd), int(device), _lib.dptr(M), _lib.ptr(match), _lib.ptr(inl), _lib.ptr(st), _lib.ptr(cnt))
    _lib.check(rc)
    _set_last_stats(st, cnt)
    gm = guide(M) if guide else None
    M = M.reshape(L.K, 3, 3)
    return _h_user_form(M) if model == "H" else M, match, inl, gm


def _stack_stores(kps_list, desc_list, kps2_list, desc2_list):
    """the per-image lists of the pair-list calls -> ((A, K1, counts1), (B, K2, counts2), one): the concatenated descriptor and keypoint
    rows of each store with its rows per image; one = no second store was given (both sides are then the same tuple)"""
    if (kps2_list is None) != (desc2_list is None):
        raise ValueError("kps2_list and desc2_list go together")
    one = desc2_list is None
    stores = []
    for kl, dl in ((kps_list, desc_list),) if one else ((kps_list, desc_list), (kps2_list, desc2_list)):
        if len(kl) != len(dl):
            raise ValueError("one keypoint array per descriptor array")
        if len(dl) == 0:
            raise ValueError("at least one image per store")
        d, k = (_rows_list(lst, "every image's arrays should be 2-D with the dtype and width of image 0") for lst in (dl, kl))
        c =[x.shape[0] for x in d]
        if [x.shape[0] for x in k] != c:
            raise ValueError("one keypoint row per descriptor row")
        stores.append((np.concatenate(d), np.concatenate(k), np.asarray(c, np.int64)))
    return stores[0], stores[-1], one


def _finish_stores(code, kind, A, K1, B, K2, one, device):
    """the stores as the library takes them: uint8 rows padded to whole words, keypoints as float64 rows; one store = the same arrays
    on both sides, which the host-pointer entry points upload once"""
    def prep(D, Kp):
        if code != NORM_L2:
            D = _pad_words(D, D)[0]
        if kind == "kpts":
            Kp = kpts_to_xyA(Kp, device)
        return np.ascontiguousarray(D), np.ascontiguousarray(Kp, np.float64)
    A, K1 = prep(A, K1)
    B, K2 = (A, K1) if one else prep(B, K2)
    return A, K1, B, K2


def match_and_verify_pairs(kps_list, desc_list, pairs, model="F", ratio=0.9, mutual=False, px_th=None, conf=None, max_iters=None,
                           laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True, enable_degeneracy_check=True, seeds=None,
                           norm=None, device=0, guided=False, fginn_th=None, kps2_list=None, desc2_list=None, *, max_dist=None):
    """match_and_verify_batch over a pair list: descriptors and keypoints are given ONCE per image (kps_list[i], desc_list[i]) and
    pairs [K, 2] says which (i, j) to run, queries = image i, train set = image j (exhaustive_pairs(n) for a whole collection).  With
    kps2_list / desc2_list the train images come from that second store (queries against a database), else from the same one.  The
    list may hold self pairs, repeats, both orders and any order; images may be empty or unused.  Each store is uploaded once, whatever
    the number of pairs.  Per pair the results are bit for bit those of match_and_verify_batch on the pair's copied arrays with the
    same seeds (one per list entry, default parallel.pair_seeds(0, K)).  Returns (models [K, 3, 3], [match_p], [inlier_p]) as
    match_and_verify_batch; guided and fginn_th are not part of this call (ValueError): guided_match_pairs takes the models it returns,
    match_and_verify_fginn_pairs runs the FGINN ratio test over a list.
    last_stats() holds the per-pair statistics."""
    return _match_verify_pairs(None, kps_list, desc_list, pairs, model, ratio, mutual, px_th, conf, max_iters, laf_consistensy_coef, error_type,
                               symmetric_error_check, enable_degeneracy_check, seeds, norm, device, guided, fginn_th, kps2_list, desc2_list, max_dist)


def match_and_verify_fginn_pairs(kps_list, desc_list, pairs, fginn_th, model="F", ratio=0.9, mutual=False, px_th=None, conf=None, max_iters=None,
                                 laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True, enable_degeneracy_check=True,
                                 seeds=None, norm=None, device=0, guided=False, kps2_list=None, desc2_list=None, *, max_dist=None):
    """match_and_verify_pairs with the FGINN ratio test of match_fginn in front of the estimator: fginn_th is the radius in pixels of the
    train image's keypoints, a finite number >= 0.  Stores (one, or two with kps2_list / desc2_list; a store named on both sides is
    uploaded once), list, seeds and the returned tuple are those of match_and_verify_pairs; per entry the results are bit for bit those
    of match_and_verify_batch(fginn_th=) on the entry's copied arrays with the same seeds.  guided=True is refused here as well:
    guided_match_pairs takes the models this call returns.  last_stats() holds the per-pair statistics."""
    r = check_fginn_th(fginn_th)
    return _match_verify_pairs(r, kps_list, desc_list, pairs, model, ratio, mutual, px_th, conf, max_iters, laf_consistensy_coef, error_type,
                               symmetric_error_check, enable_degeneracy_check, seeds, norm, device, guided, None, kps2_list, desc2_list, max_dist)


def _match_verify_pairs(fginn_r, kps_list, desc_list, pairs, model, ratio, mutual, px_th, conf, max_iters, laf_consistensy_coef, error_type,
                        symmetric_error_check, enable_degeneracy_check, seeds, norm, device, guided, fginn_th, kps2_list, desc2_list, max_dist=None):
    """the body of the two pair-list match-and-verify calls: fginn_r None = the plain call (which refuses fginn_th), a checked radius =
    the FGINN call and its entry point; ratio / mutual / max_dist: the rule of check_rule"""
    rule = check_rule(ratio, mutual, max_dist, fginn=fginn_r is not None)
    (A, K1, c1), (B, K2, c2), one = _stack_stores(kps_list, desc_list, kps2_list, desc2_list)
    code, kind, o1, o2, pr, po, sd = check_match_pairs_args(model, ratio, norm, A.shape, A.dtype, B.shape, B.dtype, K1.shape, K1.dtype, K2.shape,
                                                            K2.dtype, c1, c2, pairs, seeds, guided, fginn_th)
    prm = estimator_params(model, px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check)
    K = len(pr)
    if sd is None:
        sd = _seeds_u32(None, K)
    A, K1, B, K2 = _finish_stores(code, kind, A, K1, B, K2, one, device)              # one store: uploaded once
    L = layout(o1, o2, pr, po)
    entry = _lib.lib().mi_degensac_match_verify_pairs if fginn_r is None else _lib.lib().mi_degensac_match_verify_fginn_pairs
    M, match, inl, _ = _verify_host(entry, L, model, _lib.match_params(code, A.shape[1], rule, fginn_r), A, B, K1, K2, prm, sd, device)
    return M, _cut(L, match), _cut(L, inl, bool)


# ---- match once, verify F and H (include/mi_degensac.h mi_degensac_match_verify_fh_*) ----
_ESTIMATOR_KEYS = ("px_th", "conf", "max_iters", "laf_consistensy_coef", "error_type", "symmetric_error_check")


def two_view_params(f_params=None, h_params=None):
    """f_params / h_params of the match_and_verify_fh_* calls -> (mi_degensac_params for F, for H).  Each is None or a dict of the estimator
    keywords estimator_params takes (px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check, and for F
    enable_degeneracy_check); missing keys take findFundamentalMatrix's / findHomography's defaults.  An unknown key is a ValueError."""
    out = []
    for model, d, name in (("F", f_params, "f_params"), ("H", h_params, "h_params")):
        d = {} if d is None else d
        if not isinstance(d, dict):
            raise ValueError(f"{name} should be a dict of estimator keywords, or None")
        allowed = _ESTIMATOR_KEYS + (("enable_degeneracy_check",) if model == "F" else ())
        bad = sorted(str(k) for k in d if k not in allowed)
        if bad:
            raise ValueError(f"{name}: unknown key {', '.join(bad)} (known: {', '.join(allowed)})")
        out.append(estimator_params(model, **d))
    return tuple(out)


def two_view_config(summary, min_inliers=15, max_h_ratio=0.8):
    """The class of every pair from the summary [K, 4] = (tentatives, nF, nH, nFH) of a match_and_verify_fh_* call (numpy, or a tensor,
    which is copied to the host): int8 [K] with 0 = rejected (max(nF, nH) < min_inliers), 2 = planar or panoramic (nH > max_h_ratio * nF,
    compared in float64: the homography explains what the fundamental matrix explains), 1 = general.  This is COLMAP's H/F inlier-ratio
    test of its two-view geometry estimation; the thresholds are the caller's business (the defaults are COLMAP's min_num_inliers and
    max_H_inlier_ratio), and so is what to do with each class."""
    s = summary.detach().cpu().numpy() if hasattr(summary, "detach") else np.asarray(summary)
    if s.ndim != 2 or s.shape[1] != 4 or (s.size and not np.issubdtype(s.dtype, np.integer)):
        raise ValueError("summary should be an integer array [K, 4] = (tentatives, nF, nH, nFH)")
    nF = s[:, 1].astype(np.float64); nH = s[:, 2].astype(np.float64)
    out = np.ones(s.shape[0], np.int8)
    out[nH > float(max_h_ratio) * nF] = 2
    out[np.maximum(nF, nH) < min_inliers] = 0
    return out


def _set_last_stats_fh(stf, sth, cnt):
    """last_stats() of a two-model call: per pair the F row's dict with "tentatives", and the H row's dict under "homography" """
    from . import api
    stats = [_lib.stats_dict(s) for s in stf]
    for d, h, c in zip(stats, sth, cnt):
        d["tentatives"] = int(c); d["homography"] = _lib.stats_dict(h)
    api._tls.stats = stats


def _fh_host(L, mp, A, B, K1, K2, prm_f, prm_h, sd, device):
    """the host-pointer mi_degensac_match_verify_fh_* call of the layout L on prepared arrays.  Returns (F [K, 3, 3], H [K, 3, 3]
    user-facing, [match_p], [inlier_f_p], [inlier_h_p], summary [K, 4])."""
    K = L.K
    F, inf, stf = _verify_out(K, L.n); H, inh, sth = _verify_out(K, L.n)
    match = np.full(L.n, -1, np.int32); summ = np.zeros((K, 4), np.int32); cnt = np.zeros(K, np.int32)
    rc = getattr(_lib.lib(), f"mi_degensac_match_verify_fh_{L.name}")(
        C.byref(mp), _lib.vptr(A), _lib.vptr(B), *verify_layout(L, _lib.dptr(K1), _lib.dptr(K2), K1.shape[1]), C.byref(prm_f), C.byref(prm_h),
        _lib.ptr(sd), int(device), _lib.dptr(F), _lib.dptr(H), _lib.ptr(match), _lib.ptr(inf), _lib.ptr(inh), _lib.ptr(stf), _lib.ptr(sth),
        _lib.ptr(summ), _lib.ptr(cnt))
    _lib.check(rc)
    _set_last_stats_fh(stf, sth, cnt)
    return F.reshape(K, 3, 3), _h_user_form(H.reshape(K, 3, 3)), _cut(L, match), _cut(L, inf, bool), _cut(L, inh, bool), summ


def match_and_verify_fh_batch(kps1_list, kps2_list, desc1_list, desc2_list, ratio=0.9, mutual=False, norm=None, fginn_th=None, seeds=None,
                              f_params=None, h_params=None, device=0, *, max_dist=None):
    """match_and_verify_batch with BOTH models on the same tentatives: the matching runs once, then findFundamentalMatrix (f_params) and
    findHomography (h_params) on every pair's tentatives, each seeded with the pair's seed.  Arrays, ratio, mutual, norm, fginn_th and
    seeds as for match_and_verify_batch; f_params / h_params as for two_view_params.  Per pair F / inlier_f are bit for bit those of
    match_and_verify_batch(model="F", **f_params), H / inlier_h those of model="H" with h_params; a pair with 4 .. 7 tentatives has an H
    and a zero F, below 4 both are zero.  Returns (F [K, 3, 3], H [K, 3, 3] user-facing, [match_p], [inlier_f_p], [inlier_h_p],
    summary [K, 4] int32 = per pair (tentatives, nF, nH, nFH): its tentatives and its queries that are inliers of F, of H, of both);
    two_view_config(summary) classifies the pairs.  The guided stage is not part of this call: guided_match_batch takes either returned
    model as it is.  last_stats() holds per pair the F statistics with "tentatives", and the H statistics under "homography"."""
    rule = check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    code, kind, A, B, K1, K2, o1, o2 = _stack_pairs(kps1_list, kps2_list, desc1_list, desc2_list, "H", ratio, norm, device, fginn_th)
    K = len(o1) - 1
    prm_f, prm_h = two_view_params(f_params, h_params)
    A, B, K1, K2 = _finish_pairs(code, kind, A, B, K1, K2, device)
    sd = _seeds_u32(seeds, K)
    return _fh_host(layout(o1, o2), _lib.match_params(code, A.shape[1], rule, fginn_th), A, B, K1, K2, prm_f, prm_h, sd, device)


def match_and_verify_fh_pairs(kps_list, desc_list, pairs, ratio=0.9, mutual=False, norm=None, fginn_th=None, seeds=None, f_params=None,
                              h_params=None, device=0, kps2_list=None, desc2_list=None, *, max_dist=None):
    """match_and_verify_fh_batch over a pair list: descriptors and keypoints once per image, pairs [K, 2] the (i, j) to run (stores, list
    and seeds as for match_and_verify_pairs).  fginn_th is part of this call (None = the plain ratio test): there is no separate FGINN
    form.  Per entry and model the results are bit for bit those of match_and_verify_pairs / match_and_verify_fginn_pairs with that model
    and its parameters.  Returns (F [K, 3, 3], H [K, 3, 3] user-facing, [match_p], [inlier_f_p], [inlier_h_p], summary [K, 4] int32) as
    match_and_verify_fh_batch.  The guided stage is not part of this call: guided_match_pairs takes either returned model as it is."""
    fr = None if fginn_th is None else check_fginn_th(fginn_th)
    rule = check_rule(ratio, mutual, max_dist, fginn=fr is not None)
    (A, K1, c1), (B, K2, c2), one = _stack_stores(kps_list, desc_list, kps2_list, desc2_list)
    code, kind, o1, o2, pr, po, sd = check_match_pairs_args("H", ratio, norm, A.shape, A.dtype, B.shape, B.dtype, K1.shape, K1.dtype, K2.shape,
                                                            K2.dtype, c1, c2, pairs, seeds)
    prm_f, prm_h = two_view_params(f_params, h_params)
    K = len(pr)
    if sd is None:
        sd = _seeds_u32(None, K)
    A, K1, B, K2 = _finish_stores(code, kind, A, K1, B, K2, one, device)              # one store: uploaded once
    return _fh_host(layout(o1, o2, pr, po), _lib.match_params(code, A.shape[1], rule, fr), A, B, K1, K2, prm_f, prm_h, sd, device)


def guided_match_pairs(kps_list, desc_list, pairs, models, model="F", ratio=0.9, mutual=False, px_th=None, error_type="sampson", norm=None,
                       driver_form=False, device=0, kps2_list=None, desc2_list=None, fginn_th=None, *, max_dist=None):
    """guided_match_batch over a pair list: descriptors and keypoints are given ONCE per image, pairs [K, 2] says which (i, j) to run and
    models [K, 3, 3] float64 holds one model per LIST ENTRY (the same (i, j) may appear twice with two models) — what
    match_and_verify_pairs returned for the same list goes in as it is: F, or the user-facing H (driver_form=True: H_c = inv(H)^T).  Stores
    as for match_and_verify_pairs: kps2_list / desc2_list name a second store for the train images, each store is uploaded once and no
    row is copied per pair.  Per entry the result is bit for bit that of guided_match_batch on the entry's copied arrays.  Returns per
    list entry (query indices, train indices, distances) in query order; train indices are local to image j.
    fginn_th as in guided_match_batch (FGINN inside the gate on the keypoints of the entry's train image; a query whose only gated
    companions lie inside the radius is kept).  ratio=None, mutual="ratio" and max_dist as in guided_match_batch."""
    rule = check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    (A, K1, c1), (B, K2, c2), one = _stack_stores(kps_list, desc_list, kps2_list, desc2_list)
    code, kind, o1, o2, pr, po, _ = check_match_pairs_args(model, ratio, norm, A.shape, A.dtype, B.shape, B.dtype, K1.shape, K1.dtype, K2.shape,
                                                           K2.dtype, c1, c2, pairs)
    K = len(pr)
    M = np.asarray(models)
    px, et = check_guided_args(model, px_th, error_type, M.shape, M.dtype, K)
    fr = None if fginn_th is None else check_fginn_th(fginn_th)
    A, K1, B, K2 = _finish_stores(code, kind, A, K1, B, K2, one, device)
    L = layout(o1, o2, pr, po)
    match, _, dist, _ = _guided_host(L, code, A, B, K1, K2, _driver_models(M, model, driver_form, K), model, rule, px, et, device, fr)
    return _guided_matches(L, match, dist)


def check_correspond_args(match_shape, match_dtype, counts1, counts2, pairs, keep=None, kps1=None, kps2=None, models=None, model="F",
                          error_type="sampson", capacity=None):
    """The argument checks of the correspondence export (correspondences_pairs / _batch and their _tensors forms), on shapes and dtype names
    (numpy or torch).  pairs None = the ragged batch (entry p = pair p, counts1 / counts2 rows per pair), else an integer [K, 2] list over
    stores of counts1 / counts2 rows per image.  keep / kps1 / kps2 / models: None or (shape, dtype).  Returns (offsets1, offsets2, pairs
    as contiguous int32 [K, 2] or None, pair_offsets int64 [K + 1], "xy" / "kpts" / None, error_type code, capacity); raises ValueError."""
    from .api import _error_type, error_type_dict_fundamental, error_type_dict_homography
    if model not in ("F", "H"):
        raise ValueError("model should be 'F' or 'H'")
    et = _error_type(error_type_dict_fundamental if model == "F" else error_type_dict_homography, error_type)
    cs = [np.asarray(c) for c in (counts1, counts2)]
    for c in cs:
        if c.ndim != 1 or (c.size and not np.issubdtype(c.dtype, np.integer)) or (c < 0).any():
            raise ValueError("counts1 and counts2 should be 1-D arrays of integers >= 0")
    o1, o2 = (np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int64) for c in cs)
    if pairs is None:
        if len(cs[0]) != len(cs[1]):
            raise ValueError("counts1 and counts2 should have one entry per pair")
        pr = None; K = len(cs[0]); po = o1.copy()
        if po[-1] > 0x3fffffff or o2[-1] > 0x3fffffff:
            raise ValueError("too many rows in one pair list")
    else:
        pr, po = _check_pair_list(pairs, o1, o2)
        K = len(pr)
    N = int(po[-1])
    if tuple(match_shape) != (N,) or _dtype_name(match_dtype) != "int32":
        raise ValueError(f"match should be int32 [N] = [{N}], one value per output row of the list")
    if keep is not None and (tuple(keep[0]) != (N,) or _dtype_name(keep[1]) not in ("bool", "uint8")):
        raise ValueError(f"keep should be bool or uint8 [N] = [{N}]")
    if (kps1 is None) != (kps2 is None):
        raise ValueError("kps1 and kps2 go together")
    kind = None
    if kps1 is not None:
        kind = _kps_kind(kps1, kps2)
        if kps1[0][0] != o1[-1] or kps2[0][0] != o2[-1]:
            raise ValueError("counts do not add up to the number of keypoint rows")
    if models is not None:
        if kps1 is None:
            raise ValueError("models (the residuals) need kps1 and kps2")
        if tuple(models[0]) != (K, 3, 3):
            raise ValueError(f"models should be [K, 3, 3] = [{K}, 3, 3], one model per list entry")
        if _dtype_name(models[1]) != "float64":
            raise ValueError("models should be float64")
    cap = N if capacity is None else _integer(capacity, "capacity should be an integer >= 0 (or None = one position per output row)", 0)
    return o1, o2, pr, po, kind, et, cap


def correspond_layout(o1, o2, pr):
    """the layout arguments of the mi_degensac_correspondences_* entry points: (layout name, ctypes arguments, K)"""
    if pr is None:
        return "batch", (_lib.ptr(o1), _lib.ptr(o2), len(o1) - 1), len(o1) - 1
    return "pairs", (_lib.ptr(o1), len(o1) - 1, _lib.ptr(o2), len(o2) - 1, _lib.ptr(pr), len(pr)), len(pr)


def _correspondences(match, counts1, counts2, pairs, keep, kps_list, kps2_list, models, model, error_type, driver_form, store_rows, device):
    match = np.asarray(match)
    kp = None if keep is None else np.asarray(keep)
    if (kps_list is None) and (kps2_list is not None):
        raise ValueError("kps2_list names a second store: give kps_list too")
    K1 = K2 = None
    if kps_list is not None:
        text = "every image's keypoints should be 2-D with the dtype and width of image 0 (at least one image per store)"
        stores = [np.concatenate(_rows_list(kl, text)) for kl in ((kps_list,) if kps2_list is None else (kps_list, kps2_list))]
        K1, K2 = stores[0], stores[-1]
    M = None if models is None else np.asarray(models)
    o1, o2, pr, po, kind, et, cap = check_correspond_args(match.shape, match.dtype, counts1, counts2, pairs, _sd(kp), _sd(K1), _sd(K2), _sd(M), model,
                                                          error_type, None)
    name, layout, K = correspond_layout(o1, o2, pr)
    match = np.ascontiguousarray(match)
    if kp is not None:
        kp = np.ascontiguousarray(kp).view(np.uint8)
    if K1 is not None:
        same = K2 is K1
        K1 = np.ascontiguousarray(kpts_to_xyA(K1, device) if kind == "kpts" else K1, np.float64)
        K2 = K1 if same else np.ascontiguousarray(kpts_to_xyA(K2, device) if kind == "kpts" else K2, np.float64)
    Md = None if M is None else _driver_models(M, model, driver_form, K)
    co =np.zeros(K + 1, np.int64); total = np.zeros(1, np.int64)
    rows = np.full((cap, 2), -1, np.int32)
    pts = None if K1 is None else np.full((cap, 4), np.nan)
    resid = None if Md is None else np.full(cap, np.nan)
    gp = _lib.GuideParams(model == "H", et, 0.0)
    vp = _lib.vptr
    rc = getattr(_lib.lib(), f"mi_degensac_correspondences_{name}")(*layout, vp(match), vp(kp), _lib.CORR_STORE_ROWS if store_rows else 0, vp(K1),
                                                                   vp(K2), 0 if K1 is None else K1.shape[1], vp(Md), C.byref(gp), cap, int(device),
                                                                   vp(co), vp(total), vp(rows), None, vp(pts), vp(resid))
    _lib.check_match(rc)
    cut = lambda x, p: None if x is None else x[co[p]:co[p + 1]]          # noqa: E731
    return [{"rows": cut(rows, p), "pts": cut(pts, p), "resid": cut(resid, p)} for p in range(K)]


def correspondences_pairs(match, counts1, counts2, pairs, keep=None, kps_list=None, kps2_list=None, models=None, model="F", error_type="sampson",
                          driver_form=False, store_rows=False, device=0):
    """The verified matches of a pair list as one compact list per entry (include/mi_degensac.h mi_degensac_correspondences_pairs, blocking,
    numpy).  match [N] int32 is what a pair-list call returned per output row (train row local to image j, or -1), counts1 / counts2 the
    rows per image of the two stores and pairs [K, 2] the list.  What goes in as it is: `match` and `keep=inlier` of match_and_verify_pairs
    (concatenated in list order); `match` of guided_match_pairs' tensor form with keep=None; `keep = inlier_f & inlier_h` of the F+H call.
    A row is selected when 0 <= match < rows(image j) and (keep is None or keep != 0).  kps_list (one [n, 2] / [n, 6] float64 or [n, 4]
    float32 array per image; kps2_list for a second store) adds the coordinates, models [K, 3, 3] (F, or the user-facing H;
    driver_form=True: H_c = inv(H)^T) the estimator's own residual of error_type, the function the gate of guided matching uses.
    Returns a list of K dicts: rows [n_p, 2] int32 = (query row in image i, train row in image j) in query order — with store_rows=True
    (row of store 1, row of store 2) —, pts [n_p, 4] = x1, y1, x2, y2 or None, resid [n_p] or None."""
    if pairs is None:
        raise ValueError("pairs should be an integer array [K, 2] of (image of store 1, image of store 2)")
    return _correspondences(match, counts1, counts2, pairs, keep, kps_list, kps2_list, models, model, error_type, driver_form, store_rows, device)


def correspondences_batch(match, counts1, counts2, keep=None, kps1_list=None, kps2_list=None, models=None, model="F", error_type="sampson",
                          driver_form=False, store_rows=False, device=0):
    """correspondences_pairs on the ragged batch (mi_degensac_correspondences_batch): entry p is pair p with counts1[p] query and counts2[p]
    train rows, match [sum(counts1)] int32 the concatenated `match` of match_and_verify_batch / guided_match_batch, keep likewise (the
    concatenated `inlier`), kps1_list[p] / kps2_list[p] the pair's keypoints (both or none).  store_rows=True gives rows of the two
    concatenations."""
    if (kps1_list is None) != (kps2_list is None):
        raise ValueError("kps1_list and kps2_list go together")
    return _correspondences(match, counts1, counts2, None, keep, kps1_list, kps2_list, models, model, error_type, driver_form, store_rows, device)


def check_tracks_args(rows_shape, rows_dtype, counts, total=None):
    """The argument checks of tracks / tracks_tensors on a shape and a dtype name (numpy or torch).  counts: the rows per image of the ONE
    store both columns of `rows` index; total: None, or for the numpy form an integer (< 0 = all edges).  Returns (offsets int64
    [n_images + 1], R, M); raises ValueError."""
    c = np.asarray(counts)
    if c.ndim != 1 or (c.size and not np.issubdtype(c.dtype, np.integer)) or (c < 0).any():
        raise ValueError("counts should be a 1-D array of integers >= 0, the rows per image of the store")
    off = np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int64)
    if off[-1] > 0x7fffffff:
        raise ValueError("too many rows in the store (its rows must fit int32)")
    if len(rows_shape) != 2 or rows_shape[1] != 2 or _dtype_name(rows_dtype) != "int32":
        raise ValueError("rows should be int32 [M, 2] of store rows, as the correspondence export writes them with store_rows=True")
    if rows_shape[0] > 0x3fffffff:
        raise ValueError("too many edges in one list")
    if total is not None:
        _integer(total, "total should be an integer (or None = all edges)")
    return off, int(off[-1]), int(rows_shape[0])


def tracks(rows, counts, total=None, device=0):
    """Tracks = the connected components of verified matches over one image store (include/mi_degensac.h mi_degensac_tracks, blocking,
    numpy).  rows [M, 2] int32 holds store rows, as correspondences_pairs(..., store_rows=True) gives them for a collection matched
    against itself (concatenate the entries' rows); counts are the rows per image of that store; total: only the first min(total, M)
    edges count (None or < 0: all).  Ends outside the store (the -1 fill) drop their edge; self edges and repeats change nothing.
    Returns a dict: label [R] (the smallest store row of the keypoint's component), track [R] (its track, or -1), n_tracks, n_obs,
    track_offsets [n_tracks + 1], obs [n_obs] (the store rows of the members, track after track in ascending order of the tracks' smallest
    member, ascending inside), obs_image [n_obs] and track_images [n_tracks] (distinct images: a track is consistent iff it equals the
    track's length)."""
    rows = np.asarray(rows)
    off, R, M = check_tracks_args(rows.shape, rows.dtype, counts, total)
    rows = np.ascontiguousarray(rows)
    half = R // 2
    label = np.empty(R, np.int32); track = np.empty(R, np.int32); obs = np.empty(R, np.int32); oi = np.empty(R, np.int32)
    to = np.empty(half + 1, np.int64); ti = np.empty(half, np.int32); n = np.zeros(2, np.int64)
    vp = _lib.vptr
    rc = _lib.lib().mi_degensac_tracks(off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1, vp(rows) if M else None, M,
                                       -1 if total is None else int(total), int(device), vp(label), vp(track), vp(n[0:]), vp(n[1:]), vp(to), vp(obs),
                                       vp(oi), vp(ti))
    _lib.check_match(rc)
    nt, no = int(n[0]), int(n[1])
    return {"label": label, "track": track, "n_tracks": nt, "n_obs": no, "track_offsets": to[:nt + 1], "obs": obs[:no], "obs_image": oi[:no],
            "track_images": ti[:nt]}


def check_refit_args(pts_shape, pts_dtype, off_shape, off_dtype, models_shape, models_dtype, model="F", px_th=None, error_type="sampson",
                     max_fits=4):
    """The argument checks of refit_correspondences / refit_correspondences_tensors on shapes and dtype names (numpy or torch): pts float64
    [cap, 4], corr_offsets int64 [K + 1], models float64 [K, 3, 3], px_th >= 0 (None = the model's default), error_type one of the model's
    names, max_fits an integer >= 0.  Returns (K, cap, px_th, error_type code, max_fits); raises ValueError."""
    K, cap, (px, et) = _check_list_inputs(pts_shape, pts_dtype, off_shape, off_dtype,
                                          lambda K: check_guided_args(model, px_th, error_type, models_shape, models_dtype, K))
    return K, cap, px, et, _integer(max_fits, "max_fits should be an integer >= 0", 0)


def _check_list_inputs(pts_shape, pts_dtype, off_shape, off_dtype, check_models):
    """corr_offsets and pts of the calls on exported lists; check_models(K) runs between the two, where every such call checks its models.
    Returns (K, cap, what check_models returned); raises ValueError."""
    if len(off_shape) != 1 or off_shape[0] < 1 or _dtype_name(off_dtype) != "int64":
        raise ValueError("corr_offsets should be int64 [K + 1], as the correspondence export returns it")
    K = int(off_shape[0]) - 1
    got = check_models(K)
    if len(pts_shape) != 2 or pts_shape[1] != 4 or _dtype_name(pts_dtype) != "float64":
        raise ValueError("pts should be float64 [cap, 4] = x1, y1, x2, y2, as the correspondence export returns it")
    if pts_shape[0] > 0x3fffffff:
        raise ValueError("too many rows in one list")
    return K, int(pts_shape[0]), got


def refit_correspondences(pts, corr_offsets, models, model="F", px_th=None, error_type="sampson", driver_form=False, max_fits=4, with_resid=False,
                          device=0):
    """Refit F / H on exported correspondence lists (include/mi_degensac.h mi_degensac_refit_lists, blocking, numpy): per entry p the
    members of models[p] among the rows pts[corr_offsets[p] : corr_offsets[p + 1]] (resid <= th, the estimator's own residual of
    error_type and its threshold from px_th, None = the model's default), then at most max_fits rounds of the reference's non-minimal fit
    on the members followed by the members of the fit; a round that loses members is dropped, a round that keeps the set ends the entry.
    pts [cap, 4] = x1, y1, x2, y2 and corr_offsets [K + 1] are the concatenated `pts` of correspondences_pairs / _batch and their running
    lengths; models [K, 3, 3] what a verify call returned (F, or the user-facing H; driver_form=True: H_c = inv(H)^T in and out).
    Returns (models [K, 3, 3], inlier [cap] bool, info [K, 4] int32 = (members of the start model, members at the end, fits run,
    _lib.REFIT_* status)[, resid [cap] under the returned model])."""
    P = np.ascontiguousarray(np.asarray(pts)); o = np.ascontiguousarray(np.asarray(corr_offsets)); M = np.asarray(models)
    K, cap, px, et, mf = check_refit_args(P.shape, P.dtype, o.shape, o.dtype, M.shape, M.dtype, model, px_th, error_type, max_fits)
    Md = _driver_models(M, model, driver_form, K)
    out = np.zeros((K, 9)); user = np.zeros((K, 9)); inl = np.zeros(cap, np.uint8); info = np.zeros((K, 4), np.int32)
    resid = np.full(cap, np.nan) if with_resid else None
    gp = _lib.GuideParams(model == "H", et, px)
    vp = _lib.vptr
    rc = _lib.lib().mi_degensac_refit_lists(vp(P), vp(o), vp(Md), K, cap, C.byref(gp), mf, int(device), vp(out), vp(inl), vp(user), vp(info),
                                            vp(resid))
    _lib.check_match(rc)
    res = ((out if (model == "F" or driver_form) else user).reshape(K, 3, 3), inl.astype(bool), info)
    return res + (resid,) if with_resid else res


def check_pose_args(pts_shape, pts_dtype, off_shape, off_dtype, models_shape, models_dtype, cams1_shape, cams1_dtype, pairs=None, cams2=None, keep=None,
                    min_parallax_deg=1.5, model_text="one fundamental matrix per entry"):
    """The argument checks of relative_pose / relative_pose_tensors on shapes and dtype names (numpy or torch): pts float64 [cap, 4],
    corr_offsets int64 [K + 1], models float64 [K, 3, 3] (F); pairs, cams2 and keep are None or (shape, dtype): without pairs cams1 is
    float64 [K, 8] (one row of two cameras fx, fy, cx, cy per entry) and cams2 must be None; with pairs int32 / int64 [K, 2] cams1 is
    float64 [n_images, 4] and cams2 None (= cams1) or float64 [n_images_2, 4]; keep bool / uint8 [cap]; min_parallax_deg a number in
    [0, 180]; model_text is what the message about models calls them.  Returns (K, cap, rows of cams1, rows of cams2 or None, cos_min);
    raises ValueError."""
    def check_models(K):
        if tuple(models_shape) != (K, 3, 3) or _dtype_name(models_dtype) != "float64":
            raise ValueError("models should be float64 [K, 3, 3], " + model_text + " of corr_offsets")
    K, cap, _ = _check_list_inputs(pts_shape, pts_dtype, off_shape, off_dtype, check_models)
    if _dtype_name(cams1_dtype) != "float64":
        raise ValueError("cams1 should be float64")
    n2 = None
    if pairs is None:
        if tuple(cams1_shape) != (K, 8):
            raise ValueError("cams1 should be float64 [K, 8] = fx, fy, cx, cy of camera 1 and of camera 2 per entry (or give pairs)")
        if cams2 is not None:
            raise ValueError("cams2 names a second store: give pairs too")
    else:
        if tuple(pairs[0]) != (K, 2) or _dtype_name(pairs[1]) not in ("int32", "int64"):
            raise ValueError("pairs should be an integer array [K, 2] of (image of store 1, image of store 2)")
        if len(cams1_shape) != 2 or cams1_shape[1] != 4:
            raise ValueError("cams1 should be float64 [n_images, 4] = fx, fy, cx, cy per image of store 1")
        if cams2 is not None:
            if len(cams2[0]) != 2 or cams2[0][1] != 4 or _dtype_name(cams2[1]) != "float64":
                raise ValueError("cams2 should be float64 [n_images, 4] = fx, fy, cx, cy per image of store 2")
            n2 = int(cams2[0][0])
        if int(cams1_shape[0]) + (n2 or 0) > 0x7fffffff:
            raise ValueError("too many cameras")
    if keep is not None and (tuple(keep[0]) != (cap,) or _dtype_name(keep[1]) not in ("bool", "uint8")):
        raise ValueError("keep should be bool or uint8 [cap], one flag per row of pts")
    deg = _number(min_parallax_deg, "min_parallax_deg should be a number in [0, 180]", 0.0, 180.0)
    return K, cap, int(cams1_shape[0]), n2, float(np.cos(np.deg2rad(deg)))


def _cam_index(pairs, n1, n2):
    """pairs [K, 2] of a pose call as int32 rows of the camera table (store 1's n1 cameras, then store 2's when n2 is not None); an image
    outside its store becomes -1, so that an image of store 1 cannot reach into store 2's rows"""
    wide = pairs.astype(np.int64) + np.array([0, 0 if n2 is None else n1], np.int64)
    if n2 is not None:
        wide[(pairs[:, 0] < 0) | (pairs[:, 0] >= n1), 0] = -1
        wide[pairs[:, 1] < 0, 1] = -1
    return np.ascontiguousarray(np.clip(wide, -1, 0x7fffffff).astype(np.int32))


def _cameras(c1, c2, pr, K, n1, n2):
    """the camera table and the entries' rows in it for the pose calls -> (cams [n_cams, 4], cam_idx int32 [K, 2] or None = two rows per entry)"""
    if pr is None:
        return np.ascontiguousarray(c1).reshape(2 * K, 4), None
    return np.ascontiguousarray(c1 if c2 is None else np.concatenate([c1, c2])), _cam_index(pr, n1, n2)


def _pose_lists(from_h, pts, corr_offsets, models, cams1, pairs, cams2, keep, min_parallax_deg, with_points, with_candidates, device, rotation_eps=None,
                driver_form=False):
    """the numpy body of relative_pose (from_h False) and homography_pose (True: rotation_eps and driver_form, normal and t_over_d behind
    info, cand_normal between cand and cand_front)"""
    P = np.ascontiguousarray(np.asarray(pts)); o = np.ascontiguousarray(np.asarray(corr_offsets)); M = np.asarray(models)
    c1 = np.asarray(cams1); c2 = None if cams2 is None else np.asarray(cams2)
    pr = None if pairs is None else np.asarray(pairs)
    kp = None if keep is None else np.asarray(keep)
    shapes = (P.shape, P.dtype, o.shape, o.dtype, M.shape, M.dtype, c1.shape, c1.dtype, _sd(pr), _sd(c2), _sd(kp), min_parallax_deg)
    if from_h:
        K, cap, n1, n2, cos_min, eps = check_pose_h_args(*shapes, rotation_eps)
    else:
        K, cap, n1, n2, cos_min = check_pose_args(*shapes)
    M = np.ascontiguousarray(_h_user_form(M) if from_h and driver_form else M, np.float64).reshape(K, 9)
    cams, idx = _cameras(c1, c2, pr, K, n1, n2)
    if kp is not None:
        kp = np.ascontiguousarray(kp).view(np.uint8)
    pose = np.zeros((K, 12)); front = np.zeros(cap, np.uint8); info = np.zeros((K, 5), np.int32)
    plane = (np.zeros((K, 3)), np.zeros(K)) if from_h else ()         # normal, t_over_d
    pts3 = (np.full((cap, 3), np.nan), np.full((cap, 2), np.nan), np.full(cap, np.nan)) if with_points else (None,) * 3          # X, depth, cosang
    cand = np.zeros((K, 4, 12)) if with_candidates else None
    cn = (np.zeros((K, 4, 3)) if with_candidates else None,) if from_h else ()
    cf = np.zeros((K, 4), np.int32) if with_candidates else None
    vp = _lib.vptr
    entry = _lib.lib().mi_degensac_pose_h_lists if from_h else _lib.lib().mi_degensac_pose_lists
    rc = entry(vp(P), vp(o), vp(kp), vp(M), vp(cams), len(cams), vp(idx), K, cap, cos_min, *((eps,) if from_h else ()), int(device), vp(pose), vp(front),
               vp(info), *map(vp, plane), *map(vp, pts3), vp(cand), *map(vp, cn), vp(cf))
    _lib.check_match(rc)
    res = (pose[:, :9].reshape(K, 3, 3), pose[:, 9:], front.astype(bool), info) + plane
    if with_points:
        res += pts3
    return res + (cand,) + cn + (cf,) if with_candidates else res


def relative_pose(pts, corr_offsets, models, cams1, pairs=None, cams2=None, keep=None, min_parallax_deg=1.5, with_points=False, with_candidates=False,
                  device=0):
    """Relative pose and triangulation on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_lists, blocking, numpy):
    per entry p the essential matrix of models[p] (F, x2^T F x1 = 0) under the entry's two pinhole cameras, its four (R, t) candidates
    (X2 = R X1 + t, |t| = 1), and the one under which most used rows pts[corr_offsets[p] : corr_offsets[p + 1]] triangulate in front of
    both cameras (closed-form midpoint of the two rays).  cams1 [K, 8] = fx, fy, cx, cy of both cameras per entry; or, with pairs [K, 2],
    cams1 [n_images, 4] per image of store 1 and cams2 likewise for store 2 (None = cams1).  keep [cap]: only rows with keep != 0 are
    used (the refit's `inlier` as it is).  A front row is wide when the angle between its two rays is at least min_parallax_deg.
    Returns (R [K, 3, 3], t [K, 3], front [cap] bool, info [K, 5] int32 = (rows used, front rows of the chosen candidate, the largest
    front count of the other three, wide rows, _lib.POSE_* status)[, X [cap, 3] in the frame of camera 1, depth [cap, 2], cosang [cap]]
    [, cand [K, 4, 12], cand_front [K, 4]])."""
    return _pose_lists(False, pts, corr_offsets, models, cams1, pairs, cams2, keep, min_parallax_deg, with_points, with_candidates, device)


def check_pose_h_args(pts_shape, pts_dtype, off_shape, off_dtype, models_shape, models_dtype, cams1_shape, cams1_dtype, pairs=None, cams2=None,
                      keep=None, min_parallax_deg=1.5, rotation_eps=1e-3):
    """The argument checks of homography_pose / homography_pose_tensors: those of check_pose_args (models are homographies here), and
    rotation_eps a number >= 0.  Returns (K, cap, rows of cams1, rows of cams2 or None, cos_min, rotation_eps); raises ValueError."""
    res = check_pose_args(pts_shape, pts_dtype, off_shape, off_dtype, models_shape, models_dtype, cams1_shape, cams1_dtype, pairs, cams2, keep,
                          min_parallax_deg, "one homography per entry")
    return res + (_number(rotation_eps, "rotation_eps should be a number >= 0", 0.0),)


def homography_pose(pts, corr_offsets, models, cams1, pairs=None, cams2=None, keep=None, min_parallax_deg=1.5, rotation_eps=1e-3, driver_form=False,
                    with_points=False, with_candidates=False, device=0):
    """Relative pose from a homography on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_h_lists, blocking, numpy):
    the pose of a pair that two_view_config put into class 2, planar or panoramic, on which the F of relative_pose is degenerate.  pts,
    corr_offsets, cameras, pairs and keep exactly as relative_pose takes them; models [K, 3, 3] are the homographies of a verify, F + H or
    refit call in the caller's form (x2 ~ H x1), or with driver_form=True in the driver's.  Per entry G = K2^-1 H K1 is decomposed into
    its four solutions G = R + (t / d) n^T, and the one under which most used rows triangulate in front of both cameras and see the plane
    from its visible side is chosen (ties go to the first); a G whose singular values differ by no more than rotation_eps times the middle
    one is a pure rotation: status _lib.POSE_ROTATION, R = the rotation, t = 0.
    Returns (R [K, 3, 3], t [K, 3], front [cap] bool, info [K, 5] int32 = (rows used, front rows of the chosen candidate, the largest
    front count of the other three, wide rows, _lib.POSE_* status), normal [K, 3] = the unit plane normal in the frame of camera 1,
    t_over_d [K] = baseline over plane distance[, X [cap, 3], depth [cap, 2], cosang [cap]][, cand [K, 4, 12], cand_normal [K, 4, 3],
    cand_front [K, 4]]).  The meaning is relative_pose's: X2 = R X1 + t, |t| = 1."""
    return _pose_lists(True, pts, corr_offsets, models, cams1, pairs, cams2, keep, min_parallax_deg, with_points, with_candidates, device, rotation_eps,
                       driver_form)


def check_select_args(cls_shape, K_f, K_h):
    """the shape checks of select_pose / select_pose_tensors: both pose results are for the K pairs of cls"""
    if len(cls_shape) != 1 or K_f != cls_shape[0] or K_h != cls_shape[0]:
        raise ValueError("cls should be [K], one class per pair, and pose_f and pose_h the results of the two pose calls on the same K pairs")
    return int(cls_shape[0])


def select_pose(cls, pose_f, pose_h, corr_offsets=None):
    """Per pair the pose to keep: pose_h's R, t, front and info where cls [K] (two_view_config) says 2 and the status of pose_h is POSE_OK
    or POSE_ROTATION, else pose_f's.  pose_f = (R, t, front, info, ...) of relative_pose, pose_h likewise of homography_pose, both on the
    same lists.  front is chosen per row by the row's pair, which takes the lists' corr_offsets [K + 1]; without it front is None.
    Returns (R [K, 3, 3], t [K, 3], front [cap] bool or None, info [K, 5], use_h [K] bool, edge_keep [K] bool = the pairs whose R is
    valid, for average_rotations: status POSE_OK or POSE_ROTATION of the selected pose; a ROTATION pair has a valid R although its t is
    zero and refine_pose answers it with REFINE_BAD_POSE)."""
    c = np.asarray(cls); Rf, tf, ff, inf = (np.asarray(x) for x in pose_f[:4]); Rh, th, fh, inh = (np.asarray(x) for x in pose_h[:4])
    K = check_select_args(c.shape, len(inf), len(inh))
    sh = inh[:, 4]
    use_h = (c == 2) & ((sh == _lib.POSE_OK) | (sh == _lib.POSE_ROTATION))
    R = np.where(use_h[:, None, None], Rh, Rf); t = np.where(use_h[:, None], th, tf); info = np.where(use_h[:, None], inh, inf)
    front = None
    if corr_offsets is not None:
        o = np.asarray(corr_offsets)
        if o.shape != (K + 1,) or ff.shape != fh.shape:
            raise ValueError("corr_offsets should be [K + 1], the offsets of the lists both pose calls ran on")
        if K == 0 or len(ff) == 0:
            front = ff.copy()
        else:
            entry = np.minimum(np.searchsorted(o[1:], np.arange(len(ff)), side="right"), K - 1)
            front = np.where(use_h[entry], fh, ff)
    st = info[:, 4]
    return R, t, front, info, use_h, (st == _lib.POSE_OK) | (st == _lib.POSE_ROTATION)


def check_refine_args(pts_shape, pts_dtype, off_shape, off_dtype, R_shape, R_dtype, t_shape, t_dtype, cams1_shape, cams1_dtype, pairs=None, cams2=None,
                      keep=None, max_trials=20, ftol=1e-12):
    """The argument checks of refine_pose / refine_pose_tensors on shapes and dtype names (numpy or torch): R float64 [K, 3, 3] and t
    float64 [K, 3] as relative_pose returns them, max_trials an integer in 0 .. 100, ftol a number >= 0; everything else as
    check_pose_args, which is called for it.  Returns (K, cap, rows of cams1, rows of cams2 or None, max_trials, ftol); raises ValueError."""
    K = int(off_shape[0]) - 1 if len(off_shape) == 1 else -1
    if len(R_shape) != 3 or tuple(R_shape[1:]) != (3, 3) or (K >= 0 and R_shape[0] != K) or _dtype_name(R_dtype) != "float64":
        raise ValueError("R should be float64 [K, 3, 3], one rotation per entry of corr_offsets")
    if len(t_shape) != 2 or t_shape[1] != 3 or (K >= 0 and t_shape[0] != K) or _dtype_name(t_dtype) != "float64":
        raise ValueError("t should be float64 [K, 3], one baseline direction per entry of corr_offsets")
    K, cap, n1, n2, _ = check_pose_args(pts_shape, pts_dtype, off_shape, off_dtype, R_shape, R_dtype, cams1_shape, cams1_dtype, pairs, cams2, keep)
    return K, cap, n1, n2, _integer(max_trials, "max_trials should be an integer in 0 .. 100", 0, 100), _number(ftol, "ftol should be a number >= 0", 0.0)


def refine_pose(pts, corr_offsets, R, t, cams1, pairs=None, cams2=None, keep=None, max_trials=20, ftol=1e-12, with_resid=False, with_F=False,
                device=0, **unknown):
    """Refine relative poses on exported correspondence lists (include/mi_degensac.h mi_degensac_pose_refine_lists, blocking, numpy): per
    entry p a Levenberg-Marquardt run over the five degrees of freedom of (R[p], t[p] / |t[p]|) on the Sampson distance, in pixels, of the
    used rows pts[corr_offsets[p] : corr_offsets[p + 1]] under the entry's two pinhole cameras.  R, t are what relative_pose returned,
    cameras, pairs and keep as there (its `front` goes in as keep as it is).  At most max_trials trial steps per entry; an accepted step
    that lowers the cost by no more than ftol times the cost ends the run.
    Returns (R [K, 3, 3], t [K, 3], cost [K, 2] = (start, end), info [K, 4] int32 = (rows used, trials, trials accepted, _lib.REFINE_*
    status)[, resid [cap]: the signed Sampson distance of the used rows under the final pose, NaN elsewhere][, F [K, 3, 3] = K2^-T [t]x R
    K1^-1 of the final pose, x2^T F x1 = 0])."""
    if unknown:
        raise ValueError(f"refine_pose: unknown keyword {sorted(unknown)[0]!r}")
    P = np.ascontiguousarray(np.asarray(pts)); o = np.ascontiguousarray(np.asarray(corr_offsets)); Rm = np.asarray(R); tv = np.asarray(t)
    c1 = np.asarray(cams1); c2 = None if cams2 is None else np.asarray(cams2)
    pr = None if pairs is None else np.asarray(pairs)
    kp = None if keep is None else np.asarray(keep)
    K, cap, n1, n2, mt, ft = check_refine_args(P.shape, P.dtype, o.shape, o.dtype, Rm.shape, Rm.dtype, tv.shape, tv.dtype, c1.shape, c1.dtype, _sd(pr),
                                               _sd(c2), _sd(kp), max_trials, ftol)
    pose = np.ascontiguousarray(np.concatenate([Rm.reshape(K, 9), tv], 1))
    cams, idx = _cameras(c1, c2, pr, K, n1, n2)
    if kp is not None:
        kp = np.ascontiguousarray(kp).view(np.uint8)
    out = np.zeros((K, 12)); cost = np.full((K, 2), np.nan); info = np.zeros((K, 4), np.int32)
    resid = np.full(cap, np.nan) if with_resid else None
    F = np.zeros((K, 9)) if with_F else None
    vp = _lib.vptr
    rc = _lib.lib().mi_degensac_pose_refine_lists(vp(P), vp(o), vp(kp), vp(pose), vp(cams), len(cams), vp(idx), K, cap, mt, ft, int(device), vp(out),
                                                  vp(cost), vp(info), vp(resid), vp(F))
    _lib.check_match(rc)
    res = (out[:, :9].reshape(K, 3, 3), out[:, 9:], cost, info)
    if with_resid:
        res += (resid,)
    return res + (F.reshape(K, 3, 3),) if with_F else res


def check_triangulate_args(off_shape, off_dtype, obs_shape, obs_dtype, img_shape, img_dtype, kps_shape, kps_dtype, cams_shape, cams_dtype, R_shape,
                           R_dtype, t_shape, t_dtype, n_tracks=None, min_angle_deg=1.5, max_reproj_px=4.0, max_iters=10, ftol=1e-12):
    """The argument checks of triangulate_tracks / triangulate_tracks_tensors on shapes and dtype names (numpy or torch): track_offsets
    int64 [T + 1], obs and obs_image int32 [M], kps float64 [rows, >= 2], cams float64 [n_images, 4], R float64 [n_images, 3, 3], t float64
    [n_images, 3]; n_tracks None or (shape, dtype) = int64 [1]; min_angle_deg a number in [0, 180], max_reproj_px a number >= 0, max_iters
    an integer in 0 .. 100, ftol a number >= 0.  Returns (T, M, rows, n_images, min_angle_deg, max_reproj_px, max_iters, ftol); raises
    ValueError."""
    if len(off_shape) != 1 or off_shape[0] < 1 or _dtype_name(off_dtype) != "int64":
        raise ValueError("track_offsets should be int64 [T + 1], as the tracks call returns it")
    T = int(off_shape[0]) - 1
    if len(obs_shape) != 1 or _dtype_name(obs_dtype) != "int32":
        raise ValueError("obs should be int32 [M] of store rows, as the tracks call returns it")
    if tuple(img_shape) != tuple(obs_shape) or _dtype_name(img_dtype) != "int32":
        raise ValueError("obs_image should be int32 [M], one image per element of obs")
    if T > 0x3fffffff or obs_shape[0] > 0x3fffffff:
        raise ValueError("too many tracks or observations")
    if len(kps_shape) != 2 or kps_shape[1] < 2 or _dtype_name(kps_dtype) != "float64" or kps_shape[0] > 0x7fffffff:
        raise ValueError("kps should be float64 [rows, >= 2] with x, y in front, one row per row of the store")
    if len(cams_shape) != 2 or cams_shape[1] != 4 or _dtype_name(cams_dtype) != "float64" or cams_shape[0] > 0x7fffffff:
        raise ValueError("cams should be float64 [n_images, 4] = fx, fy, cx, cy per image")
    n = int(cams_shape[0])
    if tuple(R_shape) != (n, 3, 3) or _dtype_name(R_dtype) != "float64":
        raise ValueError("R should be float64 [n_images, 3, 3], one world-to-camera rotation per row of cams")
    if tuple(t_shape) != (n, 3) or _dtype_name(t_dtype) != "float64":
        raise ValueError("t should be float64 [n_images, 3], X_cam = R X + t")
    if n_tracks is not None and (tuple(n_tracks[0]) != (1,) or _dtype_name(n_tracks[1]) != "int64"):
        raise ValueError("n_tracks should be int64 [1], as the tracks call returns it (or None = all T)")
    ang = _number(min_angle_deg, "min_angle_deg should be a number in [0, 180]", 0.0, 180.0)
    px = _number(max_reproj_px, "max_reproj_px should be a number >= 0", 0.0)
    mi = _integer(max_iters, "max_iters should be an integer in 0 .. 100", 0, 100)
    return T, int(obs_shape[0]), int(kps_shape[0]), n, ang, px, mi, _number(ftol, "ftol should be a number >= 0", 0.0)


def triangulate_tracks(track_offsets, obs, obs_image, kps, cams, R, t, n_tracks=None, min_angle_deg=1.5, max_reproj_px=4.0, max_iters=10, ftol=1e-12,
                       with_obs=False, device=0, **unknown):
    """Triangulate tracks under known camera poses (include/mi_degensac.h mi_degensac_triangulate_tracks, blocking, numpy): per track k
    the N-view midpoint of its used observations obs[track_offsets[k] : track_offsets[k + 1]] (store rows, obs_image their images),
    refined by at most max_iters Gauss-Newton steps on the reprojection error in pixels.  kps [rows, >= 2] holds x, y per row of the
    store, cams [n_images, 4] = fx, fy, cx, cy, R [n_images, 3, 3] and t [n_images, 3] the world-to-camera poses X_cam = R X + t (the
    convention of synthetic.collection_cameras).  n_tracks: an integer, only the first min(n_tracks, T) tracks are triangulated (None:
    all T).  An observation with an index out of range, or with a keypoint, pose or focal length that is not finite, is skipped.
    Returns (X [T, 3] in the world frame, info [T, 5] int32 = (observations used, observations in front and within max_reproj_px at
    the final point, accepted steps, trial steps, _lib.TRI_* status), cost [T, 2] = the summed squared reprojection error at the linear
    and at the final point, cosang [T] = the smallest cosine between two rays of the track[, err [M] in px, ok [M] bool, depth [M] per
    used observation]).  TRI_NARROW (no two rays min_angle_deg apart) still has its point; TRI_DEGENERATE, TRI_SHORT and TRI_TRUNCATED
    have NaN."""
    if unknown:
        raise ValueError(f"triangulate_tracks: unknown keyword {sorted(unknown)[0]!r}")
    o = np.ascontiguousarray(np.asarray(track_offsets)); ob = np.ascontiguousarray(np.asarray(obs)); oi = np.ascontiguousarray(np.asarray(obs_image))
    kp = np.asarray(kps); cm = np.asarray(cams); Rm = np.asarray(R); tv = np.asarray(t)
    if n_tracks is not None:
        _integer(n_tracks, "n_tracks should be an integer (or None = all T)")
    T, M, rows, n, ang, px, mi, ft = check_triangulate_args(o.shape, o.dtype, ob.shape, ob.dtype, oi.shape, oi.dtype, kp.shape, kp.dtype, cm.shape, cm.dtype,
                                                            Rm.shape, Rm.dtype, tv.shape, tv.dtype, None, min_angle_deg, max_reproj_px, max_iters, ftol)
    xy = np.ascontiguousarray(kp[:, :2]); cm = np.ascontiguousarray(cm)
    poses = np.ascontiguousarray(np.concatenate([Rm.reshape(n, 9), tv], 1))
    X = np.full((T, 3), np.nan); info = np.zeros((T, 5), np.int32); cost = np.full((T, 2), np.nan); cosang = np.full(T, np.nan)
    err = np.full(M, np.nan) if with_obs else None
    ok = np.zeros(M, np.uint8) if with_obs else None
    depth = np.full(M, np.nan) if with_obs else None
    vp = lambda x: _lib.vptr(x, empty_none=True)          # noqa: E731
    rc = _lib.lib().mi_degensac_triangulate_tracks(vp(o), vp(ob), vp(oi), -1 if n_tracks is None else max(int(n_tracks), 0), vp(xy), rows, vp(cm),
                                                   vp(poses), n, T, M, ang, px, mi, ft, int(device), vp(X), vp(info), vp(cost), vp(cosang), vp(err),
                                                   vp(ok), vp(depth))
    _lib.check_match(rc)
    res = (X, info, cost, cosang)
    return res + (err, ok.astype(bool), depth) if with_obs else res


def check_camera_refine_args(off_shape, off_dtype, obs_shape, obs_dtype, img_shape, img_dtype, kps_shape, kps_dtype, cams_shape, cams_dtype, R_shape,
                             R_dtype, t_shape, t_dtype, X_shape, X_dtype, n_tracks=None, obs_keep=None, refine=None, max_trials=20, ftol=1e-12):
    """The argument checks of refine_cameras / refine_cameras_tensors on shapes and dtype names (numpy or torch): the tables, kps, cams, R,
    t and n_tracks as check_triangulate_args, which is called for them; X float64 [T, 3]; obs_keep None or (shape, dtype) = uint8 / bool
    [M]; refine None or (shape, dtype) = uint8 / bool [n_images]; max_trials an integer in 0 .. 100, ftol a number >= 0.  Returns (T, M,
    rows, n_images, max_trials, ftol); raises ValueError."""
    T, M, rows, n = check_triangulate_args(off_shape, off_dtype, obs_shape, obs_dtype, img_shape, img_dtype, kps_shape, kps_dtype, cams_shape, cams_dtype,
                                           R_shape, R_dtype, t_shape, t_dtype, n_tracks)[:4]
    if tuple(X_shape) != (T, 3) or _dtype_name(X_dtype) != "float64":
        raise ValueError("X should be float64 [T, 3], one point per track as the triangulation returns it")
    if obs_keep is not None and (tuple(obs_keep[0]) != (M,) or _dtype_name(obs_keep[1]) not in ("uint8", "bool")):
        raise ValueError("obs_keep should be uint8 or bool [M], one flag per element of obs")
    if refine is not None and (tuple(refine[0]) != (n,) or _dtype_name(refine[1]) not in ("uint8", "bool")):
        raise ValueError("refine should be uint8 or bool [n_images], one flag per row of cams")
    return T, M, rows, n, _integer(max_trials, "max_trials should be an integer in 0 .. 100", 0, 100), _number(ftol, "ftol should be a number >= 0", 0.0)


def refine_cameras(track_offsets, obs, obs_image, kps, cams, R, t, X, n_tracks=None, obs_keep=None, refine=None, max_trials=20, ftol=1e-12,
                   with_err=False, with_table=False, device=0, **unknown):
    """Refine camera poses against triangulated tracks (include/mi_degensac.h mi_degensac_camera_refine_tracks, blocking, numpy): with
    the points X [T, 3] of triangulate_tracks held fixed, per image a Levenberg-Marquardt run over the six degrees of freedom of its
    world-to-camera pose (R' = C(w) R, t' = t + tau) on the reprojection error, in pixels, of its used observations.  Tables, kps, cams,
    R, t and n_tracks as triangulate_tracks takes them.  An observation is used when its indices are in range, its keypoint and its
    track's point are finite and obs_keep [M] (None: all; triangulate_tracks' `ok` as it is) allows it.  refine [n_images] (None: all):
    an image with 0 is scored but not moved.  At most max_trials trial steps per image; an accepted step that lowers the cost by no more
    than ftol times the cost ends the run; a step that puts an observation behind the camera is rejected.
    Returns (R [n_images, 3, 3], t [n_images, 3], cost [n_images, 2] = (start, end), info [n_images, 4] int32 = (observations used,
    trials, trials accepted, _lib.CAMREF_* status)[, err [M]: the reprojection error in px of the used observations at the final pose, at
    their positions in obs, NaN elsewhere][, img_offsets [n_images + 1] int64, img_obs [M] int32: the positions into obs of every image's
    used observations, ascending inside an image, -1 behind the last])."""
    if unknown:
        raise ValueError(f"refine_cameras: unknown keyword {sorted(unknown)[0]!r}")
    o = np.ascontiguousarray(np.asarray(track_offsets)); ob = np.ascontiguousarray(np.asarray(obs)); oi = np.ascontiguousarray(np.asarray(obs_image))
    kp = np.asarray(kps); cm = np.asarray(cams); Rm = np.asarray(R); tv = np.asarray(t); Xm = np.asarray(X)
    ok = None if obs_keep is None else np.asarray(obs_keep)
    rf = None if refine is None else np.asarray(refine)
    if n_tracks is not None:
        _integer(n_tracks, "n_tracks should be an integer (or None = all T)")
    T, M, rows, n, mt, ft = check_camera_refine_args(o.shape, o.dtype, ob.shape, ob.dtype, oi.shape, oi.dtype, kp.shape, kp.dtype, cm.shape, cm.dtype,
                                                     Rm.shape, Rm.dtype, tv.shape, tv.dtype, Xm.shape, Xm.dtype, None, _sd(ok), _sd(rf), max_trials, ftol)
    xy = np.ascontiguousarray(kp[:, :2]); cm = np.ascontiguousarray(cm); Xm = np.ascontiguousarray(Xm)
    poses = np.ascontiguousarray(np.concatenate([Rm.reshape(n, 9), tv], 1))
    ok = None if ok is None else np.ascontiguousarray(ok).view(np.uint8)
    rf = None if rf is None else np.ascontiguousarray(rf).view(np.uint8)
    out = np.zeros((n, 12)); cost = np.full((n, 2), np.nan); info = np.zeros((n, 4), np.int32)
    err = np.full(M, np.nan) if with_err else None
    io = np.zeros(n + 1, np.int64) if with_table else None
    iobs = np.full(M, -1, np.int32) if with_table else None
    vp = lambda x: _lib.vptr(x, empty_none=True)          # noqa: E731
    rc = _lib.lib().mi_degensac_camera_refine_tracks(vp(o), vp(ob), vp(oi), -1 if n_tracks is None else max(int(n_tracks), 0), vp(xy), rows, vp(cm),
                                                     vp(poses), n, vp(Xm), vp(ok), vp(rf), T, M, mt, ft, int(device), vp(out), vp(cost), vp(info), vp(err),
                                                     vp(io), vp(iobs))
    _lib.check_match(rc)
    res = (out[:, :9].reshape(n, 3, 3), out[:, 9:], cost, info)
    if with_err:
        res += (err,)
    return res + (io, iobs) if with_table else res


def check_rotavg_args(pairs_shape, pairs_dtype, R_shape, R_dtype, n_images, weight=None, edge_keep=None, R0=None, known=None, root=0, sweeps=200,
                      damping=0.5, robust_deg=5.0, tol=1e-9):
    """The argument checks of average_rotations / average_rotations_tensors on shapes and dtype names (numpy or torch): pairs int32 or
    int64 [K, 2] over ONE store of n_images images, R_rel float64 [K, 3, 3]; weight None or (shape, dtype) = float64 [K]; edge_keep None
    or uint8 / bool [K]; R0 float64 [n_images, 3, 3] and known uint8 / bool [n_images], both or neither; n_images an integer in 1 ..
    2^24, root in 0 .. n_images - 1, sweeps in 0 .. 4096, damping a number in (0, 1], robust_deg None or a number in (0, 180), tol a
    number >= 0.  Returns (K, n_images, root, sweeps, damping, robust_deg as the library takes it (0 = none), tol); raises ValueError."""
    n = _integer(n_images, "n_images should be an integer in 1 .. 2^24", 1, 1 << 24)
    if len(pairs_shape) != 2 or pairs_shape[1] != 2 or _dtype_name(pairs_dtype) not in ("int32", "int64") or pairs_shape[0] > 0x3fffffff:
        raise ValueError("pairs should be int32 or int64 [K, 2]: both columns are images of one store (a two-store list has no global frame)")
    K = int(pairs_shape[0])
    if tuple(R_shape) != (K, 3, 3) or _dtype_name(R_dtype) != "float64":
        raise ValueError("R_rel should be float64 [K, 3, 3], X_j = R_rel X_i per row of pairs, as the pose calls return R")
    if weight is not None and (tuple(weight[0]) != (K,) or _dtype_name(weight[1]) != "float64"):
        raise ValueError("weight should be float64 [K], one per row of pairs")
    if edge_keep is not None and (tuple(edge_keep[0]) != (K,) or _dtype_name(edge_keep[1]) not in ("uint8", "bool")):
        raise ValueError("edge_keep should be uint8 or bool [K], one flag per row of pairs")
    if (R0 is None) != (known is None):
        raise ValueError("R0 and known go together: both or neither")
    if R0 is not None and (tuple(R0[0]) != (n, 3, 3) or _dtype_name(R0[1]) != "float64"):
        raise ValueError("R0 should be float64 [n_images, 3, 3]")
    if known is not None and (tuple(known[0]) != (n,) or _dtype_name(known[1]) not in ("uint8", "bool")):
        raise ValueError("known should be uint8 or bool [n_images]")
    rt = _integer(root, "root should be an integer in 0 .. n_images - 1", 0, n - 1)
    sw = _integer(sweeps, "sweeps should be an integer in 0 .. 4096", 0, 4096)
    dm = _number(damping, "damping should be a number in (0, 1]", 0.0, 1.0)
    if dm == 0.0:
        raise ValueError("damping should be a number in (0, 1]")
    rb = 0.0
    if robust_deg is not None:
        rb = _number(robust_deg, "robust_deg should be None or a number in (0, 180)", 0.0, 180.0)
        if rb in (0.0, 180.0):
            raise ValueError("robust_deg should be None or a number in (0, 180)")
    return K, n, rt, sw, dm, rb, _number(tol, "tol should be a number >= 0", 0.0)


def average_rotations(pairs, R_rel, n_images, weight=None, edge_keep=None, R0=None, known=None, root=0, sweeps=200, damping=0.5, robust_deg=5.0,
                      tol=1e-9, with_edges=False, device=0, **unknown):
    """Rotation averaging (include/mi_degensac.h mi_degensac_rotation_average, blocking, numpy): one world-to-camera rotation per image
    from the relative rotations of a pair list.  pairs [K, 2] (int32 or int64, both columns images of one store of n_images images) and
    R_rel [K, 3, 3] float64 as relative_pose / refine_pose return R for that list: X_j = R_rel X_i with i, j = pairs[k].  weight [K]
    float64 (None: 1; e.g. the pose call's info[:, 3]) and edge_keep [K] bool / uint8 (None: all; e.g. info[:, 4] == POSE_OK).  An edge
    with an end out of range, i == j, a weight that is not > 0 and finite, or an R_rel whose squared elements do not add up to 3 within
    1e-6 (the zeros of a failed pose entry) is unused.  The gauge: camera `root` is held at the identity, or the cameras with known [n]
    != 0 are held at R0 [n, 3, 3] (registering new images against an existing reconstruction).  Cameras are first set breadth-first over
    their heaviest edge, one level per sweep, then every camera that is not held moves by `damping` times the weighted mean of its
    edges' residual rotation vectors (Cayley vectors, |w| = tan(angle / 2)); with robust_deg an edge's weight is multiplied by
    (s^2 / (s^2 + |w|^2))^2, s = tan(robust_deg / 2).  At most `sweeps` Jacobi sweeps; one that sets no camera and gives no camera a
    squared mean above tol^2 is the last.
    Returns (R [n, 3, 3], zeros where a camera was never set; info [n, 4] int32 = (half-edges used, the sweep in which the camera was
    set: 0 held, -1 never, opposed edges in the last sweep, _lib.ROTAVG_KNOWN / OK / UNREACHED / ISOLATED); step [n]: the squared norm of
    the camera's last mean vector, NaN where none was formed; summary [4] int64 = (sweeps that changed something, cameras set, edges
    used, _lib.ROTAVG_CONVERGED / MAX_SWEEPS / NO_ROOT)[, edge_cos [K]: the cosine of the angle between R_rel and R_j R_i^T at the end,
    NaN for an edge that is unused or has an end that was never set])."""
    if unknown:
        raise ValueError(f"average_rotations: unknown keyword {sorted(unknown)[0]!r}")
    pr = np.asarray(pairs); Rr = np.asarray(R_rel)
    w = None if weight is None else np.asarray(weight)
    kp = None if edge_keep is None else np.asarray(edge_keep)
    r0 = None if R0 is None else np.asarray(R0)
    kn = None if known is None else np.asarray(known)
    K, n, rt, sw, dm, rb, tl = check_rotavg_args(pr.shape, pr.dtype, Rr.shape, Rr.dtype, n_images, _sd(w), _sd(kp), _sd(r0), _sd(kn), root, sweeps, damping,
                                                 robust_deg, tol)
    pr = np.ascontiguousarray(np.clip(pr, -1, 0x7fffffff).astype(np.int32)); Rr = np.ascontiguousarray(Rr)
    w = None if w is None else np.ascontiguousarray(w)
    kp = None if kp is None else np.ascontiguousarray(kp).view(np.uint8)
    r0 = None if r0 is None else np.ascontiguousarray(r0)
    kn = None if kn is None else np.ascontiguousarray(kn).view(np.uint8)
    R = np.zeros((n, 3, 3)); info = np.zeros((n, 4), np.int32); step = np.full(n, np.nan); summary = np.zeros(4, np.int64)
    cosv = np.full(K, np.nan) if with_edges else None
    vp = _lib.vptr
    ve = lambda x: _lib.vptr(x, empty_none=True)          # noqa: E731
    rc = _lib.lib().mi_degensac_rotation_average(ve(pr), ve(Rr), ve(w), ve(kp), K, n, vp(r0), vp(kn), rt, sw, dm, rb, tl, int(device), vp(R), vp(info),
                                                 vp(step), vp(summary), ve(cosv))
    _lib.check_match(rc)
    res = (R, info, step, summary)
    return res + (cosv,) if with_edges else res


def pose_config(info, min_front_ratio=0.5, min_wide_ratio=0.0):
    """What the info rows [K, 5] of relative_pose / relative_pose_tensors (numpy, or a tensor, which is copied to the host) say about a
    pair that two_view_config put into class 2, "planar or panoramic": int8 [K] with 2 = panoramic (wide <= min_wide_ratio * front,
    compared in float64: no row, or too few, with parallax, so the pose's baseline is not supported), 1 = planar with a supported pose
    (not panoramic, and front >= min_front_ratio * used), 0 = undecided (a status other than _lib.POSE_OK, or front < min_front_ratio *
    used).  COLMAP tells the two apart after its pose decomposition by the triangulation angles; the thresholds are the caller's business
    (the defaults: any wide row is parallax, half of the used rows in front), and so is what to do with each class."""
    s = info.detach().cpu().numpy() if hasattr(info, "detach") else np.asarray(info)
    if s.ndim != 2 or s.shape[1] != 5 or (s.size and not np.issubdtype(s.dtype, np.integer)):
        raise ValueError("info should be an integer array [K, 5] = (used, front, runner-up, wide, status)")
    used = s[:, 0].astype(np.float64); front = s[:, 1].astype(np.float64); wide = s[:, 3].astype(np.float64)
    out = np.ones(s.shape[0], np.int8)
    out[front < float(min_front_ratio) * used] = 0
    out[wide <= float(min_wide_ratio) * front] = 2
    out[s[:, 4] != _lib.POSE_OK] = 0
    return out
