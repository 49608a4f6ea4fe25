"""numpy restatement of mi_degensac_desc_quantize (include/mi_degensac.h): float32 descriptors -> the uint8 rows of norm "l2_u8".

Everything is float64 with one IEEE operation per step (numpy's + * / sqrt rint are correctly rounded and numpy contracts nothing into
an FMA), and the row sum follows the header's order: 64 lanes, lane i owns columns 4 i .. 4 i + 3 and adds its terms below dim in
ascending order starting from +0.0, then for m = 32, 16, 8, 4, 2, 1 every lane adds the value of lane i ^ m.

The `variant` argument builds the deliberately wrong restatements that tests/test_quantize_cpu.py must tell from this one."""
import numpy as np

NONE, L2, L1ROOT = 0, 1, 2
PRESETS = {"sift": (L2, 512.0, 0), "rootsift": (L1ROOT, 512.0, 0), "unit": (L2, 256.0, 128)}
_LANE = np.arange(64)


def row_sums(terms):
    """terms float64 [n, dim] (x^2 or |x|), dim <= 256 -> s [n] in the documented order"""
    n, dim = terms.shape
    t = np.zeros((n, 256)); t[:, :dim] = terms
    t = t.reshape(n, 64, 4)
    s = np.zeros((n, 64))
    for j in range(4):                          # a column past dim adds +0.0 to a sum >= +0.0: the same bits as leaving it out
        s = s + t[:, :, j]
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, _LANE ^ m]
    assert (s == s[:, :1]).all() or np.isnan(s).any()
    return s[:, 0]


def quantize(desc, normalize, scale, offset, variant=None):
    """-> (q uint8 [n, out_dim] with out_dim = (dim + 3) & ~3, clipped int32 [n]).  variant: None, or one of "half_up", "truncate",
    "no_clamp", "l2_for_l1", "nan_to_zero" (wrong on purpose)."""
    x32 = np.asarray(desc)
    assert x32.dtype == np.float32 and x32.ndim == 2 and 1 <= x32.shape[1] <= 256
    n, dim = x32.shape
    x = x32.astype(np.float64)
    scale = float(scale); offset = int(offset)
    with np.errstate(all="ignore"):
        if normalize == NONE:
            s = np.ones(n); y = x
        elif normalize == L2:
            s = row_sums(x * x)
            y = x / np.sqrt(s)[:, None]
        else:
            s = row_sums(np.abs(x))
            if variant == "l2_for_l1":
                s = np.sqrt(row_sums(x * x))
            y = np.copysign(np.sqrt(np.abs(x) / s[:, None]), x)
        p = scale * y
        if variant == "half_up":
            r = np.floor(p + 0.5)
        elif variant == "truncate":
            r = np.trunc(p)
        else:
            r = np.rint(p)
        v = r + float(offset)
        dead = ~np.isfinite(x).all(axis=1) | ((normalize != NONE) & (s == 0))
        clipped = ((v < 0) | (v > 255)).sum(axis=1).astype(np.int32)
        if variant == "no_clamp":
            c = np.where(np.isnan(v), 0.0, np.mod(np.where(np.isfinite(v), v, 0.0), 256.0))         # the low byte of the integer
        else:
            c = np.where(v < 0, 0.0, np.where(v > 255, 255.0, v))
        c[dead] = 0.0 if variant == "nan_to_zero" else float(offset)
        clipped[dead] = -1
    q = np.zeros((n, (dim + 3) & ~3), np.uint8)
    q[:, :dim] = c.astype(np.uint8)
    return q, clipped


def preset(desc, name):
    return quantize(desc, *PRESETS[name])


# ---- inputs shared by the CPU and the GPU tests ----
def sift_like(n, dim, seed):
    """integer-valued rows with values 0 .. 255 as float32, no all-zero row: every sum of squares and of magnitudes is an exact
    integer below 2^53 in any order"""
    rng = np.random.default_rng(seed)
    a = np.minimum(255, rng.gamma(0.6, 40.0, (n, dim))).astype(np.int64)
    if n:
        a[:, 0] = np.maximum(a[:, 0], 1)
    return a.astype(np.float32)


def float_rows(n, dim, seed, signed=True):
    """random float32 rows over a few orders of magnitude, signed or not"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, dim)) * np.exp(rng.uniform(-3, 3, (n, 1)))
    return (a if signed else np.abs(a)).astype(np.float32)


def plain_rootsift(x):
    """the RootSIFT bytes as one writes them in numpy: exact sums on integer-valued rows"""
    x = np.asarray(x, np.float64)
    return np.minimum(255, np.rint(512 * np.sqrt(x / x.sum(1, keepdims=True))))


def plain_l2(x):
    x = np.asarray(x, np.float64)
    return np.minimum(255, np.rint(512 * (x / np.sqrt((x * x).sum(1, keepdims=True)))))
