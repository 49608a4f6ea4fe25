"""TEST INFRASTRUCTURE ONLY: the scenes of tests/test_h2el_edges_cpu.py and tests/test_gpu_h2el_edges.py (ransacH2el, dg_kernel_h2el.h) and
the comparison with the CPU restatement (oracle/port.py ransacH2el).  No GPU here.  Every scene comes from fixed seeds through
pydegensac_amd.synthetic.ellipse_pairs; the restatement's results are computed once per process and shared.

th, conf and max_iters are per call (mi_degensac_h2el_params), so the pairs of one batch share them.  A pair that "never gets a model"
can therefore not have a sample budget or a threshold of its own: here it is a scene whose every row follows one homography of scale
0.1, exactly.  Every sample's model then has |det(h) / h8^3| = 0.01 < 0.1 and is turned down before it is scored (ranH2el.c's
determinant test), the model of the run after the loop is turned down by the same test, and nothing ever becomes the best model."""
import numpy as np

from pydegensac_amd import synthetic as syn
from tests import estimator_shapes as es
from tests import golden_util as gu

TAU = 18.0 * 18.0 / 7.0 / 7.0                        # ranH2el.h:31
CALL = dict(th=4.0, conf=0.99, max_iters=300)        # every batch of the two files
REUSE_SETTINGS = ((True, 0), (True, 8), (False, 0))   # (do_lo, inl_limit), per call
ROW_NS = es.E + (2, 3, 4095, 4096, 4097)
ROW_RATIOS = (0.4, 0.08)
ROW_LIMITS = (0, 16)
DEV_NS = (60, 2, 513, 2049, 9, 257)                  # the ragged batch of the device-entry tests
LONG_N = 2500
MI355X_CUS = 256                                      # what the CPU file builds the reuse batch for

_H_SMALL = np.array([[0.1, 0.002, 30.0], [-0.001, 0.1, 20.0], [1e-6, 2e-6, 1.0]])


def hds(H_raw, u10):
    """Htools.c:161-200 HDs in float64 numpy: the squared transfer error of every row under the raw model (9 doubles as returned)."""
    h = np.asarray(H_raw, np.float64).ravel(); u = np.asarray(u10, np.float64)
    x1, y1, x2, y2 = u[:, 0], u[:, 1], u[:, 5], u[:, 6]
    s = (x2, y2, np.ones_like(x2))
    r1 = sum(h[3 * j] * s[j] - h[3 * j + 2] * x1 * s[j] for j in range(3))
    r2 = sum(h[3 * j + 1] * s[j] - h[3 * j + 2] * y1 * s[j] for j in range(3))
    a = h[0] - h[2] * x1; b = h[3] - h[5] * x1; c = -h[8] - h[2] * x2 - h[5] * y2; d = h[1] - h[2] * y1; e = h[4] - h[5] * y1
    c2d2 = c * c + d * d
    pJ = [-b * d * e + a * (c * c + e * e), b * c2d2 - a * d * e, c * (c2d2 + e * e), -c * (a * d + b * e),
          d * (b * b + c * c) - a * b * e, -a * b * d + e * (a * a + c * c), None, c * (a * a + b * b + c * c)]
    pJ[6] = pJ[3]
    N = a * pJ[0] + b * pJ[1] + c * pJ[2]
    with np.errstate(all="ignore"):
        return sum(((pJ[j] / N) * r1 + (pJ[j + 4] / N) * r2) ** 2 for j in range(4))


def mask_from_model(H_raw, u10, th, rtol=1e-9):
    """(residual <= th, rows whose residual lies within rtol * th of th): what the driver's last loop must have written, and the rows
    on which float64 numpy and the device may differ in the last bit"""
    r = hds(H_raw, u10)
    return r <= th, np.abs(r - th) <= rtol * th


# ---- the restatement, once per process ----------------------------------------------------------------------------------------------
_cache = {}


def oracle(port, key, u10, seed, do_lo, inl_limit, th=None):
    k = (key, seed, bool(do_lo), int(inl_limit), th)
    if k not in _cache:
        _cache[k] = port.ransacH2el(u10, CALL["th"] if th is None else th, CALL["conf"], CALL["max_iters"], do_lo, inl_limit, seed)
    return _cache[k]


def e4_never_written(port, key, u10, seed):
    """no sample of the whole budget has a row within th * TAU: errs[4] is still the buffer as allocated at the run after the loop
    (ranH2el.c:163-171).  Without local optimisation and with th * TAU as the threshold the driver's best score is that of the first
    such sample, and until one comes the budget cannot shrink, so I == 0 there says exactly this."""
    return oracle(port, key, u10, seed, False, 0, th=CALL["th"] * TAU)[2]["I"] == 0


def agrees(got, want):
    """(H [3, 3] raw, mask, stats words) of the device against the restatement's (H, mask, stats): counters equal, mask byte for byte,
    model to 1e-6 (tests/test_gpu_h2el.py)"""
    H, m, st = got; Ho, mo, so = want
    if (int(st[0]), int(st[1]), int(st[3]), int(st[4])) != (so["samples"], so["lo_runs"], so["I"], so["models"]):
        return False
    return bool(np.array_equal(np.asarray(m).astype(bool), mo)) and bool(gu.rel(H, Ho) < 1e-6)


# ---- 1: more pairs than workgroups ---------------------------------------------------------------------------------------------------
_SPECIAL = tuple("abdab" * 4)                          # 8 of kind a, 8 of kind b, 4 of kind d, spread over the batch


def small_scale_scene(n, seed):
    return syn.ellipse_pairs(n, 1.0, 0.0, seed, 0.0, H=_H_SMALL)[0]


def reuse_batch(cus):
    """P = 2 cus + 3 pairs: (U, seeds, kinds).  kinds[i]: 'L' = 2500 rows (every seventh pair), 'a' = 5 ... 7 rows that never get a model,
    'b' = 9 ... 60 rows that never get a model and whose run after the loop starts from the unwritten errs[4] with every row on its list,
    'd' = 2 or 3 rows, 'c' = an ordinary pair of 9 ... 60 rows."""
    P = 2 * cus + 3
    assert P >= 64, "the batch needs room for its 20 special pairs between the long ones"
    kinds = ["L" if i % 7 == 3 else "c" for i in range(P)]
    for k, kind in enumerate(_SPECIAL):
        i = int((k + 0.5) * P / len(_SPECIAL))
        i += kinds[i] == "L"                           # right behind a long pair in the ticket order
        assert kinds[i] == "c"
        kinds[i] = kind
    U, seeds, n_d = [], [], 0
    for i, kind in enumerate(kinds):
        if kind == "L":
            u = syn.ellipse_pairs(LONG_N, (0.4, 0.25, 0.6)[i % 3], 1.0, 21000 + i)[0]
        elif kind == "a":
            u = small_scale_scene(5 + i % 3, 22000 + i)
        elif kind == "b":
            u = small_scale_scene(9 + (i * 37) % 52, 23000 + i)
        elif kind == "d":
            u = syn.ellipse_pairs(2 + n_d % 2, 1.0, 0.5, 24000 + i)[0]; n_d += 1
        else:
            u = syn.ellipse_pairs(9 + (i * 37) % 52, (0.5, 0.7, 0.9, 1.0, 0.35)[i % 5], 0.7, 25000 + i)[0]
        U.append(u); seeds.append(7 + 3 * i)
    assert sorted(len(U[i]) for i, k in enumerate(kinds) if k == "d") == [2, 2, 3, 3]
    return U, seeds, kinds


def reuse_sample(kinds, count=24):
    """the pairs that are also run alone: the first, the last, every pair of kinds a, b and d, and the rest evenly spaced"""
    P = len(kinds)
    ids = {0, P - 1} | {i for i, k in enumerate(kinds) if k in "abd"}
    for i in np.linspace(0, P - 1, 4 * count).astype(int):
        if len(ids) >= count:
            break
        ids.add(int(i))
    assert len(ids) == count
    return sorted(ids)


def never_a_model(res):
    H, m, _ = res
    return not np.asarray(H).any() and bool(np.asarray(m).all())


# ---- 2: row counts -------------------------------------------------------------------------------------------------------------------
def row_scene(n, j):
    """scene j (0: about 40 % inliers, 1: about 8 %) of row count n: (u10, seed)"""
    return syn.ellipse_pairs(n, ROW_RATIOS[j], 1.0, 31000 + 2 * n + j)[0], 101 + 2 * n + j


def row_batch(descending=False):
    """every row count, both scenes, in one ragged batch: (U, seeds, [(n, j)])"""
    keys = [(n, j) for n in sorted(ROW_NS, reverse=descending) for j in (0, 1)]
    sc = [row_scene(n, j) for n, j in keys]
    return [s[0] for s in sc], [s[1] for s in sc], keys


def dev_batch():
    sc = [row_scene(n, 0) for n in DEV_NS]
    return [s[0] for s in sc], [s[1] for s in sc]


# ---- 4: the fit limit ----------------------------------------------------------------------------------------------------------------
LIMIT_N, LIMIT_L, LIMIT_SEED, LIMIT_TH = 60, 30, 9, 16.0


def limit_scene():
    """60 rows: 30 inliers with 0.6 px of noise and 30 outliers at least 100 px from where the homography puts them; with th = 16 (and
    4 * th * TAU = 20 px squared for the widest list) every list of the local optimisation under a model near the true one holds the 30
    inliers and nothing else"""
    u, lab = syn.ellipse_pairs(LIMIT_N, LIMIT_L / LIMIT_N, 0.6, 41000, 0.02)
    q = np.c_[u[:, 5:7], np.ones(len(u))] @ syn.H_1_6.T
    x1 = q[:, :2] / q[:, 2:]
    near = ~lab & (np.hypot(*(u[:, :2] - x1).T) < 100.0)
    u[near, 0] = x1[near, 0] + 150.0
    assert int(lab.sum()) == LIMIT_L
    return np.ascontiguousarray(u), lab


# ---- 5: degenerate samples -----------------------------------------------------------------------------------------------------------
DUP_SEED = 17


def duplicate_scene():
    """40 rows, 10 of them exact duplicates of other rows"""
    u = syn.ellipse_pairs(30, 0.3, 0.5, 51000)[0]
    u = np.concatenate([u, u[3:13]])
    return np.ascontiguousarray(u[np.random.default_rng(51001).permutation(40)])
