"""TEST INFRASTRUCTURE ONLY: what tests/test_gpu_estimator_dev_entry.py and tests/test_estimator_dev_entry_cpu.py share.  No GPU here.

The scenes of the F / H device-entry tests (row counts of tests/estimator_shapes.py at the edges of a wave, of the 256-point wave tile and
of one pass step, pairs without a model), the store a call reads (pairs at absolute rows of a larger
store, unowned rows NaN), output buffers with guard elements and sentinels, the check that a call wrote nothing outside what it owns,
the comparison of one pair with the CPU restatement, and the table of calls that the entry must refuse before it launches anything.

A scene is a dict: kind, p1, p2 ([n, 2] or [n, 6]), seed, key (of the restatement's cache), laf_coef, max_iters (None = the kind's
F_CALL / H_CALL).  The pairs of one batch share laf_coef and max_iters, as one launch shares its parameters."""
import numpy as np

from pydegensac_amd import _lib
from pydegensac_amd import synthetic as syn
from tests import estimator_shapes as es
from tests import golden_util as gu
from tests import small_sets as ss

G = 8                                                                     # guard pairs (model, stats) / guard bytes (mask) on each side
FILL = dict(model=-7.0, mask=7, stats=-5)
PER = dict(model=9, mask=1, stats=16)
DTYPE = dict(model=np.float64, mask=np.uint8, stats=np.int32)
MIN_ROWS = {"F": 8, "H": 4}
CALL = {"F": es.F_CALL, "H": es.H_CALL}
KEYS = {"F": es.F_KEYS, "H": es.H_KEYS}
MODEL_TOL = 1e-6                                                          # relative Frobenius (tests/golden_util.rel): the parity tolerance
# the values of estimator_shapes.E up to one pass step + 1 (no 9 there); 4 and 5 rows for H from tests/small_sets.py
ROWS = {"F": (8, 63, 64, 65, 255, 256, 257, 513), "H": (4, 5, 8, 63, 64, 65, 255, 256, 257, 513)}
LAF_N = 257
FIRST_ROWS = (5, 12)
TAIL_ROWS = 9
TENSOR_SEEDS = (0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)
# the all-outlier cases of tests/test_gpu_parity_f.py / _h.py: (n, data seed, max_iters of that test, the two seeds of that test)
OUTLIERS = {"F": (300, 3, 3000, (1, 7)), "H": (200, 2, 2000, (1, 7))}


def _scene(kind, p1, p2, seed, key, laf_coef=0.0, max_iters=None):
    return dict(kind=kind, p1=np.ascontiguousarray(p1, dtype=np.float64), p2=np.ascontiguousarray(p2, dtype=np.float64), seed=int(seed), key=key,
                laf_coef=float(laf_coef), max_iters=max_iters)


def row_scene(kind, n, laf=False, max_iters=None):
    """the scene of n rows: estimator_shapes' own (its restatement result is shared with test_gpu_estimator_shapes.py), or for H on 4 / 5
    rows the noise-free pair of tests/small_sets.py"""
    if kind == "H" and n < 8:
        p1, p2 = ss.h_points("clean", n, False, seed=4100 + n)
        return _scene(kind, p1, p2, 57 + n, ("dev-small", n, max_iters), max_iters=max_iters)
    if kind == "F" and n == 8:
        # estimator_shapes' 8-row scene has 7 inliers (ratio 0.9) and these tests ask for 8: the same generator and data seed with every
        # row an inlier (tests/test_estimator_dev_entry_cpu.py asserts I = 8)
        p1, p2, _, _ = syn.two_view_fundamental(8, 1.0, 0.1, seed=3100 + n)
        return _scene(kind, p1, p2, 41 + n, ("dev-small", n, max_iters), max_iters=max_iters)
    p1, p2, seed = (es.f_scene if kind == "F" else es.h_scene)(n, laf)
    key = ("E", n, laf) if max_iters is None else ("dev-E", n, laf, max_iters)
    return _scene(kind, p1, p2, seed, key, es.LAF_COEF[kind] if laf else 0.0, max_iters)


def no_model_scene(kind, j, max_iters="parity"):
    """a pair on which the drivers find no model, under the j-th seed of the all-outlier case of tests/test_gpu_parity_*.py.  That case
    itself (n = 300 / 200, inlier ratio 0) always has a model in the restatement: seven or four arbitrary rows fit one, and it keeps
    9 ... 11 / 4 ... 5 inliers under every data seed and seed tried.  So image 2 of the same scene is collapsed to its first point, the
    input of tests/test_gpu_decide_calls.py's pair without a model: no sample yields a model that can be scored (F) or every sample is
    turned down before scoring (H).  max_iters: the parity case's budget, or None for the kind's F_CALL / H_CALL"""
    n, data_seed, budget, seeds = OUTLIERS[kind]
    if kind == "F":
        p1, p2, _, _ = syn.two_view_fundamental(n, 0.0, 0.5, seed=data_seed)
    else:
        p1, p2, _, _ = syn.homography_pairs(n=n, inlier_ratio=0.0, sigma=0.5, seed=data_seed)
    p2 = np.repeat(p2[:1], n, axis=0)
    mi = budget if max_iters == "parity" else max_iters
    if mi == CALL[kind]["max_iters"]:
        mi = None
    return _scene(kind, p1, p2, seeds[j], ("dev-none", j, mi), max_iters=mi)


def ragged_batch(kind):
    """every row count in one ragged batch"""
    return [row_scene(kind, n) for n in ROWS[kind]]


def laf_batch(kind):
    """one pair of [n, 6] rows with the LAF check: another row stride"""
    return [row_scene(kind, LAF_N, laf=True)]


def mixed_batch(kind):
    """[found, no model, found, no model] under the budget of the parity tests' all-outlier case"""
    mi = no_model_scene(kind, 0)["max_iters"]
    return [row_scene(kind, 257, max_iters=mi), no_model_scene(kind, 0), row_scene(kind, 65, max_iters=mi), no_model_scene(kind, 1)]


def reuse_batches(kind):
    """a 9-pair batch, then 3 pairs for the same buffers: a pair without a model lands on the bytes of pairs that had one"""
    first = [row_scene(kind, n) for n in ROWS[kind][-8:]] + [no_model_scene(kind, 0, None)]
    return first, [no_model_scene(kind, 1, None), row_scene(kind, 8), row_scene(kind, 65)]


def reseeded(scenes, seeds):
    """the same pairs under other seeds (the tensor form's marshalling of seeds at and above 2^31)"""
    return [dict(sc, seed=int(s), key=("dev-seed", sc["key"], int(s))) for sc, s in zip(scenes, seeds)]


def tensor_batches(kind):
    """the mixed batch and the LAF batch under TENSOR_SEEDS, cycled over their five pairs"""
    return reseeded(mixed_batch(kind), TENSOR_SEEDS[:4]), reseeded(laf_batch(kind), TENSOR_SEEDS[4:])


def all_batches(kind):
    """name -> batch: every scene the GPU file runs (tests/test_estimator_dev_entry_cpu.py walks this)"""
    first, second = reuse_batches(kind)
    t_mixed, t_laf = tensor_batches(kind)
    return dict(ragged=ragged_batch(kind), laf=laf_batch(kind), mixed=mixed_batch(kind), reuse_first=first, reuse_second=second,
                tensor_mixed=t_mixed, tensor_laf=t_laf)


def is_no_model_scene(sc):
    return sc["key"][0] == "dev-none" or (sc["key"][0] == "dev-seed" and sc["key"][1][0] == "dev-none")


def call_params(scenes):
    """(px_th, conf, max_iters, laf_coef) of the launch that runs these pairs"""
    kind = scenes[0]["kind"]
    assert len({(s["kind"], s["laf_coef"], s["max_iters"], s["p1"].shape[1]) for s in scenes}) == 1, "the pairs of a batch share the launch's parameters"
    c = CALL[kind]
    return c["px_th"], c["conf"], c["max_iters"] if scenes[0]["max_iters"] is None else scenes[0]["max_iters"], scenes[0]["laf_coef"]


def oracle(port, sc):
    """the CPU restatement on the scene, once per process: (model [3, 3], mask, stats dict)"""
    if sc["key"][0] == "E":
        return es.oracle_e(port, sc["kind"], sc["key"][1], sc["key"][2])
    f = es.oracle_f if sc["kind"] == "F" else es.oracle_h
    return f(port, sc["key"], sc["p1"], sc["p2"], sc["seed"], laf_coef=sc["laf_coef"], max_iters=sc["max_iters"])


# ---- the store and the guarded outputs -------------------------------------------------------------------------------------------------
def build_store(scenes, first_row=0, tail=0):
    """the pairs at rows first_row ... of one store with `tail` rows behind them: dict(pts1, pts2 [rows, dim] with NaN in every unowned
    row, off [P + 1] int64 ABSOLUTE rows, seeds [P] uint32, rows)"""
    dim = scenes[0]["p1"].shape[1]
    off = (first_row + np.concatenate([[0], np.cumsum([len(s["p1"]) for s in scenes])])).astype(np.int64)
    rows = int(off[-1]) + tail
    p1 = np.full((rows, dim), np.nan); p2 = np.full((rows, dim), np.nan)
    for s, b, e in zip(scenes, off[:-1], off[1:]):
        p1[b:e] = s["p1"]; p2[b:e] = s["p2"]
    return dict(pts1=p1, pts2=p2, off=off, seeds=np.array([s["seed"] for s in scenes], dtype=np.uint32), rows=rows)


def new_outputs(P, rows):
    """sentinel-filled outputs: model of P pairs, mask of `rows` bytes, stats of P pairs, G guard pairs / bytes on each side"""
    return {k: np.full((G + (rows if k == "mask" else P) + G) * PER[k], FILL[k], dtype=DTYPE[k]) for k in PER}


def body(k, P, rows):
    """the slice of output k's buffer that the call gets as its pointer's extent"""
    return slice(G * PER[k], (G + (rows if k == "mask" else P)) * PER[k])


def rearm(outs, P, off):
    """shorten the bodies to P pairs on the rows off[0] .. off[P]: everything behind them becomes guard again; the bodies keep what they hold
    (numpy arrays or device tensors)"""
    for k in ("model", "stats"):
        outs[k][(G + P) * PER[k]:] = FILL[k]
    outs["mask"][G + int(off[P]):] = FILL["mask"]


def read(outs, off, P, stats_null=False):
    """per pair (model [9], mask bytes, stats [16] or None) after everything the call does not own was found untouched: the guards, the
    mask bytes in front of off[0] and behind off[P] (unowned rows of the store), with stats_null the whole stats buffer; and every owned
    mask byte is 0 or 1"""
    for k in ("model", "stats"):
        b = outs[k]; lo = G * PER[k]; hi = (G + P) * PER[k]
        assert (b[:lo] == FILL[k]).all(), f"{k}: a guard element in front of pair 0 was written"
        assert (b[hi:] == FILL[k]).all(), f"{k}: a guard element behind pair {P - 1} was written"
    if stats_null:
        assert (outs["stats"] == FILL["stats"]).all(), "stats: written although NULL was passed"
    m = outs["mask"]; lo = G + int(off[0]); hi = G + int(off[P])
    assert (m[:lo] == FILL["mask"]).all(), "mask: a byte in front of the first owned row was written"
    assert (m[hi:] == FILL["mask"]).all(), "mask: a byte behind the last owned row was written"
    assert (m[lo:hi] <= 1).all(), "mask: an owned byte is neither 0 nor 1"
    return [(outs["model"][(G + p) * 9:(G + p + 1) * 9], m[G + int(off[p]):G + int(off[p + 1])],
             None if stats_null else outs["stats"][(G + p) * 16:(G + p + 1) * 16]) for p in range(P)]


def untouched(outs):
    """every byte, body and guards alike, still holds its sentinel"""
    return all(bool((outs[k] == FILL[k]).all()) for k in PER)


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def same_bytes(a, b, stats=True):
    """model and mask bytes, stats words 0 .. 11 (12 and 13 are device clock ticks, 14 and 15 describe the launch)"""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (not stats or np.asarray(a[2][:12], np.int32).tobytes() ==
                                                                                      np.asarray(b[2][:12], np.int32).tobytes())


def no_model(got, ref_I=0):
    """nine zeros (every byte), an all-zero mask, not discarded, and I as the restatement has it: 0 for H; 8 for F, whose driver starts
    from the score I = 8 and returns it when nothing was accepted (exp_ranF.c's return value, MI_ST_I)"""
    ok = got[0].tobytes() == bytes(72) and not got[1].any()
    return ok and (got[2] is None or (got[2][_lib.STAT_NAMES.index("I")] == ref_I and not got[2][15] & 1024))


def agrees(kind, got, ref):
    """one pair against the restatement: '' or what differs.  The shared counters equal; where the restatement has a model, the mask bit
    for bit and the model within MODEL_TOL relative Frobenius; where it has none, nine zeros and an all-zero mask (the F restatement
    leaves the mask of its unwritten residuals there, all ones: the device's contract is the zero mask, include/mi_degensac.h)"""
    Mo, mo, so = ref
    if got[2] is not None:
        diff = {k: (int(got[2][_lib.STAT_NAMES.index(k)]), so[k]) for k in KEYS[kind] if got[2][_lib.STAT_NAMES.index(k)] != so[k]}
        if diff:
            return f"counters: {diff}"
        if got[2][15] & (1024 | 2048):
            return "discarded"
    if not np.asarray(Mo).any():
        return "" if no_model(got, so["I"]) else "the restatement has no model; the device's model or mask is not zero"
    if not np.array_equal(got[1], np.asarray(mo, np.uint8)):
        return f"mask: {int((got[1] != np.asarray(mo, np.uint8)).sum())} bytes differ"
    if not got[0].any():
        return "zero model where the restatement has one"
    r = gu.rel(got[0], Mo)
    return "" if r < MODEL_TOL else f"model: relative distance {r:.3e}"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
# name, the code the call returns (a name of pydegensac_amd._lib), what differs from a good call of two 64-row pairs.
#   n_pairs / dim / device: that argument; host_null: offsets_host = NULL; rows: pair 1 has that many rows (by kind); error_type: by kind;
#   null: that pointer is NULL.  The `null` cases are host-side checks of launch_batch_impl (csrc/mi_degensac_host.inc): a library
#   without them would launch on the NULL pointer, so the GPU test first proves with REFUSAL_PROBE that the loaded library has them.
REFUSALS = (
    dict(name="n_pairs = 0", code="OK", n_pairs=0),
    dict(name="a pair below the minimum", code="EINVAL", rows={"F": 7, "H": 3}),
    dict(name="dim = 3", code="EINVAL", dim=3),
    dict(name="offsets_host = NULL", code="EINVAL", host_null=True),
    dict(name="error_type out of range", code="EINVAL", error_type={"F": 2, "H": 5}),
    dict(name="device = 63", code="EHIP", device=63),
) + tuple(dict(name=f"{p} = NULL", code="EINVAL", null=p) for p in ("pts1", "pts2", "offsets", "seeds", "model", "mask"))
# a call that no library launches: the NULL check comes before the parameters are read, a library without it stops at the error type
REFUSAL_PROBE = dict(name="probe", code="EINVAL", null="pts1", error_type={"F": 99, "H": 99})
REFUSAL_PROBE_MESSAGE = "NULL argument"
REFUSAL_ROWS = 64


def refusal_batch(kind, case):
    """the two pairs of a refusal case"""
    a = row_scene(kind, REFUSAL_ROWS); b = dict(a)
    if "rows" in case:
        n = case["rows"][kind]
        b = dict(a, p1=a["p1"][:n], p2=a["p2"][:n])
    return [a, b]
