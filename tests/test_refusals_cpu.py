"""The refusal table of pydegensac_amd.matcher and pydegensac_amd.tensor_api: every public call of the two modules that refuses arguments
before the library is entered, with the exact (exception class, text) it raises.  The numpy forms are driven with arrays, the tensor forms
with CPU torch tensors, which reach every shape, dtype, count, pair-list and parameter check and end in the device refusal (a tensor on the
"meta" device stands in for "another device").  Every function has one case with two defects that pins which text wins.

The expected texts were filled in by running this table on the commit before the marshalling of the two modules was folded into shared
helpers, where it passed as it stands: the table is the record of what the calls refused then, and in which order.  What no CPU tensor can
reach (the checks that find_*_batch_tensors, knn_match_tensors, quantize_descriptors_tensors and tracks_tensors make after their device
test, and the dim % 4 text of the uint8 descriptor pair) is not in it; match_filter_tensors, guided_entry and correspond_layout check nothing
themselves."""
import numpy as np
import pytest
import torch

from pydegensac_amd import api, matcher as m, tensor_api as t

V = ValueError
T = torch.from_numpy
rng = np.random.default_rng(0)
D = rng.normal(size=(5, 4)).astype(np.float32)             # descriptors: 5 rows, dim 4
U = rng.integers(0, 256, (5, 8), dtype=np.uint8)
X = rng.uniform(0, 50, (5, 2))                             # keypoints as float64 rows
KP = rng.uniform(1, 50, (5, 4)).astype(np.float32)         # keypoints as (x, y, size, angle)
C1, C2 = [3, 2], [2, 3]                                    # the ragged batch: K = 2 pairs
CI, PAIRS = [3, 2], [[0, 1], [1, 0]]                       # the pair list: 2 images, K = 2 entries, 5 output rows
MOD = np.zeros((2, 3, 3))
META = torch.empty((5, 2), dtype=torch.float64, device="meta")

# ---- the texts that more than one call raises ----
MODEL = "model should be 'F' or 'H'"
RATIO_NUM = "ratio should be a number, or None for no ratio test"
RATIO_POS = "ratio should be finite and > 0"
MUTUAL = 'mutual should be False, True or "ratio"'
MUTUAL_NONE = 'mutual="ratio" needs a ratio: ratio=None is no ratio test in either direction'
MD_NUM = "max_dist should be a number"
MD_POS = "max_dist should be finite and >= 0"
FGINN_RULE = 'the FGINN second neighbour belongs to the forward ratio test: it goes with max_dist, not with ratio=None or mutual="ratio"'
DESC = "descriptors should be [N1, dim] and [N2, dim] with the same dim"
DESC_DT = "descriptors should both be float32 (L2) or both uint8 (Hamming)"
NORM = "norm should be 'l2', 'hamming' or 'l2_u8'"
HAM = "the Hamming norm needs uint8 descriptors"
L2 = "the L2 norm needs float32 descriptors (norm 'l2_u8' takes uint8 rows of dim <= 256 as they are)"
U8 = "norm 'l2_u8' needs uint8 descriptors"
U8_DIM = "norm 'l2_u8' takes dim <= 256: use float32 descriptors with norm 'l2' beyond that"
KPS = "keypoints should be float64 [n, 2] / [n, 6] rows or float32 [n, 4] = (x, y, size, angle)"
KPS_LAYOUT = "kps1 and kps2 should have the same layout"
KPS_ROWS = "one keypoint row per descriptor row"
KPS_XY = "keypoints should be float64 [n, 2] / [n, 6] rows"
CNT_PAIR = "counts1 and counts2 should be 1-D with one entry per pair"
CNT_IMG = "counts1 and counts2 should be 1-D with one entry per image"
CNT_INT = "counts should be integers"
CNT_NEG = "counts should be >= 0"
CNT_SUM = "counts do not add up to the number of descriptor rows"
PAIRS_ARR = "pairs should be an integer array [K, 2] of (image of store 1, image of store 2)"
PAIRS_0 = "at least one pair"
PAIRS_RANGE = "pairs hold an image index outside its store (2 and 2 images)"
PAIRS_BIG = "too many rows in one pair list"
SEEDS = "one seed per pair"
NO_GUIDED = "guided matching is not part of this pair-list call: pass the models it returns to guided_match_pairs / guided_match_pairs_tensors"
NO_FGINN = ("fginn_th (the FGINN ratio test) is not part of the pair-list calls: use match_and_verify_batch, or "
            "match_and_verify_fginn_pairs / match_and_verify_fginn_pairs_tensors over a pair list")
GFT = ("guided_fginn_th is the FGINN radius of the guided stage: pass guided=True with it (fginn_th is the radius of the tentatives in front "
       "of the estimator)")
MODELS_PAIR = "models should be [K, 3, 3] = [2, 3, 3], one model per pair"
MODELS_ENTRY = "models should be [K, 3, 3] = [2, 3, 3], one model per list entry"
MODELS_DT = "models should be float64"
PX_NUM = "px_th should be a number"
PX_POS = "px_th should be >= 0 (and not NaN)"
ET_F = "Error type should be on of {}. Got bad instead".format(list(api.error_type_dict_fundamental.keys()))
ET_H = "Error type should be on of {}. Got bad instead".format(list(api.error_type_dict_homography.keys()))
DESC_DEV = "descriptors must be torch tensors on the same ROCm device"
DESC_T = "descriptors must be torch tensors on a ROCm device"
T4 = "kps1, kps2, desc1 and desc2 must be torch tensors on a ROCm device"
T5 = "kps1, kps2, desc1, desc2 and models must be torch tensors on a ROCm device"
T5_DEV = "kps1, kps2, desc1, desc2 and models must live on the same ROCm device"
T4_DEV = "kps1, kps2, desc1 and desc2 must live on the same ROCm device"
T3 = "desc1, desc2 and kps2 must be torch tensors on a ROCm device"
T3_DEV = "desc1, desc2 and kps2 must live on the same ROCm device"
PAIR_EVERY = "every pair's arrays should be 2-D with the dtype and width of pair 0"
IMG_EVERY = "every image's arrays should be 2-D with the dtype and width of image 0"
OFF = "corr_offsets should be int64 [K + 1], as the correspondence export returns it"
PTS = "pts should be float64 [cap, 4] = x1, y1, x2, y2, as the correspondence export returns it"
LIST_BIG = "too many rows in one list"
POSE_MODELS = "models should be float64 [K, 3, 3], one fundamental matrix per entry of corr_offsets"
CAMS8 = "cams1 should be float64 [K, 8] = fx, fy, cx, cy of camera 1 and of camera 2 per entry (or give pairs)"
CAMS1 = "cams1 should be float64 [n_images, 4] = fx, fy, cx, cy per image of store 1"
CAMS2 = "cams2 should be float64 [n_images, 4] = fx, fy, cx, cy per image of store 2"
KEEP_CAP = "keep should be bool or uint8 [cap], one flag per row of pts"
PARALLAX = "min_parallax_deg should be a number in [0, 180]"
R_K = "R should be float64 [K, 3, 3], one rotation per entry of corr_offsets"
T_K = "t should be float64 [K, 3], one baseline direction per entry of corr_offsets"
TRIALS = "max_trials should be an integer in 0 .. 100"
FTOL = "ftol should be a number >= 0"

# ---- arguments that pass every check (the tensor forms then end in their device refusal) ----
BT = dict(kps1=T(X), kps2=T(X), desc1=T(D), desc2=T(D), counts1=C1, counts2=C2)                    # ragged batch, tensors
PT = dict(kps1=T(X), kps2=T(X), desc1=T(D), desc2=T(D), counts1=CI, counts2=CI, pairs=PAIRS)       # pair list, tensors
BL = dict(kps1_list=[X[:3], X[3:]], kps2_list=[X[:2], X[2:]], desc1_list=[D[:3], D[3:]], desc2_list=[D[:2], D[2:]])
PL = dict(kps_list=[X[:3], X[3:]], desc_list=[D[:3], D[3:]], pairs=PAIRS)
GB = dict(BT, models=T(MOD))
GP = dict(PT, models=T(MOD))
GBL = dict(BL, models=MOD)
GPL = dict(PL, models=MOD)
KB = dict(desc1=T(D), desc2=T(D), counts1=C1, counts2=C2)
KPR = dict(desc1=T(D), desc2=T(D), counts1=CI, counts2=CI, pairs=PAIRS)
FB = dict(KB, kps2=T(X))
FP = dict(KPR, kps2=T(X))
MATCH = np.full(5, -1, np.int32)
CT = dict(match=T(MATCH), counts1=CI, counts2=CI, pairs=PAIRS)                                     # correspondence export
CN = dict(match=MATCH, counts1=CI, counts2=CI, pairs=PAIRS)
# exported lists: K = 2 entries over cap = 3 rows
PTS4 = np.zeros((3, 4)); OFFS = np.array([0, 2, 3], np.int64); CAM8 = np.ones((2, 8)); CAM4 = np.ones((2, 4))
RN = dict(pts=PTS4, corr_offsets=OFFS, models=MOD)
RT = dict(pts=T(PTS4), corr_offsets=T(OFFS), models=T(MOD))
PN = dict(RN, cams1=CAM8)
PTN = dict(RT, cams1=T(CAM8))
RR, TT = np.zeros((2, 3, 3)), np.zeros((2, 3))
FN = dict(pts=PTS4, corr_offsets=OFFS, R=RR, t=TT, cams1=CAM8)
FT = dict(pts=T(PTS4), corr_offsets=T(OFFS), R=T(RR), t=T(TT), cams1=T(CAM8))
# tracks: T = 1 track of M = 2 observations over 2 images of 2 rows
TO, OB, OI, KX = np.array([0, 2], np.int64), np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.zeros((4, 2))
TN = dict(track_offsets=TO, obs=OB, obs_image=OI, kps=KX, cams=CAM4, R=RR, t=TT)
TTN = {k: T(v) for k, v in TN.items()}
ROWS = np.zeros((2, 2), np.int32)
# shapes and dtypes as the check_* functions take them
SH = ((5, 4), np.float32, (5, 4), np.float32, (5, 2), np.float64, (5, 2), np.float64)
f64, i64, i32 = np.float64, np.int64, np.int32
POSE_SH = ((3, 4), f64, (3,), i64, (2, 3, 3), f64, (2, 8), f64)
POSE_SH_P = ((3, 4), f64, (3,), i64, (2, 3, 3), f64, (2, 4), f64)
REFINE_SH = ((3, 4), f64, (3,), i64, (2, 3, 3), f64, (2, 3), f64, (2, 8), f64)
TRI_SH = ((2,), i64, (2,), i32, (2,), i32, (4, 2), f64, (2, 4), f64, (2, 3, 3), f64, (2, 3), f64)


def sides(i, shape=None, dtype=None):
    """SH with the shape / dtype of array i (0, 1: descriptors, 2, 3: keypoints) replaced"""
    s = list(SH)
    if shape is not None: s[2 * i] = shape
    if dtype is not None: s[2 * i + 1] = dtype
    return tuple(s)


def put(sh, i, shape=None, dtype=None):
    s = list(sh)
    if shape is not None: s[2 * i] = shape
    if dtype is not None: s[2 * i + 1] = dtype
    return tuple(s)


CASES = []


def c(name, fn, base, over, exc, msg):
    """fn(**base, **over) raises exc with exactly msg"""
    CASES.append(pytest.param(lambda: fn(**dict(base, **over)), exc, msg, id=name))


def p(name, call, exc, msg):
    CASES.append(pytest.param(call, exc, msg, id=name))


# ---- matcher.py: the checks themselves ----
p("rule/ratio-str", lambda: m.check_rule("x"), V, RATIO_NUM)
p("rule/ratio-0", lambda: m.check_rule(0), V, RATIO_POS)
p("rule/ratio-nan", lambda: m.check_rule(float("nan")), V, RATIO_POS)
p("rule/mutual-str", lambda: m.check_rule(0.9, "both"), V, MUTUAL)
p("rule/mutual-ratio-none", lambda: m.check_rule(None, "ratio"), V, MUTUAL_NONE)
p("rule/max_dist-str", lambda: m.check_rule(0.9, False, "x"), V, MD_NUM)
p("rule/max_dist-neg", lambda: m.check_rule(0.9, False, -1), V, MD_POS)
p("rule/max_dist-huge", lambda: m.check_rule(0.9, False, 1e39), V, MD_POS)
p("rule/fginn-no-ratio", lambda: m.check_rule(None, False, None, fginn=True), V, FGINN_RULE)
p("rule/fginn-back-ratio", lambda: m.check_rule(0.9, "ratio", None, fginn=True), V, FGINN_RULE)
p("rule/2:ratio+mutual", lambda: m.check_rule("x", "both"), V, RATIO_NUM)
p("rule/2:mutual+max_dist", lambda: m.check_rule(0.9, "both", -1), V, MUTUAL)
p("rule/2:max_dist+fginn", lambda: m.check_rule(None, False, -1, fginn=True), V, MD_POS)

p("fginn_th/str", lambda: m.check_fginn_th("x"), V, "fginn_th should be a number")
p("fginn_th/neg", lambda: m.check_fginn_th(-1), V, "fginn_th should be finite and >= 0")
p("fginn_th/inf-named", lambda: m.check_fginn_th(float("inf"), "spatial_th"), V, "spatial_th should be finite and >= 0")
p("guided_fginn_th/unguided", lambda: m.check_guided_fginn_th(False, 3.0), V, GFT)
p("guided_fginn_th/str", lambda: m.check_guided_fginn_th(True, "x"), V, "guided_fginn_th should be a number")
p("guided_fginn_th/2:unguided+str", lambda: m.check_guided_fginn_th(False, "x"), V, GFT)

p("quant_params/preset", lambda: m.quant_params("bad"), V, "preset should be one of rootsift, sift, unit")
p("quant_params/normalize", lambda: m.quant_params(normalize="l3"), V, 'normalize should be "none", "l2" or "l1root"')
p("quant_params/normalize-bool", lambda: m.quant_params(normalize=True), V, 'normalize should be "none", "l2" or "l1root"')
p("quant_params/scale-str", lambda: m.quant_params(scale="x"), V, "scale should be a number")
p("quant_params/scale-0", lambda: m.quant_params(scale=0), V, "scale should be finite and > 0")
p("quant_params/offset-float", lambda: m.quant_params(offset=1.5), V, "offset should be an integer 0 .. 255")
p("quant_params/offset-bool", lambda: m.quant_params(offset=True), V, "offset should be an integer 0 .. 255")
p("quant_params/offset-256", lambda: m.quant_params(offset=256), V, "offset should be an integer 0 .. 255")
p("quant_params/2:preset+scale", lambda: m.quant_params("bad", scale=0), V, "preset should be one of rootsift, sift, unit")
p("quant_params/2:normalize+offset", lambda: m.quant_params(normalize="l3", offset=-1), V, 'normalize should be "none", "l2" or "l1root"')
p("quant_params/2:scale+offset", lambda: m.quant_params(scale=-1, offset=300), V, "scale should be finite and > 0")
p("quant_input/dtype", lambda: m.check_quantize_input((5, 4), np.float64), V, "descriptors to quantise should be float32")
p("quant_input/shape", lambda: m.check_quantize_input((5,), np.float32), V, "descriptors to quantise should be [n, dim] with 1 <= dim <= 256")
p("quant_input/dim", lambda: m.check_quantize_input((5, 257), torch.float32), V, "descriptors to quantise should be [n, dim] with 1 <= dim <= 256")
p("quant_input/2:dtype+shape", lambda: m.check_quantize_input((5,), np.uint8), V, "descriptors to quantise should be float32")

mva = m.check_match_verify_args
p("mva/model", lambda: mva("X", 0.9, None, *SH, C1, C2), V, MODEL)
p("mva/ratio-str", lambda: mva("F", "x", None, *SH, C1, C2), V, "ratio should be a number")
p("mva/ratio-0", lambda: mva("F", 0, None, *SH, C1, C2), V, RATIO_POS)
p("mva/desc-1d", lambda: mva("F", 0.9, None, *sides(0, (5,)), C1, C2), V, DESC)
p("mva/desc-dim", lambda: mva("F", 0.9, None, *sides(1, (5, 8)), C1, C2), V, DESC)
p("mva/desc-dim0", lambda: mva("F", 0.9, None, *put(sides(0, (5, 0)), 1, (5, 0)), C1, C2), V, DESC)
p("mva/desc-dtypes", lambda: mva("F", 0.9, None, *sides(1, None, np.uint8), C1, C2), V, DESC_DT)
p("mva/desc-f64", lambda: mva("F", 0.9, None, *put(sides(0, None, f64), 1, None, torch.float64), C1, C2), V, DESC_DT)
p("mva/norm", lambda: mva("F", 0.9, "l1", *SH, C1, C2), V, NORM)
p("mva/hamming-f32", lambda: mva("F", 0.9, "hamming", *SH, C1, C2), V, HAM)
p("mva/l2-u8", lambda: mva("F", 0.9, "l2", *put(sides(0, None, np.uint8), 1, None, np.uint8), C1, C2), V, L2)
p("mva/l2_u8-f32", lambda: mva("F", 0.9, "l2_u8", *SH, C1, C2), V, U8)
p("mva/l2_u8-dim", lambda: mva("F", 0.9, "l2_u8", *put(sides(0, (5, 260), np.uint8), 1, (5, 260), np.uint8), C1, C2), V, U8_DIM)
p("mva/kps-f32x2", lambda: mva("F", 0.9, None, *sides(2, None, np.float32), C1, C2), V, KPS)
p("mva/kps-width", lambda: mva("F", 0.9, None, *sides(3, (5, 3)), C1, C2), V, KPS)
p("mva/kps-layout", lambda: mva("F", 0.9, None, *sides(3, (5, 6)), C1, C2), V, KPS_LAYOUT)
p("mva/kps-kinds", lambda: mva("F", 0.9, None, *sides(3, (5, 4), np.float32), C1, C2), V, KPS_LAYOUT)
p("mva/kps-rows", lambda: mva("F", 0.9, None, *sides(2, (4, 2)), C1, C2), V, KPS_ROWS)
p("mva/counts-len", lambda: mva("F", 0.9, None, *SH, [3, 2], [5]), V, CNT_PAIR)
p("mva/counts-2d", lambda: mva("F", 0.9, None, *SH, [[3, 2]], C2), V, CNT_PAIR)
p("mva/counts-float", lambda: mva("F", 0.9, None, *SH, [3.0, 2.0], C2), V, CNT_INT)
p("mva/counts-neg", lambda: mva("F", 0.9, None, *SH, [6, -1], C2), V, CNT_NEG)
p("mva/counts-sum", lambda: mva("F", 0.9, None, *SH, C1, [2, 2]), V, CNT_SUM)
p("mva/fginn_th", lambda: mva("F", 0.9, None, *SH, C1, C2, -1), V, "fginn_th should be finite and >= 0")
p("mva/2:fginn_th+model", lambda: mva("X", 0.9, None, *SH, C1, C2, "x"), V, "fginn_th should be a number")
p("mva/2:model+ratio", lambda: mva("X", 0, None, *SH, C1, C2), V, MODEL)
p("mva/2:norm+kps", lambda: mva("F", 0.9, "l1", *sides(2, (5, 3)), C1, C2), V, NORM)
p("mva/2:kps+counts", lambda: mva("F", 0.9, None, *sides(2, (4, 2)), [9], [1]), V, KPS_ROWS)
# the ragged calls run every side under one check before the next check: side 2's float counts win over side 1's negative ones
p("mva/2:neg1+float2", lambda: mva("F", 0.9, None, *SH, [6, -1], [2.0, 3.0]), V, CNT_INT)
p("mva/2:sum1+neg2", lambda: mva("F", 0.9, None, *SH, [3, 3], [6, -1]), V, CNT_NEG)

mpa = m.check_match_pairs_args
p("mpa/guided", lambda: mpa("F", 0.9, None, *SH, CI, CI, PAIRS, None, True), V, NO_GUIDED)
p("mpa/fginn_th", lambda: mpa("F", 0.9, None, *SH, CI, CI, PAIRS, None, False, 3.0), V, NO_FGINN)
p("mpa/model", lambda: mpa("X", 0.9, None, *SH, CI, CI, PAIRS), V, MODEL)
p("mpa/counts-2d", lambda: mpa("F", 0.9, None, *SH, [[3, 2]], CI, PAIRS), V, CNT_IMG)
p("mpa/counts-float", lambda: mpa("F", 0.9, None, *SH, CI, [3.0, 2.0], PAIRS), V, CNT_INT)
p("mpa/counts-neg", lambda: mpa("F", 0.9, None, *SH, [6, -1], CI, PAIRS), V, CNT_NEG)
p("mpa/counts-sum", lambda: mpa("F", 0.9, None, *SH, CI, [3, 3], PAIRS), V, CNT_SUM)
p("mpa/pairs-1d", lambda: mpa("F", 0.9, None, *SH, CI, CI, [0, 1]), V, PAIRS_ARR)
p("mpa/pairs-3col", lambda: mpa("F", 0.9, None, *SH, CI, CI, [[0, 1, 0]]), V, PAIRS_ARR)
p("mpa/pairs-float", lambda: mpa("F", 0.9, None, *SH, CI, CI, [[0.0, 1.0]]), V, PAIRS_ARR)
p("mpa/pairs-empty", lambda: mpa("F", 0.9, None, *SH, CI, CI, np.zeros((0, 2), np.int64)), V, PAIRS_0)
p("mpa/pairs-neg", lambda: mpa("F", 0.9, None, *SH, CI, CI, [[0, -1]]), V, PAIRS_RANGE)
p("mpa/pairs-high-1", lambda: mpa("F", 0.9, None, *SH, CI, CI, [[2, 0]]), V, PAIRS_RANGE)
p("mpa/pairs-high-2", lambda: mpa("F", 0.9, None, *SH, CI, CI, [[0, 2]]), V, PAIRS_RANGE)
p("mpa/too-many-rows", lambda: mpa("F", 0.9, None, (2 ** 30, 4), np.float32, (1, 4), np.float32, (2 ** 30, 2), f64, (1, 2), f64, [2 ** 30], [1],
                                   [[0, 0]]), V, PAIRS_BIG)
p("mpa/too-many-train-rows", lambda: mpa("F", 0.9, None, (1, 4), np.float32, (2 ** 29, 4), np.float32, (1, 2), f64, (2 ** 29, 2), f64, [1], [2 ** 29],
                                         [[0, 0], [0, 0]]), V, PAIRS_BIG)
p("mpa/seeds", lambda: mpa("F", 0.9, None, *SH, CI, CI, PAIRS, [1, 2, 3]), V, SEEDS)
p("mpa/2:guided+fginn_th", lambda: mpa("F", 0.9, None, *SH, CI, CI, PAIRS, None, True, 3.0), V, NO_GUIDED)
p("mpa/2:fginn_th+model", lambda: mpa("X", 0.9, None, *SH, CI, CI, PAIRS, None, False, 3.0), V, NO_FGINN)
p("mpa/2:counts+pairs", lambda: mpa("F", 0.9, None, *SH, CI, [3, 3], [[0, 5]]), V, CNT_SUM)
p("mpa/2:pairs+seeds", lambda: mpa("F", 0.9, None, *SH, CI, CI, [[0, 2]], [1, 2, 3]), V, PAIRS_RANGE)
# the pair-list calls run every check on side 1 before any on side 2: side 1's negative counts win over side 2's float ones
p("mpa/2:neg1+float2", lambda: mpa("F", 0.9, None, *SH, [6, -1], [3.0, 2.0], PAIRS), V, CNT_NEG)
p("mpa/2:sum1+2d2", lambda: mpa("F", 0.9, None, *SH, [3, 3], [[3, 2]], PAIRS), V, CNT_SUM)

p("exhaustive_pairs/neg", lambda: m.exhaustive_pairs(-1), V, "n should be >= 0")
p("estimator_params/error_type", lambda: m.estimator_params("F", error_type="bad"), V, ET_F)
p("estimator_params/error_type-h", lambda: m.estimator_params("H", error_type="bad"), V, ET_H)
p("estimator_params/model", lambda: m.estimator_params("X"), KeyError, "'X'")
p("estimator_params/2:model+error_type", lambda: m.estimator_params("X", error_type="bad"), KeyError, "'X'")

cga = m.check_guided_args
p("cga/model", lambda: cga("X", None, "sampson", (2, 3, 3), f64, 2), V, MODEL)
p("cga/models-shape", lambda: cga("F", None, "sampson", (3, 3, 3), f64, 2), V, MODELS_PAIR)
p("cga/models-dtype", lambda: cga("F", None, "sampson", (2, 3, 3), torch.float32, 2), V, MODELS_DT)
p("cga/px_th-str", lambda: cga("F", "x", "sampson", (2, 3, 3), f64, 2), V, PX_NUM)
p("cga/px_th-neg", lambda: cga("F", -1, "sampson", (2, 3, 3), f64, 2), V, PX_POS)
p("cga/px_th-nan", lambda: cga("H", float("nan"), "sampson", (2, 3, 3), f64, 2), V, PX_POS)
p("cga/error_type", lambda: cga("H", None, "bad", (2, 3, 3), f64, 2), V, ET_H)
p("cga/2:model+models", lambda: cga("X", None, "sampson", (2, 9), f64, 2), V, MODEL)
p("cga/2:models+px_th", lambda: cga("F", -1, "sampson", (2, 3, 3), np.float32, 2), V, MODELS_DT)
p("cga/2:px_th+error_type", lambda: cga("F", -1, "bad", (2, 3, 3), f64, 2), V, PX_POS)

p("two_view_params/f-not-dict", lambda: m.two_view_params([1]), V, "f_params should be a dict of estimator keywords, or None")
p("two_view_params/h-not-dict", lambda: m.two_view_params(None, 3), V, "h_params should be a dict of estimator keywords, or None")
p("two_view_params/f-key", lambda: m.two_view_params({"px": 1}), V,
  "f_params: unknown key px (known: px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check)")
p("two_view_params/h-key", lambda: m.two_view_params(None, {"enable_degeneracy_check": True}), V,
  "h_params: unknown key enable_degeneracy_check (known: px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check)")
p("two_view_params/error_type", lambda: m.two_view_params({"error_type": "bad"}), V, ET_F)
p("two_view_params/2:f+h", lambda: m.two_view_params({"error_type": "bad"}, 3), V, ET_F)
p("two_view_config/shape", lambda: m.two_view_config(np.zeros((2, 3), np.int32)), V,
  "summary should be an integer array [K, 4] = (tentatives, nF, nH, nFH)")
p("two_view_config/dtype", lambda: m.two_view_config(torch.zeros((2, 4))), V, "summary should be an integer array [K, 4] = (tentatives, nF, nH, nFH)")
p("pose_config/shape", lambda: m.pose_config(np.zeros((2, 4), np.int32)), V, "info should be an integer array [K, 5] = (used, front, runner-up, wide, status)")
p("pose_config/dtype", lambda: m.pose_config(torch.zeros((2, 5))), V, "info should be an integer array [K, 5] = (used, front, runner-up, wide, status)")

cca = m.check_correspond_args
XY = ((5, 2), f64)
CNT12 = "counts1 and counts2 should be 1-D arrays of integers >= 0"
MATCH_N = "match should be int32 [N] = [5], one value per output row of the list"
KEEP_N = "keep should be bool or uint8 [N] = [5]"
p("cca/model", lambda: cca((5,), i32, CI, CI, PAIRS, model="X"), V, MODEL)
p("cca/error_type", lambda: cca((5,), i32, CI, CI, PAIRS, error_type="bad"), V, ET_F)
p("cca/counts-2d", lambda: cca((5,), i32, [[3, 2]], CI, PAIRS), V, CNT12)
p("cca/counts-float", lambda: cca((5,), i32, CI, [3.0, 2.0], PAIRS), V, CNT12)
p("cca/counts-neg", lambda: cca((5,), i32, CI, [6, -1], PAIRS), V, CNT12)
p("cca/batch-counts-len", lambda: cca((5,), i32, CI, [5], None), V, "counts1 and counts2 should have one entry per pair")
p("cca/pairs-1d", lambda: cca((5,), i32, CI, CI, [0, 1]), V, PAIRS_ARR)
p("cca/pairs-float", lambda: cca((5,), i32, CI, CI, [[0.0, 1.0]]), V, PAIRS_ARR)
p("cca/pairs-empty", lambda: cca((0,), i32, CI, CI, np.zeros((0, 2), np.int32)), V, PAIRS_0)
p("cca/pairs-range", lambda: cca((5,), i32, CI, CI, [[2, 0]]), V, PAIRS_RANGE)
p("cca/pairs-neg", lambda: cca((5,), i32, CI, CI, [[0, -1]]), V, PAIRS_RANGE)
p("cca/too-many-rows", lambda: cca((2 ** 30,), i32, [2 ** 30], [1], [[0, 0]]), V, PAIRS_BIG)
p("cca/too-many-train-rows", lambda: cca((1,), i32, [1], [2 ** 30], None), V, PAIRS_BIG)
p("cca/match-shape", lambda: cca((4,), i32, CI, CI, PAIRS), V, MATCH_N)
p("cca/match-dtype", lambda: cca((5,), i64, CI, CI, PAIRS), V, MATCH_N)
p("cca/keep-shape", lambda: cca((5,), i32, CI, CI, PAIRS, ((4,), np.bool_)), V, KEEP_N)
p("cca/keep-dtype", lambda: cca((5,), i32, CI, CI, PAIRS, ((5,), torch.int32)), V, KEEP_N)
p("cca/kps-one", lambda: cca((5,), i32, CI, CI, PAIRS, None, XY, None), V, "kps1 and kps2 go together")
p("cca/kps-width", lambda: cca((5,), i32, CI, CI, PAIRS, None, ((5, 3), f64), XY), V, KPS)
p("cca/kps-layout", lambda: cca((5,), i32, CI, CI, PAIRS, None, XY, ((5, 6), f64)), V, KPS_LAYOUT)
p("cca/kps-rows", lambda: cca((5,), i32, CI, CI, PAIRS, None, XY, ((4, 2), f64)), V, "counts do not add up to the number of keypoint rows")
p("cca/models-no-kps", lambda: cca((5,), i32, CI, CI, PAIRS, models=((2, 3, 3), f64)), V, "models (the residuals) need kps1 and kps2")
p("cca/models-shape", lambda: cca((5,), i32, CI, CI, PAIRS, None, XY, XY, ((3, 3, 3), f64)), V, MODELS_ENTRY)
p("cca/models-dtype", lambda: cca((5,), i32, CI, CI, PAIRS, None, XY, XY, ((2, 3, 3), np.float32)), V, MODELS_DT)
p("cca/capacity-neg", lambda: cca((5,), i32, CI, CI, PAIRS, capacity=-1), V, "capacity should be an integer >= 0 (or None = one position per output row)")
p("cca/capacity-bool", lambda: cca((5,), i32, CI, CI, PAIRS, capacity=True), V, "capacity should be an integer >= 0 (or None = one position per output row)")
p("cca/capacity-float", lambda: cca((5,), i32, CI, CI, PAIRS, capacity=2.0), V, "capacity should be an integer >= 0 (or None = one position per output row)")
p("cca/2:model+counts", lambda: cca((5,), i32, [[3, 2]], CI, PAIRS, model="X"), V, MODEL)
p("cca/2:counts+pairs", lambda: cca((5,), i32, CI, [6, -1], [0, 1]), V, CNT12)
p("cca/2:pairs+match", lambda: cca((4,), i64, CI, CI, [[2, 0]]), V, PAIRS_RANGE)
p("cca/2:match+keep", lambda: cca((4,), i32, CI, CI, PAIRS, ((4,), np.bool_)), V, MATCH_N)
p("cca/2:keep+kps", lambda: cca((5,), i32, CI, CI, PAIRS, ((5,), f64), XY, None), V, KEEP_N)
p("cca/2:kps+models", lambda: cca((5,), i32, CI, CI, PAIRS, None, XY, ((5, 6), f64), ((2, 9), f64)), V, KPS_LAYOUT)
p("cca/2:models+capacity", lambda: cca((5,), i32, CI, CI, PAIRS, None, XY, XY, ((2, 9), f64), capacity=-1), V, MODELS_ENTRY)

cta = m.check_tracks_args
p("cta/counts", lambda: cta((2, 2), i32, [[2, 2]]), V, "counts should be a 1-D array of integers >= 0, the rows per image of the store")
p("cta/counts-neg", lambda: cta((2, 2), i32, [2, -2]), V, "counts should be a 1-D array of integers >= 0, the rows per image of the store")
p("cta/store-big", lambda: cta((2, 2), i32, [2 ** 31]), V, "too many rows in the store (its rows must fit int32)")
p("cta/rows", lambda: cta((2, 3), i32, [2, 2]), V, "rows should be int32 [M, 2] of store rows, as the correspondence export writes them with store_rows=True")
p("cta/rows-dtype", lambda: cta((2, 2), i64, [2, 2]), V, "rows should be int32 [M, 2] of store rows, as the correspondence export writes them with store_rows=True")
p("cta/edges-big", lambda: cta((2 ** 30, 2), i32, [2, 2]), V, "too many edges in one list")
p("cta/total", lambda: cta((2, 2), i32, [2, 2], 1.0), V, "total should be an integer (or None = all edges)")
p("cta/total-bool", lambda: cta((2, 2), i32, [2, 2], True), V, "total should be an integer (or None = all edges)")
p("cta/2:counts+rows", lambda: cta((2, 3), i32, [2.5]), V, "counts should be a 1-D array of integers >= 0, the rows per image of the store")
p("cta/2:rows+total", lambda: cta((2,), i32, [2, 2], 1.5), V, "rows should be int32 [M, 2] of store rows, as the correspondence export writes them with store_rows=True")

cra = m.check_refit_args
R_SH = ((3, 4), f64, (3,), i64, (2, 3, 3), f64)
p("cra/offsets-shape", lambda: cra(*put(R_SH, 1, (0,))), V, OFF)
p("cra/offsets-2d", lambda: cra(*put(R_SH, 1, (3, 1))), V, OFF)
p("cra/offsets-dtype", lambda: cra(*put(R_SH, 1, None, i32)), V, OFF)
p("cra/model", lambda: cra(*R_SH, "X"), V, MODEL)
p("cra/models-shape", lambda: cra(*put(R_SH, 2, (2, 9))), V, MODELS_PAIR)
p("cra/px_th", lambda: cra(*R_SH, "F", -1), V, PX_POS)
p("cra/error_type", lambda: cra(*R_SH, "F", None, "bad"), V, ET_F)
p("cra/pts-shape", lambda: cra(*put(R_SH, 0, (3, 2))), V, PTS)
p("cra/pts-dtype", lambda: cra(*put(R_SH, 0, None, np.float32)), V, PTS)
p("cra/pts-big", lambda: cra(*put(R_SH, 0, (2 ** 30, 4))), V, LIST_BIG)
p("cra/max_fits-neg", lambda: cra(*R_SH, max_fits=-1), V, "max_fits should be an integer >= 0")
p("cra/max_fits-float", lambda: cra(*R_SH, max_fits=2.0), V, "max_fits should be an integer >= 0")
p("cra/max_fits-bool", lambda: cra(*R_SH, max_fits=True), V, "max_fits should be an integer >= 0")
p("cra/2:offsets+models", lambda: cra(*put(put(R_SH, 1, None, i32), 2, (2, 9))), V, OFF)
p("cra/2:models+pts", lambda: cra(*put(put(R_SH, 2, None, np.float32), 0, (3, 2))), V, MODELS_DT)
p("cra/2:pts+max_fits", lambda: cra(*put(R_SH, 0, (3, 2)), max_fits=-1), V, PTS)

cpa = m.check_pose_args
PR2 = ((2, 2), i64)
p("cpa/offsets", lambda: cpa(*put(POSE_SH, 1, None, i32)), V, OFF)
p("cpa/models-shape", lambda: cpa(*put(POSE_SH, 2, (3, 3, 3))), V, POSE_MODELS)
p("cpa/models-dtype", lambda: cpa(*put(POSE_SH, 2, None, np.float32)), V, POSE_MODELS)
p("cpa/pts", lambda: cpa(*put(POSE_SH, 0, (3, 3))), V, PTS)
p("cpa/pts-big", lambda: cpa(*put(POSE_SH, 0, (2 ** 30, 4))), V, LIST_BIG)
p("cpa/cams1-dtype", lambda: cpa(*put(POSE_SH, 3, None, np.float32)), V, "cams1 should be float64")
p("cpa/cams1-k8", lambda: cpa(*put(POSE_SH, 3, (2, 4))), V, CAMS8)
p("cpa/cams2-no-pairs", lambda: cpa(*POSE_SH, None, ((2, 4), f64)), V, "cams2 names a second store: give pairs too")
p("cpa/pairs-shape", lambda: cpa(*POSE_SH_P, ((3, 2), i64)), V, PAIRS_ARR)
p("cpa/pairs-dtype", lambda: cpa(*POSE_SH_P, ((2, 2), np.int16)), V, PAIRS_ARR)
p("cpa/cams1-n4", lambda: cpa(*POSE_SH, PR2), V, CAMS1)
p("cpa/cams2-shape", lambda: cpa(*POSE_SH_P, PR2, ((2, 8), f64)), V, CAMS2)
p("cpa/cams2-dtype", lambda: cpa(*POSE_SH_P, PR2, ((2, 4), np.float32)), V, CAMS2)
p("cpa/cameras-big", lambda: cpa(*put(POSE_SH_P, 3, (2 ** 31, 4)), PR2), V, "too many cameras")
p("cpa/keep-shape", lambda: cpa(*POSE_SH, None, None, ((2,), np.bool_)), V, KEEP_CAP)
p("cpa/keep-dtype", lambda: cpa(*POSE_SH, None, None, ((3,), i32)), V, KEEP_CAP)
p("cpa/parallax-str", lambda: cpa(*POSE_SH, min_parallax_deg="x"), V, PARALLAX)
p("cpa/parallax-bool", lambda: cpa(*POSE_SH, min_parallax_deg=True), V, PARALLAX)
p("cpa/parallax-181", lambda: cpa(*POSE_SH, min_parallax_deg=181), V, PARALLAX)
p("cpa/parallax-nan", lambda: cpa(*POSE_SH, min_parallax_deg=float("nan")), V, PARALLAX)
p("cpa/2:offsets+pts", lambda: cpa(*put(put(POSE_SH, 1, (0,)), 0, (3, 3))), V, OFF)
p("cpa/2:models+pts", lambda: cpa(*put(put(POSE_SH, 2, (2, 9)), 0, (3, 3))), V, POSE_MODELS)
p("cpa/2:pts+cams1", lambda: cpa(*put(put(POSE_SH, 0, (3, 3)), 3, None, np.float32)), V, PTS)
p("cpa/2:cams1+keep", lambda: cpa(*put(POSE_SH, 3, (2, 4)), None, None, ((2,), np.bool_)), V, CAMS8)
p("cpa/2:pairs+cams2", lambda: cpa(*POSE_SH_P, ((3, 2), i64), ((2, 8), f64)), V, PAIRS_ARR)
p("cpa/2:keep+parallax", lambda: cpa(*POSE_SH, None, None, ((2,), np.bool_), -1), V, KEEP_CAP)

cfa = m.check_refine_args
p("cfa/R-shape", lambda: cfa(*put(REFINE_SH, 2, (2, 9))), V, R_K)
p("cfa/R-K", lambda: cfa(*put(REFINE_SH, 2, (3, 3, 3))), V, R_K)
p("cfa/R-dtype", lambda: cfa(*put(REFINE_SH, 2, None, np.float32)), V, R_K)
p("cfa/t-shape", lambda: cfa(*put(REFINE_SH, 3, (2, 4))), V, T_K)
p("cfa/t-K", lambda: cfa(*put(REFINE_SH, 3, (3, 3))), V, T_K)
p("cfa/t-dtype", lambda: cfa(*put(REFINE_SH, 3, None, np.float32)), V, T_K)
p("cfa/offsets", lambda: cfa(*put(REFINE_SH, 1, (3, 1))), V, OFF)
p("cfa/pts", lambda: cfa(*put(REFINE_SH, 0, (3, 3))), V, PTS)
p("cfa/cams1", lambda: cfa(*put(REFINE_SH, 4, (2, 4))), V, CAMS8)
p("cfa/keep", lambda: cfa(*REFINE_SH, None, None, ((3,), f64)), V, KEEP_CAP)
p("cfa/max_trials-101", lambda: cfa(*REFINE_SH, max_trials=101), V, TRIALS)
p("cfa/max_trials-float", lambda: cfa(*REFINE_SH, max_trials=2.0), V, TRIALS)
p("cfa/max_trials-bool", lambda: cfa(*REFINE_SH, max_trials=True), V, TRIALS)
p("cfa/ftol-neg", lambda: cfa(*REFINE_SH, ftol=-1.0), V, FTOL)
p("cfa/ftol-str", lambda: cfa(*REFINE_SH, ftol="x"), V, FTOL)
p("cfa/ftol-nan", lambda: cfa(*REFINE_SH, ftol=float("nan")), V, FTOL)
p("cfa/2:R+t", lambda: cfa(*put(put(REFINE_SH, 2, (2, 9)), 3, (2, 4))), V, R_K)
p("cfa/2:t+offsets", lambda: cfa(*put(put(REFINE_SH, 3, (2, 4)), 1, None, i32)), V, T_K)
p("cfa/2:pts+max_trials", lambda: cfa(*put(REFINE_SH, 0, (3, 3)), max_trials=-1), V, PTS)
p("cfa/2:max_trials+ftol", lambda: cfa(*REFINE_SH, max_trials=-1, ftol=-1), V, TRIALS)

cga3 = m.check_triangulate_args
TRI_OFF = "track_offsets should be int64 [T + 1], as the tracks call returns it"
TRI_OBS = "obs should be int32 [M] of store rows, as the tracks call returns it"
TRI_IMG = "obs_image should be int32 [M], one image per element of obs"
TRI_KPS = "kps should be float64 [rows, >= 2] with x, y in front, one row per row of the store"
TRI_CAMS = "cams should be float64 [n_images, 4] = fx, fy, cx, cy per image"
TRI_R = "R should be float64 [n_images, 3, 3], one world-to-camera rotation per row of cams"
TRI_T = "t should be float64 [n_images, 3], X_cam = R X + t"
TRI_NT = "n_tracks should be int64 [1], as the tracks call returns it (or None = all T)"
TRI_ANG = "min_angle_deg should be a number in [0, 180]"
TRI_PX = "max_reproj_px should be a number >= 0"
TRI_IT = "max_iters should be an integer in 0 .. 100"
p("tri/offsets", lambda: cga3(*put(TRI_SH, 0, (0,))), V, TRI_OFF)
p("tri/offsets-dtype", lambda: cga3(*put(TRI_SH, 0, None, i32)), V, TRI_OFF)
p("tri/obs", lambda: cga3(*put(TRI_SH, 1, (2, 1))), V, TRI_OBS)
p("tri/obs-dtype", lambda: cga3(*put(TRI_SH, 1, None, i64)), V, TRI_OBS)
p("tri/obs_image", lambda: cga3(*put(TRI_SH, 2, (3,))), V, TRI_IMG)
p("tri/obs_image-dtype", lambda: cga3(*put(TRI_SH, 2, None, i64)), V, TRI_IMG)
p("tri/too-many", lambda: cga3(*put(put(TRI_SH, 1, (2 ** 30,)), 2, (2 ** 30,))), V, "too many tracks or observations")
p("tri/kps", lambda: cga3(*put(TRI_SH, 3, (4, 1))), V, TRI_KPS)
p("tri/kps-dtype", lambda: cga3(*put(TRI_SH, 3, None, np.float32)), V, TRI_KPS)
p("tri/cams", lambda: cga3(*put(TRI_SH, 4, (2, 8))), V, TRI_CAMS)
p("tri/R", lambda: cga3(*put(TRI_SH, 5, (3, 3, 3))), V, TRI_R)
p("tri/t", lambda: cga3(*put(TRI_SH, 6, None, np.float32)), V, TRI_T)
p("tri/n_tracks", lambda: cga3(*TRI_SH, ((2,), i64)), V, TRI_NT)
p("tri/n_tracks-dtype", lambda: cga3(*TRI_SH, ((1,), i32)), V, TRI_NT)
p("tri/angle", lambda: cga3(*TRI_SH, None, 181.0), V, TRI_ANG)
p("tri/angle-bool", lambda: cga3(*TRI_SH, None, True), V, TRI_ANG)
p("tri/reproj", lambda: cga3(*TRI_SH, None, 1.5, -1.0), V, TRI_PX)
p("tri/reproj-str", lambda: cga3(*TRI_SH, None, 1.5, "x"), V, TRI_PX)
p("tri/max_iters", lambda: cga3(*TRI_SH, None, 1.5, 4.0, 101), V, TRI_IT)
p("tri/max_iters-float", lambda: cga3(*TRI_SH, None, 1.5, 4.0, 5.0), V, TRI_IT)
p("tri/ftol", lambda: cga3(*TRI_SH, None, 1.5, 4.0, 10, -1.0), V, FTOL)
p("tri/ftol-bool", lambda: cga3(*TRI_SH, None, 1.5, 4.0, 10, False), V, FTOL)
p("tri/2:offsets+obs", lambda: cga3(*put(put(TRI_SH, 0, (0,)), 1, (2, 1))), V, TRI_OFF)
p("tri/2:obs_image+kps", lambda: cga3(*put(put(TRI_SH, 2, (3,)), 3, (4, 1))), V, TRI_IMG)
p("tri/2:cams+R", lambda: cga3(*put(put(TRI_SH, 4, (2, 8)), 5, (3, 3, 3))), V, TRI_CAMS)
p("tri/2:t+n_tracks", lambda: cga3(*put(TRI_SH, 6, (2, 4)), ((2,), i64)), V, TRI_T)
p("tri/2:angle+reproj", lambda: cga3(*TRI_SH, None, -1, -1), V, TRI_ANG)
p("tri/2:max_iters+ftol", lambda: cga3(*TRI_SH, None, 1.5, 4.0, -1, -1), V, TRI_IT)

# ---- matcher.py: the numpy calls ----
PREP = "descriptors should be arrays [n1, dim] and [n2, dim] with the same dim"
for name, fn, base in (("knn_match", m.knn_match, {}), ("match_snn", m.match_snn, {}), ("match_nn", m.match_nn, {}), ("match_mnn", m.match_mnn, {}),
                       ("match_smnn", m.match_smnn, {}), ("tentative_points", m.tentative_points, dict(kps1=X, kps2=X)),
                       ("match_fginn", m.match_fginn, dict(kps2=X))):
    b = dict(base, desc1=D, desc2=D)
    c(f"{name}/desc-1d", fn, b, dict(desc1=D[0]), V, PREP)
    c(f"{name}/desc-dim", fn, b, dict(desc2=D[:, :3]), V, PREP)
    c(f"{name}/norm", fn, b, dict(norm="l1"), V, "norm should be 'l2', 'hamming' or 'l2_u8'")
    c(f"{name}/hamming-f32", fn, b, dict(norm="hamming"), V, HAM)
    c(f"{name}/l2_u8-f32", fn, b, dict(norm="l2_u8", desc1=U), V, PREP)
    c(f"{name}/l2_u8-mixed", fn, b, dict(norm="l2_u8", desc1=U, desc2=U.astype(np.float32)), V, U8)
    c(f"{name}/l2_u8-dim", fn, b, dict(norm="l2_u8", desc1=np.zeros((2, 260), np.uint8), desc2=np.zeros((2, 260), np.uint8)), V, U8_DIM)
    c(f"{name}/2:desc+norm", fn, b, dict(desc1=D[0], norm="l1"), V, PREP)
for name, fn in (("match_snn", m.match_snn), ("tentative_points", m.tentative_points), ("match_fginn", m.match_fginn)):
    b = dict(desc1=D, desc2=D, kps2=X) if name != "match_snn" else dict(desc1=D, desc2=D)
    if name == "tentative_points": b["kps1"] = X
    c(f"{name}/ratio-str", fn, b, dict(ratio="x"), V, RATIO_NUM)
    c(f"{name}/ratio-neg", fn, b, dict(ratio=-1), V, RATIO_POS)
    c(f"{name}/mutual", fn, b, dict(mutual="both"), V, MUTUAL)
    c(f"{name}/max_dist", fn, b, dict(max_dist=-1), V, MD_POS)
    c(f"{name}/2:ratio+desc", fn, b, dict(ratio=0, desc1=D[0]), V, RATIO_POS)
c("match_nn/max_dist", m.match_nn, dict(desc1=D, desc2=D), dict(max_dist="x"), V, MD_NUM)
c("match_nn/2:max_dist+desc", m.match_nn, dict(desc1=D, desc2=D), dict(max_dist=-1, norm="l1"), V, MD_POS)
c("match_mnn/max_dist", m.match_mnn, dict(desc1=D, desc2=D), dict(max_dist=float("inf")), V, MD_POS)
c("match_mnn/2:max_dist+desc", m.match_mnn, dict(desc1=D, desc2=D), dict(max_dist=-1, desc2=D[0]), V, MD_POS)
c("match_smnn/ratio-none", m.match_smnn, dict(desc1=D, desc2=D), dict(ratio=None), V,
  "match_smnn is the ratio test in both directions: ratio should be a number (match_mnn has none)")
c("match_smnn/ratio", m.match_smnn, dict(desc1=D, desc2=D), dict(ratio=0), V, RATIO_POS)
c("match_smnn/2:ratio+max_dist", m.match_smnn, dict(desc1=D, desc2=D), dict(ratio=None, max_dist=-1), V,
  "match_smnn is the ratio test in both directions: ratio should be a number (match_mnn has none)")
c("match_fginn/mutual-ratio", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(mutual="ratio"), V, FGINN_RULE)
c("match_fginn/ratio-none", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(ratio=None), V, FGINN_RULE)
c("match_fginn/spatial_th", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(spatial_th=-1), V, "spatial_th should be finite and >= 0")
c("match_fginn/spatial_th-str", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(spatial_th="x"), V, "spatial_th should be a number")
c("match_fginn/kps2-rows", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(kps2=X[:4]), V,
  "kps2 should hold one keypoint row (x, y, ...) per row of desc2")
c("match_fginn/kps2-width", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(kps2=X[:, :1]), V,
  "kps2 should hold one keypoint row (x, y, ...) per row of desc2")
c("match_fginn/2:desc+spatial_th", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(desc1=D[0], spatial_th=-1), V, PREP)
c("match_fginn/2:spatial_th+kps2", m.match_fginn, dict(desc1=D, desc2=D, kps2=X), dict(spatial_th=-1, kps2=X[:4]), V, "spatial_th should be finite and >= 0")

c("kpts_to_xyA/width", m.kpts_to_xyA, {}, dict(kpts=np.zeros((3, 5))), V, "keypoints should be an array [n, 4] = (x, y, size, angle)")
c("kpts_to_xyA/1d", m.kpts_to_xyA, {}, dict(kpts=np.zeros(4)), V, "keypoints should be an array [n, 4] = (x, y, size, angle)")
c("quantize/dtype", m.quantize_descriptors, dict(desc=D), dict(desc=D.astype(np.float64)), V, "descriptors to quantise should be float32")
c("quantize/shape", m.quantize_descriptors, dict(desc=D), dict(desc=D[0]), V, "descriptors to quantise should be [n, dim] with 1 <= dim <= 256")
c("quantize/preset", m.quantize_descriptors, dict(desc=D), dict(preset="bad"), V, "preset should be one of rootsift, sift, unit")
c("quantize/scale", m.quantize_descriptors, dict(desc=D), dict(scale=-1), V, "scale should be finite and > 0")
c("quantize/2:dtype+preset", m.quantize_descriptors, dict(desc=D), dict(desc=U, preset="bad"), V, "descriptors to quantise should be float32")

STACK = "kps1_list, kps2_list, desc1_list and desc2_list should hold one entry per pair"
for name, fn, base in (("guided_batch", m.guided_match_batch, GBL), ("mv_batch", m.match_and_verify_batch, BL), ("fh_batch", m.match_and_verify_fh_batch, BL)):
    c(f"{name}/ratio", fn, base, dict(ratio="x"), V, RATIO_NUM)
    c(f"{name}/mutual", fn, base, dict(mutual="both"), V, MUTUAL)
    c(f"{name}/fginn-rule", fn, base, dict(ratio=None, fginn_th=3.0), V, FGINN_RULE)
    c(f"{name}/lists-len", fn, base, dict(kps2_list=[X]), V, STACK)
    c(f"{name}/no-pair", fn, base, dict(kps1_list=[], kps2_list=[], desc1_list=[], desc2_list=[]), V, PAIRS_0)
    c(f"{name}/pair-1d", fn, base, dict(desc1_list=[D[:3], D[3]]), V, PAIR_EVERY)
    c(f"{name}/pair-dtype", fn, base, dict(kps2_list=[X[:2], X[2:].astype(np.float32)]), V, PAIR_EVERY)
    c(f"{name}/pair-width", fn, base, dict(desc2_list=[D[:2], D[2:, :3]]), V, PAIR_EVERY)
    c(f"{name}/kps-rows", fn, base, dict(kps1_list=[X[:2], X[2:]]), V, KPS_ROWS)
    c(f"{name}/desc-dtypes", fn, base, dict(desc2_list=[U[:2, :4], U[2:, :4]]), V, DESC_DT)
    c(f"{name}/norm", fn, base, dict(norm="l1"), V, NORM)
    c(f"{name}/kps", fn, base, dict(kps1_list=[X[:3, :1], X[3:, :1]]), V, KPS)
    c(f"{name}/kps-layout", fn, base, dict(kps2_list=[KP[:2], KP[2:]]), V, KPS_LAYOUT)
    c(f"{name}/2:ratio+lists", fn, base, dict(ratio=0, kps2_list=[X]), V, RATIO_POS)
    c(f"{name}/2:lists+norm", fn, base, dict(desc1_list=[D[:3], D[3]], norm="l1"), V, PAIR_EVERY)
c("guided_batch/model", m.guided_match_batch, GBL, dict(model="X"), V, MODEL)
c("guided_batch/models-shape", m.guided_match_batch, GBL, dict(models=np.zeros((3, 3, 3))), V, MODELS_PAIR)
c("guided_batch/models-dtype", m.guided_match_batch, GBL, dict(models=MOD.astype(np.float32)), V, MODELS_DT)
c("guided_batch/px_th", m.guided_match_batch, GBL, dict(px_th=-1), V, PX_POS)
c("guided_batch/error_type", m.guided_match_batch, GBL, dict(error_type="bad"), V, ET_F)
c("guided_batch/fginn_th", m.guided_match_batch, GBL, dict(fginn_th=-1), V, "fginn_th should be finite and >= 0")
c("guided_batch/2:norm+models", m.guided_match_batch, GBL, dict(norm="l1", models=np.zeros((3, 3, 3))), V, NORM)
c("guided_batch/2:px_th+fginn_th", m.guided_match_batch, GBL, dict(px_th=-1, fginn_th=-1), V, PX_POS)
c("guided_match/models", m.guided_match, dict(kps1=X, kps2=X, desc1=D, desc2=D, M=np.zeros((3, 3))), dict(M=np.zeros((2, 3))), V,
  "models should be [K, 3, 3] = [1, 3, 3], one model per pair")
c("guided_match/kps-rows", m.guided_match, dict(kps1=X, kps2=X, desc1=D, desc2=D, M=np.zeros((3, 3))), dict(kps1=X[:4]), V, KPS_ROWS)
c("guided_match/2:ratio+models", m.guided_match, dict(kps1=X, kps2=X, desc1=D, desc2=D, M=np.zeros((3, 3))), dict(ratio=0, M=np.zeros((2, 3))), V, RATIO_POS)
c("mv_batch/guided_fginn_th", m.match_and_verify_batch, BL, dict(guided_fginn_th=3.0), V, GFT)
c("mv_batch/guided_fginn_th-rule", m.match_and_verify_batch, BL, dict(guided=True, guided_fginn_th=3.0, ratio=None), V, FGINN_RULE)
c("mv_batch/model", m.match_and_verify_batch, BL, dict(model="X"), V, MODEL)
c("mv_batch/fginn_th", m.match_and_verify_batch, BL, dict(fginn_th="x"), V, "fginn_th should be a number")
c("mv_batch/error_type", m.match_and_verify_batch, BL, dict(error_type="bad"), V, ET_F)
c("mv_batch/seeds", m.match_and_verify_batch, BL, dict(seeds=[1, 2, 3]), V, SEEDS)
c("mv_batch/2:guided_fginn_th+ratio", m.match_and_verify_batch, BL, dict(guided_fginn_th=3.0, ratio=0), V, GFT)
c("mv_batch/2:model+error_type", m.match_and_verify_batch, BL, dict(model="X", error_type="bad"), V, MODEL)
c("mv_batch/2:error_type+seeds", m.match_and_verify_batch, BL, dict(error_type="bad", seeds=[1]), V, ET_F)
c("fh_batch/f_params", m.match_and_verify_fh_batch, BL, dict(f_params=3), V, "f_params should be a dict of estimator keywords, or None")
c("fh_batch/seeds", m.match_and_verify_fh_batch, BL, dict(seeds=[1]), V, SEEDS)
c("fh_batch/2:norm+f_params", m.match_and_verify_fh_batch, BL, dict(norm="l1", f_params=3), V, NORM)
c("fh_batch/2:f_params+seeds", m.match_and_verify_fh_batch, BL, dict(f_params=3, seeds=[1]), V, "f_params should be a dict of estimator keywords, or None")

for name, fn, base in (("mv_pairs", m.match_and_verify_pairs, PL), ("mv_fginn_pairs", m.match_and_verify_fginn_pairs, dict(PL, fginn_th=3.0)),
                       ("fh_pairs", m.match_and_verify_fh_pairs, PL), ("guided_pairs", m.guided_match_pairs, GPL)):
    c(f"{name}/ratio", fn, base, dict(ratio=0), V, RATIO_POS)
    c(f"{name}/max_dist", fn, base, dict(max_dist="x"), V, MD_NUM)
    c(f"{name}/store2-half", fn, base, dict(kps2_list=[X]), V, "kps2_list and desc2_list go together")
    c(f"{name}/store-len", fn, base, dict(kps_list=[X]), V, "one keypoint array per descriptor array")
    c(f"{name}/store-empty", fn, base, dict(kps_list=[], desc_list=[]), V, "at least one image per store")
    c(f"{name}/image-1d", fn, base, dict(desc_list=[D[:3], D[3]]), V, IMG_EVERY)
    c(f"{name}/image-width", fn, base, dict(kps_list=[X[:3], KP[3:]]), V, IMG_EVERY)
    c(f"{name}/store2-image", fn, base, dict(kps2_list=[X[:3], X[3:]], desc2_list=[D[:3], U[3:]]), V, IMG_EVERY)
    c(f"{name}/kps-rows", fn, base, dict(kps_list=[X[:2], X[2:]]), V, KPS_ROWS)
    c(f"{name}/desc-dtype", fn, base, dict(desc_list=[D[:3].astype(np.float64), D[3:].astype(np.float64)]), V, DESC_DT)
    c(f"{name}/hamming", fn, base, dict(norm="hamming"), V, HAM)
    c(f"{name}/pairs", fn, base, dict(pairs=[[0, 1, 2]]), V, PAIRS_ARR)
    c(f"{name}/pairs-empty", fn, base, dict(pairs=np.zeros((0, 2), np.int32)), V, PAIRS_0)
    c(f"{name}/pairs-range", fn, base, dict(pairs=[[0, 2]]), V, PAIRS_RANGE)
    c(f"{name}/2:ratio+store", fn, base, dict(ratio=0, kps_list=[X]), V, RATIO_POS)
    c(f"{name}/2:store+pairs", fn, base, dict(desc_list=[D[:3], D[3]], pairs=[[0, 2]]), V, IMG_EVERY)
    c(f"{name}/2:norm+pairs", fn, base, dict(norm="l1", pairs=[[0, 2]]), V, NORM)
for name, fn, base in (("mv_pairs", m.match_and_verify_pairs, PL), ("mv_fginn_pairs", m.match_and_verify_fginn_pairs, dict(PL, fginn_th=3.0))):
    c(f"{name}/guided", fn, base, dict(guided=True), V, NO_GUIDED)
    c(f"{name}/model", fn, base, dict(model="X"), V, MODEL)
    c(f"{name}/seeds", fn, base, dict(seeds=[1]), V, SEEDS)
    c(f"{name}/error_type", fn, base, dict(error_type="bad"), V, ET_F)
    c(f"{name}/2:guided+store", fn, base, dict(guided=True, kps_list=[X]), V, "one keypoint array per descriptor array")
    c(f"{name}/2:guided+model", fn, base, dict(guided=True, model="X"), V, NO_GUIDED)
    c(f"{name}/2:seeds+error_type", fn, base, dict(seeds=[1], error_type="bad"), V, SEEDS)
c("mv_pairs/fginn_th", m.match_and_verify_pairs, PL, dict(fginn_th=3.0), V, NO_FGINN)
c("mv_pairs/2:fginn_th+rule", m.match_and_verify_pairs, PL, dict(fginn_th=3.0, ratio=None), V, NO_FGINN)
c("mv_fginn_pairs/fginn_th", m.match_and_verify_fginn_pairs, PL, dict(fginn_th=-1), V, "fginn_th should be finite and >= 0")
c("mv_fginn_pairs/rule", m.match_and_verify_fginn_pairs, PL, dict(fginn_th=3.0, mutual="ratio"), V, FGINN_RULE)
c("mv_fginn_pairs/2:fginn_th+ratio", m.match_and_verify_fginn_pairs, PL, dict(fginn_th=-1, ratio=0), V, "fginn_th should be finite and >= 0")
c("fh_pairs/fginn_th", m.match_and_verify_fh_pairs, PL, dict(fginn_th="x"), V, "fginn_th should be a number")
c("fh_pairs/rule", m.match_and_verify_fh_pairs, PL, dict(fginn_th=3.0, ratio=None), V, FGINN_RULE)
c("fh_pairs/seeds", m.match_and_verify_fh_pairs, PL, dict(seeds=[1]), V, SEEDS)
c("fh_pairs/h_params", m.match_and_verify_fh_pairs, PL, dict(h_params={"x": 1}), V,
  "h_params: unknown key x (known: px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check)")
c("fh_pairs/2:fginn_th+ratio", m.match_and_verify_fh_pairs, PL, dict(fginn_th=-1, ratio=0), V, "fginn_th should be finite and >= 0")
c("fh_pairs/2:seeds+h_params", m.match_and_verify_fh_pairs, PL, dict(seeds=[1], h_params=3), V, SEEDS)
c("guided_pairs/model", m.guided_match_pairs, GPL, dict(model="X"), V, MODEL)
c("guided_pairs/models", m.guided_match_pairs, GPL, dict(models=np.zeros((2, 9))), V, MODELS_PAIR)
c("guided_pairs/px_th", m.guided_match_pairs, GPL, dict(px_th="x"), V, PX_NUM)
c("guided_pairs/fginn_th", m.guided_match_pairs, GPL, dict(fginn_th=-1), V, "fginn_th should be finite and >= 0")
c("guided_pairs/rule", m.guided_match_pairs, GPL, dict(fginn_th=3.0, ratio=None), V, FGINN_RULE)
c("guided_pairs/2:pairs+models", m.guided_match_pairs, GPL, dict(pairs=[[0, 2]], models=np.zeros((2, 9))), V, PAIRS_RANGE)
c("guided_pairs/2:models+fginn_th", m.guided_match_pairs, GPL, dict(models=np.zeros((2, 9)), fginn_th=-1), V, MODELS_PAIR)

KL = [X[:3], X[3:]]
c("corr_pairs/no-pairs", m.correspondences_pairs, CN, dict(pairs=None), V, PAIRS_ARR)
c("corr_pairs/kps2-alone", m.correspondences_pairs, CN, dict(kps2_list=KL), V, "kps2_list names a second store: give kps_list too")
c("corr_pairs/kps-image", m.correspondences_pairs, CN, dict(kps_list=[X[:3], X[3]]), V,
  "every image's keypoints should be 2-D with the dtype and width of image 0 (at least one image per store)")
c("corr_pairs/kps-empty", m.correspondences_pairs, CN, dict(kps_list=[]), V,
  "every image's keypoints should be 2-D with the dtype and width of image 0 (at least one image per store)")
c("corr_pairs/match", m.correspondences_pairs, CN, dict(match=MATCH[:4]), V, MATCH_N)
c("corr_pairs/keep", m.correspondences_pairs, CN, dict(keep=np.zeros(5)), V, KEEP_N)
c("corr_pairs/kps-rows", m.correspondences_pairs, CN, dict(kps_list=[X[:3], X[3:4]]), V, "counts do not add up to the number of keypoint rows")
c("corr_pairs/models-no-kps", m.correspondences_pairs, CN, dict(models=MOD), V, "models (the residuals) need kps1 and kps2")
c("corr_pairs/models", m.correspondences_pairs, CN, dict(kps_list=KL, models=np.zeros((2, 9))), V, MODELS_ENTRY)
c("corr_pairs/model", m.correspondences_pairs, CN, dict(model="X"), V, MODEL)
c("corr_pairs/pairs-range", m.correspondences_pairs, CN, dict(pairs=[[0, 2]]), V, PAIRS_RANGE)
c("corr_pairs/2:kps2+model", m.correspondences_pairs, CN, dict(kps2_list=KL, model="X"), V, "kps2_list names a second store: give kps_list too")
c("corr_pairs/2:kps-image+match", m.correspondences_pairs, CN, dict(kps_list=[], match=MATCH[:4]), V,
  "every image's keypoints should be 2-D with the dtype and width of image 0 (at least one image per store)")
c("corr_pairs/2:counts+match", m.correspondences_pairs, CN, dict(counts1=[3.0, 2.0], match=MATCH[:4]), V, CNT12)
CNB = dict(match=MATCH, counts1=C1, counts2=C2)
c("corr_batch/kps-one", m.correspondences_batch, CNB, dict(kps1_list=KL), V, "kps1_list and kps2_list go together")
c("corr_batch/counts-len", m.correspondences_batch, CNB, dict(counts2=[5]), V, "counts1 and counts2 should have one entry per pair")
c("corr_batch/match", m.correspondences_batch, CNB, dict(match=MATCH.astype(np.int64)), V, MATCH_N)
c("corr_batch/2:kps+counts", m.correspondences_batch, CNB, dict(kps1_list=KL, counts2=[5]), V, "kps1_list and kps2_list go together")

c("tracks/counts", m.tracks, dict(rows=ROWS, counts=[2, 2]), dict(counts=[2, -2]), V, "counts should be a 1-D array of integers >= 0, the rows per image of the store")
c("tracks/rows", m.tracks, dict(rows=ROWS, counts=[2, 2]), dict(rows=ROWS.astype(np.int64)), V,
  "rows should be int32 [M, 2] of store rows, as the correspondence export writes them with store_rows=True")
c("tracks/total", m.tracks, dict(rows=ROWS, counts=[2, 2]), dict(total=1.5), V, "total should be an integer (or None = all edges)")
c("tracks/2:counts+total", m.tracks, dict(rows=ROWS, counts=[2, 2]), dict(counts=[2.5], total=1.5), V,
  "counts should be a 1-D array of integers >= 0, the rows per image of the store")

c("refit/offsets", m.refit_correspondences, RN, dict(corr_offsets=OFFS.astype(np.int32)), V, OFF)
c("refit/models", m.refit_correspondences, RN, dict(models=np.zeros((2, 9))), V, MODELS_PAIR)
c("refit/model", m.refit_correspondences, RN, dict(model="X"), V, MODEL)
c("refit/pts", m.refit_correspondences, RN, dict(pts=PTS4[:, :3]), V, PTS)
c("refit/max_fits", m.refit_correspondences, RN, dict(max_fits=-1), V, "max_fits should be an integer >= 0")
c("refit/error_type", m.refit_correspondences, RN, dict(error_type="bad", model="H"), V, ET_H)
c("refit/2:offsets+pts", m.refit_correspondences, RN, dict(corr_offsets=OFFS[:0], pts=PTS4[:, :3]), V, OFF)
c("refit/2:models+max_fits", m.refit_correspondences, RN, dict(models=np.zeros((2, 9)), max_fits=-1), V, MODELS_PAIR)

c("pose/offsets", m.relative_pose, PN, dict(corr_offsets=OFFS.astype(np.int32)), V, OFF)
c("pose/models", m.relative_pose, PN, dict(models=np.zeros((2, 9))), V, POSE_MODELS)
c("pose/pts", m.relative_pose, PN, dict(pts=PTS4[:, :3]), V, PTS)
c("pose/cams1-dtype", m.relative_pose, PN, dict(cams1=CAM8.astype(np.float32)), V, "cams1 should be float64")
c("pose/cams1", m.relative_pose, PN, dict(cams1=CAM4), V, CAMS8)
c("pose/cams2", m.relative_pose, PN, dict(cams2=CAM4), V, "cams2 names a second store: give pairs too")
c("pose/pairs", m.relative_pose, PN, dict(cams1=CAM4, pairs=[[0, 1]]), V, PAIRS_ARR)
c("pose/pairs-cams1", m.relative_pose, PN, dict(pairs=PAIRS), V, CAMS1)
c("pose/pairs-cams2", m.relative_pose, PN, dict(cams1=CAM4, pairs=PAIRS, cams2=CAM8), V, CAMS2)
c("pose/keep", m.relative_pose, PN, dict(keep=np.zeros(2, bool)), V, KEEP_CAP)
c("pose/parallax", m.relative_pose, PN, dict(min_parallax_deg=-1), V, PARALLAX)
c("pose/2:models+cams1", m.relative_pose, PN, dict(models=np.zeros((2, 9)), cams1=CAM4), V, POSE_MODELS)
c("pose/2:pairs+keep", m.relative_pose, PN, dict(cams1=CAM4, pairs=[[0, 1]], keep=np.zeros(2, bool)), V, PAIRS_ARR)

c("refine/unknown", m.refine_pose, FN, dict(max_trails=3), V, "refine_pose: unknown keyword 'max_trails'")
c("refine/R", m.refine_pose, FN, dict(R=np.zeros((2, 9))), V, R_K)
c("refine/t", m.refine_pose, FN, dict(t=np.zeros((3, 3))), V, T_K)
c("refine/offsets", m.refine_pose, FN, dict(corr_offsets=OFFS.astype(np.int32)), V, OFF)
c("refine/cams1", m.refine_pose, FN, dict(cams1=CAM4), V, CAMS8)
c("refine/max_trials", m.refine_pose, FN, dict(max_trials=101), V, TRIALS)
c("refine/ftol", m.refine_pose, FN, dict(ftol=-1.0), V, FTOL)
c("refine/2:unknown+R", m.refine_pose, FN, dict(zz=1, R=np.zeros((2, 9))), V, "refine_pose: unknown keyword 'zz'")
c("refine/2:R+ftol", m.refine_pose, FN, dict(R=np.zeros((2, 9)), ftol=-1.0), V, R_K)

c("triangulate/unknown", m.triangulate_tracks, TN, dict(max_iter=3), V, "triangulate_tracks: unknown keyword 'max_iter'")
c("triangulate/n_tracks", m.triangulate_tracks, TN, dict(n_tracks=1.0), V, "n_tracks should be an integer (or None = all T)")
c("triangulate/n_tracks-bool", m.triangulate_tracks, TN, dict(n_tracks=True), V, "n_tracks should be an integer (or None = all T)")
c("triangulate/offsets", m.triangulate_tracks, TN, dict(track_offsets=TO.astype(np.int32)), V, TRI_OFF)
c("triangulate/obs_image", m.triangulate_tracks, TN, dict(obs_image=OI[:1]), V, TRI_IMG)
c("triangulate/kps", m.triangulate_tracks, TN, dict(kps=KX[:, :1]), V, TRI_KPS)
c("triangulate/R", m.triangulate_tracks, TN, dict(R=np.zeros((2, 9))), V, TRI_R)
c("triangulate/max_iters", m.triangulate_tracks, TN, dict(max_iters=101), V, TRI_IT)
c("triangulate/2:n_tracks+offsets", m.triangulate_tracks, TN, dict(n_tracks=1.0, track_offsets=TO.astype(np.int32)), V,
  "n_tracks should be an integer (or None = all T)")
c("triangulate/2:kps+ftol", m.triangulate_tracks, TN, dict(kps=KX[:, :1], ftol=-1.0), V, TRI_KPS)

# ---- tensor_api.py: CPU tensors reach every check in front of the device refusal ----
XT = dict(pts1=T(X), pts2=T(X), counts=[5])
for name, fn in (("find_f_t", t.find_fundamental_batch_tensors), ("find_h_t", t.find_homography_batch_tensors)):
    c(f"{name}/error_type", fn, XT, dict(error_type="bad"), KeyError, "'bad'")
    c(f"{name}/not-tensors", fn, XT, dict(pts1=X), V, "pts1/pts2 must be torch tensors on the GPU")
    c(f"{name}/device", fn, XT, {}, V, "pts1/pts2 must live on the same ROCm device")
    c(f"{name}/2:error_type+tensors", fn, XT, dict(error_type="bad", pts1=X), KeyError, "'bad'")
    c(f"{name}/2:device+counts", fn, XT, dict(pts1=T(X.astype(np.float32)), counts=[4]), V, "pts1/pts2 must live on the same ROCm device")
c("knn_t/not-tensors", t.knn_match_tensors, dict(desc1=T(D), desc2=T(D)), dict(desc2=D), V, DESC_DEV)
c("knn_t/device", t.knn_match_tensors, dict(desc1=T(D), desc2=T(D)), {}, V, DESC_DEV)
c("knn_t/2:device+norm", t.knn_match_tensors, dict(desc1=T(D), desc2=T(D)), dict(norm="l1"), V, DESC_DEV)
DEC = dict(idx=T(np.zeros((5, 2), np.int32)), dist=T(np.zeros((5, 2), np.float32)))
BACK = "back_ratio=True needs back and back_dist, the idx and dist of the reverse search"
c("decide_t/back_ratio", t.match_decide_tensors, DEC, dict(back_ratio=True), V, BACK)
c("decide_t/back_ratio-no-dist", t.match_decide_tensors, DEC, dict(back_ratio=True, back=DEC["idx"]), V, BACK)
c("decide_t/ratio", t.match_decide_tensors, DEC, dict(ratio="x"), V, RATIO_NUM)
c("decide_t/back_ratio-ratio-none", t.match_decide_tensors, DEC, dict(ratio=None, back_ratio=True, back=DEC["idx"], back_dist=DEC["dist"]), V, MUTUAL_NONE)
c("decide_t/max_dist", t.match_decide_tensors, DEC, dict(max_dist=-1), V, MD_POS)
c("decide_t/2:back_ratio+ratio", t.match_decide_tensors, DEC, dict(back_ratio=True, ratio=0), V, BACK)
c("decide_t/2:ratio+max_dist", t.match_decide_tensors, DEC, dict(ratio=0, max_dist=-1), V, RATIO_POS)
SNN = dict(desc1=T(D), desc2=T(D))
c("snn_t/ratio", t.match_snn_tensors, SNN, dict(ratio="x"), V, RATIO_NUM)
c("snn_t/mutual", t.match_snn_tensors, SNN, dict(mutual="both"), V, MUTUAL)
c("snn_t/mutual-ratio-none", t.match_snn_tensors, SNN, dict(ratio=None, mutual="ratio"), V, MUTUAL_NONE)
c("snn_t/max_dist", t.match_snn_tensors, SNN, dict(max_dist="x"), V, MD_NUM)
c("snn_t/device", t.match_snn_tensors, SNN, {}, V, DESC_DEV)
c("snn_t/device-decide", t.match_snn_tensors, SNN, dict(ratio=None), V, DESC_DEV)
c("snn_t/2:ratio+device", t.match_snn_tensors, SNN, dict(ratio=0, desc1=D), V, RATIO_POS)
KPT = "keypoints should be a float32 tensor [n, 4] = (x, y, size, angle) on a ROCm device"
c("kpts_t/device", t.kpts_to_xyA_tensors, dict(kpts=T(KP)), {}, V, KPT)
c("kpts_t/not-tensor", t.kpts_to_xyA_tensors, dict(kpts=KP), {}, V, KPT)
c("kpts_t/2:device+shape", t.kpts_to_xyA_tensors, dict(kpts=T(X)), {}, V, KPT)
c("quantize_t/device", t.quantize_descriptors_tensors, dict(desc=T(D)), {}, V, "descriptors must be a torch tensor on a ROCm device")
c("quantize_t/not-tensor", t.quantize_descriptors_tensors, dict(desc=D), {}, V, "descriptors must be a torch tensor on a ROCm device")
c("quantize_t/2:device+preset", t.quantize_descriptors_tensors, dict(desc=T(D)), dict(preset="bad"), V, "descriptors must be a torch tensor on a ROCm device")

for name, fn, base, cnt in (("knn_batch_t", t.knn_match_batch_tensors, KB, CNT_PAIR), ("knn_pairs_t", t.knn_match_pairs_tensors, KPR, CNT_IMG)):
    c(f"{name}/not-tensors", fn, base, dict(desc1=D), V, DESC_T)
    c(f"{name}/desc", fn, base, dict(desc2=T(D[:, :3])), V, DESC)
    c(f"{name}/desc-dtypes", fn, base, dict(desc2=T(U[:, :4])), V, DESC_DT)
    c(f"{name}/norm", fn, base, dict(norm="l1"), V, NORM)
    c(f"{name}/l2-u8", fn, base, dict(norm="l2", desc1=T(U), desc2=T(U)), V, L2)
    c(f"{name}/l2_u8-f32", fn, base, dict(norm="l2_u8"), V, U8)
    c(f"{name}/counts-2d", fn, base, dict(counts1=[[3, 2]]), V, cnt)
    c(f"{name}/counts-sum", fn, base, dict(counts2=[1, 1]), V, CNT_SUM)
    c(f"{name}/device", fn, base, {}, V, DESC_DEV)
    c(f"{name}/2:tensors+norm", fn, base, dict(desc1=D, norm="l1"), V, DESC_T)
    c(f"{name}/2:norm+counts", fn, base, dict(norm="l1", counts2=[1, 1]), V, NORM)
    c(f"{name}/2:counts+device", fn, base, dict(counts1=[6, -1]), V, CNT_NEG)
c("knn_batch_t/counts-len", t.knn_match_batch_tensors, KB, dict(counts2=[5]), V, CNT_PAIR)
c("knn_pairs_t/pairs", t.knn_match_pairs_tensors, KPR, dict(pairs=[0, 1]), V, PAIRS_ARR)
c("knn_pairs_t/pairs-range", t.knn_match_pairs_tensors, KPR, dict(pairs=[[2, 0]]), V, PAIRS_RANGE)
c("knn_pairs_t/2:counts+pairs", t.knn_match_pairs_tensors, KPR, dict(counts2=[1, 1], pairs=[0, 1]), V, CNT_SUM)
for name, fn, base in (("fginn_batch_t", t.knn_match_fginn_batch_tensors, FB), ("fginn_pairs_t", t.knn_match_fginn_pairs_tensors, FP)):
    c(f"{name}/not-tensors", fn, base, dict(kps2=X), V, T3)
    c(f"{name}/spatial_th", fn, base, dict(spatial_th="x"), V, "spatial_th should be a number")
    c(f"{name}/spatial_th-neg", fn, base, dict(spatial_th=-1), V, "spatial_th should be finite and >= 0")
    c(f"{name}/kps2-dtype", fn, base, dict(kps2=T(KP)), V, KPS_XY)
    c(f"{name}/kps2-width", fn, base, dict(kps2=T(np.zeros((5, 3)))), V, KPS_XY)
    c(f"{name}/kps2-rows", fn, base, dict(kps2=T(X[:4])), V, KPS_ROWS)
    c(f"{name}/norm", fn, base, dict(norm="l1"), V, NORM)
    c(f"{name}/counts", fn, base, dict(counts1=[3.0, 2.0]), V, CNT_INT)
    c(f"{name}/kps2-device", fn, base, dict(kps2=META), V, T3_DEV)
    c(f"{name}/device", fn, base, {}, V, DESC_DEV)
    c(f"{name}/2:tensors+spatial_th", fn, base, dict(kps2=X, spatial_th=-1), V, T3)
    c(f"{name}/2:spatial_th+kps2", fn, base, dict(spatial_th=-1, kps2=T(KP)), V, "spatial_th should be finite and >= 0")
    c(f"{name}/2:kps2+norm", fn, base, dict(kps2=T(KP), norm="l1"), V, KPS_XY)
    c(f"{name}/2:counts+kps2-device", fn, base, dict(counts1=[3.0, 2.0], kps2=META), V, CNT_INT)
c("fginn_pairs_t/pairs", t.knn_match_fginn_pairs_tensors, FP, dict(pairs=np.zeros((0, 2), np.int64)), V, PAIRS_0)

for name, fn, base, txt, dev in (("guided_batch_t", t.guided_match_batch_tensors, GB, T5, T5_DEV), ("guided_pairs_t", t.guided_match_pairs_tensors, GP, T5, T5_DEV),
                                 ("mv_batch_t", t.match_and_verify_batch_tensors, BT, T4, T4_DEV), ("mv_pairs_t", t.match_and_verify_pairs_tensors, PT, T4, T4_DEV),
                                 ("mv_fginn_pairs_t", t.match_and_verify_fginn_pairs_tensors, dict(PT, fginn_th=3.0), T4, T4_DEV),
                                 ("fh_batch_t", t.match_and_verify_fh_batch_tensors, BT, T4, T4_DEV), ("fh_pairs_t", t.match_and_verify_fh_pairs_tensors, PT, T4, T4_DEV)):
    c(f"{name}/ratio", fn, base, dict(ratio="x"), V, RATIO_NUM)
    c(f"{name}/mutual", fn, base, dict(mutual="both"), V, MUTUAL)
    c(f"{name}/max_dist", fn, base, dict(max_dist=-1), V, MD_POS)
    c(f"{name}/not-tensors", fn, base, dict(kps1=X), V, txt)
    c(f"{name}/desc", fn, base, dict(desc1=T(D[:, :3])), V, DESC)
    c(f"{name}/desc-dtypes", fn, base, dict(desc1=T(U[:, :4])), V, DESC_DT)
    c(f"{name}/norm", fn, base, dict(norm="l1"), V, NORM)
    c(f"{name}/hamming", fn, base, dict(norm="hamming"), V, HAM)
    c(f"{name}/kps", fn, base, dict(kps1=T(np.zeros((5, 3)))), V, KPS)
    c(f"{name}/kps-layout", fn, base, dict(kps2=T(KP)), V, KPS_LAYOUT)
    c(f"{name}/kps-rows", fn, base, dict(kps2=T(X[:4])), V, KPS_ROWS)
    c(f"{name}/counts-float", fn, base, dict(counts1=[3.0, 2.0]), V, CNT_INT)
    c(f"{name}/counts-sum", fn, base, dict(counts2=[1, 1]), V, CNT_SUM)
    c(f"{name}/other-device", fn, base, dict(kps2=META), V, dev)
    c(f"{name}/2:ratio+tensors", fn, base, dict(ratio=0, kps1=X), V, RATIO_POS)
    c(f"{name}/2:tensors+norm", fn, base, dict(kps1=X, norm="l1"), V, txt)
    c(f"{name}/2:norm+device", fn, base, dict(norm="l1", kps2=META), V, NORM)
for name, fn, base in (("guided_batch_t", t.guided_match_batch_tensors, GB), ("guided_pairs_t", t.guided_match_pairs_tensors, GP)):
    c(f"{name}/model", fn, base, dict(model="X"), V, MODEL)
    c(f"{name}/models-shape", fn, base, dict(models=T(np.zeros((2, 9)))), V, MODELS_PAIR)
    c(f"{name}/models-dtype", fn, base, dict(models=T(MOD.astype(np.float32))), V, MODELS_DT)
    c(f"{name}/px_th", fn, base, dict(px_th=-1), V, PX_POS)
    c(f"{name}/error_type", fn, base, dict(error_type="bad"), V, ET_F)
    c(f"{name}/fginn_th", fn, base, dict(fginn_th=-1), V, "fginn_th should be finite and >= 0")
    c(f"{name}/rule", fn, base, dict(fginn_th=3.0, mutual="ratio"), V, FGINN_RULE)
    c(f"{name}/device", fn, base, {}, V, T5_DEV)
    c(f"{name}/2:counts+models", fn, base, dict(counts2=[1, 1], models=T(np.zeros((2, 9)))), V, CNT_SUM)
    c(f"{name}/2:models+fginn_th", fn, base, dict(models=T(np.zeros((2, 9))), fginn_th=-1), V, MODELS_PAIR)
    c(f"{name}/2:fginn_th+device", fn, base, dict(fginn_th=-1, kps2=META), V, "fginn_th should be finite and >= 0")
c("guided_batch_t/counts-len", t.guided_match_batch_tensors, GB, dict(counts2=[5]), V, CNT_PAIR)
c("guided_pairs_t/pairs-range", t.guided_match_pairs_tensors, GP, dict(pairs=[[0, 2]]), V, PAIRS_RANGE)
c("guided_pairs_t/2:pairs+models", t.guided_match_pairs_tensors, GP, dict(pairs=[[0, 2]], models=T(np.zeros((2, 9)))), V, PAIRS_RANGE)
for name, fn, base in (("mv_batch_t", t.match_and_verify_batch_tensors, BT), ("mv_pairs_t", t.match_and_verify_pairs_tensors, PT),
                       ("mv_fginn_pairs_t", t.match_and_verify_fginn_pairs_tensors, dict(PT, fginn_th=3.0))):
    c(f"{name}/model", fn, base, dict(model="X"), V, MODEL)
    c(f"{name}/device", fn, base, {}, V, DESC_DEV)
    c(f"{name}/error_type", fn, base, dict(error_type="bad"), V, ET_F)
    c(f"{name}/2:device+error_type", fn, base, dict(kps2=META, error_type="bad"), V, T4_DEV)
c("mv_batch_t/guided_fginn_th", t.match_and_verify_batch_tensors, BT, dict(guided_fginn_th=3.0), V, GFT)
c("mv_batch_t/guided_fginn_th-rule", t.match_and_verify_batch_tensors, BT, dict(guided=True, guided_fginn_th=3.0, mutual="ratio"), V, FGINN_RULE)
c("mv_batch_t/fginn_th", t.match_and_verify_batch_tensors, BT, dict(fginn_th=-1), V, "fginn_th should be finite and >= 0")
c("mv_batch_t/counts-len", t.match_and_verify_batch_tensors, BT, dict(counts2=[5]), V, CNT_PAIR)
c("mv_batch_t/seeds", t.match_and_verify_batch_tensors, BT, dict(seeds=[1]), V, DESC_DEV)
c("mv_batch_t/2:guided_fginn_th+ratio", t.match_and_verify_batch_tensors, BT, dict(guided_fginn_th=3.0, ratio=0), V, GFT)
c("mv_batch_t/2:fginn_th+model", t.match_and_verify_batch_tensors, BT, dict(fginn_th=-1, model="X"), V, "fginn_th should be finite and >= 0")
for name, fn, base in (("mv_pairs_t", t.match_and_verify_pairs_tensors, PT), ("mv_fginn_pairs_t", t.match_and_verify_fginn_pairs_tensors, dict(PT, fginn_th=3.0))):
    c(f"{name}/guided", fn, base, dict(guided=True), V, NO_GUIDED)
    c(f"{name}/pairs", fn, base, dict(pairs=[[0.5, 1]]), V, PAIRS_ARR)
    c(f"{name}/pairs-range", fn, base, dict(pairs=[[-1, 0]]), V, PAIRS_RANGE)
    c(f"{name}/seeds", fn, base, dict(seeds=[1]), V, SEEDS)
    c(f"{name}/2:guided+tensors", fn, base, dict(guided=True, kps1=X), V, T4)
    c(f"{name}/2:pairs+seeds", fn, base, dict(pairs=[[0, 2]], seeds=[1]), V, PAIRS_RANGE)
    c(f"{name}/2:seeds+device", fn, base, dict(seeds=[1], kps2=META), V, SEEDS)
c("mv_pairs_t/fginn_th", t.match_and_verify_pairs_tensors, PT, dict(fginn_th=3.0), V, NO_FGINN)
c("mv_pairs_t/2:guided+fginn_th", t.match_and_verify_pairs_tensors, PT, dict(guided=True, fginn_th=3.0), V, NO_GUIDED)
c("mv_fginn_pairs_t/fginn_th", t.match_and_verify_fginn_pairs_tensors, PT, dict(fginn_th="x"), V, "fginn_th should be a number")
c("mv_fginn_pairs_t/rule", t.match_and_verify_fginn_pairs_tensors, PT, dict(fginn_th=3.0, ratio=None), V, FGINN_RULE)
c("mv_fginn_pairs_t/2:fginn_th+ratio", t.match_and_verify_fginn_pairs_tensors, PT, dict(fginn_th=-1, ratio=0), V, "fginn_th should be finite and >= 0")
for name, fn, base in (("fh_batch_t", t.match_and_verify_fh_batch_tensors, BT), ("fh_pairs_t", t.match_and_verify_fh_pairs_tensors, PT)):
    c(f"{name}/fginn_th", fn, base, dict(fginn_th=-1), V, "fginn_th should be finite and >= 0")
    c(f"{name}/rule", fn, base, dict(fginn_th=3.0, ratio=None), V, FGINN_RULE)
    c(f"{name}/seeds", fn, base, dict(seeds=[1]), V, SEEDS)
    c(f"{name}/f_params", fn, base, dict(f_params=3), V, "f_params should be a dict of estimator keywords, or None")
    c(f"{name}/h_params", fn, base, dict(h_params={"error_type": "bad"}), V, ET_H)
    c(f"{name}/device", fn, base, {}, V, DESC_DEV)
    c(f"{name}/2:seeds+f_params", fn, base, dict(seeds=[1], f_params=3), V, SEEDS)
    c(f"{name}/2:f_params+device", fn, base, dict(f_params=3, kps2=META), V, "f_params should be a dict of estimator keywords, or None")
c("fh_batch_t/counts-len", t.match_and_verify_fh_batch_tensors, BT, dict(counts2=[5]), V, CNT_PAIR)
c("fh_pairs_t/pairs", t.match_and_verify_fh_pairs_tensors, PT, dict(pairs=[[0, 2]]), V, PAIRS_RANGE)
c("fh_pairs_t/2:tensors+fginn_th", t.match_and_verify_fh_pairs_tensors, PT, dict(kps1=X, fginn_th=-1), V, T4)

CT5 = "match, keep, kps1, kps2 and models must be torch tensors on a ROCm device"
CT5_DEV = "match, keep, kps1, kps2 and models must live on the same ROCm device"
c("corr_pairs_t/no-pairs", t.correspondences_pairs_tensors, CT, dict(pairs=None), V, PAIRS_ARR)
c("corr_pairs_t/not-tensors", t.correspondences_pairs_tensors, CT, dict(keep=np.zeros(5, bool)), V, CT5)
c("corr_pairs_t/model", t.correspondences_pairs_tensors, CT, dict(model="X"), V, MODEL)
c("corr_pairs_t/counts", t.correspondences_pairs_tensors, CT, dict(counts1=[3.0, 2.0]), V, CNT12)
c("corr_pairs_t/pairs", t.correspondences_pairs_tensors, CT, dict(pairs=[[0, 2]]), V, PAIRS_RANGE)
c("corr_pairs_t/match", t.correspondences_pairs_tensors, CT, dict(match=T(MATCH[:4].copy())), V, MATCH_N)
c("corr_pairs_t/keep", t.correspondences_pairs_tensors, CT, dict(keep=T(np.zeros(5))), V, KEEP_N)
c("corr_pairs_t/kps-one", t.correspondences_pairs_tensors, CT, dict(kps1=T(X)), V, "kps1 and kps2 go together")
c("corr_pairs_t/kps-rows", t.correspondences_pairs_tensors, CT, dict(kps1=T(X), kps2=T(X[:4])), V, "counts do not add up to the number of keypoint rows")
c("corr_pairs_t/models", t.correspondences_pairs_tensors, CT, dict(kps1=T(X), kps2=T(X), models=T(np.zeros((2, 9)))), V, MODELS_ENTRY)
c("corr_pairs_t/capacity", t.correspondences_pairs_tensors, CT, dict(capacity=-1), V, "capacity should be an integer >= 0 (or None = one position per output row)")
c("corr_pairs_t/other-device", t.correspondences_pairs_tensors, CT, dict(kps1=T(X), kps2=META), V, CT5_DEV)
c("corr_pairs_t/device", t.correspondences_pairs_tensors, CT, {}, V, CT5_DEV)
c("corr_pairs_t/2:tensors+model", t.correspondences_pairs_tensors, CT, dict(match=MATCH, model="X"), V, CT5)
c("corr_pairs_t/2:match+device", t.correspondences_pairs_tensors, CT, dict(match=T(MATCH[:4].copy()), kps1=T(X), kps2=META), V, MATCH_N)
CTB = dict(match=T(MATCH), counts1=C1, counts2=C2)
c("corr_batch_t/counts-len", t.correspondences_batch_tensors, CTB, dict(counts2=[5]), V, "counts1 and counts2 should have one entry per pair")
c("corr_batch_t/device", t.correspondences_batch_tensors, CTB, {}, V, CT5_DEV)
c("corr_batch_t/2:counts+capacity", t.correspondences_batch_tensors, CTB, dict(counts2=[5], capacity=-1), V, "counts1 and counts2 should have one entry per pair")

TRK = dict(rows=T(ROWS), counts=[2, 2])
TRK_T = "rows (and total) must be torch tensors on a ROCm device"
c("tracks_t/not-tensor", t.tracks_tensors, TRK, dict(rows=ROWS), V, TRK_T)
c("tracks_t/total-not-tensor", t.tracks_tensors, TRK, dict(total=2), V, TRK_T)
c("tracks_t/counts", t.tracks_tensors, TRK, dict(counts=[2, -2]), V, "counts should be a 1-D array of integers >= 0, the rows per image of the store")
c("tracks_t/rows", t.tracks_tensors, TRK, dict(rows=T(ROWS.astype(np.int64))), V,
  "rows should be int32 [M, 2] of store rows, as the correspondence export writes them with store_rows=True")
c("tracks_t/rows-strided", t.tracks_tensors, TRK, dict(rows=T(np.zeros((2, 4), np.int32))[:, ::2]), V, "rows should be a contiguous int32 [M, 2] tensor")
c("tracks_t/total", t.tracks_tensors, TRK, dict(total=T(np.zeros(2, np.int64))), V,
  "total should be int64 [1] on the device, as the correspondence export returns it")
c("tracks_t/device", t.tracks_tensors, TRK, {}, V, "rows and total must live on the same ROCm device")
c("tracks_t/2:tensor+counts", t.tracks_tensors, TRK, dict(total=2, counts=[2, -2]), V, TRK_T)
c("tracks_t/2:rows+total", t.tracks_tensors, TRK, dict(rows=T(np.zeros((2, 4), np.int32))[:, ::2], total=T(np.zeros(2, np.int64))), V,
  "rows should be a contiguous int32 [M, 2] tensor")

c("refit_t/not-tensors", t.refit_correspondences_tensors, RT, dict(models=MOD), V, "pts, corr_offsets and models must be torch tensors on a ROCm device")
c("refit_t/offsets", t.refit_correspondences_tensors, RT, dict(corr_offsets=T(OFFS.astype(np.int32))), V, OFF)
c("refit_t/models", t.refit_correspondences_tensors, RT, dict(models=T(np.zeros((2, 9)))), V, MODELS_PAIR)
c("refit_t/pts", t.refit_correspondences_tensors, RT, dict(pts=T(PTS4.astype(np.float32))), V, PTS)
c("refit_t/max_fits", t.refit_correspondences_tensors, RT, dict(max_fits=True), V, "max_fits should be an integer >= 0")
c("refit_t/device", t.refit_correspondences_tensors, RT, {}, V, "pts, corr_offsets and models must live on the same ROCm device")
c("refit_t/2:tensors+offsets", t.refit_correspondences_tensors, RT, dict(models=MOD, corr_offsets=T(OFFS.astype(np.int32))), V,
  "pts, corr_offsets and models must be torch tensors on a ROCm device")
c("refit_t/2:max_fits+device", t.refit_correspondences_tensors, RT, dict(max_fits=-1, models=T(MOD).to("meta")), V, "max_fits should be an integer >= 0")

POSE_T = "pts, corr_offsets, models, cams1 (and pairs, cams2, keep) must be torch tensors on a ROCm device"
POSE_DEV = "pts, corr_offsets, models, cams1 (and pairs, cams2, keep) must live on the same ROCm device"
c("pose_t/not-tensors", t.relative_pose_tensors, PTN, dict(keep=np.zeros(3, bool)), V, POSE_T)
c("pose_t/pairs-not-tensor", t.relative_pose_tensors, PTN, dict(pairs=PAIRS), V, POSE_T)
c("pose_t/offsets", t.relative_pose_tensors, PTN, dict(corr_offsets=T(OFFS[:0].copy())), V, OFF)
c("pose_t/models", t.relative_pose_tensors, PTN, dict(models=T(np.zeros((2, 9)))), V, POSE_MODELS)
c("pose_t/cams1", t.relative_pose_tensors, PTN, dict(cams1=T(CAM4)), V, CAMS8)
c("pose_t/pairs", t.relative_pose_tensors, PTN, dict(cams1=T(CAM4), pairs=T(np.zeros((3, 2), np.int64))), V, PAIRS_ARR)
c("pose_t/cams2", t.relative_pose_tensors, PTN, dict(cams1=T(CAM4), pairs=T(np.array(PAIRS)), cams2=T(CAM8)), V, CAMS2)
c("pose_t/keep", t.relative_pose_tensors, PTN, dict(keep=T(np.zeros(3))), V, KEEP_CAP)
c("pose_t/parallax", t.relative_pose_tensors, PTN, dict(min_parallax_deg=200), V, PARALLAX)
c("pose_t/device", t.relative_pose_tensors, PTN, {}, V, POSE_DEV)
c("pose_t/other-device", t.relative_pose_tensors, PTN, dict(keep=torch.zeros(3, dtype=torch.bool, device="meta")), V, POSE_DEV)
c("pose_t/2:tensors+models", t.relative_pose_tensors, PTN, dict(pairs=PAIRS, models=T(np.zeros((2, 9)))), V, POSE_T)
c("pose_t/2:parallax+device", t.relative_pose_tensors, PTN, dict(min_parallax_deg=-1, keep=torch.zeros(3, dtype=torch.bool, device="meta")), V, PARALLAX)

REF_T = "pts, corr_offsets, R, t, cams1 (and pairs, cams2, keep) must be torch tensors on a ROCm device"
REF_DEV = "pts, corr_offsets, R, t, cams1 (and pairs, cams2, keep) must live on the same ROCm device"
c("refine_t/unknown", t.refine_pose_tensors, FT, dict(max_trails=3), V, "refine_pose_tensors: unknown keyword 'max_trails'")
c("refine_t/not-tensors", t.refine_pose_tensors, FT, dict(R=RR), V, REF_T)
c("refine_t/R", t.refine_pose_tensors, FT, dict(R=T(np.zeros((2, 9)))), V, R_K)
c("refine_t/t", t.refine_pose_tensors, FT, dict(t=T(np.zeros((2, 3), np.float32))), V, T_K)
c("refine_t/pts", t.refine_pose_tensors, FT, dict(pts=T(PTS4[:, :3].copy())), V, PTS)
c("refine_t/max_trials", t.refine_pose_tensors, FT, dict(max_trials=-1), V, TRIALS)
c("refine_t/ftol", t.refine_pose_tensors, FT, dict(ftol="x"), V, FTOL)
c("refine_t/device", t.refine_pose_tensors, FT, {}, V, REF_DEV)
c("refine_t/2:unknown+tensors", t.refine_pose_tensors, FT, dict(zz=1, R=RR), V, "refine_pose_tensors: unknown keyword 'zz'")
c("refine_t/2:tensors+R", t.refine_pose_tensors, FT, dict(t=TT, R=T(np.zeros((2, 9)))), V, REF_T)
c("refine_t/2:ftol+device", t.refine_pose_tensors, FT, dict(ftol=-1, t=T(TT).to("meta")), V, FTOL)

TRI_TT = "track_offsets, obs, obs_image, kps, cams, R, t (and n_tracks) must be torch tensors on a ROCm device"
TRI_DEV = "track_offsets, obs, obs_image, kps, cams, R, t (and n_tracks) must live on the same ROCm device"
c("triangulate_t/unknown", t.triangulate_tracks_tensors, TTN, dict(max_iter=3), V, "triangulate_tracks_tensors: unknown keyword 'max_iter'")
c("triangulate_t/not-tensors", t.triangulate_tracks_tensors, TTN, dict(kps=KX), V, TRI_TT)
c("triangulate_t/n_tracks-not-tensor", t.triangulate_tracks_tensors, TTN, dict(n_tracks=1), V, TRI_TT)
c("triangulate_t/offsets", t.triangulate_tracks_tensors, TTN, dict(track_offsets=T(TO.astype(np.int32))), V, TRI_OFF)
c("triangulate_t/obs", t.triangulate_tracks_tensors, TTN, dict(obs=T(OB.astype(np.int64))), V, TRI_OBS)
c("triangulate_t/cams", t.triangulate_tracks_tensors, TTN, dict(cams=T(CAM8)), V, TRI_CAMS)
c("triangulate_t/t", t.triangulate_tracks_tensors, TTN, dict(t=T(np.zeros((2, 4)))), V, TRI_T)
c("triangulate_t/n_tracks", t.triangulate_tracks_tensors, TTN, dict(n_tracks=T(np.zeros(2, np.int64))), V, TRI_NT)
c("triangulate_t/reproj", t.triangulate_tracks_tensors, TTN, dict(max_reproj_px=-1), V, TRI_PX)
c("triangulate_t/device", t.triangulate_tracks_tensors, TTN, {}, V, TRI_DEV)
c("triangulate_t/2:unknown+tensors", t.triangulate_tracks_tensors, TTN, dict(zz=1, kps=KX), V, "triangulate_tracks_tensors: unknown keyword 'zz'")
c("triangulate_t/2:tensors+offsets", t.triangulate_tracks_tensors, TTN, dict(n_tracks=1, track_offsets=T(TO.astype(np.int32))), V, TRI_TT)
c("triangulate_t/2:ftol+device", t.triangulate_tracks_tensors, TTN, dict(ftol=-1, kps=torch.zeros((4, 2), dtype=torch.float64, device="meta")), V, FTOL)


@pytest.mark.parametrize("call, exc, msg", CASES)
def test_refusal(call, exc, msg):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and str(e.value) == msg


def test_every_case_has_its_own_name():
    ids = [x.id for x in CASES]
    assert len(ids) == len(set(ids))
