"""TEST INFRASTRUCTURE ONLY (CPU, numpy): the whole match-and-verify pipeline restated from what the repository already trusts, and
scenes in which the caller STATES which queries become tentatives (tests/test_verify_stage_cpu.py, tests/test_gpu_verify_stage.py).

The restatement of one pair: the decisions of oracle.matcher_np.match_snn, the tentatives in ascending query order, then
oracle.port.find_fundamental / find_homography on them with the pair's own seed; match, inlier, model, tentative count and the counters
(samples, lo_runs, I) in pair order, zeros for a pair with fewer than 8 (F) / 4 (H) tentatives.  A pair list is expanded entry by entry
through tests/pairs_ref.py.

The designed scenes.  A descriptor is the code of an id: component c < 12 holds bit c of the id times 4 (255 under Hamming), components
12 ... 15 are zero but for the two perturbations below.  Two ids are at least 4 apart under L2 and 8 bits under Hamming, and every squared
distance is a small integer, exact in float32 in any accumulation order, so idx, dist and every decision are the same numbers for "l2",
"l2_u8" and "hamming" on any device.  A kept query has its exact copy among the train rows (d0 = 0 < ratio * d1).  Every other query is
dropped for a stated reason:
  tie0   the train set holds its code twice: d0 = d1 = 0;
  tie1   the train set holds its code + 1 in component 12 and its code + 1 in component 13: d0 = d1 = 1;
  edge   the train set holds its code + 1 in component 12 and its code + 2 (two bits under Hamming) in component 13: d0 = 1, d1 = 2, and
         at ratio = 0.5 the strict comparison 1 < 0.5 * 2 drops it (the builder refuses the kind at any larger ratio);
  dup    (under mutual only) it repeats the code of a kept query in front of it: the reverse search finds the lower index.  Without
         mutual it is one more tentative on the same train row;
  and a pair with fewer than two train rows keeps nothing.
The keypoints of the kept queries, in query order, are the correspondences of pydegensac_amd.synthetic.two_view_fundamental ([n, 2],
model F) / homography_pairs with frames ([n, 6], model H) with a stated share of outliers; every other keypoint row is random.  For H the
frames go through float32 (x, y, size, angle) keypoints first, so the same scene runs as [n, 6] rows and as [n, 4] keypoints."""
import numpy as np

from oracle import matcher_np as mo
from pydegensac_amd import synthetic as syn
from tests import pairs_ref as pr

MIN_PTS = {"F": 8, "H": 4}
NORMS = ("l2", "l2_u8", "hamming")
# the estimator budget of every family, stated once: the keywords of the match_and_verify_* calls
BUDGET = {"F": dict(px_th=0.5, conf=0.9999, max_iters=2000, laf_consistensy_coef=-1.0, error_type="sampson"),
          "H": dict(px_th=2.0, conf=0.999, max_iters=2000, laf_consistensy_coef=3.0, error_type="symm_max")}
_ERROR_CODE = {"sampson": 0, "symm_max": 2}
MODEL_RTOL = 1e-9                       # least-squares models, relative Frobenius


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def estimate(port, model, A, B, seed):
    """the estimator of the restatement under BUDGET[model] -> (model [3, 3] in the user's form, mask, (samples, lo_runs, I))"""
    b = BUDGET[model]
    et = _ERROR_CODE[b["error_type"]]; laf = max(0.0, b["laf_consistensy_coef"]); seed = int(seed) & 0xFFFFFFFF
    if model == "F":
        M, mask, st = port.find_fundamental(A, B, b["px_th"], b["conf"], b["max_iters"], et, True, laf, True, seed=seed)
    else:
        M, mask, st = port.find_homography(A, B, b["px_th"], b["conf"], b["max_iters"], et, True, laf, seed=seed)
        if np.abs(M).sum() != 0:
            M = np.linalg.inv(M.T)                                     # the driver's H_c -> the user's H (matcher._h_user_form)
    return np.asarray(M, float), mask, (st["samples"], st["lo_runs"], st["I"])


def tentatives(d1, d2, ratio=0.9, mutual=False, norm="l2"):
    """(query rows ascending, train rows) of oracle.matcher_np.match_snn; uint8 rows under l2_u8 are the float32 path on the same values"""
    if len(d2) == 0 or len(d1) == 0:                                   # match_snn's reverse lookup needs a train row; fewer than two keep nothing
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    q, t, _ = mo.match_snn(d1, d2, ratio, mutual, "l2" if norm == "l2_u8" else norm)
    return q, t


def result(model, n1, q, t, est):
    """a pair's outputs from its tentatives (q, t) and est = (model, mask over the tentatives, counters) or None for a short pair"""
    match = np.full(n1, -1, np.int32); match[q] = t
    inl = np.zeros(n1, bool)
    M = np.zeros((3, 3)); ctr = (0, 0, 0)
    if est is not None:
        M, mask, ctr = est
        inl[q] = mask
    return dict(model=M, match=match, inlier=inl, cnt=len(q), counters=tuple(int(c) for c in ctr))


def pair_ref(port, model, k1, k2, d1, d2, seed, ratio=0.9, mutual=False, norm="l2"):
    q, t = tentatives(d1, d2, ratio, mutual, norm)
    est = estimate(port, model, k1[q], k2[t], seed) if len(q) >= MIN_PTS[model] else None
    return result(model, len(d1), q, t, est)


def batch_ref(port, model, K1, K2, D1, D2, seeds, ratio=0.9, mutual=False, norm="l2"):
    return [pair_ref(port, model, K1[p], K2[p], D1[p], D2[p], seeds[p], ratio, mutual, norm) for p in range(len(D1))]


def pairs_ref(port, model, kps1, desc1, counts1, kps2, desc2, counts2, pairs, seeds, ratio=0.9, mutual=False, norm="l2"):
    """the restatement over a pair list on image stores: entry p on the rows tests/pairs_ref.py copies out for it"""
    (e_k1, e_d1), (e_k2, e_d2), c1, c2, _ = pr.expand((kps1, desc1), counts1, (kps2, desc2), counts2, pairs)
    o1, o2 = pr.offsets(c1), pr.offsets(c2)
    cut = lambda a, o: [a[o[p]:o[p + 1]] for p in range(len(o) - 1)]
    return batch_ref(port, model, cut(e_k1, o1), cut(e_k2, o2), cut(e_d1, o1), cut(e_d2, o2), seeds, ratio, mutual, norm)


def disagreements(got, want):
    """what the GPU tests assert of a pair, as a list of the fields that differ (empty = agreement): match, inlier, cnt and the counters
    bit for bit, the model within MODEL_RTOL relative Frobenius (a zero model exactly)"""
    bad = [k for k in ("match", "inlier") if not np.array_equal(got[k], want[k])]
    bad += [k for k in ("cnt", "counters") if got[k] != want[k]]
    nw = np.linalg.norm(want["model"])
    if not (np.linalg.norm(np.asarray(got["model"]) - want["model"]) <= MODEL_RTOL * nw):
        bad.append("model")
    return bad


# ---- mutations of the restatement: what a wrong rank, a dropped row or a wrong seed mapping would compute ----------------------------
def mutated(port, model, sc, seed, mutation, mutual=False, other_seed=None):
    """The restatement of scene sc with one defect between the filter and the estimator.  The estimator sees the tentatives in a wrong
    order and its mask goes back through the same wrong order (as a wrong rank would do it in gather and scatter):
      rotate   tentative k sits at row (k + 1) mod m;
      swap256  the last tentative in front of query row 256 and the first one behind it trade rows;
      drop     the middle tentative is missing from the estimator's input (and is no inlier);
      seed     the pair runs under other_seed."""
    q, t = tentatives(sc["d1"], sc["d2"], sc["ratio"], mutual, sc["norm"])
    m = len(q); row = np.arange(m)                                      # row[k]: the estimator's input row of tentative k
    if mutation == "rotate":
        row = (row + 1) % m
    elif mutation == "swap256":
        k = int(np.searchsorted(q, 256))
        assert 0 < k < m, "the scene has no tentatives on both sides of query row 256"
        row[k - 1], row[k] = k, k - 1
    elif mutation == "drop":
        sel = np.delete(np.arange(m), m // 2)
        M, mask, ctr = estimate(port, model, sc["k1"][q[sel]], sc["k2"][t[sel]], seed)
        full = np.zeros(m, bool); full[sel] = mask
        return result(model, sc["n1"], q, t, (M, full, ctr))
    elif mutation == "seed":
        seed = other_seed
    else:
        raise ValueError(mutation)
    at = np.argsort(row)                                                # at[r]: the tentative at input row r
    M, mask, ctr = estimate(port, model, sc["k1"][q[at]], sc["k2"][t[at]], seed)
    return result(model, sc["n1"], q, t, (M, mask[row], ctr))


# ---- designed scenes ------------------------------------------------------------------------------------------------------------------
DIM, ID_BITS = 16, 12
GROUPS = 3                              # dropped queries of one kind share one of three codes (and its two train rows)


def _codes(ids, norm):
    ids = np.asarray(ids, np.int64).reshape(-1)
    assert ids.size == 0 or (0 < ids.min() and ids.max() < (1 << ID_BITS))
    out = np.zeros((ids.size, DIM), np.uint8)
    out[:, :ID_BITS] = ((ids[:, None] >> np.arange(ID_BITS)) & 1) * (255 if norm == "hamming" else 4)
    return out


def _bump(code, comp, dist, norm):
    """the code at distance `dist` (1 or 2) from `code`, by component `comp` alone"""
    c = code.copy()
    c[comp] = {1: 1, 2: 3 if norm == "hamming" else 2}[dist]
    return c


def xyA_np(k4):
    """matcher.kpts_to_xyA in numpy: float32 (x, y, size, angle in degrees) -> float64 (x, y, s cos a, s sin a, -s sin a, s cos a)"""
    k = np.asarray(k4, np.float32).astype(np.float64)
    r = k[:, 3] * 3.141592653589793 / 180.0
    cs, sn = np.cos(r), np.sin(r)
    return np.stack([k[:, 0], k[:, 1], k[:, 2] * cs, k[:, 2] * sn, -k[:, 2] * sn, k[:, 2] * cs], 1)


def _kpts4(rows6):
    """[n, 6] frames -> float32 (x, y, size, angle): the similarity part of the frame (as tests/test_gpu_match_verify.py builds them)"""
    r = np.asarray(rows6, float)
    s = np.sqrt(np.abs(r[:, 2] * r[:, 5] - r[:, 3] * r[:, 4])); ang = np.degrees(np.arctan2(r[:, 3], r[:, 2]))
    return np.stack([r[:, 0], r[:, 1], s, ang], 1).astype(np.float32)


def outlier_share(m):
    """the stated share of outliers among m kept queries: a quarter of a set that is barely eligible, 40 % of a larger one"""
    return 0.25 if m < 16 else 0.4


def designed_pair(model, n1, kept, norm="l2", ratio=0.9, dups=(), kinds=("tie0", "tie1"), train="full", fillers=5, seed=0):
    """One pair of n1 queries whose tentatives are exactly `kept` (ascending query rows) with mutual, and `kept` plus the rows of `dups`
    without it.  dups: (row j, kept row i < j) pairs, query j repeats query i.  kinds: the reasons the other queries take in turn
    (row r takes kinds[r % len]).  train: "full", or "none" / "one" for a train set of 0 / 1 rows (then nothing is kept).
    Returns a dict: n1, n2, d1, d2 (float32 for "l2", else uint8), k1, k2 (float64 [n, 2] for F, [n, 6] for H), k4_1, k4_2 (H only:
    the float32 [n, 4] keypoints k1 / k2 were made from), kept = {False: rows without mutual, True: rows with it}, train_of [n1] = the
    stated train row of a tentative or -1, model, ratio, norm."""
    assert model in MIN_PTS and norm in NORMS and train in ("full", "none", "one")
    rng = np.random.default_rng([seed, n1, len(kept)])
    kept = np.asarray(kept, np.int64).reshape(-1); dups = [(int(j), int(i)) for j, i in dups]
    assert np.all(np.diff(kept) > 0) and (kept.size == 0 or (kept[0] >= 0 and kept[-1] < n1))
    assert all(i in kept and j not in kept and i < j < n1 for j, i in dups) and len({j for j, _ in dups}) == len(dups)
    assert "edge" not in kinds or np.float32(ratio) * np.float32(2) <= np.float32(1), "the edge kind is a drop at ratio <= 0.5 only"
    assert set(kinds) <= {"tie0", "tie1", "edge"} and np.float32(ratio) <= 1
    assert train == "full" or (kept.size == 0 and not dups)
    m = kept.size
    next_id = iter(range(1, 1 << ID_BITS))
    q_id = np.zeros(n1, np.int64); kind_of = np.full(n1, "", dtype=object)
    kept_id = np.array([next(next_id) for _ in range(m)], np.int64)
    q_id[kept] = kept_id; kind_of[kept] = "kept"
    for j, i in dups:
        q_id[j] = q_id[i]; kind_of[j] = "dup"
    group_id = {}
    for r in range(n1):
        if kind_of[r] == "":
            key = (kinds[r % len(kinds)], (r // len(kinds)) % GROUPS)
            if key not in group_id:
                group_id[key] = next(next_id)
            q_id[r] = group_id[key]; kind_of[r] = key[0]
    d1 = _codes(q_id, norm)
    # the train rows: the copies of the kept queries first (train row k belongs to kept[k] until the shuffle), then the rows that make
    # the drops, then rows of ids no query has
    t_rows = [c for c in _codes(kept_id, norm)]
    for (kind, _), gid in sorted(group_id.items()):
        c = _codes([gid], norm)[0]
        t_rows += {"tie0": [c, c.copy()], "tie1": [_bump(c, 12, 1, norm), _bump(c, 13, 1, norm)],
                   "edge": [_bump(c, 12, 1, norm), _bump(c, 13, 2, norm)]}[kind]
    t_rows += [c for c in _codes([next(next_id) for _ in range(fillers)], norm)]
    d2 = np.array(t_rows, np.uint8).reshape(-1, DIM)
    perm = rng.permutation(len(d2))
    place = np.argsort(perm)                                            # place[r]: where row r of the unshuffled train set went
    d2 = d2[perm]
    if train == "none":
        d2 = d2[:0]
    elif train == "one":
        d2 = d1[:1].copy() if n1 else d2[:1]                            # the exact copy of query 0: nearest at distance 0, and no second row
    n2 = len(d2)
    train_of = np.full(n1, -1, np.int64)
    train_of[kept] = place[:m]
    for j, i in dups:
        train_of[j] = train_of[i]
    # keypoints: random rows, the scene's correspondences on the kept queries and their train rows
    kd = 2 if model == "F" else 6
    def rand_rows(n):
        xy = rng.uniform(0, [syn.IMG_W, syn.IMG_H], (n, 2)) if model == "F" else rng.uniform(0, [788.0, 522.0], (n, 2))
        return xy if kd == 2 else np.c_[xy, rng.normal(0, 5.0, (n, 4))]
    k1, k2 = rand_rows(n1), rand_rows(n2)
    if m:
        share = 1.0 - outlier_share(m)
        if model == "F":
            p1, p2, _, _ = syn.two_view_fundamental(m, share, 0.3, seed=1000 + seed)
        else:
            p1, p2, _, _ = syn.homography_pairs(m, share, 0.5, seed=1000 + seed, laf=True)
        k1[kept] = p1; k2[train_of[kept]] = p2
    sc = dict(model=model, n1=n1, n2=n2, ratio=ratio, norm=norm, train_of=train_of,
              kept={True: kept, False: np.sort(np.r_[kept, [j for j, _ in dups]]).astype(np.int64)})
    if model == "H":
        sc["k4_1"], sc["k4_2"] = _kpts4(k1), _kpts4(k2)
        k1, k2 = xyA_np(sc["k4_1"]), xyA_np(sc["k4_2"])
    sc.update(k1=np.ascontiguousarray(k1), k2=np.ascontiguousarray(k2), d2=np.ascontiguousarray(d2 if norm != "l2" else d2.astype(np.float32)),
              d1=np.ascontiguousarray(d1 if norm != "l2" else d1.astype(np.float32)))
    return sc


# ---- the family table -----------------------------------------------------------------------------------------------------------------
# Rank positions: where the kept queries lie relative to the 64-lane ballot, the four-wave prefix and the 256-row sweep of
# mt_filter_rank_kernel.  Every selector leaves at least 8 kept queries at the sizes listed for it, so F and H are both estimated.
RANK_SIZES = (64, 65, 256, 257, 512, 513, 600)
RANK_SELECTORS = {
    "first8": (lambda n: np.arange(8), RANK_SIZES),
    "last8": (lambda n: np.arange(n - 8, n), RANK_SIZES),
    "wave": (lambda n: np.arange(60, 68), (256, 257, 512, 513, 600)),                                   # straddles lanes 63 | 64
    "sweep": (lambda n: np.arange(252, 260), (512, 513, 600)),                                          # straddles rows 255 | 256
    "sweep2": (lambda n: np.array([512, 513, 540, 575, 576, 577, 598, 599]), (600,)),                   # nothing in sweeps 0 and 1
    "per_wave": (lambda n: np.array([w * 64 + min((17 * w + 5) % 64, n - 1 - w * 64) for w in range((n + 63) // 64)]), (512, 513, 600)),
    "every2": (lambda n: np.arange(0, n, 2), RANK_SIZES),
    "all": (lambda n: np.arange(n), RANK_SIZES),
}
RANK_CASES = [(sel, n) for sel, (_, sizes) in RANK_SELECTORS.items() for n in sizes]
# the mutations each rank case is claimed to notice (tests/test_verify_stage_cpu.py shows it on the restatement alone): every case
# notices a rotation, a dropped row and the neighbour's seed; a swap across row 256 needs tentatives on both sides of it
ORDER_MUTATIONS = ("rotate", "drop", "seed")


# (scene variant, estimator seed) of every rank case: the first of variants 0 ... 5 x seeds 11 ... 50 under which the restatement notices
# every mutation claimed for the case (searched on the restatement alone; tests/test_verify_stage_cpu.py checks each entry)
RANK_CHOICE = {
    ("F", "first8", 64): (0, 11), ("F", "first8", 65): (0, 11), ("F", "first8", 256): (0, 11), ("F", "first8", 257): (0, 11), ("F", "first8", 512): (0, 11),
    ("F", "first8", 513): (0, 11), ("F", "first8", 600): (0, 11), ("F", "last8", 64): (0, 11), ("F", "last8", 65): (0, 11), ("F", "last8", 256): (0, 11),
    ("F", "last8", 257): (1, 14), ("F", "last8", 512): (0, 11), ("F", "last8", 513): (0, 11), ("F", "last8", 600): (1, 12), ("F", "wave", 256): (0, 12),
    ("F", "wave", 257): (0, 11), ("F", "wave", 512): (1, 12), ("F", "wave", 513): (1, 14), ("F", "wave", 600): (2, 14), ("F", "sweep", 512): (1, 15),
    ("F", "sweep", 513): (0, 12), ("F", "sweep", 600): (0, 46), ("F", "sweep2", 600): (0, 15), ("F", "per_wave", 512): (0, 12), ("F", "per_wave", 513): (0, 17),
    ("F", "per_wave", 600): (0, 15), ("F", "every2", 64): (0, 11), ("F", "every2", 65): (0, 11), ("F", "every2", 256): (0, 11), ("F", "every2", 257): (1, 12),
    ("F", "every2", 512): (0, 24), ("F", "every2", 513): (0, 21), ("F", "every2", 600): (0, 13), ("F", "all", 64): (0, 11), ("F", "all", 65): (0, 11),
    ("F", "all", 256): (0, 11), ("F", "all", 257): (0, 11), ("F", "all", 512): (0, 13), ("F", "all", 513): (0, 15), ("F", "all", 600): (1, 15),
    ("H", "first8", 64): (0, 12), ("H", "first8", 65): (0, 13), ("H", "first8", 256): (0, 12), ("H", "first8", 257): (0, 11), ("H", "first8", 512): (0, 12),
    ("H", "first8", 513): (0, 13), ("H", "first8", 600): (0, 13), ("H", "last8", 64): (0, 11), ("H", "last8", 65): (0, 11), ("H", "last8", 256): (0, 13),
    ("H", "last8", 257): (0, 11), ("H", "last8", 512): (0, 13), ("H", "last8", 513): (0, 11), ("H", "last8", 600): (0, 12), ("H", "wave", 256): (0, 11),
    ("H", "wave", 257): (0, 12), ("H", "wave", 512): (0, 11), ("H", "wave", 513): (0, 11), ("H", "wave", 600): (0, 11), ("H", "sweep", 512): (0, 29),
    ("H", "sweep", 513): (0, 11), ("H", "sweep", 600): (0, 24), ("H", "sweep2", 600): (0, 11), ("H", "per_wave", 512): (1, 15), ("H", "per_wave", 513): (0, 12),
    ("H", "per_wave", 600): (0, 12), ("H", "every2", 64): (0, 19), ("H", "every2", 65): (0, 11), ("H", "every2", 256): (0, 11), ("H", "every2", 257): (0, 15),
    ("H", "every2", 512): (0, 18), ("H", "every2", 513): (0, 17), ("H", "every2", 600): (0, 14), ("H", "all", 64): (0, 11), ("H", "all", 65): (0, 11),
    ("H", "all", 256): (0, 12), ("H", "all", 257): (0, 35), ("H", "all", 512): (0, 23), ("H", "all", 513): (4, 37), ("H", "all", 600): (0, 33),
}


def crosses_256(sel, n):
    k = RANK_SELECTORS[sel][0](n)
    return bool((k < 256).any() and (k >= 256).any())


def rank_seed(model, sel, n):
    """the pair's estimator seed (the neighbour's, for the seed mutation, is this + 1)"""
    return RANK_CHOICE[model, sel, n][1]


_cache = {}


def rank_scene(model, sel, n):
    """the designed pair of a rank case; the norm goes round the three norms with the case index"""
    key = ("rank", model, sel, n)
    if key not in _cache:
        i = RANK_CASES.index((sel, n))
        _cache[key] = designed_pair(model, n, RANK_SELECTORS[sel][0](n), norm=NORMS[i % 3], seed=i + 100 * RANK_CHOICE[model, sel, n][0])
    return _cache[key]


# Count threshold: (kept with mutual, duplicated queries) among 300 queries, the last tentative in the second sweep.  Without mutual the
# pair has core + dups tentatives: (7, 1) and (3, 1) are eligible without mutual and short with it.
COUNT_N = 300
COUNT_ROWS = np.array([3, 63, 64, 130, 200, 255, 256, 270, 299])
COUNT_CASES = {"F": [(7, 0), (8, 0), (9, 0), (7, 1), (7, 2)], "H": [(3, 0), (4, 0), (5, 0), (3, 1), (3, 2)]}


def count_scene(model, core, n_dups, norm="l2"):
    key = ("count", model, core, n_dups, norm)
    if key not in _cache:
        rows = np.r_[COUNT_ROWS[:core - 1], COUNT_ROWS[-1]]            # the last tentative is row 299 whatever the count
        dups = [(rows[k] + 1 + k, rows[k]) for k in range(n_dups)]      # behind their originals, in front of the last row
        _cache[key] = designed_pair(model, COUNT_N, rows, norm=norm, dups=dups, seed=40 + core + 10 * n_dups)
    return _cache[key]


# Batch composition: K = 12 from five kinds of pair.  "E": eligible (its size and kept set follow its position), "S": short (5 kept for F,
# 3 for H, among 40), "Q": no queries, "T": no train rows, "O": one train row.
BATCH_K = 12
ARRANGEMENTS = {
    "all_short": "SQTOSSQTOSSS",
    "all_eligible": "EEEEEEEEEEEE",
    "short_first": "SQTOSSEEEEEE",
    "short_last": "EEEEEESOTQSS",
    "around_one": "SQTSOQETSOQS",
}


# one seed per pair, all distinct: 90001 + 1000 a + 61 p, moved up by one to three where a neighbour's seed would have given an eligible pair
# the same result (searched on the restatement alone; tests/test_verify_stage_cpu.py checks it)
BATCH_SEEDS = {
    "all_short": [90001, 90062, 90123, 90184, 90245, 90306, 90367, 90428, 90489, 90550, 90611, 90672],
    "all_eligible": [91001, 91062, 91123, 91184, 91245, 91306, 91367, 91430, 91489, 91550, 91611, 91672],
    "short_first": [92001, 92062, 92123, 92184, 92245, 92306, 92367, 92428, 92489, 92551, 92611, 92672],
    "short_last": [93001, 93062, 93123, 93184, 93245, 93307, 93367, 93428, 93489, 93550, 93611, 93672],
    "around_one": [94001, 94062, 94123, 94184, 94245, 94306, 94367, 94429, 94489, 94550, 94611, 94672],
}


def batch_seeds(name):
    return BATCH_SEEDS[name]


def batch_scene(model, name, norm="l2"):
    """[designed pair] of an arrangement"""
    key = ("batch", model, name, norm)
    if key not in _cache:
        out = []
        for p, kind in enumerate(ARRANGEMENTS[name]):
            s = 500 + 20 * list(ARRANGEMENTS).index(name) + p
            if kind == "E":
                n = (20, 64, 65, 70, 129, 140)[p % 6]
                out.append(designed_pair(model, n, np.arange(p % 3, n, 2 + p % 2), norm=norm, seed=s))
            elif kind == "S":
                out.append(designed_pair(model, 40, np.array([1, 9, 20, 33, 39])[:{"F": 5, "H": 3}[model]], norm=norm, seed=s))
            elif kind == "Q":
                out.append(designed_pair(model, 0, [], norm=norm, seed=s))
            else:
                out.append(designed_pair(model, 30, [], norm=norm, train="none" if kind == "T" else "one", seed=s))
        _cache[key] = out
    return _cache[key]


# Decision edges inside the batch: (ratio, the kinds the dropped queries take in turn)
EDGE_CASES = [(0.5, ("tie0", "tie1", "edge")), (1.0, ("tie0", "tie1")), (0.9, ("tie1", "tie0"))]


def edge_scene(model, ratio, kinds, norm):
    """130 queries, every third one kept, two duplicated queries (dropped under mutual), the others dropped kind after kind"""
    key = ("edge", model, ratio, kinds, norm)
    if key not in _cache:
        kept = np.arange(1, 130, 3)
        _cache[key] = designed_pair(model, 130, kept, norm=norm, ratio=ratio, kinds=kinds, dups=[(3, 1), (66, 64)], seed=300 + EDGE_CASES.index((ratio, kinds)))
    return _cache[key]


def scene_ref(port, sc, seed, mutual=False):
    """the restatement of a designed pair"""
    return pair_ref(port, sc["model"], sc["k1"], sc["k2"], sc["d1"], sc["d2"], seed, sc["ratio"], mutual, sc["norm"])
