"""TEST INFRASTRUCTURE ONLY (CPU, numpy): the summary of the match_and_verify_fh_* calls restated from their per-row outputs, and the
scenes the two-view tests share.

summary_ref counts, per pair, what the scatter stage counts on the device: the rows with a match (tentatives), with inlier_f, with
inlier_h and with both, between the pair's output offsets.

alternating_scenes is the arrangement the scatter stage can get wrong: pairs with 5 tentatives (a homography, no fundamental matrix)
alternate with pairs of at least 9 (both), with an empty pair in between, so the eligible index and the row base of a pair differ between
the two estimators for every pair behind the first."""
import numpy as np

from tests import verify_ref as vr


def summary_ref(match, inlier_f, inlier_h, pair_offsets):
    """[K, 4] int32 = per pair (tentatives, nF, nH, nFH) from match [N] (-1 = no tentative), inlier_f / inlier_h [N] and pair_offsets [K + 1]"""
    match = np.asarray(match); f = np.asarray(inlier_f).astype(bool); h = np.asarray(inlier_h).astype(bool); po = np.asarray(pair_offsets, np.int64)
    assert match.shape == f.shape == h.shape == (int(po[-1]),)
    out = np.zeros((len(po) - 1, 4), np.int32)
    for p in range(len(po) - 1):
        r = slice(int(po[p]), int(po[p + 1]))
        out[p] = ((match[r] >= 0).sum(), f[r].sum(), h[r].sum(), (f[r] & h[r]).sum())
    return out


# the alternating arrangement: "5" = five tentatives among 40 queries, "E" = at least 9, "Q" = no queries
ALTERNATING = "5QE5EQ5E5QEE"
ALTERNATING_SEEDS = [95001 + 61 * p for p in range(len(ALTERNATING))]


def alternating_scenes(model="F", norm="l2"):
    """[designed pair] of ALTERNATING; `model` only chooses the keypoint layout ([n, 2] for "F", [n, 6] / [n, 4] for "H")"""
    out = []
    for p, kind in enumerate(ALTERNATING):
        s = 800 + p
        if kind == "5":
            out.append(vr.designed_pair(model, 40, np.array([1, 9, 20, 33, 39]), norm=norm, seed=s))
        elif kind == "E":
            n = (20, 64, 65, 70, 129, 140)[p % 6]
            out.append(vr.designed_pair(model, n, np.arange(p % 3, n, 2 + p % 2), norm=norm, seed=s))
        else:
            out.append(vr.designed_pair(model, 0, [], norm=norm, seed=s))
    return out


def other(model):
    return "H" if model == "F" else "F"


def both_ref(port, sc, seed, mutual=False):
    """the restatement of a designed pair under BOTH models of verify_ref.BUDGET on the pair's own keypoint rows -> {"F": ..., "H": ...}"""
    return {m: vr.pair_ref(port, m, sc["k1"], sc["k2"], sc["d1"], sc["d2"], seed, sc["ratio"], mutual, sc["norm"]) for m in ("F", "H")}


# ---- the end-to-end scene: one pair that sees one plane, one that sees a general scene -------------------------------------------------
# seed of the scene, and (nF, nH) of the CPU restatement for (planar pair, general pair) under E2E_PARAMS; tests/test_two_view_cpu.py
# computes them again and checks that neither nH / nF lies within 10 % of the 0.8 boundary
E2E_SEED = 5
E2E_N = 300
E2E_PARAMS = {"F": dict(px_th=0.5, conf=0.9999, max_iters=2000, laf_consistensy_coef=-1.0, error_type="sampson"),
              "H": dict(px_th=2.0, conf=0.999, max_iters=2000, laf_consistensy_coef=-1.0, error_type="symm_max")}
E2E_EST_SEEDS = [7, 8]
E2E_NF_NH = ((143, 138), (176, 20))          # the restatement's (nF, nH): planar pair nH / nF = 0.97, general pair 0.11


def e2e_scene():
    """(kps_list, desc_list, pairs): images 0 / 1 see one plane (synthetic.homography_pairs), images 2 / 3 a general scene
    (synthetic.two_view_fundamental); a query's descriptor is the code of its row and its train row holds the same code, so every
    correspondence of the synthetic pair is a tentative and nothing else is"""
    from pydegensac_amd import synthetic as syn
    rng = np.random.default_rng(E2E_SEED)
    kps, desc = [], []
    for k, make in enumerate((lambda: syn.homography_pairs(E2E_N, 0.7, 0.5, seed=E2E_SEED),
                              lambda: syn.two_view_fundamental(E2E_N, 0.7, 0.3, seed=E2E_SEED))):
        res = make()
        p1, p2 = np.asarray(res[0], float)[:, :2], np.asarray(res[1], float)[:, :2]
        d = vr._codes(np.arange(1, E2E_N + 1), "l2").astype(np.float32)
        perm = rng.permutation(E2E_N)
        kps += [np.ascontiguousarray(p1), np.ascontiguousarray(p2[perm])]; desc += [d, d[perm]]
    return kps, desc, [(0, 1), (2, 3)]


def e2e_ref(port):
    """summary [2, 4] of the end-to-end scene by the CPU restatement alone (oracle.matcher_np + oracle.port)"""
    kps, desc, pairs = e2e_scene()
    out = np.zeros((len(pairs), 4), np.int32)
    for p, (i, j) in enumerate(pairs):
        q, t = vr.tentatives(desc[i], desc[j], 0.9, False, "l2")
        masks = {}
        for m, b in E2E_PARAMS.items():
            et = vr._ERROR_CODE[b["error_type"]]; A, B = kps[i][q], kps[j][t]
            if m == "F":
                _, masks[m], _ = port.find_fundamental(A, B, b["px_th"], b["conf"], b["max_iters"], et, True, 0.0, True, seed=E2E_EST_SEEDS[p])
            else:
                _, masks[m], _ = port.find_homography(A, B, b["px_th"], b["conf"], b["max_iters"], et, True, 0.0, seed=E2E_EST_SEEDS[p])
        f, h = np.asarray(masks["F"], bool), np.asarray(masks["H"], bool)
        out[p] = (len(q), f.sum(), h.sum(), (f & h).sum())
    return out


