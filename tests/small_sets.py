"""TEST INFRASTRUCTURE ONLY: the input families of the small-set tests (tests/test_small_sets_cpu.py, tests/test_gpu_small_sets.py) and
an independent float64 fit.

Homographies on 4 ... 10 correspondences, inlier lists of 4 ... 6 inside larger sets, fundamental matrices on 8 ... 16 and ransacH2el on
2 ... 14 ellipse pairs all reach the 4-point branch of u2h (Htools.c:106-114) or its short-list least squares.  The unmodified
reference reads uninitialised memory in that branch; oracle/dg_oracle.c and the device zero-fill, so on these inputs the
device is compared with the restatement, whose counters `u2h_4pt` / `u2h_short` say which branch a call took.

A family is a list of GROUPS: the pairs of one group share every parameter of a launch (threshold, confidence, budget, metric, checks),
so a group is one ragged batch call on the device.  Everything is generated from fixed seeds; all coordinates are finite and valid."""
import numpy as np

from pydegensac_amd import synthetic as syn

H_NS = (4, 5, 6, 7, 8, 9, 10)
H_VARIATIONS = ("clean", "noisy", "outliers", "quantised", "repeated")
H_BUDGETS = (1, 49, 50, 51, 300)             # around the 50-sample rule of the first local optimisation (exp_ranH.c ITER_SAM)
FEW_NS = (12, 64, 65, 200)
FEW_KS = (4, 5, 6)
F_NS = tuple(range(8, 17))
F_PLANE = (0.6, 1.0)
E_NS = (2, 3, 4, 5, 8, 9, 14)
E_LIMITS = (0, 4, 16)
E_BUDGETS = (1, 3, 50, 200)


def h_points(variation, n, laf, seed):
    """One homography pair of the tiny family."""
    if variation == "clean":
        p1, p2, _, _ = syn.homography_pairs(n, 1.0, 0.0, seed=seed, laf=laf)
    elif variation == "outliers":
        p1, p2, _, _ = syn.homography_pairs(n, 0.6, 0.3, seed=seed, laf=laf)
    else:
        p1, p2, _, _ = syn.homography_pairs(n, 1.0, 0.3, seed=seed, laf=laf)
    if variation == "quantised":
        p1[:, :2] = np.round(p1[:, :2]); p2[:, :2] = np.round(p2[:, :2])
    if variation == "repeated":
        k = max(1, n // 3)                   # rows 1..k repeat row 0 (tools/gpu_fuzz.py run_edges)
        p1[1:k + 1] = p1[0]; p2[1:k + 1] = p2[0]
    return p1, p2


def _group(kind, **kw):
    g = dict(kind=kind, A=[], B=[], seeds=[], tags=[])
    g.update(kw)
    return g


def h_tiny_groups():
    """n = 4..10 x five variations, crossed with metric 0..4, LAF rows on / off, symmetric check on / off, at every budget:
    100 groups of 35 pairs."""
    out = []; gi = 0
    for et in range(5):
        for laf in (False, True):
            for sym in (True, False):
                for mi in H_BUDGETS:
                    g = _group("H", px_th=1.5, conf=0.999, max_iters=mi, et=et, sym=sym, laf_coef=3.0 if laf else 0.0)
                    for vi, var in enumerate(H_VARIATIONS):
                        for n in H_NS:
                            # the points depend on (variation, n, metric, LAF, check) but not on the budget: the same pair is cut off
                            # at 1, 49, 50, 51 samples and run to its end
                            p1, p2 = h_points(var, n, laf, seed=1000 + 97 * (gi // len(H_BUDGETS)) + 10 * vi + n)
                            g["A"].append(p1); g["B"].append(p2); g["seeds"].append(7 + 31 * gi + 5 * vi + n)
                            g["tags"].append((var, n))
                    out.append(g); gi += 1
    return out


def h_few_groups():
    """Exactly 4, 5 or 6 rows follow one homography among n = 12, 64, 65, 200, the rest are outliers: the best sample's inlier
    list has that many entries when the local optimisation fits it, at sizes that are staged like any ordinary pair."""
    out = []
    for gi, (et, laf, sym, mi) in enumerate([(0, False, True, 300), (0, True, False, 51), (1, False, False, 300), (2, True, True, 300),
                                             (3, False, True, 50), (4, False, True, 300)]):
        g = _group("H", px_th=1.5, conf=0.999, max_iters=mi, et=et, sym=sym, laf_coef=3.0 if laf else 0.0)
        for n in FEW_NS:
            for k in FEW_KS:
                for rep in range(2):
                    p1, p2, _, _ = syn.homography_pairs(n, k / n, 0.1 * rep, seed=5000 + 100 * gi + 10 * k + rep + n, laf=laf)
                    g["A"].append(p1); g["B"].append(p2); g["seeds"].append(11 + 13 * gi + 3 * k + rep + n)
                    g["tags"].append((n, k))
        out.append(g)
    return out


def f_groups():
    """Fundamental matrices on 8 ... 16 correspondences, most or all of them on one plane: DEGENSAC's plane branch fits a homography
    to a short list."""
    out = []
    for gi, (et, sym, mi) in enumerate([(0, True, 300), (1, True, 300), (0, False, 51), (1, False, 50)]):
        g = _group("F", px_th=1.0, conf=0.9999, max_iters=mi, et=et, sym=sym, laf_coef=0.0, degen=True)
        for n in F_NS:
            for pf in F_PLANE:
                for rep in range(2):
                    p1, p2, _, _ = syn.two_view_fundamental(n, 1.0 if rep else 0.8, 0.1, seed=7000 + 100 * gi + 2 * n + rep, plane_fraction=pf)
                    g["A"].append(p1); g["B"].append(p2); g["seeds"].append(17 + 29 * gi + 2 * n + rep)
                    g["tags"].append((n, pf))
        out.append(g)
    return out


def e_groups():
    """ransacH2el on 2 ... 14 ellipse pairs: fit limit 0 / 4 / 16, local optimisation on / off, budgets 1 ... 200."""
    out = []; gi = 0
    for lim in E_LIMITS:
        for do_lo in (True, False):
            for mi in E_BUDGETS:
                g = _group("E", th=4.0, conf=0.99, max_iters=mi, do_lo=do_lo, inl_limit=lim, U=[])
                for n in E_NS:
                    for rep, (ir, sig) in enumerate([(1.0, 0.3), (0.7, 1.0)]):
                        g["U"].append(syn.ellipse_pairs(n, ir, sig, 9000 + 50 * gi + 2 * n + rep, 0.02)[0])
                        g["seeds"].append(3 + 7 * gi + 2 * n + rep); g["tags"].append((n, ir))
                out.append(g); gi += 1
    return out


FAMILIES = {"h_tiny": h_tiny_groups, "h_few": h_few_groups, "f": f_groups, "e": e_groups}
_groups = {}
_port = {}


def groups(name):
    """The groups of a family, generated once per process."""
    if name not in _groups:
        _groups[name] = FAMILIES[name]()
    return _groups[name]


def port_call(port, g, i):
    """The restatement on pair i of group g: (raw model [3, 3], mask, stats)."""
    if g["kind"] == "H":
        return port.find_homography(g["A"][i], g["B"][i], g["px_th"], g["conf"], g["max_iters"], g["et"], g["sym"], g["laf_coef"], seed=g["seeds"][i])
    if g["kind"] == "F":
        return port.find_fundamental(g["A"][i], g["B"][i], g["px_th"], g["conf"], g["max_iters"], g["et"], g["sym"], g["laf_coef"], g["degen"],
                                     seed=g["seeds"][i])
    return port.ransacH2el(g["U"][i], g["th"], g["conf"], g["max_iters"], g["do_lo"], g["inl_limit"], g["seeds"][i])


def port_results(port, name):
    """[group][pair] -> (model, mask, stats) of the restatement, computed once per process and shared by every test."""
    if name not in _port:
        _port[name] = [[port_call(port, g, i) for i in range(len(g["seeds"]))] for g in groups(name)]
    return _port[name]


def dump(path):
    """Every case of every family as one flat float64 .npy for the stand-alone MemorySanitizer program (oracle/port_msan_main.c has
    the record layout)."""
    rec = []
    for name in sorted(FAMILIES):
        for g in groups(name):
            for i, seed in enumerate(g["seeds"]):
                if g["kind"] == "E":
                    u = np.asarray(g["U"][i], float)
                    head = [2, u.shape[0], 10, seed, g["th"], g["conf"], g["max_iters"], int(g["do_lo"]), g["inl_limit"], 0, 0, 0]; data = [u.ravel()]
                else:
                    a = np.asarray(g["A"][i], float); b = np.asarray(g["B"][i], float)
                    head = [0 if g["kind"] == "H" else 1, a.shape[0], a.shape[1], seed, g["px_th"], g["conf"], g["max_iters"], g["et"], int(g["sym"]),
                            g["laf_coef"], int(g.get("degen", True)), 0]
                    data = [a.ravel(), b.ravel()]
                rec.append(np.asarray(head, float)); rec.extend(data)
    np.save(path, np.concatenate(rec))


def clean4_cases():
    """(group index, pair index) of the noise-free all-inlier n = 4 pairs of the tiny family: every metric, check and budget."""
    return [(gi, i) for gi, g in enumerate(groups("h_tiny")) for i, t in enumerate(g["tags"]) if t == ("clean", 4)]


def dlt4_float64(p1, p2):
    """Plain float64 DLT of four correspondences, independent of both restatements: the right singular vector of the 8 x 9 system
    [x2 x1^T, ... ] h = 0 for the matrix G with x1 ~ G x2 (the drivers' homography maps image 2 to image 1), returned in the driver's
    raw layout (column-wise: raw.reshape(3, 3) is G transposed), unit Frobenius norm."""
    rows = []
    for (x1, y1), (x2, y2) in zip(np.asarray(p1)[:, :2], np.asarray(p2)[:, :2]):
        X = np.array([x2, y2, 1.0])
        rows.append(np.r_[X, 0.0, 0.0, 0.0, -x1 * X])
        rows.append(np.r_[0.0, 0.0, 0.0, X, -y1 * X])
    _, _, vt = np.linalg.svd(np.array(rows))
    G = vt[-1].reshape(3, 3)
    return (G / np.linalg.norm(G)).T


def model_distance(M, R):
    """Frobenius distance of two homogeneous 3 x 3 models after scale and sign normalisation."""
    a = np.asarray(M, float).ravel(); b = np.asarray(R, float).ravel()
    a = a / np.linalg.norm(a); b = b / np.linalg.norm(b)
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


# Worst model_distance(restatement, dlt4_float64) over the 100 clean4_cases(), measured on the CPU (tests/test_small_sets_cpu.py prints
# it): 1.1808e-11.  The 8 x 9 system is built from raw pixel coordinates (the 4-point branch does not normalise), so its condition
# number, not the format, sets that figure.  The tests allow ten times the measured distance, for the restatement and the device alike.
DLT4_MEASURED = 1.1808e-11
DLT4_BOUND = 10 * DLT4_MEASURED
