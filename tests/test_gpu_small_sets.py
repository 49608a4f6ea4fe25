"""GPU: the drivers on their smallest inputs — homographies on 4 ... 10 correspondences, inlier lists of 4 ... 6 inside larger sets,
fundamental matrices on 8 ... 16, ransacH2el on 2 ... 14 ellipse pairs — against the CPU restatement, which zero-fills in the 4-point
branch of u2h exactly as the device does (the unmodified reference reads uninitialised memory there, so its goldens cannot
serve).  tests/small_sets.py has the input families; tests/test_small_sets_cpu.py shows that the restatement is repeatable on them and
that they run the 4-point fit and the short-list least squares (dg_u2h_4pt_mv, dg_lsq.h "len <= 10").  The device follows the oracle's
trajectory — equal counters below — so where the oracle ran those fits the device ran them too.

Every family goes through ragged batch launches (one per group of pairs that share the launch parameters), in each of the three
workgroup-size variants: a pair here has fewer rows than a wave has lanes."""
import numpy as np
import pytest

import pydegensac_amd as pd
from pydegensac_amd import _lib, api
from pydegensac_amd import synthetic as syn
from tests import small_sets as ss

pytestmark = pytest.mark.gpu

VARIANT = {512: _lib.TUNE_LATENCY, 256: _lib.TUNE_THROUGHPUT, 128: _lib.TUNE_THROUGHPUT4}
H_KEYS = ("samples", "lo_runs", "rejected", "I", "models", "best_sample")
F_KEYS = H_KEYS + ("degen", "Ih", "full_passes", "ex_passes")
E_KEYS = ("samples", "lo_runs", "I", "models")
_dev = {}


def _launch(g, tuning=0, flags=0, pick=None):
    """one ragged batch launch of a group (or of the pairs `pick` of it): (models [P, 3, 3], masks, stats)"""
    idx = range(len(g["seeds"])) if pick is None else pick
    seeds = [g["seeds"][i] for i in idx]
    if g["kind"] == "E":
        M, m = pd.ransacH2el_batch([g["U"][i] for i in idx], g["th"], g["conf"], g["max_iters"], g["do_lo"], g["inl_limit"], seeds=seeds, raw=True)
    else:
        M, m = api._batch(g["kind"], [g["A"][i] for i in idx], [g["B"][i] for i in idx], g["px_th"], g["conf"], g["max_iters"], g["et"], g["sym"],
                          g["laf_coef"], g.get("degen", True), seeds, 0, tuning, flags)
    return np.asarray(M).copy(), [np.asarray(x).copy() for x in m], pd.last_stats()


def device_results(family, variant):
    """[group] -> (models, masks, stats) of one variant (0: the library's own choice), computed once per process"""
    if (family, variant) not in _dev:
        _dev[family, variant] = [_launch(g, VARIANT.get(variant, 0)) for g in ss.groups(family)]
    return _dev[family, variant]


def _mismatches(family, dev, ref, keys):
    """the assertions of tools/gpu_fuzz.py, pair by pair: shared counters equal, mask bit for bit, raw model within 1e-9 relative
    Frobenius; where the oracle found no model, nine zeros and an all-false mask"""
    bad = []
    for gi, g in enumerate(ss.groups(family)):
        M, masks, st = dev[gi]
        for i in range(len(g["seeds"])):
            Mo, mo, so = ref[gi][i]; Mg = M[i].ravel(); Mo = np.asarray(Mo, float).ravel()
            diff = {k: (st[i][k], so[k]) for k in keys if st[i][k] != so[k]}
            if st[i].get("discarded") or st[i].get("rerun"):
                diff["discarded/rerun"] = (st[i].get("discarded"), st[i].get("rerun"))
            if np.abs(Mo).sum() == 0:
                # ransacH2el's raw mask is "residual <= th" over a zero-filled buffer then, on both sides (dg_kernel_h2el.h): still equal
                ok = np.abs(Mg).sum() == 0 and (np.array_equal(masks[i], mo) if g["kind"] == "E" else not masks[i].any()); rel = float(np.abs(Mg).sum())
            else:
                rel = np.linalg.norm(Mg - Mo) / np.linalg.norm(Mo)
                ok = np.array_equal(masks[i], mo) and rel < 1e-9
            if diff or not ok:
                bad.append((gi, i, g["tags"][i], "rel %.3g" % rel, diff))
    return bad


def _same_bits(a, b):
    return all(np.array_equal(x[0], y[0], equal_nan=True) and all(np.array_equal(p, q) for p, q in zip(x[1], y[1])) for x, y in zip(a, b))


@pytest.mark.parametrize("family,keys", [("h_tiny", H_KEYS), ("h_few", H_KEYS), ("f", F_KEYS)], ids=["h_tiny", "h_few", "f"])
def test_family_matches_port_in_every_variant(oracle_port, family, keys):
    """h_tiny: n = 4..10 x {noise-free, noisy, outliers, whole pixels, repeated rows} x metric 0..4 x LAF rows x symmetric check at
    budgets 1 / 49 / 50 / 51 / 300 (3500 pairs, 100 launches per variant); h_few: 4, 5, 6 consistent rows among 12 / 64 / 65 / 200;
    f: 8..16 correspondences on or near one plane, with the F counters of the sweep.  The three variants must agree to the bit."""
    ref = ss.port_results(oracle_port, family)
    for variant in (512, 256, 128):
        bad = _mismatches(family, device_results(family, variant), ref, keys)
        assert not bad, (variant, len(bad), bad[:8])
    assert _same_bits(device_results(family, 512), device_results(family, 256))
    assert _same_bits(device_results(family, 512), device_results(family, 128))


def test_single_call_path_equals_the_batch(oracle_port):
    """pd.findHomography_ on one pair per n and per metric (noisy, all inliers, no LAF rows, symmetric check, budget 300): model bits,
    mask and counters of the pair's batch result"""
    G = ss.groups("h_tiny"); dev = device_results("h_tiny", 0); seen = set()
    for gi, g in enumerate(G):
        if g["laf_coef"] or not g["sym"] or g["max_iters"] != 300:
            continue
        for i, tag in enumerate(g["tags"]):
            if tag[0] != "noisy":
                continue
            H, m = pd.findHomography_(g["A"][i], g["B"][i], g["px_th"], g["conf"], g["max_iters"], g["et"], g["sym"], g["laf_coef"], seed=g["seeds"][i])
            st = pd.last_stats(); seen.add((g["et"], tag[1]))
            assert np.array_equal(np.asarray(H), dev[gi][0][i]), (g["et"], tag)
            assert np.array_equal(np.asarray(m), dev[gi][1][i]), (g["et"], tag)
            assert all(st[k] == dev[gi][2][i][k] for k in H_KEYS), (g["et"], tag)
    assert seen == {(et, n) for et in range(5) for n in ss.H_NS}
    assert not _mismatches("h_tiny", dev, ss.port_results(oracle_port, "h_tiny"), H_KEYS)


def test_tiny_pairs_between_long_pairs_equal_their_own_batches():
    """thirty pairs of 4 ... 10 rows interleaved with three of 3000 rows, helper workgroups on and off: every pair as in a batch of
    its own"""
    g = dict(kind="H", px_th=1.5, conf=0.999, max_iters=1000, et=0, sym=True, laf_coef=0.0, A=[], B=[], seeds=[], tags=[])
    for i in range(33):
        if i % 11 == 5:
            p1, p2, _, _ = syn.homography_pairs(3000, 0.25, 0.5, seed=400 + i); n = 3000
        else:
            n = ss.H_NS[i % 7]; p1, p2 = ss.h_points(ss.H_VARIATIONS[i % 5], n, False, seed=400 + i)
        g["A"].append(p1); g["B"].append(p2); g["seeds"].append(21 + i); g["tags"].append(n)
    assert sorted(g["tags"]).count(3000) == 3 and len(g["tags"]) == 33
    own = [_launch(g, pick=[i]) for i in range(33)]
    for flags in (0, _lib.FLAG_NO_HJOB):
        M, masks, st = _launch(g, flags=flags)
        for i in range(33):
            assert np.array_equal(M[i], own[i][0][0]), (flags, i, g["tags"][i])
            assert np.array_equal(masks[i], own[i][1][0]), (flags, i, g["tags"][i])
            assert all(st[i][k] == own[i][2][0][k] for k in H_KEYS), (flags, i, g["tags"][i])
            assert not st[i].get("discarded") and not st[i].get("rerun"), (flags, i)
    assert any(np.abs(own[i][0][0]).sum() > 0 for i in range(33) if g["tags"][i] == 3000)


def test_ellipse_family_matches_port(oracle_port):
    """ransacH2el on 2 ... 14 ellipse pairs, fit limit 0 / 4 / 16 (the limit of 4 sends every fit of the local optimisation through the
    4-point branch), LO on / off, budgets 1 / 3 / 50 / 200"""
    bad = _mismatches("e", device_results("e", 0), ss.port_results(oracle_port, "e"), E_KEYS)
    assert not bad, (len(bad), bad[:8])


def test_ellipse_seeded_sweep(oracle_port):
    """tools/gpu_fuzz_h2el.py in small: six random ragged batches, sizes 9 ... 1500, no pair skipped"""
    rng = np.random.default_rng(11); bad = []; tot = 0
    for b in range(6):
        P = int(rng.integers(1, 12)); U = []
        for i in range(P):
            n = int(rng.choice([9, 14, 30, 100, 400, 1500])); ir = float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.7]))
            U.append(syn.ellipse_pairs(n, ir, float(rng.choice([0.3, 1.0, 2.0])), 200000 + 100 * b + i, float(rng.choice([0.0, 0.05, 0.2])))[0])
        seeds = [int(x) for x in rng.integers(1, 2**31 - 1, P)]
        do_lo = bool(rng.random() < 0.8); lim = int(rng.choice([0, 4, 16, 40])); th = float(rng.choice([0.01, 1.0, 4.0, 9.0], p=[0.1, 0.3, 0.3, 0.3]))
        mi = int(rng.choice([1, 3, 49, 50, 51, 200, 2000])); conf = float(rng.choice([0.95, 0.99, 0.999]))
        H, m = pd.ransacH2el_batch(U, th, conf, mi, do_lo, lim, seeds=seeds, raw=True); st = pd.last_stats()
        for p in range(P):
            Ho, mo, so = oracle_port.ransacH2el(U[p], th, conf, mi, do_lo, lim, seeds[p]); tot += 1
            a = np.asarray(H[p]).ravel(); o = np.asarray(Ho).ravel()
            if np.abs(o).sum() == 0:
                ok = np.abs(a).sum() == 0 and np.array_equal(np.asarray(m[p]), mo)
            else:
                ok = np.array_equal(np.asarray(m[p]), mo) and np.linalg.norm(a - o) / np.linalg.norm(o) < 1e-9
            if not ok or any(st[p][k] != so[k] for k in E_KEYS):
                bad.append((b, p, U[p].shape[0], do_lo, lim, th, mi, seeds[p]))
    assert tot >= 6 and not bad, (len(bad), bad[:8])


def test_four_point_models_against_a_plain_float64_dlt():
    """noise-free, all inliers, n = 4: every variant's model against numpy's SVD of the 8 x 9 system, with the bound measured for the
    restatement on the CPU (tests/small_sets.py DLT4_BOUND)"""
    G = ss.groups("h_tiny"); worst = 0.0
    for variant in (512, 256, 128):
        dev = device_results("h_tiny", variant)
        for gi, i in ss.clean4_cases():
            M = dev[gi][0][i]
            assert np.abs(M).sum() > 0 and dev[gi][1][i].all(), (variant, gi, i)
            worst = max(worst, ss.model_distance(M, ss.dlt4_float64(G[gi]["A"][i], G[gi]["B"][i])))
    print(f"worst distance of a device model to the float64 DLT: {worst:.4e} (bound {ss.DLT4_BOUND:.4e})")
    assert worst <= ss.DLT4_BOUND
