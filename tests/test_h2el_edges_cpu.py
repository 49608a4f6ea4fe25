"""CPU: the scenes of tests/test_gpu_h2el_edges.py must keep exercising the branches they were built for.  Everything here is asserted with
the restatement alone (oracle/port.py ransacH2el), through the builders of tests/h2el_ref.py that the GPU file uses."""
import numpy as np
import pytest

from tests import golden_util as gu
from tests import h2el_ref as hr

TH = hr.CALL["th"]


@pytest.fixture(scope="module")
def reuse():
    return hr.reuse_batch(hr.MI355X_CUS)


def test_reuse_batch_holds_every_kind_often_enough(oracle_port, reuse):
    U, seeds, kinds = reuse
    P = len(U)
    assert P == 2 * hr.MI355X_CUS + 3 and len(set(seeds)) == P
    assert all(len(U[i]) == hr.LONG_N for i in range(3, P, 7)) and kinds.count("L") == len(range(3, P, 7))
    assert sum(kinds[i + 1] != "L" and len(U[i + 1]) <= 60 for i in range(3, P - 1, 7)) >= 60        # a short pair right behind a long one
    assert all(np.isfinite(u).all() for u in U)
    n_a = n_b = n_c = 0
    for i, k in enumerate(kinds):
        res = {(lo, lim): hr.oracle(oracle_port, ("reuse", i), U[i], seeds[i], lo, lim) for lo, lim in hr.REUSE_SETTINGS}
        if k in "ab":
            # never a model, whatever the setting: zero model, the mask of the unwritten errs[3]; and errs[4] unwritten at the run after the loop
            assert all(hr.never_a_model(r) for r in res.values()), (i, k)
            assert hr.e4_never_written(oracle_port, ("reuse", i), U[i], seeds[i]), (i, k)
            assert all(res[s][2]["samples"] == hr.CALL["max_iters"] for s in res) and res[True, 0][2]["lo_runs"] == 1, (i, k)
            if k == "a":
                n_a += 1
                assert res[True, 0][2]["models"] <= 2, (i, res[True, 0][2])          # fewer than 8 rows: the repetitions do not start
            else:
                n_b += 1
                assert all(res[lo, lim][2]["models"] > 20 for lo, lim in hr.REUSE_SETTINGS if lo), (i, res[True, 0][2])     # they all ran
        elif k == "c":
            ok = not hr.e4_never_written(oracle_port, ("reuse", i), U[i], seeds[i])
            n_c += ok and all(res[lo, lim][2]["lo_runs"] >= 1 and res[lo, lim][2]["I"] >= 8 for lo, lim in hr.REUSE_SETTINGS if lo)
    assert n_a >= 8 and n_b >= 8 and n_c >= 8, (n_a, n_b, n_c)
    assert n_c >= 0.8 * kinds.count("c"), (n_c, kinds.count("c"))
    # the fit limit of 8 changes something in the batch, so the three runs are three runs
    assert any(not np.array_equal(hr.oracle(oracle_port, ("reuse", i), U[i], seeds[i], True, 0)[0],
                                  hr.oracle(oracle_port, ("reuse", i), U[i], seeds[i], True, 8)[0]) for i in range(P))
    ids = hr.reuse_sample(kinds)
    assert len(ids) == 24 and ids[0] == 0 and ids[-1] == P - 1 and all(i in ids for i, k in enumerate(kinds) if k in "abd")


def test_reuse_batch_builds_for_other_device_sizes():
    for cus in (32, 64, 120, 304):
        U, seeds, kinds = hr.reuse_batch(cus)
        assert len(U) == 2 * cus + 3 and (kinds.count("a"), kinds.count("b"), kinds.count("d")) == (8, 8, 4)
        assert len(hr.reuse_sample(kinds)) == 24


@pytest.mark.parametrize("n", hr.ROW_NS)
def test_row_count_scenes(oracle_port, n):
    both = 0
    for j in (0, 1):
        u, seed = hr.row_scene(n, j)
        assert u.shape == (n, 10) and np.isfinite(u).all()
        for lim in hr.ROW_LIMITS:
            H, m, s = hr.oracle(oracle_port, ("row", n, j), u, seed, True, lim)
            assert s["lo_runs"] >= 1
            want, close = hr.mask_from_model(H, u, TH)
            assert close.sum() <= 0.01 * n, (n, j, lim, int(close.sum()))
            if H.any():
                assert np.array_equal(want[~close], m[~close]), (n, j, lim)      # hds() is the restatement's HDs
            both += bool(m.any() and not m.all())
    if n >= 8:
        assert both == 4, (n, both)                    # (2 rows are one sample, and 3 rows leave one row to differ: no such demand there)
    if n >= 63:
        # a local optimisation whose repetitions ran (8 inliers or more), under both limits
        assert all(any(hr.oracle(oracle_port, ("row", n, j), *hr.row_scene(n, j), True, lim)[2]["I"] >= 8 for j in (0, 1)) for lim in hr.ROW_LIMITS)


def test_row_batches_hold_every_count_in_both_orders():
    for desc in (False, True):
        U, seeds, keys = hr.row_batch(desc)
        ns = [len(u) for u in U]
        assert ns == sorted(ns, reverse=desc) and set(ns) == set(hr.ROW_NS) and len(U) == 2 * len(hr.ROW_NS)
        assert all(np.array_equal(U[i], hr.row_scene(*k)[0]) and seeds[i] == hr.row_scene(*k)[1] for i, k in enumerate(keys))
    U, seeds = hr.dev_batch()
    assert [len(u) for u in U] == list(hr.DEV_NS) and 2 in hr.DEV_NS and 2049 in hr.DEV_NS and len(U) == 6


def test_fit_limit_scene_separates_the_list_length_from_one_below(oracle_port):
    u, lab = hr.limit_scene()
    L = hr.LIMIT_L
    assert u.shape == (hr.LIMIT_N, 10) and np.isfinite(u).all()
    r = {lim: hr.oracle(oracle_port, "limit", u, hr.LIMIT_SEED, True, lim, th=hr.LIMIT_TH) for lim in (L - 1, L, L + 1, 0)}
    assert np.array_equal(r[0][1], lab) and r[0][2]["I"] == L          # the inliers and nothing else
    for lim in (L, L + 1):
        # a list of L rows is not cut at a limit of L: no draw, the same run as without a limit
        assert np.array_equal(r[lim][0], r[0][0]) and np.array_equal(r[lim][1], r[0][1]) and r[lim][2] == r[0][2], lim
    # ... and at L - 1 it is: the fit runs on a random 29 of the 30, further apart than two results within 1e-6 of one model can be
    assert r[L - 1][2]["samples"] != r[L][2]["samples"] or gu.rel(r[L - 1][0], r[L][0]) > 3e-6, gu.rel(r[L - 1][0], r[L][0])


def test_duplicate_scene_has_samples_of_two_identical_rows(oracle_port):
    u = hr.duplicate_scene()
    assert u.shape == (40, 10) and np.isfinite(u).all()
    assert len(np.unique(u, axis=0)) == 30
    H, m, s = hr.oracle(oracle_port, "dup", u, hr.DUP_SEED, True, 0)
    assert s["lo_runs"] >= 1 and H.any() and m.any() and not m.all()
    # without local optimisation every scored sample is one model, so samples - models counts the samples that were turned down (with it
    # `models` also counts the models of the local optimisation)
    s0 = hr.oracle(oracle_port, "dup", u, hr.DUP_SEED, False, 0)[2]
    assert s0["samples"] > s0["models"]
    # a sample of two identical rows is turned down by the null-space test: two copies of one row alone never give a model
    two = np.ascontiguousarray(np.repeat(u[:1], 2, axis=0))
    s2 = hr.oracle(oracle_port, "dup-two", two, hr.DUP_SEED, False, 0)
    assert s2[2]["models"] == 0 and s2[2]["samples"] == hr.CALL["max_iters"] and not s2[0].any()
