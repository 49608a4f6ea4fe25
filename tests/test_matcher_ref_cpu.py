"""CPU: the float64 check of tests/matcher_ref.py on the numpy oracle itself, over every width, shape and family that
test_gpu_matcher_shapes.py runs on the device — the oracle alone satisfies the derived bound g = (dim + 2) * 2**-24 on every query
of every input before a GPU is involved — and on three deliberately broken oracles, which the check must reject (a check that
cannot fail would make the GPU tests worthless).  Also: the non-finite rule of oracle/matcher_np.py, and the split cases the GPU
tests claim, from the restated launch rule at the MI355X's 256 CUs."""
import numpy as np
import pytest

from oracle import matcher_np as mo
from tests import matcher_ref as mr


def _check_oracle(a, b, norm):
    idx, dist = mo.knn2(a, b, norm)
    mr.check_knn2_against_exact(idx, dist, a, b, norm)
    return idx, dist


@pytest.mark.parametrize("family", mr.L2_FAMILIES)
@pytest.mark.parametrize("dim", mr.L2_DIMS)
def test_oracle_inside_the_bound_width_sweep_l2(dim, family):
    a, b = mr.descs(1, *mr.WIDTH_SHAPE, dim, family)
    _check_oracle(a, b, "l2")


@pytest.mark.parametrize("nbytes", mr.HAMMING_BYTES)
def test_oracle_exact_width_sweep_hamming(nbytes):
    a, b = mr.descs(2, *mr.WIDTH_SHAPE, nbytes, "hamming")
    _check_oracle(a, b, "hamming")


@pytest.mark.parametrize("n2", mr.ROW_N2)
def test_oracle_inside_the_bound_row_sweep(n2):
    for n1 in mr.ROW_N1:
        for family in mr.L2_FAMILIES:
            a, b = mr.descs(3, n1, n2, mr.ROW_L2_DIM, family)
            _check_oracle(a, b, "l2")
        a, b = mr.descs(4, n1, n2, mr.ROW_HAMMING_BYTES, "hamming")
        _check_oracle(a, b, "hamming")


@pytest.mark.parametrize("case", mr.SPLIT_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_split_shapes_hit_the_cases_they_claim_and_the_oracle_is_inside_the_bound(case):
    n1, n2, dim, (left, right), want_single, want_batch = case
    t_chunk, splits = mr.single_split(n1, n2)
    assert mr.split_case(mr.split_rows(n2, t_chunk, splits)) == want_single
    t_chunk, splits = mr.batch_split([left[0], n1, right[0]], [left[1], n2, right[1]])
    assert mr.split_case(mr.split_rows(n2, t_chunk, splits)) == want_batch
    a, b = mr.descs(5, n1, n2, dim, "normal")
    _check_oracle(a, b, "l2")


# ---- the check can fail: three broken oracles ------------------------------------------------------------------------------
def _skip_last_word(a, b, norm):
    if a.shape[1] == 1:
        return mo.knn2(np.zeros_like(a), np.zeros_like(b), norm)      # nothing is left of a one-word row
    return mo.knn2(a[:, :-1], b[:, :-1], norm)


def _skip_last_row(a, b, norm):
    return mo.knn2(a, b[:-1], norm)


def _swapped(a, b, norm):
    idx, dist = mo.knn2(a, b, norm)
    return idx[:, ::-1].copy(), dist[:, ::-1].copy()


@pytest.mark.parametrize("mutant", [_skip_last_word, _skip_last_row, _swapped])
@pytest.mark.parametrize("norm,dim,family", [("l2", 1, "normal"), ("l2", 65, "normal"), ("l2", 129, "sift"), ("l2", 512, "tiny"),
                                             ("hamming", 5, "hamming"), ("hamming", 260, "hamming")])
def test_the_check_rejects_a_broken_oracle(mutant, norm, dim, family):
    a, b = mr.descs(6, *mr.WIDTH_SHAPE, dim, family)
    _check_oracle(a, b, norm)                                         # the sound oracle passes on the same input
    idx, dist = mutant(a, b, norm)
    with pytest.raises(AssertionError):
        mr.check_knn2_against_exact(idx, dist, a, b, norm)


def test_the_check_rejects_a_wrong_gate_and_a_spurious_minus_one():
    a, b = mr.descs(7, 40, 90, 33, "normal")
    rng = np.random.default_rng(7)
    gate = rng.random((40, 90)) < 0.1
    gate[0] = False; gate[1] = False; gate[1, 17] = True              # no candidate, one candidate
    idx, dist = mo.top2(mo.dist_matrix(a, b, "l2"), gate)
    mr.check_knn2_against_exact(idx, dist, a, b, "l2", gate)
    assert (idx[0] == -1).all() and idx[1, 0] == 17 and idx[1, 1] == -1
    with pytest.raises(AssertionError):                               # the ungated answer is not the gated one
        mr.check_knn2_against_exact(*mo.knn2(a, b, "l2"), a, b, "l2", gate)
    bad = idx.copy(); bad[5] = -1
    with pytest.raises(AssertionError):
        mr.check_knn2_against_exact(bad, dist, a, b, "l2", gate)


# ---- the non-finite rule ---------------------------------------------------------------------------------------------------
def test_oracle_non_finite_distances_are_not_neighbours():
    a, b = mr.descs(8, 6, 12, 9, "normal")
    ref_i, ref_d = mo.knn2(a, b[[0, 1, 2, 3, 8, 9, 10, 11]], "l2")   # what is left when rows 4..7 are no neighbours
    b[4, 2] = np.nan; b[5, 0] = np.inf; b[6, 8] = -np.inf; b[7, 3] = 3e19          # (3e19)^2 overflows fp32
    idx, dist = mo.knn2(a, b, "l2")
    remap = np.array([0, 1, 2, 3, 8, 9, 10, 11])
    assert np.array_equal(idx, remap[ref_i]) and np.array_equal(dist.view(np.uint32), ref_d.view(np.uint32))
    a[2, 1] = np.nan; a[3, 1] = np.inf                                # a query with no finite distance at all
    idx, dist = mo.knn2(a, b, "l2")
    assert (idx[2:4] == -1).all() and np.isposinf(dist[2:4]).all()
    assert len(mo.match_snn(a, b, 0.9, mutual=True)[0]) == len(mo.match_snn(a[[0, 1, 4, 5]], b, 0.9, mutual=True)[0])
    one = np.full((1, 9), np.inf, np.float32)                         # inf against inf: NaN
    idx, dist = mo.knn2(one, np.concatenate([one, b[:1]]), "l2")
    assert (idx == -1).all() and np.isposinf(dist).all()
