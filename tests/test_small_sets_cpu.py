"""CPU: the restatement (oracle/dg_oracle.c) as an oracle for the smallest sets — the families of tests/small_sets.py.  The unmodified
reference reads uninitialised memory in the 4-point branch of u2h (Htools.c:106-114), so it cannot be the yardstick there; the
restatement zero-fills.  These tests show that it is repeatable on those inputs, that the inputs really run the 4-point
fit and the short-list least squares (counters `u2h_4pt`, `u2h_short`), and that the 4-point fit is a homography fit at all: a plain
numpy DLT agrees.  tests/test_gpu_small_sets.py then compares the device with it on the same inputs."""
import numpy as np
import pytest

from tests import small_sets as ss


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("family", sorted(ss.FAMILIES))
def test_port_is_repeatable_with_a_dirtied_heap(oracle_port, family):
    """Model bits, mask and every counter of a second call equal the first, with a few MB of garbage allocated, written and freed in
    between (a read of memory the call did not write would see other bytes the second time)."""
    first = ss.port_results(oracle_port, family)
    rng = np.random.default_rng(5)
    bad = []
    for gi, g in enumerate(ss.groups(family)):
        junk = [rng.integers(0, 255, size, dtype=np.uint8) for size in (1 << 12, 1 << 16, 1 << 20, 3 << 20)]
        for j in junk:
            j[:] = 0xA5
        del junk
        for i in range(len(g["seeds"])):
            if not _same(first[gi][i], ss.port_call(oracle_port, g, i)):
                bad.append((gi, i, g["tags"][i]))
    assert not bad, (len(bad), bad[:10])


def test_four_point_fit_is_reached_in_every_family(oracle_port):
    """The counters behind the GPU tests' claim to cover the 4-point fit.  Measured: all 500 tiny H cases with n = 4; 11 or 12 of the
    12 pairs of every (n, 4) of the four-consistent-rows family; 16 of the 112 ransacH2el cases with a fit limit of 4; and the F
    family reaches it too (28 of its 144 pairs, through DEGENSAC's plane branch), so nothing had to be searched for."""
    def count(name, pick, key="u2h_4pt"):
        return sum(st[key] > 0 for g, r in zip(ss.groups(name), ss.port_results(oracle_port, name))
                   for t, (_, _, st) in zip(g["tags"], r) if pick(g, t))
    assert count("h_tiny", lambda g, t: t[1] == 4) == sum(t[1] == 4 for g in ss.groups("h_tiny") for t in g["tags"])
    for n in ss.H_NS[1:]:
        assert count("h_tiny", lambda g, t: t[1] == n, "u2h_short") > 0, n
    for n in ss.FEW_NS:
        assert count("h_few", lambda g, t: t == (n, 4)) > 0, n
        assert count("h_few", lambda g, t: t[0] == n) > count("h_few", lambda g, t: t == (n, 4)), n     # lists of 5 and 6 that shrink to 4
    assert count("e", lambda g, t: g["inl_limit"] == 4) > 0
    assert count("e", lambda g, t: g["inl_limit"] == 4, "u2h_short") > 0
    assert count("f", lambda g, t: True) > 0
    assert count("f", lambda g, t: True, "u2h_short") > 0
    # every tiny H call ran a local optimisation: the 4-point fit above is the one inside it (or the least squares before it)
    assert all(st["lo_runs"] > 0 for r in ss.port_results(oracle_port, "h_tiny") for _, _, st in r)


def test_four_point_fit_against_a_plain_float64_dlt(oracle_port):
    """noise-free, all inliers, n = 4: the returned model is the 4-point fit of the four rows; numpy's SVD of the 8 x 9 system,
    scale- and sign-normalised, is independent of both restatements.  Every one of the cases returns a model (one sample suffices)."""
    G = ss.groups("h_tiny"); R = ss.port_results(oracle_port, "h_tiny"); worst = 0.0
    cases = ss.clean4_cases()
    assert len(cases) == 100
    for gi, i in cases:
        M, mask, st = R[gi][i]
        assert np.abs(M).sum() > 0 and mask.all() and st["u2h_4pt"] > 0, (gi, i)
        worst = max(worst, ss.model_distance(M, ss.dlt4_float64(G[gi]["A"][i], G[gi]["B"][i])))
    print(f"worst distance of the restatement to the float64 DLT: {worst:.4e} (bound {ss.DLT4_BOUND:.4e})")
    assert worst <= ss.DLT4_BOUND


def test_zero_filled_four_point_branch_returns_the_last_unit_vector(oracle_port):
    """What the documented convention amounts to.  lin_hg's 9 x 8 block is transposed as if it were 9 x 9, so the nine
    never-written entries 72..80 become column 8; zero-filled, that column is free and the null vector is (0, ..., 0, 1) whatever the
    four points are.  u2h's 4-point branch therefore never yields a model that scores, and a driver-level comparison sees a wrong
    4-point fit only when the fit is wrong in a way that scores (a restatement that transposes the 8 x 9 system properly differs in
    636 of the 3500 tiny H cases and 31 of the 336 ellipse cases; one that leaves out either zero-fill, or the transposition, in
    none).  The models the float64 DLT test checks are the minimal-sample fits of the main loop, which build their 9 x 9 system row by row."""
    import ctypes as C
    G = ss.groups("h_tiny"); inl = np.arange(4, dtype=np.int32)
    for gi, i in ss.clean4_cases()[:20]:
        p1, p2 = G[gi]["A"][i][:, :2], G[gi]["B"][i][:, :2]
        u = np.ascontiguousarray(np.c_[p1, np.ones(4), p2, np.ones(4)]); H = np.full(9, 7.0)
        oracle_port.lib().dg_oracle_u2h(oracle_port.dp(u), oracle_port.ip(inl), 4, oracle_port.dp(H))
        assert np.array_equal(np.abs(H), np.r_[np.zeros(8), 1.0]), (gi, i, H)
