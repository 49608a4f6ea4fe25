"""GPU: the cubic-root math of the 7-point solver as compiled for the device.  dg_cr_cos / dg_cr_acos / dg_cr_pow13 (dg_crmath.h,
mi_degensac_mat3 ops 8 / 9 / 10) must return the correctly rounded value from the DEVICE library's starting points, and dg_rroots3
(op 4) the restated operation sequence's bits on every branch and edge (tests/crmath_ref.py; fixture tests/golden/crmath_cr.npz,
which tests/test_crmath_fixture_cpu.py pins to the reference and to the host build of the header)."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib
from tests import crmath_ref as cr

pytestmark = pytest.mark.gpu

GUARD = -12345.678
I32 = C.POINTER(C.c_int32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run_op(op, x, ni=1, no=1):
    """one call of mi_degensac_mat3 on len(x) problems, with a guard element on each side of both host outputs -> (out, flag)"""
    x = np.ascontiguousarray(x, np.float64).reshape(-1, ni)
    n = len(x)
    inp = np.ascontiguousarray(np.concatenate([x.ravel(), [0.0]]))                    # never an empty buffer behind the pointer
    out = np.full(n * no + 2, GUARD); flag = np.full(n + 2, -77, np.int32)
    _lib.check(_lib.lib().mi_degensac_mat3(op, _lib.dptr(inp), n, 0, _lib.dptr(out[1:]), flag[1:].ctypes.data_as(I32)))
    assert out[0] == GUARD and out[-1] == GUARD and flag[0] == -77 and flag[-1] == -77, (op, n)
    return out[1:-1].reshape(n, no).copy(), flag[1:-1].copy()


@pytest.fixture(scope="module")
def cat():
    return cr.load()


@pytest.fixture(scope="module")
def full(cat):
    """ops 8 / 9 / 10 over the whole fixture, once"""
    res = {}
    for name, op in cr.OPS.items():
        y, flag = run_op(op, cat[name + "_x"])
        assert not flag.any(), name
        res[name] = y[:, 0]
    return res


def check_values(name, x, got, want):
    m = cr.bit_tested(name, x)
    bad = np.flatnonzero(bits(got)[m] != bits(want)[m])                                # int64 views: the sign of zero counts
    assert len(bad) == 0, (name, len(bad), int(m.sum()), [(float.hex(float(x[m][i])), float.hex(float(got[m][i])), float.hex(float(want[m][i]))) for i in bad[:8]])
    # outside the ranges the header rounds on it hands out the device library's value
    assert (np.abs(got[~m] - want[~m]) <= 1e-14 * np.abs(want[~m])).all(), (name, x[~m], got[~m], want[~m])


def check_cubics(po, nr_d, R, nr, roots, branch):
    assert np.array_equal(nr_d, nr), np.flatnonzero(nr_d != nr)[:8]
    bad = []
    for i in range(len(po)):
        k = int(nr[i]); g = R[i, :k]; w = roots[i, :k]
        if branch[i] == cr.FALLBACK:
            # the library's pow on both sides: to the scale, as tests/test_gpu_units.py holds the solver's roots; where the restated
            # root is not finite (A = 0 or inf) the device's is the same infinity or NaN
            fin = np.isfinite(w)
            with np.errstate(all="ignore"):
                scale = max(1.0, np.abs(w[fin]).max() if fin.any() else 0.0, abs(po[i, 1] / po[i, 0]) / 3)
            ok = np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[np.isinf(w)], w[np.isinf(w)]) \
                and (np.abs(g[fin] - w[fin]) <= 1e-14 * scale).all()
        else:
            ng, nw = np.isnan(g), np.isnan(w)
            ok = np.array_equal(ng, nw) and np.array_equal(bits(g)[~ng], bits(w)[~nw])
        if not ok:
            bad.append((i, cr.BRANCHES[int(branch[i])], po[i].tolist(), g.tolist(), w.tolist()))
    assert not bad, (len(bad), len(po), bad[:6])


def test_device_cos_acos_pow13_are_the_rounded_values_on_the_whole_fixture(cat, full):
    for name in cr.OPS:
        check_values(name, cat[name + "_x"], full[name], cat[name + "_y"])


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 129])
def test_counts_at_the_edges_of_the_64_lane_block(cat, full, count):
    for name, op in cr.OPS.items():
        y, flag = run_op(op, cat[name + "_x"][:count])                                 # run_op checks the guards
        assert y.shape == (count, 1) and not flag.any()
        assert np.array_equal(bits(y[:, 0]), bits(full[name][:count])), (name, count)


def test_device_rroots3_on_every_branch_and_edge_bit_for_bit(cat):
    po = cat["cubic_po"]
    R, nr_d = run_op(4, po, ni=4, no=3)
    check_cubics(po, nr_d, R, cat["cubic_nr"], cat["cubic_roots"], cat["cubic_branch"])
    for count in (1, 65):
        Rc, nc = run_op(4, po[:count], ni=4, no=3)
        assert np.array_equal(nc, nr_d[:count]) and np.array_equal(np.isnan(Rc), np.isnan(R[:count]))
        assert np.array_equal(bits(Rc)[~np.isnan(Rc)], bits(R[:count])[~np.isnan(Rc)])


def test_live_sample_from_another_seed_against_200_bit_arithmetic():
    pytest.importorskip("mpmath")
    for name, x in cr.live_args(seed=77, n=20000).items():
        y, _ = run_op(cr.OPS[name], x)
        check_values(name, x, y[:, 0], np.array([cr.CR[name](v) for v in x]))
    po = cr.live_cubics(seed=78, n=5000)
    res = [cr.rroots3(q) for q in po]
    R, nr_d = run_op(4, po, ni=4, no=3)
    check_cubics(po, nr_d, R, np.array([r[0] for r in res]), np.array([r[1] for r in res]), np.array([r[2] for r in res]))
