"""tests/golden/crmath_cr.npz, the fixture the GPU tests of the cubic-root math read (tests/test_gpu_crmath.py), and the reference that
makes it (tests/crmath_ref.py): the fixture is what a rebuild gives, its catalogue visits every branch and edge of rroots3
(Ftools.c:251-298), the host build of dg_crmath.h equals it, and the restated rroots3 is the oracle's operation sequence -- it differs
from a host run only where the host's libm misrounds."""
import ctypes as C
import ctypes.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")
from tests import crmath_ref as cr                                   # noqa: E402

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pydegensac_amd", "csrc", "dg_crmath.h")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(a, b):
    """bit for bit; a NaN equals a NaN (0/0 is -nan on x86 and +nan elsewhere)"""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


@pytest.fixture(scope="module")
def cat():
    return cr.load()


@pytest.fixture(scope="module")
def libm():
    l = C.CDLL(ctypes.util.find_library("m"))
    for f in (l.cos, l.acos):
        f.restype = C.c_double; f.argtypes = [C.c_double]
    l.pow.restype = C.c_double; l.pow.argtypes = [C.c_double, C.c_double]
    return {"cos": lambda x: l.cos(float(x)), "acos": lambda x: l.acos(float(x)), "pow13": lambda x: l.pow(float(x), 1.0 / 3)}


def test_committed_fixture_equals_a_rebuild_byte_for_byte():
    with open(cr.FIXTURE, "rb") as f:
        have = f.read()
    assert have == cr.fixture_bytes()
    assert len(have) < 100 * 1024


def test_catalogue_visits_every_branch_and_edge_of_rroots3(cat):
    po = cat["cubic_po"]; br = cat["cubic_branch"]
    for k in cr.BRANCHES:
        assert (br == k).sum() >= 16, (cr.BRANCHES[k], int((br == k).sum()))
    hi = lo = qz = nan = 0
    for i, q in enumerate(po):
        info = {}
        nr, r, b = cr.rroots3(q, info=info)
        assert nr == cat["cubic_nr"][i] and b == br[i] and same_bits(r, cat["cubic_roots"][i]), i
        hi += info["clamp"] > 0; lo += info["clamp"] < 0
        qz += nr == 3 and info["q_zero"] and not np.isnan(r).any()
        nan += nr == 3 and bool(np.isnan(r).all())
    assert hi >= 4 and qz >= 4 and nan >= 1, (hi, qz, nan)
    # the lower clamp (cos phi < -1) cannot be taken: R = e sqrt(-p) carries the sign e of q (e = -1 for q <= 0 and for NaN), so
    # q / (R R R) is >= +0, -0 (q == 0) or NaN for every input.  No catalogue can visit it; what it can meet is that none claims to
    assert lo == 0, lo
    for name in cr.CR:
        x = cat[name + "_x"]
        assert len(x) >= 1024 and cr.bit_tested(name, x).sum() >= 1024, name
    assert (~cr.bit_tested("pow13", cat["pow13_x"])).sum() == 10 and (~cr.bit_tested("cos", cat["cos_x"])).sum() == 4


def test_host_build_of_the_header_equals_the_fixture(cat):
    d = tempfile.mkdtemp()
    src = os.path.join(d, "h.c")
    with open(src, "w") as f:
        f.write(f'#include "{HDR}"\n' + "".join(
            f"void v_{n}(const double *x, int n, double *o) {{ for (int i = 0; i < n; i++) o[i] = dg_cr_{n}(x[i]); }}\n" for n in cr.CR))
    so = os.path.join(d, "h.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src, "-lm"])
    L = C.CDLL(so); dp = C.POINTER(C.c_double)
    for name in cr.CR:
        x = np.ascontiguousarray(cat[name + "_x"]); out = np.zeros_like(x)
        getattr(L, "v_" + name)(x.ctypes.data_as(dp), len(x), out.ctypes.data_as(dp))
        m = cr.bit_tested(name, x)
        bad = np.flatnonzero(bits(out)[m] != bits(cat[name + "_y"])[m])
        assert len(bad) == 0, (name, [float.hex(float(v)) for v in x[m][bad][:8]])
        assert np.allclose(out[~m], cat[name + "_y"][~m], rtol=1e-14, atol=0), name


def test_restated_rroots3_is_the_oracles_sequence_and_differs_only_where_libm_misrounds(cat, libm, oracle_port):
    P = oracle_port.lib(); dp = oracle_port.dp
    po = cat["cubic_po"]
    n_diff = 0; n_cmp = 0
    for i, q in enumerate(po):
        want = np.zeros(3); nr = P.dg_oracle_rroots3(dp(np.ascontiguousarray(q)), dp(want))
        # with the host libm's functions in it the restatement is a host run of the reference: every bit, every cubic
        il = {}
        nl, rl, _ = cr.rroots3(q, fns=libm, info=il)
        assert nl == nr and same_bits(rl[:nr], want[:nr]), (i, q, rl, want)
        ic = {}
        nc, rc, br = cr.rroots3(q, info=ic)
        assert nc == nr == cat["cubic_nr"][i], i
        if br == cr.FALLBACK:
            continue
        for k in range(nr):
            n_cmp += 1
            if same_bits(rc[k], want[k]):
                continue
            n_diff += 1
            # the calls behind root k: pow, or acos and the root's own cos.  The first one where the two runs part had the same
            # argument in both; there the host's value, not the restatement's, is off the rounded exact value
            chain = [0] if nr == 1 else [0, 1 + k]
            first = next((j for j in chain if il["calls"][j][2] != ic["calls"][j][2]), None)
            assert first is not None, (i, k, "roots differ although every call agrees")
            name, x, host = il["calls"][first]
            assert ic["calls"][first][:2] == (name, x), (i, k)
            mp.mp.prec = 200
            exact = {"cos": mp.cos, "acos": mp.acos, "pow13": lambda v: mp.power(v, mp.mpf(1.0 / 3))}[name](mp.mpf(x))
            assert cr._round(exact) == ic["calls"][first][2] and host != cr._round(exact), (i, k, name, x)
            assert abs(exact - mp.mpf(ic["calls"][first][2])) < abs(exact - mp.mpf(host)), (i, k, name, x)
    assert n_cmp > 800
    print(f"rroots3 restated against the oracle: {n_diff} of {n_cmp} roots differ, each by one misrounded libm call")


def test_solve7_scene_oracle_and_restatement_pass_the_same_roots(oracle_port):
    """the premise of tests/test_gpu_units.py::test_solve7_matches_oracle_nullspace_cubic_and_orientation: on its scene the host's
    roots and the restated ones send the same roots through the oriented-epipolar test in all but at most 1 % of the samples"""
    p1, p2, u, samples = cr.solve7_scene()
    cases = cr.solve7_oracle(oracle_port, u, samples)
    n = 0; n_skip = 0
    for t, c in cases.items():
        if c is None:
            continue
        f1, f2, poly, nr, roots = c
        n += 1
        nr_r, roots_r, _ = cr.rroots3(poly)
        assert nr_r == nr, t
        a = [i for i, _ in cr.solve7_models(oracle_port, u, samples[t], f1, f2, nr, roots)]
        b = [i for i, _ in cr.solve7_models(oracle_port, u, samples[t], f1, f2, nr_r, roots_r)]
        n_skip += a != b
    print(f"solve7 scene: {n_skip} of {n} samples where the restated roots change the orientation filter's verdict")
    assert n > 1900 and n_skip <= 0.01 * n, (n, n_skip)
