"""Reference for the cubic-root math of the 7-point solver (pydegensac_amd/csrc/dg_crmath.h, dg_dev_small.h dg_rroots3 = Ftools.c:251-298):

  cr_cos / cr_acos / cr_pow13   the function in 200-bit arithmetic (mpmath), rounded to the nearest double: what dg_crmath.h promises
  rroots3(po)                   dg_rroots3 restated one IEEE operation at a time in numpy float64 scalars, the three functions taken
                                from the cr_* above (or from `fns`, e.g. the host libm's, to replay a host run of the reference)
  catalogue() / build()         the argument catalogues (fixed seed, branch edges on purpose) and tests/golden/crmath_cr.npz made of them

The catalogues are made of rng.random / rng.integers and IEEE + - * / only (exp through mpmath), so a rebuild gives the same bytes on
every host.  `python -m tests.crmath_ref` rewrites the fixture.  No device, nothing outside this repository."""
import io
import math
import os
import zipfile

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crmath_cr.npz")

PIO2 = float.fromhex("0x1.921fb54442d18p+0")             # DG_CR_PIO2_1
PI = 2.0 * PIO2                                          # dg_cr_cos rounds correctly on [0, PI]
COS_SW1 = 0.5 * PIO2                                     # x < this: the cos kernel on x itself
COS_SW2 = float.fromhex("0x1.2d97c7f3321d2p+1")          # x <= this: sin(pi/2 - x); beyond: -cos(pi - x)
PIT = 1.0471975511965967                                 # DG_PIT
POW_LO, POW_HI = 1e-290, 1e290                           # dg_cr_pow13 rounds correctly on the open interval
THIRD = 1.0 / 3                                          # the double the reference passes to pow

ONE_POS, ONE_NONPOS, THREE, FALLBACK = 0, 1, 2, 3        # branch classes of rroots3
BRANCHES = {ONE_POS: "one root, A > 0", ONE_NONPOS: "one root, A <= 0", THREE: "three roots", FALLBACK: "library fallback"}
F64 = np.float64


def _mp():
    import mpmath
    return mpmath


def _round(v):
    """nearest double (ties to even) of an mpf, by Python's own correctly rounded int -> float; no result here is subnormal"""
    sign, man, exp, _ = v._mpf_
    if not man:
        return float(v)                                  # 0, inf, nan
    f = math.ldexp(float(man), exp)
    return -f if sign else f


def _exact(fn, x):
    mp = _mp()
    with mp.workprec(200):
        return _round(fn(mp, mp.mpf(float(x))))


def cr_cos(x):
    x = float(x)
    if not math.isfinite(x):
        return F64(np.nan)
    return F64(_exact(lambda mp, v: mp.cos(v), x))


def cr_acos(c):
    c = float(c)
    if not (-1.0 <= c <= 1.0):
        return F64(np.nan)
    return F64(_exact(lambda mp, v: mp.acos(v), c))


def cr_pow13(a):
    """pow(a, 1.0/3) with the DOUBLE 1.0/3 = 1/3 - 2^-54/3 as the exponent, as the reference passes it"""
    a = float(a)
    if math.isnan(a) or a < 0:
        return F64(np.nan)
    if a == 0 or math.isinf(a):
        return F64(abs(a))                               # pow(+-0, y) = +0 and pow(inf, y) = inf for y > 0 not an odd integer
    return F64(_exact(lambda mp, v: mp.power(v, mp.mpf(THIRD)), a))


CR = {"cos": cr_cos, "acos": cr_acos, "pow13": cr_pow13}
OPS = {"cos": 8, "acos": 9, "pow13": 10}                 # mi_degensac_mat3 ops


def bit_tested(name, x):
    """where dg_crmath.h promises the rounded value; elsewhere it returns the library's own"""
    x = np.asarray(x, F64)
    if name == "cos":
        return np.abs(x) <= PI
    if name == "pow13":
        return (x > POW_LO) & (x < POW_HI)
    return np.ones(x.shape, bool)


def rroots3(po, fns=None, info=None):
    """dg_rroots3 (Ftools.c:251-298) -> (nr, roots[3], branch).  Every comparison is false for NaN, as in C.  `fns` replaces the three
    functions; `info` (a dict) receives the calls made as (name, argument, value), the clamps taken and q == 0."""
    f = dict(CR); f.update(fns or {})
    calls = []

    def call(name, x):
        v = F64(f[name](x)); calls.append((name, float(x), float(v))); return v

    r = np.zeros(3)
    clamp = 0; q_zero = False
    with np.errstate(all="ignore"):
        po = np.asarray(po, F64)
        b = po[1] / po[0]
        c = po[2] / po[0]
        b2 = b * b
        bt = b / F64(3)
        p = (F64(3) * c - b2) / F64(9)
        q = (((F64(2) * b2) * b) / F64(27) - (b * c) / F64(3) + po[3] / po[0]) / F64(2)
        D = q * q + (p * p) * p
        if D > 0:
            A = np.sqrt(D) - q
            if A > 0:
                arg = A; v = call("pow13", arg); r[0] = (v - p / v) - bt
                branch = ONE_POS
            else:
                arg = -A; v = call("pow13", arg); r[0] = (p / v - v) - bt
                branch = ONE_NONPOS
            if not (arg > POW_LO and arg < POW_HI):
                branch = FALLBACK
            nr = 1
        else:
            e = F64(1) if q > 0 else F64(-1)
            q_zero = bool(q == 0)
            R = e * np.sqrt(-p)
            _2R = R * F64(2)
            cosphi = q / ((R * R) * R)
            if cosphi > 1:
                cosphi = F64(1); clamp = 1
            elif cosphi < -1:
                cosphi = F64(-1); clamp = -1
            phit = call("acos", cosphi) / F64(3)
            r[0] = (-_2R) * call("cos", phit) - bt
            r[1] = _2R * call("cos", F64(PIT) - phit) - bt
            r[2] = _2R * call("cos", F64(PIT) + phit) - bt
            nr = 3; branch = THREE
    if info is not None:
        info.update(calls=calls, clamp=clamp, q_zero=q_zero)
    return nr, r, branch


# ---------------------------------------------------------------------------------------------------------------------------------
# catalogues

def ulps(x, ks):
    """the doubles k units in the last place from x (k in ks, along the ordered bit patterns), x != 0 finite"""
    i = np.array([x], F64).view(np.int64)[0]
    s = 1 if x > 0 else -1
    return np.array([i + s * k for k in ks], np.int64).view(F64)


def _exp(u):
    mp = _mp()
    with mp.workprec(200):
        return np.array([_round(mp.exp(mp.mpf(float(t)))) for t in u])


def _args(rng):
    around = range(-4, 5)
    cos = np.concatenate([
        rng.random(1024) * PI,
        [0.0, 5e-324, 1e-300, -8.9e-16],
        ulps(COS_SW1, around), ulps(COS_SW2, around),
        ulps(PIO2, around), PIO2 + np.array([1e-12, -1e-12, 1e-6, -1e-6]),
        ulps(PI, [0, -1]),
        ulps(PI, [1, 2, 3, 4]),                                           # beyond pi: the library's value, not bit-tested
    ])
    acos = np.concatenate([
        2.0 * rng.random(768) - 1.0,
        1.0 - _exp(-35.0 * rng.random(128)), -1.0 + _exp(-35.0 * rng.random(128)),
        ulps(0.5, around), ulps(-0.5, around),
        [1.0, -1.0], ulps(1.0, [-1]), ulps(-1.0, [1]),
        [0.0, 5e-324, -5e-324, 1e-8, -1e-8],
    ])
    pow13 = np.concatenate([
        _exp(1200.0 * rng.random(768) - 600.0), _exp(6.0 * rng.random(256) - 3.0),
        [1.0, 8.0, 27.0], [math.ldexp(3.0, s * k) for k in (1, 2, 3, 10, 100, 300, 900) for s in (1, -1)],
        ulps(POW_LO, around), ulps(POW_HI, around),                       # only the doubles inside (1e-290, 1e290) are bit-tested
    ])
    return {"cos": cos, "acos": acos, "pow13": pow13}


def _dy(rng, lo, hi, bits):
    """a random dyadic number of `bits` bits in +-[lo, hi): short enough that the expansions below are exact"""
    m = int(rng.integers(1 << (bits - 1), 1 << bits)); s = 1 - 2 * int(rng.integers(0, 2))
    return s * (lo + (hi - lo) * m / float(1 << bits))


def _expand(lead, r1, r2, r3):
    """lead (x - r1)(x - r2)(x - r3) expanded in floating point"""
    r1, r2, r3, lead = F64(r1), F64(r2), F64(r3), F64(lead)
    return [lead, -lead * ((r1 + r2) + r3), lead * ((r1 * r2 + r1 * r3) + r2 * r3), -lead * ((r1 * r2) * r3)]


def _cubics(rng):
    C = []
    with np.errstate(all="ignore"):
        # 7-point-like: det(x F1 + (1 - x) F2) of unit-norm null vectors, coefficients of mixed size and sign
        for _ in range(216):
            C.append([(2.0 * rng.random() - 1.0) * math.ldexp(1.0, int(rng.integers(-8, 9))) for _ in range(4)])
        # (x - a)^2 (x - b): D lands at 0 and a few ulp on each side, cos phi at +-1 and a few ulp beyond (both clamps)
        for k in range(96):
            if k < 48:
                a, b = _dy(rng, 0.25, 4.0, 6), _dy(rng, 0.25, 4.0, 6)
            else:
                a, b = (2.0 * rng.random() - 1.0) * 3.0, (2.0 * rng.random() - 1.0) * 3.0
            C.append(_expand(_dy(rng, 0.5, 2.0, 4) if k % 2 else 1.0, a, a, b))
        # (x - a)^3 with exact coefficients: p = q = 0, cos phi = 0/0, three NaN roots
        for _ in range(8):
            a = _dy(rng, 0.5, 2.0, 5); C.append(_expand(_dy(rng, 0.5, 2.0, 3), a, a, a))
        # q == 0 with p < 0 (the e = -1 side): (x - h)^3 - s^2 (x - h), exact for dyadic h, s; h = 0 among them
        for k in range(16):
            h = 0.0 if k < 4 else _dy(rng, 0.5, 2.0, 4); s = _dy(rng, 0.5, 2.0, 4)
            C.append(_expand(1.0 if k % 2 else _dy(rng, 0.5, 2.0, 3), h - s, h, h + s))
        # p < 0, D > 0, q > 0: A = sqrt(D) - q < 0, the root through pow(-A)
        for _ in range(40):
            b = (2.0 * rng.random() - 1.0); c = -(0.1 + rng.random()); d = 2.0 + 8.0 * rng.random()
            C.append([1.0, b, c + b * b / 3.0, d])
        # p > 0 so small that sqrt(q^2 + p^3) == q: A = 0, pow(-0.0) -- the library fallback, roots +-inf
        for k in range(12):
            lead = _dy(rng, 0.5, 2.0, 3)
            C.append([lead, 0.0, lead * 3.0 * math.ldexp(1.0 + rng.random(), -40 - k), lead * 2.0 * (0.5 + rng.random())])
        # q^2 overflows: A = inf, the library fallback again
        for k in range(8):
            C.append([1.0, 2.0 * rng.random() - 1.0, 2.0 * rng.random() - 1.0, -(1.0 + rng.random()) * 1e200 * 10.0 ** (10 * k)])
        base = [list(map(float, po)) for po in C]
        # all of the above scaled by 1e+-100 (every eighth, so that each family is met)
        for k, po in enumerate(base):
            if k % 8 == 0:
                C.append([x * 1e100 for x in po])
            if k % 8 == 4:
                C.append([x * 1e-100 for x in po])
        # po[0] at 1e-300 (next to coefficients of ordinary size: the ratios overflow; and next to its like) and at 0
        for k in range(24):
            po = [2.0 * rng.random() - 1.0 for _ in range(4)]
            if k < 8:
                po[0] = 1e-300
            elif k < 16:
                po = [x * 1e-300 for x in po]; po[0] = 1e-300
            else:
                po[0] = 0.0 if k % 2 else -0.0
                if k >= 20:
                    po[1] = 0.0
            C.append(po)
    return np.array(C, F64)


def catalogue(seed=20240607):
    """-> {"cos_x", "cos_y", ..., "cubic_po", "cubic_nr", "cubic_roots", "cubic_branch"}; the committed fixture is seed's default"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, x in _args(rng).items():
        x = np.ascontiguousarray(x, F64)
        out[name + "_x"] = x
        out[name + "_y"] = np.array([CR[name](v) for v in x], F64)
    po = _cubics(rng)
    res = [rroots3(q) for q in po]
    out["cubic_po"] = po
    out["cubic_nr"] = np.array([r[0] for r in res], np.int8)
    out["cubic_roots"] = np.array([r[1] for r in res], F64)
    out["cubic_branch"] = np.array([r[2] for r in res], np.int8)
    return out


def fixture_bytes(cat=None):
    """the catalogue as an uncompressed .npz with fixed member dates: the same bytes from every build"""
    cat = catalogue() if cat is None else cat
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for k in sorted(cat):
            m = io.BytesIO(); np.lib.format.write_array(m, np.ascontiguousarray(cat[k]), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)); zi.external_attr = 0o644 << 16
            z.writestr(zi, m.getvalue())
    return buf.getvalue()


def build(path=FIXTURE):
    with open(path, "wb") as f:
        f.write(fixture_bytes())
    return path


def load(path=FIXTURE):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------------------------------------------------------------
# live samples from another seed (tests that have mpmath)

def live_args(seed, n):
    rng = np.random.default_rng(seed)
    h = n // 2
    return {"cos": rng.random(n) * PI,
            "acos": np.concatenate([2.0 * rng.random(h) - 1.0, 1.0 - _exp(-35.0 * rng.random(n // 4)), -1.0 + _exp(-35.0 * rng.random(n - h - n // 4))]),
            "pow13": np.concatenate([_exp(1200.0 * rng.random(h) - 600.0), _exp(6.0 * rng.random(n - h) - 3.0)])}


def live_cubics(seed, n):
    """fresh cubics: the catalogue's families from another seed, repeated until there are n"""
    rng = np.random.default_rng(seed)
    parts = []
    while sum(len(p) for p in parts) < n:
        parts.append(_cubics(rng))
    return np.concatenate(parts)[:n]


# ---------------------------------------------------------------------------------------------------------------------------------
# the 7-point solver's unit test scene (tests/test_gpu_units.py, and the CPU check of its premise)

def solve7_scene():
    from pydegensac_amd import synthetic as syn
    n = 1500
    p1, p2, lab, _ = syn.two_view_fundamental(n, 0.5, 0.1, seed=4)
    u = np.ones((n, 6)); u[:, 0:2] = p1; u[:, 3:5] = p2
    rng = np.random.default_rng(1)
    S = 2000
    samples = np.stack([rng.choice(n, 7, replace=False) for _ in range(S)]).astype(np.int32)
    inl = np.flatnonzero(lab)
    samples[:300] = np.stack([rng.choice(inl, 7, replace=False) for _ in range(300)])      # all-inlier samples: valid models
    samples[300, 1] = samples[300, 0]                                                       # a rank-deficient sample
    return p1, p2, u, samples


def solve7_oracle(port, u, samples):
    """per sample with a two-dimensional null space: t -> (f1, f2, poly, nr, roots) as the oracle (host libm) computes them"""
    P = port.lib(); dp = port.dp
    out = {}
    for t in range(len(samples)):
        A = np.zeros(81)
        for i, q in enumerate(samples[t]):                                   # rows in draw order (rtools.c:74-92)
            A[9 * i:9 * i + 9] = np.outer(u[q, 3:6], u[q, 0:3]).ravel()
        ns = np.zeros(81)
        if P.dg_oracle_nullspace(dp(A), dp(ns), 9) != 2:
            out[t] = None
            continue
        f1 = ns[0:9].copy(); f2 = ns[9:18].copy(); poly = np.zeros(4); roots = np.zeros(3)
        P.dg_oracle_slcm(dp(f1), dp(f2), dp(poly))                           # f2 := f1 - f2 (Ftools.c:70)
        nr = P.dg_oracle_rroots3(dp(poly), dp(roots))
        out[t] = (f1, f2, poly, nr, roots)
    return out


def solve7_models(port, u, sample, f1, f2, nr, roots):
    """[(root index, model)] of the roots whose model passes the oracle's oriented-epipolar test (exp_ranF.c:1351-1372)"""
    P = port.lib()
    samidx = np.ascontiguousarray(sample[::-1])                              # pool tail = reverse draw order (rtools.c:17-20)
    want = []
    for i in range(nr):
        f = f1 * roots[i] + f2 * (1 - roots[i])                              # exp_ranF.c:1365-1368
        if P.dg_oracle_all_ori_valid(port.dp(np.ascontiguousarray(f)), port.dp(u), port.ip(samidx), 7):
            want.append((i, f))
    return want


if __name__ == "__main__":
    print(build())
