"""Rotation averaging without a device (include/mi_degensac.h mi_degensac_rotation_average*, matcher.average_rotations,
tensor_api.average_rotations_tensors): every refusal of both C entry points with its message and its place in the order (each comes back
as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), the Python keyword, shape and dtype
checks, and the restatement tests/rotavg_ref.py itself on graphs written by hand: closed forms, every status, the unused edges, the
tie rule, the order of the sums, orthogonality, what averaging and the robust factor buy, and three broken restatements that these
scenes reject."""
import math

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, synthetic
from tests import rotavg_ref as Q

EINVAL = -1
NAMES = ("dev", "host")
Z = (0.0, 0.0, 1.0)
I3 = np.eye(3)


def _abi(which, K=3, n=4, root=0, sweeps=10, damping=0.5, robust=5.0, tol=1e-9, null=(), known=False, R0=False):
    """(rc, message) of one entry point; data pointers hold an address (never read: every call here is refused first) unless in `null`"""
    L = _lib.lib(); buf = np.zeros(64); addr = buf.ctypes.data
    A = lambda name: None if name in null else addr                    # noqa: E731
    head = (A("pairs"), A("pairs"), None, None, K, n, addr if R0 else None, addr if known else None, root, sweeps, damping, robust, tol, 0)
    outs = (A("out"), A("out"), A("out"), A("out"), None)
    if which == "dev":
        rc = L.mi_degensac_rotation_average_dev(*head, None, *outs)
    else:
        rc = L.mi_degensac_rotation_average(*head, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and part in msg, (which, rc, msg)


def test_tile_constants_and_status_codes_are_mirrored():
    L = _lib.lib()
    assert [L.mi_degensac_rotation_average_tile(i) for i in range(4)] == [_lib.rotavg_group(), _lib.ROTAVG_GRID, _lib.ROTAVG_CAMERAS, -1]
    assert _lib.rotavg_group() * _lib.ROTAVG_CAMERAS == 256
    assert (_lib.ROTAVG_KNOWN, _lib.ROTAVG_OK, _lib.ROTAVG_UNREACHED, _lib.ROTAVG_ISOLATED) == (Q.KNOWN, Q.OK, Q.UNREACHED, Q.ISOLATED) == tuple(range(4))
    assert (_lib.ROTAVG_CONVERGED, _lib.ROTAVG_MAX_SWEEPS, _lib.ROTAVG_NO_ROOT) == (Q.CONVERGED, Q.MAX_SWEEPS, Q.NO_ROOT) == tuple(range(3))


def test_refusals_and_their_order():
    nan = float("nan")
    for n in (0, -1, (1 << 24) + 1):
        _refused(b"n_images", n=n)
    _refused(b"n_pairs < 0", K=-1)
    _refused(b"too many pairs", K=0x40000000)
    for s in (-1, 4097):
        _refused(b"sweeps", sweeps=s)
    for d in (0.0, -0.5, 1.0000001, nan, float("inf")):
        _refused(b"damping", damping=d)
    for r in (-1.0, 180.0, 200.0, nan):
        _refused(b"robust_deg", robust=r)
    for t in (nan, -1e-300):
        _refused(b"tol", tol=t)
    for r in (-1, 4):
        _refused(b"root", root=r)
    _refused(b"root", root=4, known=True, R0=True)                     # also with known cameras
    _refused(b"pairs and R_rel", null=("pairs",))
    _refused(b"both or neither", known=True)
    _refused(b"both or neither", R0=True)
    _refused(b"R, info, step and summary", null=("out",))
    # each refusal hides every later one
    kw = dict(n=0, K=-1, sweeps=-1, damping=nan, robust=nan, tol=nan, root=-1, null=("pairs", "out"), known=True)
    order = [("n", b"n_images"), ("K", b"n_pairs < 0"), ("sweeps", b"sweeps"), ("damping", b"damping"), ("robust", b"robust_deg"), ("tol", b"tol"),
             ("root", b"root"), ("null", b"pairs and R_rel")]
    for key, part in order:
        _refused(part, **kw)
        kw.pop(key)
    _refused(b"both or neither", **kw)
    _refused(b"R, info, step and summary", null=("out",))
    # the closed ends that are allowed pass on to the next refusal; nothing is asked of an empty pair list
    _refused(b"summary", n=1 << 24, K=0x3fffffff, sweeps=4096, damping=1.0, robust=0.0, tol=0.0, root=(1 << 24) - 1, null=("out",))
    _refused(b"summary", sweeps=0, robust=179.9, tol=float("inf"), null=("out",))
    _refused(b"summary", K=0, null=("pairs", "out"))


def test_no_pairs_is_not_refused():
    """K == 0 passes every check: the call then needs a device like any other (there is always a camera to write)"""
    try:
        R, info, step, summary = matcher.average_rotations(np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), 3)
    except _lib.MiDegensacError as e:
        assert "no HIP device" in str(e)
        return
    assert info[:, 3].tolist() == [Q.KNOWN, Q.ISOLATED, Q.ISOLATED] and summary.tolist() == [0, 1, 0, Q.CONVERGED]


# ---- the Python checks ----
def _np(K=3, n=4):
    return np.zeros((K, 2), np.int32), np.zeros((K, 3, 3)), n


@pytest.mark.parametrize("kw, part", [
    (dict(sweeps=-1), "sweeps"), (dict(sweeps=4097), "sweeps"), (dict(sweeps=2.0), "sweeps"), (dict(sweeps=True), "sweeps"),
    (dict(damping=0), "damping"), (dict(damping=1.5), "damping"), (dict(damping=float("nan")), "damping"), (dict(damping="x"), "damping"),
    (dict(robust_deg=0), "robust_deg"), (dict(robust_deg=180), "robust_deg"), (dict(robust_deg=-5.0), "robust_deg"), (dict(robust_deg=True), "robust_deg"),
    (dict(tol=-1e-9), "tol"), (dict(tol=float("nan")), "tol"), (dict(root=4), "root"), (dict(root=-1), "root"), (dict(root=1.0), "root"),
    (dict(cams2=None), "unknown keyword 'cams2'"), (dict(n_images2=3), "unknown keyword 'n_images2'"),
    (dict(weight=np.zeros(2)), "weight"), (dict(weight=np.zeros(3, np.float32)), "weight"), (dict(edge_keep=np.zeros(4, bool)), "edge_keep"),
    (dict(edge_keep=np.zeros(3, np.int32)), "edge_keep"), (dict(known=np.zeros(4, bool)), "both or neither"), (dict(R0=np.zeros((4, 3, 3))), "both or neither"),
    (dict(R0=np.zeros((3, 3, 3)), known=np.zeros(4, bool)), "R0 should"), (dict(R0=np.zeros((4, 3, 3)), known=np.zeros(4)), "known should"),
    (dict(R0=np.zeros((4, 3, 3), np.float32), known=np.zeros(4, bool)), "R0 should"),
])
def test_keyword_checks(kw, part):
    with pytest.raises(ValueError, match=part):
        matcher.average_rotations(*_np(), **kw)


def test_shape_and_dtype_checks():
    pr, Rr, n = _np()
    chk = lambda p, r, n, **kw: matcher.check_rotavg_args(p.shape, p.dtype, r.shape, r.dtype, n, **kw)          # noqa: E731
    assert chk(pr, Rr, n) == (3, 4, 0, 200, 0.5, 5.0, 1e-9)
    assert chk(pr.astype(np.int64), Rr, 1, robust_deg=None, sweeps=0, damping=1, tol=0) == (3, 1, 0, 0, 1.0, 0.0, 0.0)
    bad = [((pr[:, :1], Rr, n), "pairs should"), ((np.zeros((3, 2, 2), np.int32), Rr, n), "pairs should"), ((pr.astype(np.float64), Rr, n), "pairs should"),
           ((pr, Rr[:2], n), "R_rel should"), ((pr, Rr.astype(np.float32), n), "R_rel should"), ((pr, Rr.reshape(3, 9), n), "R_rel should"),
           ((pr, Rr, 0), "n_images"), ((pr, Rr, (1 << 24) + 1), "n_images"), ((pr, Rr, 4.0), "n_images")]
    for args, part in bad:
        with pytest.raises(ValueError, match=part):
            chk(*args)


def test_tensor_form_refuses_before_a_device_is_needed():
    import torch
    from pydegensac_amd import tensor_api as T
    pr, Rr, n = _np()
    with pytest.raises(ValueError, match="unknown keyword 'cams2'"):
        T.average_rotations_tensors(pr, Rr, n, cams2=None)
    with pytest.raises(ValueError, match="must be torch tensors"):
        T.average_rotations_tensors(pr, Rr, n)
    tp, tr = torch.from_numpy(pr), torch.from_numpy(Rr)
    with pytest.raises(ValueError, match="sweeps"):
        T.average_rotations_tensors(tp, tr, n, sweeps=5000)
    with pytest.raises(ValueError, match="R_rel should"):
        T.average_rotations_tensors(tp, tr[:2], n)
    with pytest.raises(ValueError, match="same ROCm device"):
        T.average_rotations_tensors(tp, tr, n)


# ---- the restatement on graphs written by hand ----
def _close(A, B, tol=1e-12):
    d = np.abs(np.asarray(A) - np.asarray(B))
    assert d.size == 0 or d.max() <= tol, d.max()


def test_single_edge_in_both_orientations():
    A = Q.rot((1, 2, 3), 40.0)
    R, info, step, summary, cosv = Q.average([[0, 1]], A[None], 2)      # X_1 = A X_0, camera 0 is the world: R_1 = A
    _close(R[1], A); _close(R[0], I3, 0)
    assert info.tolist() == [[1, 0, 0, Q.KNOWN], [1, 1, 0, Q.OK]] and summary.tolist() == [1, 2, 1, Q.CONVERGED]
    assert abs(cosv[0] - 1) < 1e-15 and np.isnan(step[0]) and step[1] < 1e-30
    R = Q.average([[1, 0]], A[None], 2)[0]                             # X_0 = A X_1: R_1 = A^T
    _close(R[1], A.T)
    R, info = Q.average([[0, 1]], A[None], 2, root=1)[:2]               # the other end holds the gauge
    _close(R[0], A.T); _close(R[1], I3, 0)
    assert info[:, 3].tolist() == [Q.OK, Q.KNOWN]


def test_path_is_set_one_level_per_sweep():
    Rg = Q.random_rotations(5, np.random.default_rng(1)); Rg[0] = I3
    pairs = [[0, 1], [2, 1], [2, 3], [4, 3]]
    Rr = Q.relative(Rg, pairs)
    for sweeps in (2, 4, 5, 50):
        R, info, step, summary, cosv = Q.average(pairs, Rr, 5, sweeps=sweeps)
        reach = min(sweeps, 4)
        assert info[:, 1].tolist() == [0] + [s if s <= reach else -1 for s in range(1, 5)]
        assert info[:, 3].tolist() == [Q.KNOWN] + [Q.OK if s <= reach else Q.UNREACHED for s in range(1, 5)]
        _close(R[:reach + 1], Rg[:reach + 1]); _close(R[reach + 1:], 0, 0)
        # sweeps 1 .. 4 set a camera; the fifth finds nothing to do
        assert summary.tolist() == [min(sweeps, 4), reach + 1, 4, Q.CONVERGED if sweeps >= 5 else Q.MAX_SWEEPS]
        assert np.isnan(cosv).tolist() == [False] * reach + [True] * (4 - reach)


def test_star_from_both_ends():
    Rg = Q.random_rotations(6, np.random.default_rng(2))
    pairs = [[0, k] if k % 2 else [k, 0] for k in range(1, 6)]
    Rr = Q.relative(Rg, pairs)
    R, info, _, summary, _ = Q.average(pairs, Rr, 6, root=0)           # from the hub: one level
    _close(R, Rg @ Rg[0].T)
    assert info[:, 1].tolist() == [0, 1, 1, 1, 1, 1] and info[:, 0].tolist() == [5, 1, 1, 1, 1, 1] and summary[0] == 1
    R, info, _, summary, _ = Q.average(pairs, Rr, 6, root=3)           # from a leaf: two levels
    _close(R, Rg @ Rg[3].T)
    assert info[:, 1].tolist() == [1, 2, 2, 0, 2, 2] and summary.tolist() == [2, 6, 5, Q.CONVERGED]


@pytest.mark.parametrize("m", [3, 4])
def test_exact_cycles_keep_the_generators_rotations(m):
    Rg = Q.random_rotations(m, np.random.default_rng(m)); Rg[0] = I3
    pairs = [[k, (k + 1) % m] for k in range(m)]
    R, info, step, summary, cosv = Q.average(pairs, Q.relative(Rg, pairs), m)
    _close(R, Rg)
    assert summary[3] == Q.CONVERGED and (np.abs(cosv - 1) < 1e-14).all() and (info[:, 2] == 0).all()


def test_two_components_and_isolated_cameras():
    Rg = Q.random_rotations(7, np.random.default_rng(5)); Rg[0] = I3
    pairs = [[0, 1], [1, 2], [4, 5]]                                   # 3 and 6 have no edge, 4-5 is out of reach
    R, info, step, summary, cosv = Q.average(pairs, Q.relative(Rg, pairs), 7)
    assert info[:, 3].tolist() == [Q.KNOWN, Q.OK, Q.OK, Q.ISOLATED, Q.UNREACHED, Q.UNREACHED, Q.ISOLATED]
    assert summary.tolist() == [2, 3, 3, Q.CONVERGED] and np.isnan(cosv).tolist() == [False, False, True]
    _close(R[:3], Rg[:3]); _close(R[3:], 0, 0)


def test_two_known_cameras_and_no_root():
    Rg = Q.random_rotations(5, np.random.default_rng(6))
    pairs = [[0, 1], [1, 2], [2, 3], [3, 4]]
    Rr = Q.relative(Rg, pairs)
    known = np.array([1, 0, 0, 0, 1], np.uint8)
    R0 = np.zeros((5, 3, 3)); R0[0] = Rg[0]; R0[4] = Rg[4]; R0[2] = 7.0          # (the row of a camera that is not known is not read)
    R, info, step, summary, _ = Q.average(pairs, Rr, 5, R0=R0, known=known, root=2)
    _close(R, Rg)
    assert info[:, 3].tolist() == [Q.KNOWN, Q.OK, Q.OK, Q.OK, Q.KNOWN] and info[:, 1].tolist() == [0, 1, 2, 1, 0]
    assert (R[0] == Rg[0]).all() and (R[4] == Rg[4]).all()             # held: the same bytes
    # an inconsistent pair of known cameras: they stay, the middle spreads the disagreement
    R0[4] = Q.rot(Z, 8.0) @ Rg[4]
    R2, info2 = Q.average(pairs, Rr, 5, R0=R0, known=known, robust_deg=None, sweeps=2000)[:2]
    assert (R2[4] == R0[4]).all() and (R2[0] == Rg[0]).all()
    _close(Q.angle_deg(R2[1:4], Rg[1:4]), [2.0, 4.0, 6.0], 1e-3)
    R, info, step, summary, cosv = Q.average(pairs, Rr, 5, R0=R0, known=np.zeros(5, np.uint8))
    assert summary.tolist() == [0, 0, 4, Q.NO_ROOT] and (info[:, 3] == Q.UNREACHED).all() and (R == 0).all() and np.isnan(cosv).all()


def test_sweeps_zero_is_the_start_state():
    R, info, step, summary, cosv = Q.average([[0, 1]], Q.rot(Z, 3.0)[None], 2, sweeps=0)
    assert summary.tolist() == [0, 1, 1, Q.MAX_SWEEPS] and info[:, 3].tolist() == [Q.KNOWN, Q.UNREACHED] and np.isnan(cosv[0]) and np.isnan(step).all()


def test_exact_collection_ends_at_the_generators_rotations():
    for m in (8, 13):
        Rg = np.stack([R for R, _ in synthetic.collection_cameras(m)[1]])
        pairs = matcher.exhaustive_pairs(m)
        R, info, step, summary, cosv = Q.average(pairs, Q.relative(Rg, pairs), m, root=m // 2)
        _close(R, Rg @ Rg[m // 2].T, 1e-12)
        assert summary[3] == Q.CONVERGED and summary[1] == m and summary[2] == len(pairs) and (cosv > 1 - 1e-12).all()


def test_an_edge_at_exactly_pi_is_opposed():
    """two edges 0 -> 1, diag(1, 1, 1) first (it sets the camera) and diag(-1, -1, 1): Q = diag(-1, -1, 1), q = 1 + (-1) is exactly 0"""
    Rr = np.stack([I3, np.diag([-1.0, -1.0, 1.0])])
    R, info, step, summary, cosv = Q.average([[0, 1], [0, 1]], Rr, 2, robust_deg=None)
    assert (R[1] == I3).all() and info[1].tolist() == [2, 1, 1, Q.OK] and step[1] == 0.0 and cosv.tolist() == [1.0, -1.0]
    assert summary.tolist() == [1, 2, 2, Q.CONVERGED]
    # alone, the opposed edge still sets the camera; afterwards it agrees with itself
    R, info = Q.average([[0, 1]], Rr[1:], 2)[:2]
    assert (R[1] == Rr[1]).all() and info[1, 2] == 0


def test_unused_edges():
    A = Q.rot((1, 0, 0), 10.0)
    nan, inf = float("nan"), float("inf")
    bad = [np.zeros((3, 3)), np.full((3, 3), nan), 1.001 * A, A + np.array([[0, 0, 1e-3], [0, 0, 0], [0, 0, 0]]), np.where(np.eye(3) > 0, inf, 0.0)]
    for B in bad:
        assert Q.used_edges([[0, 1]], B[None], 2).tolist() == [False]
    assert Q.used_edges([[0, 1]], (A * (1 + 1e-8))[None], 2).tolist() == [True]          # inside the 1e-6 band
    for w in (0.0, -1.0, nan, inf, -inf):
        assert Q.used_edges([[0, 1]], A[None], 2, weight=[w]).tolist() == [False]
    assert Q.used_edges([[0, 1]], A[None], 2, weight=[1e-300]).tolist() == [True]
    pairs = [[0, 1], [1, 1], [-1, 1], [0, 2], [1, 0], [0, 1]]
    Rr = np.stack([A] * 6)
    assert Q.used_edges(pairs, Rr, 2, edge_keep=[1, 1, 1, 1, 1, 0]).tolist() == [True, False, False, False, True, False]
    # a scene where every bad edge would wreck camera 1 if it were used
    pairs = [[0, 1]] * 6
    Rr = np.stack([A] + bad)
    R, info, _, summary, cosv = Q.average(pairs, Rr, 2)
    _close(R[1], A); assert info[1, 0] == 1 and summary[2] == 1 and np.isnan(cosv[1:]).all()


def test_weight_ties_go_to_the_lowest_position():
    A, B, C = Q.rot(Z, 10.0), Q.rot(Z, 20.0), Q.rot(Z, 30.0)
    Rr = np.stack([A, B, C])
    first = lambda w: Q.average([[0, 1]] * 3, Rr, 2, weight=w, sweeps=1)[0][1]          # noqa: E731
    assert (first([1.0, 1.0, 1.0]) == A).all() and (first([1.0, 2.0, 2.0]) == B).all() and (first([1.0, 2.0, 3.0]) == C).all()
    # positions follow the half-edge index 2 e + side: for camera 1, edge 0 = (1, 0) comes before edge 1 = (0, 1)
    R = Q.average([[1, 0], [0, 1]], np.stack([A, B]), 2, sweeps=1)[0]
    assert (R[1] == A.T).all()
    # and across lanes: 40 equal edges, the first wins; a heavier one at position 37 wins
    Rr = np.stack([Q.rot(Z, float(k + 1)) for k in range(40)])
    assert (Q.average([[0, 1]] * 40, Rr, 2, sweeps=1)[0][1] == Rr[0]).all()
    w = np.ones(40); w[37] = 1.5; w[39] = 1.5
    assert (Q.average([[0, 1]] * 40, Rr, 2, weight=w, sweeps=1)[0][1] == Rr[37]).all()


def test_the_damped_step_in_closed_form():
    """two edges 0 -> 1 about one axis, 10 and 30 degrees: sweep 1 takes the first, sweep 2 sees the Cayley vectors 0 and tan(10 deg), their
    mean tan(10 deg) / 2 and moves by damping times that: the angle is 10 + 2 atan(tan(10 deg) / 4).  The fixed point is 20 degrees."""
    Rr = np.stack([Q.rot(Z, 10.0), Q.rot(Z, 30.0)])
    tr = []
    R, info, step, summary, cosv = Q.average([[0, 1]] * 2, Rr, 2, robust_deg=None, trace=tr)
    t10 = math.tan(math.radians(10.0))
    _close(tr[0][1], Rr[0], 0)
    _close(tr[1][1], Q.rot(Z, 10.0 + 2 * math.degrees(math.atan(t10 / 4))), 1e-15)
    _close(R[1], Q.rot(Z, 20.0), 1e-9)
    assert summary[3] == Q.CONVERGED and abs(step[1]) < 1e-18
    _close(cosv, [math.cos(math.radians(10.0))] * 2, 1e-9)
    # the robust factor at m = tan^2(10 deg) with sigma = tan(2.5 deg)
    tr2 = []
    Q.average([[0, 1]] * 2, Rr, 2, robust_deg=5.0, trace=tr2, sweeps=2)
    s2 = math.tan(math.radians(2.5)) ** 2; f = (s2 / (s2 + t10 * t10)) ** 2
    _close(tr2[1][1], Q.rot(Z, 10.0 + 2 * math.degrees(math.atan(0.5 * f * t10 / (1 + f)))), 1e-15)


def test_the_order_of_the_sums():
    """numbers whose sum depends on the order: 1 in lane 0, 2^-53 in every other position.  Lane by lane and then by the butterfly the
    small terms meet each other first (G = 16: 15 of them make 15 * 2^-53, which 1 + . keeps as one ulp after rounding to even); added to
    1 one at a time every one of them is lost."""
    G = Q.group()
    e = 2.0 ** -53
    T = np.full((1, 2 * G), e); T[0, 0] = 1.0
    lanes = [T[0, l] + T[0, l + G] for l in range(G)]                  # lane l: position l, then l + G
    m = G // 2
    while m >= 1:
        lanes = [lanes[l] + lanes[l ^ m] for l in range(G)]
        m //= 2
    assert Q.lane_sum(T, G)[0] == lanes[0]
    assert len(set(lanes)) == 1
    one_by_one = 1.0
    for _ in range(2 * G - 1):
        one_by_one = one_by_one + e
    assert one_by_one == 1.0 and lanes[0] > 1.0                        # the two orders differ on these numbers
    # a third round and a ragged end: the padding adds +0.0
    T3 = np.zeros((1, 3 * G)); T3[0, :2 * G + 3] = np.arange(1, 2 * G + 4) * 0.1
    lanes = [(T3[0, l] + T3[0, l + G]) + T3[0, l + 2 * G] for l in range(G)]
    m = G // 2
    while m >= 1:
        lanes = [lanes[l] + lanes[l ^ m] for l in range(G)]
        m //= 2
    assert Q.lane_sum(T3, G)[0] == lanes[0]


def test_rotations_stay_orthogonal_over_1000_sweeps():
    rng = np.random.default_rng(11)
    n = 10
    Rg = Q.random_rotations(n, rng)
    pairs = matcher.exhaustive_pairs(n)
    Rr = Q.relative(Rg, pairs, rng, 3.0)
    R, info, step, summary, _ = Q.average(pairs, Rr, n, sweeps=1000, tol=0.0, robust_deg=None)
    assert summary[0] >= 999                                           # tol = 0: the sweeps go on as long as a bit moves
    _close(np.einsum("nij,nkj->nik", R, R), np.broadcast_to(I3, (n, 3, 3)), 1e-12)
    assert (np.linalg.det(R) > 0.999).all()


def _noisy_complete(seed, n=12, noise=2.0):
    rng = np.random.default_rng(seed)
    Rg = Q.random_rotations(n, rng); Rg[0] = I3
    pairs = matcher.exhaustive_pairs(n)
    return Rg, pairs, Q.relative(Rg, pairs, rng, noise), rng


def test_averaging_lowers_the_error_of_the_star():
    """K12, every relative rotation off by a random rotation of 2 degrees (standard deviation).  Sweep 1 is the star from the root: every
    camera carries the whole error of its one edge.  Measured over the seeds below: the RMS error of the cameras 1 .. 11 at the end is
    0.35 .. 0.60 of the RMS error after sweep 1 (0.48 in the mean; independent errors over 11 edges per camera would give about
    sqrt(2 / 12) = 0.41).  The test asks for every seed to end below the star."""
    ratios = []
    for seed in range(8):
        Rg, pairs, Rr, _ = _noisy_complete(seed)
        tr = []
        R, info, step, summary, _ = Q.average(pairs, Rr, 12, robust_deg=None, trace=tr)
        assert summary[3] == Q.CONVERGED
        e1 = Q.angle_deg(tr[0], Rg)[1:]; e2 = Q.angle_deg(R, Rg)[1:]
        ratios.append(math.sqrt((e2 ** 2).mean() / (e1 ** 2).mean()))
    print("ratios", np.round(ratios, 3), "mean", np.mean(ratios))
    assert max(ratios) < 1.0


def test_the_robust_factor_resists_outliers():
    """K12 with 0.5 degrees of noise and 12 of the 66 edges replaced by random rotations (none at the root, so that both runs start from the
    same clean star).  Measured over the seeds below: the RMS error at the end is 0.19 .. 0.28 degrees with robust_deg = 5 against 15 .. 35
    degrees without, and the edges whose edge_cos lies below cos 5 degrees are exactly the replaced ones."""
    for seed in range(6):
        Rg, pairs, Rr, rng = _noisy_complete(100 + seed, noise=0.5)
        cand = np.flatnonzero((pairs[:, 0] != 0) & (pairs[:, 1] != 0))
        out = rng.choice(cand, 12, replace=False)
        Rr[out] = Q.random_rotations(12, rng)
        res = {}
        for rb in (5.0, None):
            R, info, step, summary, cosv = Q.average(pairs, Rr, 12, robust_deg=rb)
            res[rb] = math.sqrt((Q.angle_deg(R, Rg)[1:] ** 2).mean())
            if rb:
                flagged = np.flatnonzero(cosv < math.cos(math.radians(5.0)))
                assert set(flagged) == set(out)                        # the residual is the filter for the wrong pairs
        print("seed", seed, res)
        assert res[5.0] < res[None] and res[5.0] < 0.5


# ---- three broken restatements that the scenes above reject ----
def test_broken_restatements_are_rejected():
    A = Q.rot((1, 2, 3), 40.0)
    # the transpose on the wrong side: the single edge
    R = Q.average([[0, 1]], A[None], 2, broken="transpose")[0]
    assert np.abs(R[1] - A).max() > 0.5 and np.abs(R[1] - A.T).max() < 1e-12
    # Gauss-Seidel instead of Jacobi: the path is set in one sweep instead of one level per sweep
    Rg = Q.random_rotations(5, np.random.default_rng(1)); Rg[0] = I3
    pairs = [[0, 1], [2, 1], [2, 3], [4, 3]]
    info = Q.average(pairs, Q.relative(Rg, pairs), 5, broken="gauss_seidel")[1]
    assert info[:, 1].tolist() == [0, 1, 1, 1, 1] != [0, 1, 2, 3, 4]
    # damping left out: the closed form of the second sweep
    Rr = np.stack([Q.rot(Z, 10.0), Q.rot(Z, 30.0)])
    tr = []
    Q.average([[0, 1]] * 2, Rr, 2, robust_deg=None, trace=tr, broken="no_damping")
    t10 = math.tan(math.radians(10.0))
    want = Q.rot(Z, 10.0 + 2 * math.degrees(math.atan(t10 / 4)))
    assert np.abs(tr[1][1] - want).max() > 1e-3
    _close(tr[1][1], Q.rot(Z, 10.0 + 2 * math.degrees(math.atan(t10 / 2))), 1e-15)          # the full step
    # and on a bipartite graph without a held camera in between the full step keeps swinging where the lazy one settles: 0 - 1 - 2 with
    # an inconsistent repeat on each edge
    pairs = [[0, 1], [0, 1], [1, 2], [1, 2]]
    Rr = np.stack([Q.rot(Z, 10.0), Q.rot(Z, 30.0), Q.rot(Z, 5.0), Q.rot(Z, 25.0)])
    lazy = Q.average(pairs, Rr, 3, robust_deg=None, sweeps=400)
    full = Q.average(pairs, Rr, 3, robust_deg=None, sweeps=400, broken="no_damping")
    assert lazy[3][3] == Q.CONVERGED
    _close(lazy[0][1], Q.rot(Z, 20.0), 1e-8); _close(lazy[0][2], Q.rot(Z, 35.0), 1e-8)
    assert full[3][0] != lazy[3][0]
