"""The refinement of relative poses on exported correspondence lists without a device (include/mi_degensac.h
mi_degensac_pose_refine_lists*, matcher.refine_pose, tensor_api.refine_pose_tensors): every refusal of both C entry points with its message
and its place in the order (each comes back as EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for),
K == 0 and cap == 0, the Python keyword and shape checks, and the restatement tests/pose_refine_ref.py itself: its Jacobian against central
differences of its own residual through its own retraction, exact and noisy scenes, every status on a scene written by hand, a pure
rotation, three broken restatements that these tests reject, and F against numpy's inverse."""
import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import pose_ref as P
from tests import pose_refine_ref as Q

EINVAL = -1
NAMES = ("dev", "host")
ALL = ("off", "pose", "cams", "pose_out", "cost", "info", "pts")


def _abi(which, K=2, cap=10, n_cams=4, max_trials=20, ftol=1e-12, null=()):
    """(rc, message) of one entry point; data pointers hold an address (never read: every call here is refused first) unless in `null`"""
    L = _lib.lib(); buf = np.zeros(64); addr = buf.ctypes.data
    A = lambda name: None if name in null else addr                    # noqa: E731
    head = (A("pts"), A("off"), None, A("pose"), A("cams"), n_cams, None, K, cap, max_trials, ftol, 0)
    outs = (A("pose_out"), A("cost"), A("info"), None, None)
    rc = L.mi_degensac_pose_refine_lists_dev(*head, None, *outs) if which == "dev" else L.mi_degensac_pose_refine_lists(*head, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and part in msg, (which, rc, msg)


def test_tile_constants_and_status_codes_are_mirrored():
    L = _lib.lib()
    assert L.mi_degensac_pose_refine_tile(0) == _lib.REFINE_STEP == 1024 and L.mi_degensac_pose_refine_tile(1) == _lib.REFINE_GRID == 256
    assert L.mi_degensac_pose_refine_tile(2) == -1
    assert (_lib.REFINE_CONVERGED, _lib.REFINE_STALLED, _lib.REFINE_MAX_TRIALS, _lib.REFINE_SHORT, _lib.REFINE_NOT_FINITE, _lib.REFINE_BAD_POSE,
            _lib.REFINE_BAD_CAMERA, _lib.REFINE_TRUNCATED) == \
        (Q.CONVERGED, Q.STALLED, Q.MAX_TRIALS, Q.SHORT, Q.NOT_FINITE, Q.BAD_POSE, Q.BAD_CAMERA, Q.TRUNCATED) == tuple(range(8))


def test_refusals_and_their_order():
    _refused(b"n_entries", K=-1)
    _refused(b"cap < 0", cap=-1)
    _refused(b"0x3fffffff", cap=0x40000000)
    _refused(b"n_cams", n_cams=-1)
    for m in (-1, 101, 1 << 20):
        _refused(b"max_trials", max_trials=m)
    for f in (float("nan"), -1e-300, -1.0, float("-inf")):
        _refused(b"ftol", ftol=f)
    _refused(b"corr_offsets", null=("off",))
    _refused(b"corr_offsets", null=("off",), K=0, cap=0)
    _refused(b"pose and cams", null=("pose",))
    _refused(b"pose and cams", null=("cams",))
    for name in ("pose_out", "cost", "info"):
        _refused(b"pose_out, cost and info", null=(name,))
    _refused(b"NULL argument: pts", null=("pts",))
    # each refusal hides every later one
    _refused(b"n_entries", K=-1, cap=-1, n_cams=-1, max_trials=-1, ftol=-1.0, null=ALL)
    _refused(b"cap < 0", cap=-1, n_cams=-1, max_trials=-1, ftol=-1.0, null=ALL)
    _refused(b"n_cams", n_cams=-1, max_trials=-1, ftol=-1.0, null=ALL)
    _refused(b"max_trials", max_trials=-1, ftol=-1.0, null=ALL)
    _refused(b"ftol", ftol=-1.0, null=ALL)
    _refused(b"corr_offsets", null=ALL)
    _refused(b"pose and cams", null=ALL[1:])
    _refused(b"pose_out, cost and info", null=ALL[3:])
    for m, f in ((0, 0.0), (100, float("inf")), (20, 1.0)):            # the closed ends are allowed: refused later, for the pointer
        _refused(b"NULL argument: pts", max_trials=m, ftol=f, null=("pts",))


def test_k0_and_cap0_succeed_without_a_device():
    for which in NAMES:
        rc, _ = _abi(which, K=0, cap=0, n_cams=0, null=ALL[1:])
        assert rc == 0, which


# ---- the Python checks ----
def _np(K=2, cap=10):
    return np.zeros((cap, 4)), np.zeros(K + 1, np.int64), np.zeros((K, 3, 3)), np.zeros((K, 3)), np.ones((K, 8))


@pytest.mark.parametrize("kw, part", [
    (dict(max_trials=-1), "max_trials"), (dict(max_trials=101), "max_trials"), (dict(max_trials=2.0), "max_trials"), (dict(max_trials=True), "max_trials"),
    (dict(ftol=-1e-9), "ftol"), (dict(ftol=float("nan")), "ftol"), (dict(ftol="x"), "ftol"), (dict(ftol=True), "ftol"),
    (dict(cams2=np.ones((3, 4))), "cams2"), (dict(pairs=np.zeros((2, 2), np.int32)), "cams1"), (dict(pairs=np.zeros((3, 2), np.int32)), "pairs"),
    (dict(keep=np.zeros(9, bool)), "keep"), (dict(keep=np.zeros(10, np.int32)), "keep"), (dict(min_parallax_deg=1.0), "unknown keyword"),
    (dict(with_points=True), "unknown keyword"),
])
def test_keyword_checks(kw, part):
    pts, off, R, t, cams = _np()
    with pytest.raises(ValueError, match=part):
        matcher.refine_pose(pts, off, R, t, cams, **kw)


def test_shape_and_dtype_checks():
    pts, off, R, t, cams = _np()
    table = np.ones((5, 4)); pr = ((2, 2), np.dtype(np.int32))
    chk = lambda a, b, c, d, e, **kw: matcher.check_refine_args(a.shape, a.dtype, b.shape, b.dtype, c.shape, c.dtype, d.shape, d.dtype, e.shape,  # noqa: E731
                                                                e.dtype, **kw)
    bad = [(pts[:, :3], off, R, t, cams, "pts"), (pts.astype(np.float32), off, R, t, cams, "pts"), (pts, off.astype(np.int32), R, t, cams, "corr_offsets"),
           (pts, off[:0], R, t, cams, "corr_offsets"), (pts, off.reshape(1, -1), R, t, cams, "corr_offsets"),
           (pts, off, R[:1], t, cams, "R should"), (pts, off, R.reshape(2, 9), t, cams, "R should"), (pts, off, R.astype(np.float32), t, cams, "R should"),
           (pts, off, R, t[:1], cams, "t should"), (pts, off, R, t[:, :2], cams, "t should"), (pts, off, R, t.astype(np.float32), cams, "t should"),
           (pts, off, R, t.ravel(), cams, "t should"), (pts, off, R, t, cams[:1], "cams1"), (pts, off, R, t, cams.astype(np.float32), "cams1")]
    for a, b, c, d, e, part in bad:
        with pytest.raises(ValueError, match=part):
            chk(a, b, c, d, e)
    assert chk(pts, off, R, t, cams) == (2, 10, 2, None, 20, 1e-12)
    assert chk(pts, off, R, t, table, pairs=pr, cams2=((3, 4), np.dtype(np.float64)), keep=((10,), np.dtype(bool)), max_trials=0, ftol=0) == (2, 10, 5, 3, 0, 0.0)
    assert chk(pts, off, R, t, table, pairs=pr, max_trials=np.int64(100), ftol=np.float32(1.0))[4:] == (100, 1.0)


def test_tensor_call_wants_tensors():
    from pydegensac_amd import tensor_api
    pts, off, R, t, cams = _np()
    with pytest.raises(ValueError, match="torch tensors"):
        tensor_api.refine_pose_tensors(pts, off, R, t, cams)
    import torch
    ts = [torch.from_numpy(x) for x in (pts, off, R, t, cams)]
    with pytest.raises(ValueError, match="ROCm device"):
        tensor_api.refine_pose_tensors(*ts)
    with pytest.raises(ValueError, match="unknown keyword"):
        tensor_api.refine_pose_tensors(*ts, min_parallax_deg=2.0)
    with pytest.raises(ValueError, match="max_trials"):
        tensor_api.refine_pose_tensors(*ts, max_trials=200)


# ---- the restatement ----
ONES = np.ones(200, bool)


def _scene(k, seed, sigma, deg=3.0):
    """200 rows of pair k of pose_ref.PAIRS under two different cameras, and a start pose `deg` degrees off in R and in t"""
    i, j = P.PAIRS[k]
    rows, F, Rg, tg, ci, cj = P.pair_rows(200, i, j, seed, sigma=sigma)
    return rows, Rg, tg, ci, cj, Q.perturbed(Rg, tg, [seed, k], deg)


def _jac_error(broken=None):
    """largest |J - central difference| over the largest |J| of the column, at perturbed poses of four noisy scenes"""
    worst = 0.0; h = 1e-5
    for k in range(4):
        rows, Rg, tg, ci, cj, q = _scene(k, 60, 0.5)
        Rm, t = q[:9].reshape(3, 3), q[9:]
        d = Q.rays(rows, ci, cj)
        Ms, u, v = Q.model(Rm, t, broken)
        r, J = Q.row_terms(Ms, ci, cj, d, broken)
        at = lambda dl: Q.row_terms(Q.model(*Q.retract(Rm, t, u, v, dl))[0][:1], ci, cj, d)[0]          # noqa: E731
        for c in range(5):
            dl = np.zeros(5); dl[c] = h
            num = (at(dl) - at(-dl)) / (2 * h)
            worst = max(worst, float(np.abs(num - J[c]).max() / np.abs(J[c]).max()))
    return worst


def test_jacobian_against_central_differences():
    """measured on these four scenes with h = 1e-5: 2.2e-10 of the column's largest entry; the bound is that with a margin of 100"""
    err = _jac_error()
    print("jacobian error", err)
    assert err <= 2.2e-8


@pytest.mark.parametrize("k", range(8))
def test_exact_scene_ends_at_the_generators_pose(k):
    """noise-free rows, the start 3 degrees off in R and in t: measured on these eight scenes, |R - Rg|_F <= 5.8e-16 and |t - tg| <= 3.1e-15
    (the cost falls from ~1e4 to ~1e-25 px^2); the bounds are those with a margin of 10.  No arccos: it cannot resolve below 1e-8."""
    rows, Rg, tg, ci, cj, q = _scene(k, 61, 0.0)
    out = Q.refine_entry(rows, ONES, q, ci, cj)
    eR = float(np.linalg.norm(out["pose"][:9].reshape(3, 3) - Rg)); et = float(np.linalg.norm(out["pose"][9:] - tg))
    print("exact scene", k, out["info"], out["cost"], eR, et)
    assert out["info"][3] in (Q.CONVERGED, Q.STALLED, Q.MAX_TRIALS) and out["info"][2] >= 3
    assert eR <= 5.8e-15 and et <= 3.1e-14 and out["cost"][1] < 1e-20 < 1e2 < out["cost"][0]


@pytest.mark.parametrize("k", range(8))
def test_noisy_scene_converges_below_the_generators_cost(k):
    """0.5 px of noise: CONVERGED, the cost falls, the end cost is at most the cost at the generator's pose by a plain numpy formula on
    numpy's inverse, and the gradient shrinks: measured max |g| end / start <= 8e-12 on these scenes, asserted with a margin of 100"""
    rows, Rg, tg, ci, cj, q = _scene(k, 62, 0.5)
    trace = []
    out = Q.refine_entry(rows, ONES, q, ci, cj, trace=trace)
    cg = Q.sampson_cost(Rg, tg, ci, cj, rows)
    own = Q.sampson_cost(out["pose"][:9], out["pose"][9:], ci, cj, rows)
    g0, g1 = np.abs(trace[0][1:6]).max(), np.abs(trace[-1][1:6]).max()
    print("noisy scene", k, out["info"], out["cost"], cg, own, g0, g1, g1 / g0)
    assert out["info"][3] == Q.CONVERGED and out["info"][0] == 200 and 1 <= out["info"][2] <= out["info"][1] <= 20
    assert out["cost"][1] <= out["cost"][0] and out["cost"][1] <= cg
    assert abs(own - out["cost"][1]) <= 1e-9 * own and abs(Q.sampson_cost(q[:9], q[9:], ci, cj, rows) - out["cost"][0]) <= 1e-9 * out["cost"][0]
    assert g1 <= 8e-10 * g0
    assert np.array_equal(out["resid"] ** 2 @ np.ones(200) > 0, True) and abs(float((out["resid"] ** 2).sum()) - out["cost"][1]) <= 1e-12 * out["cost"][1]
    Rm = out["pose"][:9].reshape(3, 3)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.norm(out["pose"][9:]) - 1) < 1e-15


def test_every_status_on_a_scene_written_by_hand():
    rows, Rg, tg, ci, cj, q = _scene(0, 62, 0.5)
    sc = dict(pts=rows, off=np.array([0, 200], np.int64), cams=np.array([ci, cj]), idx=None, keep=None, pose=q.reshape(1, 12))
    st = lambda s, *a: Q.reference(s, *a)                              # noqa: E731
    good = st(sc)
    assert good["info"][0].tolist() == [200, 13, 5, Q.CONVERGED]
    # STALLED: from the refined pose with ftol = 0 nothing is left to gain; lambda climbs past 1e12
    again = st(dict(sc, pose=good["pose"]), 100, 0.0)
    assert again["info"][0, 3] == Q.STALLED and again["info"][0, 1] < 100 and again["cost"][0, 1] <= again["cost"][0, 0]
    for mt in (0, 1, 3):
        r = st(sc, mt)
        assert r["info"][0].tolist()[1:] == [mt, min(mt, 3), Q.MAX_TRIALS] or mt == 3 and r["info"][0, 3] == Q.MAX_TRIALS
    zero = st(sc, 0)
    assert np.array_equal(zero["pose"], sc["pose"]) and zero["cost"][0, 0] == zero["cost"][0, 1] == good["cost"][0, 0]
    assert np.array_equal(zero["F"][0], Q.f_of(q[:9].reshape(3, 3), q[9:], ci, cj).ravel())
    one = st(sc, 20, 1.0)                                              # ftol = 1: the first accepted step ends the run
    assert one["info"][0].tolist()[1:] == [1, 1, Q.CONVERGED]
    keep = np.zeros(200, np.uint8); keep[[3, 70, 130, 199]] = 1
    short = st(dict(sc, keep=keep))
    assert short["info"][0].tolist() == [4, 0, 0, Q.SHORT] and np.array_equal(short["pose"], sc["pose"]) and np.isnan(short["cost"]).all()
    assert np.isnan(short["resid"]).all() and short["F"].any()
    keep[0] = 1
    assert st(dict(sc, keep=keep))["info"][0, 0] == 5 and st(dict(sc, keep=keep))["info"][0, 3] <= Q.MAX_TRIALS
    bad = rows.copy(); bad[17, 2] = np.nan
    nf = st(dict(sc, pts=bad))
    assert nf["info"][0].tolist() == [200, 0, 0, Q.NOT_FINITE] and np.array_equal(nf["pose"], sc["pose"]) and np.isnan(nf["cost"]).all()
    keep = np.ones(200, np.uint8); keep[17] = 0                        # the same row kept out: a run like any other
    assert st(dict(sc, pts=bad, keep=keep))["info"][0].tolist()[::3] == [199, Q.CONVERGED]
    for pose in (np.zeros(12), np.concatenate([q[:9], [0, 0, 0]]), np.concatenate([q[:9], [0, 1e-170, 0]]), np.where(np.arange(12) == 4, np.nan, q),
                 np.where(np.arange(12) == 10, np.inf, q)):
        bp = st(dict(sc, pose=pose.reshape(1, 12)))
        assert bp["info"][0].tolist() == [0, 0, 0, Q.BAD_POSE] and not bp["pose"].any() and not bp["F"].any() and np.isnan(bp["cost"]).all()
    for cams in (np.array([[0.0, 790, 500, 375], cj]), np.array([ci, [800, np.nan, 500, 375]]), np.array([ci, [np.inf, 790, 500, 375]])):
        bc = st(dict(sc, cams=cams, pose=np.zeros((1, 12))))           # BAD_CAMERA comes before BAD_POSE: the pose is copied through
        assert bc["info"][0].tolist() == [0, 0, 0, Q.BAD_CAMERA] and not bc["F"].any()
    assert st(dict(sc, idx=np.array([[0, 2]], np.int32)))["info"][0, 3] == Q.BAD_CAMERA
    for off in ([0, 201], [-1, 100], [150, 100], [201, 201]):
        tr = st(dict(sc, off=np.array(off, np.int64), cams=np.zeros((2, 4)), pose=np.full((1, 12), np.nan)))          # TRUNCATED comes first
        assert tr["info"][0].tolist() == [0, 0, 0, Q.TRUNCATED] and np.isnan(tr["pose"]).all() and not tr["F"].any()


def test_pure_rotation_ends_with_a_finite_pose():
    """two views from one centre: t is not observable.  Noise-free and with noise the run ends STALLED or CONVERGED within 100 trials, the
    pose is finite, R is the generator's rotation"""
    sc = Q.rotation_scene()
    a = 0.3; Rg = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    noisy = Q.reference(sc, 100)
    assert noisy["info"][0, 3] in (Q.STALLED, Q.CONVERGED) and np.isfinite(noisy["pose"]).all() and np.isfinite(noisy["cost"]).all()
    assert np.abs(noisy["pose"][0, :9].reshape(3, 3) - Rg).max() < 1e-3
    from pydegensac_amd import synthetic as syn
    rng = np.random.default_rng(49)
    cam = P.cam_of(0, False); X = np.stack([rng.uniform(-2, 2, 60), rng.uniform(-1.5, 1.5, 60), rng.uniform(4, 8, 60)], 1)
    rows = np.concatenate([syn._project(P.kmat(cam), np.eye(3), np.zeros(3), X), syn._project(P.kmat(cam), Rg, np.zeros(3), X)], 1)
    exact = Q.refine_entry(rows, np.ones(60, bool), sc["pose"][0], cam, cam, 100)
    assert exact["info"][3] in (Q.STALLED, Q.CONVERGED) and np.isfinite(exact["pose"]).all() and exact["cost"][1] < 1e-20
    assert np.abs(exact["pose"][:9].reshape(3, 3) - Rg).max() < 1e-12 and abs(np.linalg.norm(exact["pose"][9:]) - 1) < 1e-15


def test_sums_follow_the_header_on_numbers_written_by_hand():
    """g_0 = sum J_0 r with J_0 = 1 and r = 2^53 in row 0, 1 in rows 1, 33, 256 and 512.  Thread 0 adds rows 0, 256, 512 in turn: 2^53 + 1
    rounds back to 2^53 twice.  In wave 0 lane 1 takes v[1] + v[33] = 2 at m = 32 and lane 0 takes 2^53 + 2 at m = 1: the sum is 2^53 + 2.
    Taken lane after lane it would be 2^53; with the rows of a thread added last, 2^53 + 4."""
    r = np.zeros(600); r[[1, 33, 256, 512]] = 1.0; r[0] = 2.0 ** 53
    J = np.zeros((5, 600)); J[0] = 1.0
    use = np.ones(600, bool)
    assert Q.sums(r, J, use)[1] == 2.0 ** 53 + 2
    assert Q.sums(r, J, use, "tree")[1] == 2.0 ** 53
    use[33] = False                                                    # a row that is not used adds nothing
    assert Q.sums(r, J, use)[1] == 2.0 ** 53
    r2 = np.zeros(600); r2[[0, 64, 128, 192]] = [2.0 ** 53, 1.0, 1.0, 2.0]          # across the waves: ((w0 + w1) + w2) + w3
    assert Q.sums(r2, J, np.ones(600, bool))[1] == 2.0 ** 53 + 2


def test_broken_restatements_are_rejected():
    """the denominator's derivative dropped and the generators of a left-multiplied rotation: the Jacobian is off the central differences
    by far more than the bound, and the noisy scene no longer ends where the rule ends; the wave's sum taken lane after lane: other bits
    (test_sums_follow_the_header_on_numbers_written_by_hand) and another end pose"""
    assert _jac_error("nodenom") > 1e-3 and _jac_error("left") > 1e-3
    rows, Rg, tg, ci, cj, q = _scene(0, 62, 0.5)
    good = Q.refine_entry(rows, ONES, q, ci, cj)
    for broken in ("nodenom", "left", "tree"):
        other = Q.refine_entry(rows, ONES, q, ci, cj, broken=broken)
        assert not np.array_equal(other["pose"], good["pose"]), broken
    assert Q.refine_entry(rows, ONES, q, ci, cj, broken="left")["cost"][1] > 2 * good["cost"][1]


def test_F_against_numpys_inverse():
    for k in range(4):
        rows, Rg, tg, ci, cj, q = _scene(k, 62, 0.5)
        out = Q.refine_entry(rows, ONES, q, ci, cj)
        want = P.f_from_pose(out["pose"][:9].reshape(3, 3), out["pose"][9:], ci, cj)
        assert np.abs(out["F"].reshape(3, 3) - want).max() <= 1e-12 * np.abs(want).max()
        x1 = np.concatenate([rows[:, :2], np.ones((200, 1))], 1); x2 = np.concatenate([rows[:, 2:], np.ones((200, 1))], 1)
        F = out["F"].reshape(3, 3); l2 = x1 @ F.T; l1 = x2 @ F
        r = np.einsum("ni,ni->n", x2, l2) / np.sqrt(l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)
        assert np.abs(r - out["resid"]).max() <= 1e-9                  # the call's residual is the signed Sampson distance of its F, in pixels


def test_gpu_scene_catalogue_holds_the_edges():
    S = Q.gpu_scenes()
    k = S["keep"]; b = int(k["off"][1])
    assert np.flatnonzero(k["keep"][b:b + 1100]).min() >= 1024 + 64 and np.diff(k["off"]).tolist() == [0, 1100, 0, 700, 300, 90, 0]
    b = int(k["off"][3]); w = np.flatnonzero(k["keep"][b:b + 700]) // 64
    assert w.tolist() == list(range(11)) and k["keep"][int(k["off"][4]):int(k["off"][5])].sum() == 5 and not k["keep"][int(k["off"][5]):].any()
    st = lambda n: Q.reference(S[n])["info"][:, 3].tolist()            # noqa: E731
    assert st("offsets") == [Q.CONVERGED, Q.TRUNCATED, Q.TRUNCATED, Q.TRUNCATED, Q.CONVERGED]
    assert st("cameras") == [Q.BAD_CAMERA] * 5 + [Q.CONVERGED]
    assert st("poses")[:3] == [Q.BAD_POSE] * 3 and st("poses")[7:] == [Q.BAD_POSE, Q.CONVERGED]
    assert st("bad_rows") == [Q.NOT_FINITE, Q.NOT_FINITE, Q.CONVERGED, Q.NOT_FINITE]
    assert st("keep") == [Q.SHORT, Q.CONVERGED, Q.SHORT, Q.CONVERGED, Q.MAX_TRIALS, Q.SHORT, Q.SHORT]
    assert len(S["many"]["off"]) - 1 == 300 > _lib.REFINE_GRID
