"""Rotation averaging on the device (include/mi_degensac.h mi_degensac_rotation_average_dev, tensor_api.average_rotations_tensors,
matcher.average_rotations): every output at full length, between guard elements, bit for bit against the restatement tests/rotavg_ref.py
(tested by itself in tests/test_rotavg_cpu.py), at both sides of a group of G lanes, of a second stride, of a workgroup of cameras, of the
diameter of a path, with every kind of unused edge, both gauges, opposed edges, the parameter grid, absent outputs, reused outputs, a
second stream, the numpy form, the chain from relative_pose_tensors under the sync-debug mode "error", and ten calls with the same
bytes."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, synthetic
from tests import rotavg_ref as Q

pytestmark = pytest.mark.gpu
GUARD = 8
I3 = np.eye(3)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _guarded(shape, dtype):
    """(the whole tensor with GUARD sentinel elements on either side, the view between them, the sentinel)"""
    import torch
    n = int(np.prod(shape))
    fill = 7.25 if dtype.is_floating_point else 77
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=_dev())
    return whole, whole[GUARD:GUARD + n].view(*shape), fill


def run_dev(pairs, R_rel, n, weight=None, edge_keep=None, R0=None, known=None, root=0, sweeps=200, damping=0.5, robust_deg=5.0, tol=1e-9,
            with_edges=True, outs=None):
    """the _dev entry point on guarded outputs -> numpy (R, info, step, summary, edge_cos or None); the guards are checked"""
    import torch
    dev = _dev()
    K = len(pairs)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt))).to(dev)          # noqa: E731
    pr = up(np.asarray(pairs, np.int32).reshape(K, 2), np.int32); Rr = up(np.asarray(R_rel).reshape(K, 9), np.float64)
    w = up(weight, np.float64); kp = up(edge_keep, np.uint8); r0 = up(R0, np.float64); kn = up(known, np.uint8)
    if outs is None:
        outs = [_guarded((n, 9), torch.float64), _guarded((n, 4), torch.int32), _guarded((n,), torch.float64), _guarded((4,), torch.int64),
                _guarded((max(K, 1),), torch.float64)]
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()          # noqa: E731
    stream = torch.cuda.current_stream(dev)
    rc = _lib.lib().mi_degensac_rotation_average_dev(p(pr), p(Rr), p(w), p(kp), K, n, p(r0), p(kn), root, sweeps, damping,
                                                     0.0 if robust_deg is None else robust_deg, tol, 0, C.c_void_p(stream.cuda_stream),
                                                     *[o[1].data_ptr() for o in outs[:4]], outs[4][1].data_ptr() if with_edges else None)
    _lib.check_match(rc)
    torch.cuda.synchronize()
    for whole, view, fill in outs if with_edges else outs[:4]:
        g = whole.cpu().numpy()
        assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), "a guard element was written"
    if not with_edges:
        assert (outs[4][0].cpu().numpy() == outs[4][2]).all(), "edge_cos was written though it is absent"
    res = [o[1].cpu().numpy() for o in outs[:4]]
    res[0] = res[0].reshape(n, 3, 3)
    return res + [outs[4][1].cpu().numpy()[:K] if with_edges else None], outs


def same(got, want, what=""):
    """bit for bit, NaN payloads included"""
    names = ("R", "info", "step", "summary", "edge_cos")
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        g = np.ascontiguousarray(g); w = np.ascontiguousarray(w).astype(g.dtype)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.dtype == np.float64:
            gn, wn = np.isnan(g), np.isnan(w)
            assert (gn == wn).all(), (what, name, "NaN positions")
            ok = (g.view(np.int64) == w.view(np.int64)) | gn
        else:
            ok = g == w
        assert ok.all(), (what, name, np.argwhere(~ok)[:5].tolist(), g[~ok][:5], w[~ok][:5])


def check(pairs, R_rel, n, what="", **kw):
    got, _ = run_dev(pairs, R_rel, n, **kw)
    kw.pop("with_edges", None)
    want = Q.average(pairs, R_rel, n, **kw)
    same(got, want, what)
    return got


def graph(n, rng, chords=2, noise=2.0):
    """a ring with random chords in random orientations, noisy relative rotations of random cameras"""
    Rg = Q.random_rotations(n, rng)
    pairs = [[c, (c + 1) % n] for c in range(n)] if n > 2 else [[0, 1]] * (n - 1)
    pairs += [list(rng.integers(0, n, 2)) for _ in range(chords * n if n > 3 else 0)]          # (self edges among them: unused)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    ok = pairs[:, 0] != pairs[:, 1]
    Rr = np.zeros((len(pairs), 3, 3))
    Rr[ok] = Q.relative(Rg, pairs[ok], rng, noise)
    Rr[~ok] = I3
    return Rg, pairs, Rr


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 255, 256, 257])
def test_camera_counts_at_both_sides_of_a_workgroup(n):
    rng = np.random.default_rng(n)
    Rg, pairs, Rr = graph(n, rng)
    w = rng.uniform(0.5, 2.0, len(pairs))
    got = check(pairs, Rr, n, f"n={n}", weight=w, sweeps=12, root=n // 3)
    assert got[3][1] == n


@pytest.mark.parametrize("d", [0, 1, 15, 16, 17, 63, 64, 65, 257])
def test_hub_degrees_at_both_sides_of_a_group_and_a_stride(d):
    """camera 1 is a hub of degree d that is not held: its d half-edges meet in one group's sums; camera 0 holds the gauge"""
    rng = np.random.default_rng(1000 + d)
    n = max(d + 1, 2)
    Rg = Q.random_rotations(n, rng)
    others = [0] + list(range(2, n))
    pairs = np.array([[1, others[k % len(others)]] if k % 3 else [others[k % len(others)], 1] for k in range(d)], np.int64).reshape(-1, 2)
    Rr = Q.relative(Rg, pairs, rng, 3.0)
    w = rng.uniform(0.5, 2.0, len(pairs))
    for rb in (None, 5.0):
        got = check(pairs, Rr, n, f"d={d}", weight=w, sweeps=6, robust_deg=rb, tol=0.0)
        assert got[1][1, 0] == d


@pytest.mark.parametrize("n", [5, 17, 33])
def test_paths_below_at_and_above_the_diameter(n):
    rng = np.random.default_rng(n)
    Rg = Q.random_rotations(n, rng)
    pairs = np.array([[c, c + 1] if c % 2 else [c + 1, c] for c in range(n - 1)])
    Rr = Q.relative(Rg, pairs, rng, 1.0)
    cams, glob = set(), []
    for sweeps in (n - 3, n - 1, n + 4):
        got = check(pairs, Rr, n, f"path {n} sweeps {sweeps}", sweeps=sweeps)
        assert got[3][1] == min(sweeps + 1, n)
        glob.append(int(got[3][3])); cams.update(got[1][:, 3].tolist())
    assert Q.UNREACHED in cams and glob == [Q.MAX_SWEEPS, Q.MAX_SWEEPS, Q.CONVERGED]


@pytest.mark.parametrize("n", [16, 17])
def test_complete_graphs_and_stars(n):
    rng = np.random.default_rng(n)
    Rg = Q.random_rotations(n, rng)
    pairs = matcher.exhaustive_pairs(n)
    Rr = Q.relative(Rg, pairs, rng, 2.0)
    got = check(pairs, Rr, n, f"K{n}", robust_deg=None)
    assert got[3][3] == Q.CONVERGED
    check(pairs, Rr, n, f"K{n} tol 0", tol=0.0, sweeps=60)
    star = np.array([[0, k] if k % 2 else [k, 0] for k in range(1, n)])
    Rs = Q.relative(Rg, star, rng, 2.0)
    for root in (0, n - 1):
        check(star, Rs, n, f"star {n} root {root}", root=root)


def test_unused_edges_and_cameras_without_edges():
    rng = np.random.default_rng(3)
    n = 40                                                             # cameras 0 .. 2, 20 .. 22 and 37 .. 39 have no used edge
    Rg = Q.random_rotations(n, rng)
    live = [c for c in range(3, 37) if not 20 <= c <= 22]
    pairs = [[live[k], live[k + 1]] for k in range(len(live) - 1)]
    pairs += [[b, a] for a, b in pairs[::3]] + pairs[::4]             # both orientations and repeats
    good = len(pairs)
    pairs += [[5, 5], [-1, 4], [4, n], [n + 7, -3], [0x7fffffff, 2], [0, 1], [20, 21], [38, 39]]
    pairs = np.asarray(pairs, np.int64)
    Rr = np.stack([I3] * len(pairs))
    Rr[:good] = Q.relative(Rg, pairs[:good], rng, 1.0)
    keep = np.ones(len(pairs), np.uint8); keep[-3:] = 0
    got = check(pairs, Rr, n, "unused", edge_keep=keep, root=live[0], sweeps=60)
    assert got[3][2] == good and sorted(np.flatnonzero(got[1][:, 3] == Q.ISOLATED)) == [0, 1, 2, 20, 21, 22, 37, 38, 39]
    got = check(pairs, Rr, n, "keep all zero", edge_keep=np.zeros(len(pairs), np.uint8), root=4)
    assert got[3].tolist() == [0, 1, 0, Q.CONVERGED] and np.isnan(got[4]).all()
    # matrices and weights that are not finite, or not rotations
    w = rng.uniform(0.5, 2.0, len(pairs)); w[1] = 0.0; w[2] = np.nan; w[3] = -1.0; w[4] = np.inf
    Rb = Rr.copy(); Rb[6] = 0.0; Rb[7] = np.nan; Rb[8] = 1.01 * Rb[8]; Rb[9][0, 0] = np.inf
    got = check(pairs, Rb, n, "not finite", weight=w, edge_keep=keep, root=live[0], sweeps=60)
    assert np.isnan(got[4][[1, 2, 3, 4, 6, 7, 8, 9]]).all()


def test_two_components_roots_and_known_cameras():
    rng = np.random.default_rng(4)
    n = 20
    Rg = Q.random_rotations(n, rng)
    pairs = np.array([[c, c + 1] for c in range(9)] + [[c, c + 1] for c in range(10, 19)] + [[0, 9], [10, 19]])
    Rr = Q.relative(Rg, pairs, rng, 1.0)
    got = check(pairs, Rr, n, "root 13", root=13)
    assert (got[1][:10, 3] == Q.UNREACHED).all() and (got[1][10:, 3] != Q.UNREACHED).all()
    known = np.zeros(n, np.uint8); known[[2, 15]] = 1
    R0 = np.full((n, 3, 3), 3.5); R0[2] = Rg[2]; R0[15] = Rg[15]
    got = check(pairs, Rr, n, "two known", R0=R0, known=known, root=7)
    assert got[3][1] == n and (got[0][2] == Rg[2]).all() and (got[0][15] == Rg[15]).all()
    got = check(pairs, Rr, n, "no root", R0=R0, known=np.zeros(n, np.uint8))
    assert got[3].tolist() == [0, 0, len(pairs), Q.NO_ROOT]


def test_opposed_edges():
    Rr = np.stack([I3, np.diag([-1.0, -1.0, 1.0]), Q.rot((0, 0, 1), 179.9999), Q.rot((0, 0, 1), 170.0)])
    got = check([[0, 1]] * 4, Rr, 2, "opposed", robust_deg=None, sweeps=2)
    assert got[1][1, 2] == 2                                           # the edges at 180 and 179.9999 degrees; the one at 170 counts


@pytest.mark.parametrize("sweeps", [0, 1, 200])
@pytest.mark.parametrize("damping", [0.5, 1.0])
@pytest.mark.parametrize("robust_deg", [None, 5.0])
def test_parameter_grid(sweeps, damping, robust_deg):
    rng = np.random.default_rng(9)
    Rg, pairs, Rr = graph(23, rng, noise=3.0)
    check(pairs, Rr, 23, "grid", sweeps=sweeps, damping=damping, robust_deg=robust_deg, tol=0.0 if damping == 1.0 else 1e-9)


def test_absent_and_reused_outputs_a_second_stream_and_the_numpy_form():
    import torch
    from pydegensac_amd import tensor_api as T
    rng = np.random.default_rng(12)
    Rg, pairs, Rr = graph(30, rng)
    want = Q.average(pairs, Rr, 30)
    got, outs = run_dev(pairs, Rr, 30, with_edges=False)
    same(got, want, "no edge_cos")
    # the same outputs again, for another problem and then for the first: nothing of the earlier call is left
    Rg2, pairs2, Rr2 = graph(30, np.random.default_rng(13))
    pairs2 = pairs2[:len(pairs)]; Rr2 = Rr2[:len(pairs)]
    same(run_dev(pairs2, Rr2, 30, outs=outs)[0], Q.average(pairs2, Rr2, 30), "reused 1")
    same(run_dev(pairs, Rr, 30, outs=outs)[0], want, "reused 2")
    # the tensor form on a second stream, int64 pairs, bool keep
    dev = _dev()
    keep = rng.random(len(pairs)) < 0.9
    want_k = Q.average(pairs, Rr, 30, edge_keep=keep)
    side = torch.cuda.Stream(dev)
    tp = torch.from_numpy(pairs).to(dev); tr = torch.from_numpy(Rr).to(dev); tk = torch.from_numpy(keep).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        res = T.average_rotations_tensors(tp, tr, 30, edge_keep=tk, with_edges=True)
    side.synchronize()
    same([x.cpu().numpy() for x in res], want_k, "second stream")
    assert len(T.average_rotations_tensors(tp, tr, 30)) == 4
    # the numpy form
    same(matcher.average_rotations(pairs, Rr, 30, edge_keep=keep, with_edges=True), want_k, "numpy")
    same(matcher.average_rotations(pairs.astype(np.int32), Rr, 30), want[:4], "numpy, no edges")
    same(matcher.average_rotations(np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), 3, with_edges=True), Q.average(np.zeros((0, 2)), np.zeros((0, 3, 3)), 3),
         "no pairs")


def test_ten_calls_give_the_same_bytes():
    rng = np.random.default_rng(21)
    Rg, pairs, Rr = graph(257, rng, noise=3.0)
    first = run_dev(pairs, Rr, 257, sweeps=40, tol=0.0)[0]
    for _ in range(9):
        same(run_dev(pairs, Rr, 257, sweeps=40, tol=0.0)[0], first, "repeat")


def test_chain_from_the_pose_calls_without_a_synchronisation():
    """descriptors -> verify -> export -> refit -> pose -> refine -> average with torch's sync-debug mode at "error" from the pose call on;
    the result equals the restatement on the refined rotations, and the cameras come out near the generator's"""
    import torch
    from pydegensac_amd import tensor_api as T
    M, n, px = 6, 600, 0.5
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, 64, seed=0)
    Kc, poses = synthetic.collection_cameras(M)
    pairs = matcher.exhaustive_pairs(M)
    dev = _dev()
    counts = [len(x) for x in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F, match, inlier, stats, n_tent, po = T.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", px_th=px)
    rows, co, total, _, pts, resid = T.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inlier, kps1=k, kps2=k, models=F)
    F2, member, info_r = T.refit_correspondences_tensors(pts, co, F, "F", px_th=px)
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * M, dtype=torch.float64, device=dev)
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        R, t, front, info = T.relative_pose_tensors(pts, co, F2, cams, pairs=pr, keep=member)
        R2, t2, cost, info2 = T.refine_pose_tensors(pts, co, R, t, cams, pairs=pr, keep=front)
        weight = info[:, 3].double(); keep = info[:, 4] == _lib.POSE_OK
        Rg, ginfo, step, summary, ecos = T.average_rotations_tensors(pr, R2, M, weight=weight, edge_keep=keep, with_edges=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = [x.cpu().numpy() for x in (Rg, ginfo, step, summary, ecos)]
    want = Q.average(pairs, R2.cpu().numpy(), M, weight=weight.cpu().numpy(), edge_keep=keep.cpu().numpy())
    same(got, want, "chain")
    truth = np.stack([Rm for Rm, _ in poses])
    assert got[3][1] == M and got[3][3] == Q.CONVERGED and keep.all()
    # The bound.  At the fixed point a camera's weighted mean residual is zero, so to first order its error is the weighted mean of
    # (neighbour's error + edge's error) over its edges; the root's error is 0 and every camera has an edge to it (complete graph), so the
    # largest camera error E obeys E <= (1 - s) E + eps with s the smallest share of the root's edge in a camera's weights and eps the
    # largest error of a pairwise rotation: E <= eps / s.
    R2n = R2.cpu().numpy(); wn = weight.cpu().numpy()
    eps = max(float(Q.angle_deg(R2n[e], truth[j] @ truth[i].T)) for e, (i, j) in enumerate(pairs))
    share = min(wn[[e for e, (i, j) in enumerate(pairs) if 0 in (i, j) and c in (i, j)][0]] / wn[[e for e, (i, j) in enumerate(pairs) if c in (i, j)]].sum()
                for c in range(1, M))
    err = Q.gauge_errors(got[0], truth)
    print("pairwise error", eps, "share", share, "camera errors", err)
    assert err.max() <= eps / share + 1e-6
