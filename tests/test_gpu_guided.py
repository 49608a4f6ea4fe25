"""GPU: guided matching (include/mi_degensac.h mi_degensac_match_guided_*; tensor_api.guided_match_batch_tensors,
matcher.guided_match_batch, the guided=True stage of the batched match-and-verify calls).  The guided restatement (tests/guided_ref.py) forms every
(query, train) residual with the CPU oracle's own metric functions, gates it with `<=`, ranks the gated rows by the matcher's numpy
distances, and must agree with the device bit for bit: indices, distances, decisions and counts."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, parallel, synthetic as syn, tensor_api
from tests.guided_ref import oracle as _oracle

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _scene(model, n1, n2, seed, dim, norm, dup=True):
    """keypoints of a geometric scene (the pair's true model) + descriptors with true matches and exact duplicate train rows (ties)"""
    rng = np.random.default_rng(seed)
    n = max(n1, n2, 8)
    if model == "F":
        p1, p2, _, Mt = syn.two_view_fundamental(n, 0.6, 0.3, seed=seed)
        Md = Mt
    else:
        p1, p2, _, Mt = syn.homography_pairs(n, 0.6, 0.5, seed=seed)
        Md = np.linalg.inv(Mt).T
    k1, k2 = p1[:n1], p2[rng.permutation(n)[:n2]]
    if norm == "l2":
        d2 = rng.normal(size=(n2, dim)).astype(np.float32); d1 = rng.normal(size=(n1, dim)).astype(np.float32)
        m = min(n1, n2) // 2
        if m:
            d1[:m] = d2[rng.permutation(n2)[:m]] + 0.3 * rng.normal(size=(m, dim)).astype(np.float32)
    else:
        d2 = rng.integers(0, 256, size=(n2, dim), dtype=np.uint8); d1 = rng.integers(0, 256, size=(n1, dim), dtype=np.uint8)
        m = min(n1, n2) // 2
        if m:
            d1[:m] = d2[rng.permutation(n2)[:m]] ^ (rng.random((m, dim)) < 0.1).astype(np.uint8)
    if dup and n2 > 8:
        d2[5] = d2[3]; d2[7] = d2[3]; k2[5] = k2[3]
    return k1, k2, d1, d2, Md


SIZES = [(0, 50), (40, 0), (70, 1), (1, 3), (130, 2), (3, 0), (64, 64), (65, 200), (300, 280), (250, 320), (40, 2100)]


def _batch(model, norm, dim, seed):
    K1, K2, D1, D2, M = [], [], [], [], []
    for i, (n1, n2) in enumerate(SIZES):
        k1, k2, d1, d2, Md = _scene(model, n1, n2, seed * 100 + i, dim, norm)
        K1.append(k1); K2.append(k2); D1.append(d1); D2.append(d2); M.append(Md)
    M[-3] = np.zeros((3, 3))                                             # a short / failed pair
    return K1, K2, D1, D2, np.stack(M)


def _run(K1, K2, D1, D2, M, model, **kw):
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    match, idx, dist = tensor_api.guided_match_batch_tensors(_t(np.concatenate(K1)), _t(np.concatenate(K2)), _t(np.concatenate(D1)),
                                                             _t(np.concatenate(D2)), c1, c2, _t(M), model=model, driver_form=True, **kw)
    o = np.zeros(len(c1) + 1, np.int64); o[1:] = np.cumsum(c1)
    match, idx, dist = match.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()
    return [(match[o[p]:o[p + 1]], idx[o[p]:o[p + 1]], dist[o[p]:o[p + 1]]) for p in range(len(c1))]


_KINDS = [("F", 0), ("F", 1), ("H", 0), ("H", 1), ("H", 2), ("H", 3), ("H", 4)]
# every error type with and without mutual on L2 / 37; the Sampson kinds and the square-root transfer error on L2 / 128 and Hamming
_EXACT = ([(m, e, "l2", 37, mu) for m, e in _KINDS for mu in (False, True)]
          + [(m, e, n, d, False) for m, e in [("F", 0), ("H", 0), ("H", 2)] for n, d in [("l2", 128), ("hamming", 32)]])


@pytest.mark.parametrize("model,et,norm,dim,mutual", _EXACT)
def test_bit_exact_against_the_oracle(oracle_port, model, et, norm, dim, mutual):
    px = 12.0 if (model == "H" and et in (2, 4)) else 6.0              # a band of a few percent of the image
    name = {"F": ["sampson", "symm_epipolar"], "H": ["sampson", "symm_sq_max", "symm_max", "symm_sq_sum", "symm_sum"]}[model][et]
    K1, K2, D1, D2, M = _batch(model, norm, dim, seed=et + 7 * (dim == 128))
    got = _run(K1, K2, D1, D2, M, model, ratio=0.9, mutual=mutual, px_th=px, error_type=name)
    passed = 0
    for p in range(len(SIZES)):
        oi, od, om = _oracle(oracle_port, model, et, px, M[p], K1[p], K2[p], D1[p], D2[p], norm, 0.9, mutual)
        gm, gi, gd = got[p]
        assert np.array_equal(gi, oi), (p, np.flatnonzero((gi != oi).any(1))[:5])
        assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), p
        assert np.array_equal(gm, om), p
        passed += int((gi[:, 0] >= 0).sum())
    assert passed > 200                                                  # the gates let real candidates through
    # the counts of the device entry point
    mp = _lib.MatchParams(0 if norm == "l2" else 1, dim, 0.9, mutual); gp = _lib.GuideParams(model == "H", et, px)
    c1 = np.array([len(x) for x in D1]); c2 = np.array([len(x) for x in D2])
    o1 = np.zeros(len(c1) + 1, np.int64); o1[1:] = np.cumsum(c1); o2 = np.zeros(len(c2) + 1, np.int64); o2[1:] = np.cumsum(c2)
    A, B = np.ascontiguousarray(np.concatenate(D1)), np.ascontiguousarray(np.concatenate(D2))
    X1, X2 = np.ascontiguousarray(np.concatenate(K1)), np.ascontiguousarray(np.concatenate(K2))
    idx = np.zeros((len(A), 2), np.int32); dist = np.zeros((len(A), 2), np.float32); match = np.zeros(len(A), np.int32); cnt = np.zeros(len(c1), np.int32)
    Mh = np.ascontiguousarray(M.reshape(-1, 9))
    _lib.check_match(_lib.lib().mi_degensac_match_guided_batch(C.byref(mp), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p),
                     o1.ctypes.data_as(C.POINTER(C.c_int64)), o2.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(X1), _lib.dptr(X2), 2,
                     len(c1), _lib.dptr(Mh), C.byref(gp), 0, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                     dist.ctypes.data_as(C.POINTER(C.c_float)), match.ctypes.data_as(C.POINTER(C.c_int32)), cnt.ctypes.data_as(C.POINTER(C.c_int32))))
    assert list(cnt) == [int((g[0] >= 0).sum()) for g in got]
    assert np.array_equal(match, np.concatenate([g[0] for g in got]))


@pytest.mark.parametrize("model,et", [("F", 0), ("F", 1), ("H", 0), ("H", 3)])
@pytest.mark.parametrize("norm,dim", [("l2", 37), ("l2", 128), ("hamming", 32)])
def test_gate_wide_open_equals_the_unguided_matcher(model, et, norm, dim):
    rng = np.random.default_rng(dim + et)
    sizes = [(70, 1), (64, 64), (65, 200), (300, 280), (40, 2100), (130, 1500)]
    K1, K2, D1, D2, M = [], [], [], [], []
    for i, (n1, n2) in enumerate(sizes):
        k1, k2, d1, d2, _ = _scene(model, n1, n2, 300 + i, dim, norm)
        K1.append(k1); K2.append(k2); D1.append(d1); D2.append(d2)
        M.append(rng.normal(size=(3, 3)))                              # any model: every residual is below 1e200
    name = {"F": ["sampson", "symm_epipolar"], "H": ["sampson", "symm_sq_max", "symm_max", "symm_sq_sum"]}[model][et]
    got = _run(K1, K2, D1, D2, np.stack(M), model, px_th=1e100, error_type=name)
    ui, ud = tensor_api.knn_match_batch_tensors(_t(np.concatenate(D1)), _t(np.concatenate(D2)), [len(x) for x in D1], [len(x) for x in D2])
    ui, ud = ui.cpu().numpy(), ud.cpu().numpy()
    o = 0
    for p, (n1, _) in enumerate(sizes):
        assert np.array_equal(got[p][1], ui[o:o + n1]), p
        assert np.array_equal(got[p][2].view(np.uint32), ud[o:o + n1].view(np.uint32)), p
        o += n1


def test_zero_models_and_batch_composition():
    K1, K2, D1, D2, M = _batch("F", "l2", 64, seed=3)
    kw = dict(ratio=0.9, mutual=True, px_th=6.0)
    zero = _run(K1, K2, D1, D2, np.zeros_like(M), "F", **kw)
    for m, i, d in zero:
        assert (m == -1).all() and (i == -1).all() and np.isinf(d).all()
    full = _run(K1, K2, D1, D2, M, "F", **kw)
    assert sum(int((g[0] >= 0).sum()) for g in full) > 50
    keep = [0, 2, 4, 6, 7, 10]
    part = _run([K1[p] for p in keep], [K2[p] for p in keep], [D1[p] for p in keep], [D2[p] for p in keep], M[keep], "F", **kw)
    for j, p in enumerate(keep):
        alone = _run([K1[p]], [K2[p]], [D1[p]], [D2[p]], M[p:p + 1], "F", **kw)
        for other in (part[j], alone[0]):
            assert all(np.array_equal(u, v) for u, v in zip(full[p], other)), p


def _f_pairs(sizes, seed, dim=64):
    rng = np.random.default_rng(seed)
    K1, K2, D1, D2 = [], [], [], []
    for i, n in enumerate(sizes):
        p1, p2, lab, _ = syn.two_view_fundamental(max(n, 50), 0.5, 0.1, seed=seed * 1000 + i)
        p1, p2, lab = p1[:n], p2[:n], lab[:n]
        d1 = rng.normal(size=(n, dim)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32)
        d2[~lab] = rng.normal(size=((~lab).sum(), dim)).astype(np.float32)
        perm = rng.permutation(n)
        K1.append(p1); K2.append(p2[perm]); D1.append(d1); D2.append(d2[perm])
    return K1, K2, D1, D2


@pytest.mark.parametrize("model,mutual", [("F", False), ("F", True), ("H", False)])
def test_guided_stage_of_match_and_verify_composes(model, mutual):
    sizes = [600, 5, 1100, 0, 900]
    K1, K2, D1, D2 = _f_pairs(sizes, seed=9)
    seeds = parallel.pair_seeds(0, len(sizes))
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    args = (_t(np.concatenate(K1)), _t(np.concatenate(K2)), _t(np.concatenate(D1)), _t(np.concatenate(D2)), c1, c2)
    kw = dict(model=model, mutual=mutual, seeds=seeds, px_th=2.0, max_iters=5000)
    plain = tensor_api.match_and_verify_batch_tensors(*args, **kw)
    both = tensor_api.match_and_verify_batch_tensors(*args, guided=True, **kw)
    assert len(plain) == 5 and len(both) == 6
    for u, v in zip(plain[:3], both[:3]):
        assert np.array_equal(u.cpu().numpy(), v.cpu().numpy())
    det = [c for c in range(16) if c not in (12, 13)]                    # every stats column but the device clock ticks
    assert np.array_equal(plain[3].cpu().numpy()[:, det], both[3].cpu().numpy()[:, det])
    assert np.array_equal(plain[4], both[4])
    gm = both[5].cpu().numpy()
    assert (gm >= 0).sum() > 0
    if model == "F":                                                     # F: the returned models are the driver's form
        ref = tensor_api.guided_match_batch_tensors(*args, both[0], model="F", mutual=mutual, px_th=2.0, driver_form=True)[0]
        assert np.array_equal(gm, ref.cpu().numpy())
    # host-pointer form: same first three elements as without guided, guided matches equal to the tensor form
    h0 = matcher.match_and_verify_batch(K1, K2, D1, D2, model=model, mutual=mutual, seeds=seeds, px_th=2.0, max_iters=5000)
    h1 = matcher.match_and_verify_batch(K1, K2, D1, D2, model=model, mutual=mutual, seeds=seeds, px_th=2.0, max_iters=5000, guided=True)
    assert len(h0) == 3 and len(h1) == 4
    assert np.array_equal(h0[0], h1[0]) and all(np.array_equal(u, v) for a, b in zip(h0[1:], h1[1:3]) for u, v in zip(a, b))
    o = np.zeros(len(c1) + 1, np.int64); o[1:] = np.cumsum(c1)
    for p in range(len(sizes)):
        assert np.array_equal(h1[3][p], gm[o[p]:o[p + 1]]), p


def _decoy_scene(model, n, seed, dim=64):
    """every true correspondence gets a decoy train row: a near-duplicate descriptor at a keypoint far outside the model's band"""
    rng = np.random.default_rng(seed)
    if model == "F":
        p1, p2, lab, M = syn.two_view_fundamental(n, 1.0, 0.1, seed=seed)
        l2 = np.c_[p1, np.ones(n)] @ M.T                               # epipolar lines in image 2 (x2^T F x1 = 0)
        nrm = l2[:, :2] / np.linalg.norm(l2[:, :2], axis=1, keepdims=True)
        dec = p2 + 40.0 * nrm * rng.choice([-1.0, 1.0], (n, 1))
    else:
        p1, p2, lab, M = syn.homography_pairs(n, 1.0, 0.3, seed=seed)
        a = rng.uniform(0, 2 * np.pi, n)
        dec = p2 + 40.0 * np.c_[np.cos(a), np.sin(a)]
    d1 = rng.normal(size=(n, dim)).astype(np.float32)
    dt = d1 + 0.05 * rng.normal(size=d1.shape).astype(np.float32)
    dd = d1 + 0.05 * rng.normal(size=d1.shape).astype(np.float32)
    perm = rng.permutation(2 * n)
    k2 = np.concatenate([p2, dec])[perm]; d2 = np.concatenate([dt, dd])[perm]
    truth = np.argsort(perm)[:n]                                         # train row of query i's true match
    return p1, k2, d1, d2, M, truth


@pytest.mark.parametrize("model", ["F", "H"])
def test_guided_matching_recovers_what_the_ratio_test_loses(model):
    K1, K2, D1, D2, M, T = [], [], [], [], [], []
    for i in range(4):
        k1, k2, d1, d2, m, truth = _decoy_scene(model, 800, 70 + i)
        K1.append(k1); K2.append(k2); D1.append(d1); D2.append(d2); M.append(m); T.append(truth)
    n_true = sum(len(t) for t in T)
    unguided = sum(int((t == T[p][q]).sum()) for p in range(4) for q, t, _ in [matcher.match_snn(D1[p], D2[p], 0.9)])
    assert unguided < 0.5 * n_true, unguided                             # the decoys defeat the plain ratio test
    res = matcher.guided_match_batch(K1, K2, D1, D2, np.stack(M), model=model, px_th=2.0)
    good = bad = 0
    for p, (q, t, _) in enumerate(res):
        ok = t == T[p][q]
        good += int(ok.sum()); bad += int((~ok).sum())
    assert good >= 0.9 * n_true, (good, n_true)
    assert bad <= 0.01 * n_true, (bad, n_true)                           # false matches: at most 1 % of the true ones
    # one pair through the single-pair form gives the same
    q, t, d = matcher.guided_match(K1[1], K2[1], D1[1], D2[1], M[1], model=model, px_th=2.0)
    assert np.array_equal(q, res[1][0]) and np.array_equal(t, res[1][1]) and np.array_equal(d, res[1][2])
