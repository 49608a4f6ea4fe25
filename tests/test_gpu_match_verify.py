"""GPU: batched match-and-verify (include/mi_degensac.h mi_degensac_match_knn2_batch_dev / mi_degensac_match_verify_batch[_dev]).
Every stage equals its single-pair counterpart bit for bit: the batched 2-NN equals matcher.knn_match and the numpy oracle, the
tentatives equal match_snn, and the models / masks / counters equal findFundamentalMatrixBatch / findHomographyBatch on those
tentatives, whatever else is in the batch."""
import ctypes as C
import functools

import numpy as np
import pytest

import pydegensac_amd as pd
from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher, parallel, synthetic as syn, tensor_api

pytestmark = pytest.mark.gpu

MI_ST_SAMPLES, MI_ST_LO_RUNS, MI_ST_I = 0, 1, 3


def _descs(rng, n1, n2, dim, kind):
    # copy of tests/test_matcher.py::_descs: true matches, exact duplicate train rows (ties)
    if kind == "l2":
        b = rng.normal(size=(n2, dim)).astype(np.float32)
        a = rng.normal(size=(n1, dim)).astype(np.float32)
        m = min(n1, n2) // 2
        a[:m] = b[rng.permutation(n2)[:m]] + 0.05 * rng.normal(size=(m, dim)).astype(np.float32)
        if n2 > 8:
            b[5] = b[3]; b[7] = b[3]
        return a, b
    b = rng.integers(0, 256, size=(n2, dim), dtype=np.uint8)
    a = rng.integers(0, 256, size=(n1, dim), dtype=np.uint8)
    m = min(n1, n2) // 2
    a[:m] = b[rng.permutation(n2)[:m]] ^ (rng.random((m, dim)) < 0.03).astype(np.uint8)
    if n2 > 8:
        b[5] = b[3]
    return a, b


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _ragged(kind, dim, sizes, seed):
    rng = np.random.default_rng(seed)
    D1, D2 = [], []
    for n1, n2 in sizes:
        a, b = _descs(rng, n1, n2, dim, kind)
        if kind == "hamming":
            _, a, b = matcher._prep(a, b, "hamming")                   # padded to whole 32-bit words
        D1.append(a); D2.append(b)
    return D1, D2


def _sizes(rng, K, lo, hi):
    s = [(0, 50), (40, 0), (70, 1), (1, 3), (130, 2), (64, 64), (65, 200)]
    return s + [(int(a), int(b)) for a, b in zip(rng.integers(lo, hi, K - len(s)), rng.integers(lo, hi, K - len(s)))]


@pytest.mark.parametrize("kind,dim", [("l2", 37), ("l2", 64), ("l2", 128), ("hamming", 32), ("hamming", 61)])
@pytest.mark.parametrize("large", [False, True])
def test_batched_knn2_equals_single_pair_and_oracle(kind, dim, large):
    import torch
    rng = np.random.default_rng(dim + 7 * large)
    sizes = _sizes(rng, 40, 1000, 1400) if large else _sizes(rng, 40, 2, 300)
    tiles = sum((n1 + 63) // 64 for n1, _ in sizes)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (tiles >= 2 * cus) == large                                 # small: the train split is taken; large: it is not
    D1, D2 = _ragged(kind, dim, sizes, seed=dim)
    idx, dist = tensor_api.knn_match_batch_tensors(_t(np.concatenate(D1)), _t(np.concatenate(D2)), [s[0] for s in sizes], [s[1] for s in sizes])
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy()
    o = 0
    for p, (a, b) in enumerate(zip(D1, D2)):
        n1 = a.shape[0]
        si, sd = matcher.knn_match(a, b, kind)
        assert np.array_equal(idx[o:o + n1], si), p
        assert np.array_equal(dist[o:o + n1].view(np.uint32), sd.view(np.uint32)), p
        if not large or p < 8:                                         # the numpy oracle is slow on the large pairs
            ri, rd = mo.knn2(a, b, kind)
            assert np.array_equal(idx[o:o + n1], ri) and np.array_equal(dist[o:o + n1], rd), p
        o += n1


def _f_batch(sizes, seed, dim=64):
    """two-view pairs with descriptors as examples/simple_example_amd.py builds them; image 2 permuted"""
    rng = np.random.default_rng(seed)
    K1, K2, D1, D2 = [], [], [], []
    for i, n in enumerate(sizes):
        if n == 0:
            K1.append(np.zeros((0, 2))); K2.append(np.zeros((0, 2)))
            D1.append(np.zeros((0, dim), np.float32)); D2.append(np.zeros((0, dim), np.float32)); continue
        p1, p2, lab, _ = syn.two_view_fundamental(max(n, 50), 0.5, 0.1, seed=seed * 1000 + i)
        p1, p2, lab = p1[:n], p2[:n], lab[:n]
        d1 = rng.normal(size=(n, dim)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32)
        d2[~lab] = rng.normal(size=((~lab).sum(), dim)).astype(np.float32)
        perm = rng.permutation(n)
        K1.append(p1); K2.append(p2[perm]); D1.append(d1); D2.append(d2[perm])
    return K1, K2, D1, D2


def _run_tensors(K1, K2, D1, D2, **kw):
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    M, match, inl, st, cnt = tensor_api.match_and_verify_batch_tensors(_t(np.concatenate(K1)), _t(np.concatenate(K2)), _t(np.concatenate(D1)),
                                                                       _t(np.concatenate(D2)), c1, c2, **kw)
    o = np.zeros(len(c1) + 1, np.int64); o[1:] = np.cumsum(c1)
    match = match.cpu().numpy(); inl = inl.cpu().numpy()
    return (M.cpu().numpy(), [match[o[p]:o[p + 1]] for p in range(len(c1))], [inl[o[p]:o[p + 1]] for p in range(len(c1))], st.cpu().numpy(), cnt)


def _tentatives(K1, K2, match):
    q = [np.flatnonzero(m >= 0) for m in match]
    return [K1[p][q[p]] for p in range(len(q))], [K2[p][match[p][q[p]]] for p in range(len(q))], q


@pytest.mark.parametrize("mutual", [False, True])
def test_tentatives_equal_match_snn(mutual):
    rng = np.random.default_rng(5 + mutual)
    sizes = _sizes(rng, 24, 10, 900)
    D1, D2 = _ragged("l2", 64, sizes, seed=3)
    K1 = [rng.uniform(0, 500, (a.shape[0], 2)) for a in D1]; K2 = [rng.uniform(0, 500, (b.shape[0], 2)) for b in D2]
    _, match, _, _, cnt = _run_tensors(K1, K2, D1, D2, model="H", ratio=0.9, mutual=mutual, max_iters=2000)
    for p in range(len(sizes)):
        q, t, _ = matcher.match_snn(D1[p], D2[p], 0.9, mutual, "l2")
        assert np.array_equal(np.flatnonzero(match[p] >= 0), q) and np.array_equal(match[p][q], t), p
        assert cnt[p] == len(q), p


def test_fundamental_end_to_end_equals_composed_api(oracle_port):
    rng = np.random.default_rng(11)
    sizes = [int(n) for n in rng.integers(300, 2500, 46)] + [6, 0]
    K1, K2, D1, D2 = _f_batch(sizes, seed=2)
    K = len(sizes); seeds = parallel.pair_seeds(100, 100 + K)
    M, match, inl, st, cnt = _run_tensors(K1, K2, D1, D2, model="F", seeds=seeds)
    A, B, q = _tentatives(K1, K2, match)
    assert list(cnt) == [len(x) for x in q]
    elig = [p for p in range(K) if cnt[p] >= 8]
    assert K - 2 <= len(elig) < K and cnt[K - 1] == 0 and cnt[K - 2] < 8
    Fh, mh = pd.findFundamentalMatrixBatch([A[p] for p in elig], [B[p] for p in elig], seeds=[seeds[p] for p in elig])
    sth = np.array([[s["samples"], s["lo_runs"], s["I"]] for s in pd.last_stats()])
    for e, p in enumerate(elig):
        assert np.array_equal(M[p], Fh[e]), p
        assert np.array_equal(inl[p][q[p]], mh[e]) and not inl[p][match[p] < 0].any(), p
        assert np.array_equal(st[p, [MI_ST_SAMPLES, MI_ST_LO_RUNS, MI_ST_I]], sth[e]), p
    for p in set(range(K)) - set(elig):                                   # short pairs
        assert not M[p].any() and not st[p].any() and not inl[p].any(), p
    for p in sorted(elig, key=lambda p: cnt[p])[:3]:                      # ... and three pairs straight against the CPU oracle
        Fo, mo_, so = oracle_port.find_fundamental(A[p], B[p], 0.5, 0.9999, 100000, seed=int(seeds[p]))
        assert (int(st[p, 0]), int(st[p, 1])) == (so["samples"], so["lo_runs"]), p
        assert np.array_equal(inl[p][q[p]], mo_), p
        assert np.linalg.norm(M[p].ravel() - np.asarray(Fo).ravel()) <= 1e-9 * np.linalg.norm(Fo), p


def test_homography_end_to_end_with_laf():
    rng = np.random.default_rng(4)
    sizes = [900, 300, 1500, 3, 700]
    K4a, K4b, D1, D2 = [], [], [], []
    for i, n in enumerate(sizes):
        p1, p2, lab, _ = syn.homography_pairs(max(n, 20), 0.5, 0.5, seed=40 + i, laf=True)
        p1, p2, lab = p1[:n], p2[:n], lab[:n]
        ang2 = np.degrees(np.arctan2(p2[:, 3], p2[:, 2])); s2 = np.sqrt(np.abs(p2[:, 2] * p2[:, 5] - p2[:, 3] * p2[:, 4]))
        K4a.append(np.c_[p1[:, :2], np.full(n, 5.0), np.zeros(n)].astype(np.float32))
        K4b.append(np.c_[p2[:, :2], s2, ang2].astype(np.float32))
        d1 = rng.normal(size=(n, 64)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32); d2[~lab] = rng.normal(size=((~lab).sum(), 64)).astype(np.float32)
        D1.append(d1); D2.append(d2)
    X1 = [matcher.kpts_to_xyA(k) for k in K4a]; X2 = [matcher.kpts_to_xyA(k) for k in K4b]
    seeds = [3, 5, 7, 9, 11]
    kw = dict(model="H", px_th=2.0, conf=0.999, max_iters=20000, laf_consistensy_coef=3.0, error_type="symm_max", seeds=seeds)
    r6 = _run_tensors(X1, X2, D1, D2, **kw)
    r4 = _run_tensors(K4a, K4b, D1, D2, **kw)
    cols = [MI_ST_SAMPLES, MI_ST_LO_RUNS, MI_ST_I]
    assert np.array_equal(r6[0], r4[0]) and np.array_equal(r6[3][:, cols], r4[3][:, cols]) and np.array_equal(r6[4], r4[4])
    assert all(np.array_equal(u, v) for u, v in zip(r6[1], r4[1])) and all(np.array_equal(u, v) for u, v in zip(r6[2], r4[2]))
    M, match, inl, st, cnt = r6
    A, B, q = _tentatives(X1, X2, match)
    elig = [p for p in range(len(sizes)) if cnt[p] >= 4]
    assert 3 not in elig and len(elig) == 4
    Hh, mh = pd.findHomographyBatch([A[p] for p in elig], [B[p] for p in elig], 2.0, 0.999, 20000, 3.0, "symm_max", True,
                                    seeds=[seeds[p] for p in elig])
    sth = np.array([[s["samples"], s["lo_runs"], s["I"]] for s in pd.last_stats()])
    for e, p in enumerate(elig):
        assert np.array_equal(inl[p][q[p]], mh[e]), p
        assert np.array_equal(st[p, [MI_ST_SAMPLES, MI_ST_LO_RUNS, MI_ST_I]], sth[e]), p
        # inv() runs in numpy on the host path and in torch.linalg on the device path: same to rounding
        assert np.linalg.norm(M[p] - Hh[e]) <= 1e-9 * max(np.linalg.norm(Hh[e]), 1e-300), p
    assert not M[3].any() and not inl[3].any()


def test_results_do_not_depend_on_batch_composition():
    sizes = [800, 6, 1200, 0, 500, 7, 1500]
    K1, K2, D1, D2 = _f_batch(sizes, seed=7)
    seeds = parallel.pair_seeds(0, len(sizes))
    full = _run_tensors(K1, K2, D1, D2, model="F", seeds=seeds)
    keep = [0, 2, 4, 6]
    part = _run_tensors([K1[p] for p in keep], [K2[p] for p in keep], [D1[p] for p in keep], [D2[p] for p in keep], model="F",
                        seeds=[seeds[p] for p in keep])
    cols = [MI_ST_SAMPLES, MI_ST_LO_RUNS, MI_ST_I]
    for j, p in enumerate(keep):
        alone = _run_tensors([K1[p]], [K2[p]], [D1[p]], [D2[p]], model="F", seeds=[seeds[p]])
        for other, k in ((part, j), (alone, 0)):
            assert np.array_equal(full[0][p], other[0][k]), p
            assert np.array_equal(full[1][p], other[1][k]) and np.array_equal(full[2][p], other[2][k]), p
            assert np.array_equal(full[3][p, cols], other[3][k, cols]) and full[4][p] == other[4][k], p
    assert full[3][:, MI_ST_SAMPLES][keep].min() > 0


def test_host_pointer_form_equals_tensor_form():
    sizes = [600, 5, 1100, 0, 900]
    K1, K2, D1, D2 = _f_batch(sizes, seed=9)
    seeds = parallel.pair_seeds(0, len(sizes))
    for mutual in (False, True):
        M, match, inl, st, cnt = _run_tensors(K1, K2, D1, D2, model="F", mutual=mutual, seeds=seeds)
        Mh, mh, ih = matcher.match_and_verify_batch(K1, K2, D1, D2, model="F", mutual=mutual, seeds=seeds)
        sth = pd.last_stats()
        assert np.array_equal(M, Mh)
        for p in range(len(sizes)):
            assert np.array_equal(match[p], mh[p]) and np.array_equal(inl[p], ih[p]), p
            assert [sth[p][k] for k in ("samples", "lo_runs", "I")] == list(st[p, [MI_ST_SAMPLES, MI_ST_LO_RUNS, MI_ST_I]]), p
            assert sth[p]["tentatives"] == cnt[p]


# ---- the two sides of a ragged batch with different layouts -------------------------------------------------------------------------
# a partly filled second query tile against a train set shorter than a tile, an empty side on either side, a full tile against a train
# set longer than two: no two offsets of the two sides agree after pair 0
UNEVEN1, UNEVEN2 = [65, 0, 1, 64], [2, 70, 0, 129]
DET = [c for c in range(16) if c not in (12, 13)]                         # every stats column but the two device clock readings


def _uneven_descs(norm, dim, seed):
    rng = np.random.default_rng(seed)
    n1, n2 = sum(UNEVEN1), sum(UNEVEN2)
    if norm == "l2":
        a = rng.normal(size=(n1, dim)).astype(np.float32); b = rng.normal(size=(n2, dim)).astype(np.float32)
        b[72:72 + 64:2] = a[66:66 + 32] + 0.05 * rng.normal(size=(32, dim)).astype(np.float32)
    else:
        a = rng.integers(0, 256, (n1, dim), dtype=np.uint8); b = rng.integers(0, 256, (n2, dim), dtype=np.uint8)
        b[72:72 + 64:2] = a[66:66 + 32] ^ (rng.random((32, dim)) < 0.03).astype(np.uint8)
    b[80] = b[76]                                                       # a tie inside pair 3's train set
    return a, b


@functools.lru_cache(maxsize=None)
def _uneven_scene():
    """(K1 [130, 2], K2 [201, 2], D1, D2 float32 [., 32]) under UNEVEN1 / UNEVEN2: pair 3 is a two-view scene (64 queries; their 64
    second views, 21 twins 1.5 px from a second view with a near-equal descriptor and 44 unrelated rows as train set, shuffled), the
    other pairs random rows"""
    rng = np.random.default_rng(31)
    n1, n2, dim = sum(UNEVEN1), sum(UNEVEN2), 32
    K1 = rng.uniform(0, 500, (n1, 2)); K2 = rng.uniform(0, 500, (n2, 2))
    D1 = rng.normal(size=(n1, dim)).astype(np.float32); D2 = rng.normal(size=(n2, dim)).astype(np.float32)
    p1, p2, lab, _ = syn.two_view_fundamental(64, 0.8, 0.1, seed=32)
    d2 = D1[66:] + 0.15 * rng.normal(size=(64, dim)).astype(np.float32)
    d2[~lab] = rng.normal(size=((~lab).sum(), dim)).astype(np.float32)
    tw = rng.permutation(64)[:21]
    perm = rng.permutation(129)
    K1[66:] = p1[:, :2]
    K2[72:] = np.r_[p2[:, :2], p2[tw, :2] + [1.5, 0.0], K2[72 + 85:]][perm]
    D2[72:] = np.r_[d2, d2[tw] + 0.002 * rng.normal(size=(21, dim)).astype(np.float32), D2[72 + 85:]][perm]
    return K1, K2, D1, D2


@pytest.mark.parametrize("norm,dim", [("l2", 65), ("hamming", 8), ("l2_u8", 128)])
def test_knn2_batch_whose_first_offsets_are_above_zero(norm, dim):
    """the C ABI takes batch offsets that do not start at 0: the rows in front of offsets[0] are never read, the output rows outside
    [offsets1[0], offsets1[K]) never written"""
    import torch
    code = {"l2": 0, "hamming": 1, "l2_u8": 4}[norm]
    a, b = _uneven_descs(norm, dim, 41)
    want_idx, want_dist = tensor_api.knn_match_batch_tensors(_t(a), _t(b), UNEVEN1, UNEVEN2, norm)
    ja, jb = _uneven_descs(norm, dim, 42)
    A = _t(np.concatenate([ja[:5], a, ja[5:8]])); B = _t(np.concatenate([jb[:12], b, jb[12:14]]))
    o1 = np.r_[0, np.cumsum(UNEVEN1)].astype(np.int64) + 5; o2 = np.r_[0, np.cumsum(UNEVEN2)].astype(np.int64) + 12
    n = A.shape[0]
    idx = torch.full((n, 2), -7, dtype=torch.int32, device=_dev()); dist = torch.full((n, 2), -7.0, dtype=torch.float32, device=_dev())
    lp = C.POINTER(C.c_int64)
    rc = _lib.lib().mi_degensac_match_knn2_batch_dev(code, A.data_ptr(), B.data_ptr(), o1.ctypes.data_as(lp), o2.ctypes.data_as(lp), len(UNEVEN1), dim, 0,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream), idx.data_ptr(), dist.data_ptr())
    assert rc == 0, _lib.lib().mi_degensac_match_last_error()
    torch.cuda.synchronize()
    own = slice(int(o1[0]), int(o1[-1]))
    assert torch.equal(idx[own], want_idx) and torch.equal(dist[own].view(torch.int32), want_dist.view(torch.int32))
    assert (idx[:own.start] == -7).all() and (idx[own.stop:] == -7).all() and (dist[:own.start] == -7).all() and (dist[own.stop:] == -7).all()
    assert (want_idx[:65, 1] >= 0).all() and (want_idx[66:, 0] >= 0).all()


def test_match_verify_batch_whose_first_offsets_are_above_zero():
    """the same through mi_degensac_match_verify_batch_dev with the mutual check: the identity rows are relative, every pointer (both
    descriptor and keypoint arrays, match, inlier) moves by its side's first offset"""
    import torch
    K1, K2, D1, D2 = _uneven_scene()
    K = len(UNEVEN1); seeds = [3, 5, 7, 4000000000]
    want = tensor_api.match_and_verify_batch_tensors(_t(K1), _t(K2), _t(D1), _t(D2), UNEVEN1, UNEVEN2, model="F", mutual=True, max_iters=2000, seeds=seeds)
    rng = np.random.default_rng(43)
    junk = lambda n, like: rng.normal(size=(n,) + like.shape[1:]).astype(like.dtype)
    a = _t(np.concatenate([junk(5, D1), D1, junk(3, D1)])); b = _t(np.concatenate([junk(12, D2), D2, junk(2, D2)]))
    k1 = _t(np.concatenate([junk(5, K1), K1, junk(3, K1)])); k2 = _t(np.concatenate([junk(12, K2), K2, junk(2, K2)]))
    o1 = np.r_[0, np.cumsum(UNEVEN1)].astype(np.int64) + 5; o2 = np.r_[0, np.cumsum(UNEVEN2)].astype(np.int64) + 12
    n = a.shape[0]; dev = _dev()
    M = torch.zeros((K, 9), dtype=torch.float64, device=dev); st = torch.zeros((K, 16), dtype=torch.int32, device=dev)
    match = torch.full((n,), -7, dtype=torch.int32, device=dev); inl = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    d_seeds = _t(np.asarray(seeds, np.uint32).view(np.int32)); cnt = np.zeros(K, np.int32)
    mp = _lib.MatchParams(0, D1.shape[1], 0.9, True); prm = matcher.estimator_params("F", max_iters=2000)
    lp = C.POINTER(C.c_int64)
    rc = _lib.lib().mi_degensac_match_verify_batch_dev(0, C.byref(mp), a.data_ptr(), b.data_ptr(), o1.ctypes.data_as(lp), o2.ctypes.data_as(lp),
                                                       k1.data_ptr(), k2.data_ptr(), 2, K, C.byref(prm), d_seeds.data_ptr(), 0,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream), M.data_ptr(), match.data_ptr(),
                                                       inl.data_ptr(), st.data_ptr(), cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, _lib.lib().mi_degensac_last_error()
    torch.cuda.synchronize()
    own = slice(int(o1[0]), int(o1[-1]))
    assert torch.equal(M.view(K, 3, 3), want[0]) and torch.equal(match[own], want[1]) and torch.equal(inl[own].to(torch.bool), want[2])
    assert torch.equal(st[:, DET], want[3][:, DET]) and np.array_equal(cnt, want[4])
    assert (match[:own.start] == -7).all() and (match[own.stop:] == -7).all() and (inl[:own.start] == 7).all() and (inl[own.stop:] == 7).all()
    assert cnt[3] >= 8 and bool(want[0][3].any()) and int(want[2].sum()) >= 8      # the planted pair is estimated


@pytest.mark.parametrize("mutual", [False, True])
def test_uneven_sides_with_fginn_equal_the_composed_calls(mutual):
    """match_and_verify_batch_tensors with fginn_th on the uneven batch = the FGINN 2-NN, the reverse plain 2-NN, the filter per pair
    and the batch estimator on the tentatives"""
    import torch
    K1, K2, D1, D2 = _uneven_scene()
    K = len(UNEVEN1); seeds = [3, 5, 7, 4000000000]; r = 3.0
    o1 = np.r_[0, np.cumsum(UNEVEN1)]; o2 = np.r_[0, np.cumsum(UNEVEN2)]
    k1, k2, a, b = _t(K1), _t(K2), _t(D1), _t(D2)
    M, match, inl, st, cnt = tensor_api.match_and_verify_batch_tensors(k1, k2, a, b, UNEVEN1, UNEVEN2, model="F", mutual=mutual, max_iters=2000,
                                                                       seeds=seeds, fginn_th=r)
    idx, dist = tensor_api.knn_match_fginn_batch_tensors(a, b, k2, UNEVEN1, UNEVEN2, r)
    back = tensor_api.knn_match_batch_tensors(b, a, UNEVEN2, UNEVEN1)[0] if mutual else None
    P1, P2, elig = [], [], []
    for p in range(K):
        q = slice(int(o1[p]), int(o1[p + 1]))
        bk = back[o2[p]:o2[p + 1]] if mutual and UNEVEN2[p] > 0 else None
        keep = tensor_api.match_filter_tensors(idx[q], dist[q], 0.9, bk).to(torch.bool)
        want = torch.where(keep, idx[q, 0], torch.full_like(idx[q, 0], -1))
        assert torch.equal(match[q], want) and cnt[p] == int(keep.sum()), p
        if cnt[p] >= 8:
            elig.append(p); P1.append(k1[q][keep]); P2.append(k2[o2[p]:o2[p + 1]][want[keep].long()])
        else:
            assert not bool(M[p].any()) and not bool(st[p].any()) and not bool(inl[q].any()), p
    assert 3 in elig                                                    # >= 8 planted matches in the one pair that can hold them
    Fe, me, ste, oe = tensor_api.find_fundamental_batch_tensors(torch.cat(P1), torch.cat(P2), [len(x) for x in P1], max_iters=2000,
                                                                seeds=[seeds[p] for p in elig])
    cols = [MI_ST_SAMPLES, MI_ST_LO_RUNS, MI_ST_I]                      # the other columns follow the launch the pair ran in
    for e, p in enumerate(elig):
        q = slice(int(o1[p]), int(o1[p + 1]))
        assert torch.equal(M[p], Fe[e]) and torch.equal(inl[q][match[q] >= 0], me[oe[e]:oe[e + 1]]) and not bool(inl[q][match[q] < 0].any()), p
        assert torch.equal(st[p, cols], ste[e, cols]), p
    assert int(inl[int(o1[3]):].sum()) >= 8
    plain = tensor_api.match_and_verify_batch_tensors(k1, k2, a, b, UNEVEN1, UNEVEN2, model="F", mutual=mutual, max_iters=2000, seeds=seeds)
    assert cnt[3] > plain[4][3]                                         # the twins veto matches under the plain rule only


# ---- the host-pointer forms with and without their optional outputs -------------------------------------------------------------------
# three views of one scene and a list whose entries are: estimated by both models; short for both (< 4 tentatives); estimated by H only
# (4 .. 7); entry 0 the other way round
FOLD_COUNTS = [41, 39, 40]
FOLD_LIST = [(0, 1), (2, 1), (0, 2), (1, 0)]
FOLD_SEEDS = [5, 4000000000, 7, 11]
FOLD_RATIO = 0.8


@functools.lru_cache(maxsize=None)
def _fold_scene():
    """(xy [120, 2], desc float32 [120, 32]) under FOLD_COUNTS: image 0 is the first view of a two-view scene; image 1 holds the second
    views of its rows 0 .. 29 with near-equal descriptors and 9 unrelated rows, image 2 those of its rows 30 .. 35 and 34 unrelated
    rows, both shuffled.  Under FOLD_RATIO with the mutual check the list's tentative counts are 30, 1, 7, 30 (stated by the tests)."""
    rng = np.random.default_rng(55)
    n, dim = sum(FOLD_COUNTS), 32
    p1, p2, _, _ = syn.two_view_fundamental(41, 0.8, 0.1, seed=52)
    xy = rng.uniform(0, 500, (n, 2)); desc = rng.normal(size=(n, dim)).astype(np.float32)
    near = lambda rows: desc[rows] + 0.1 * rng.normal(size=(len(rows), dim)).astype(np.float32)          # noqa: E731
    xy[:41] = p1[:, :2]
    perm = rng.permutation(39)
    xy[41:80] = np.r_[p2[:30, :2], xy[71:80]][perm]; desc[41:80] = np.r_[near(np.arange(30)), desc[71:80]][perm]
    perm = rng.permutation(40)
    xy[80:] = np.r_[p2[30:36, :2], xy[86:]][perm]; desc[80:] = np.r_[near(np.arange(30, 36)), desc[86:]][perm]
    return xy, desc


def _fold_stores(front=3, back=2):
    """_fold_scene between junk rows (the stores' first offsets are above zero): (desc, xy, a second copy of each in other memory, the
    offsets [4])"""
    xy, desc = _fold_scene(); rng = np.random.default_rng(56)
    frame = lambda x: np.concatenate([rng.normal(size=(front,) + x.shape[1:]), x, rng.normal(size=(back,) + x.shape[1:])]).astype(x.dtype)          # noqa: E731
    A, X = frame(desc), frame(xy)
    return A, X, A.copy(), X.copy(), np.r_[0, np.cumsum(FOLD_COUNTS)].astype(np.int64) + front


def _fold_pairs_host(entry, head, prms, outs, optional, second):
    """one call of a pair-list host-pointer entry on _fold_stores: head = the arguments in front of the match params, prms = the
    estimator params, outs = the required output arrays, optional = the optional ones or None for NULL each; second = pass side 2 as
    distinct arrays of equal content (else the same store is named on both sides)"""
    A, X, A2, X2, o = _fold_stores()
    if not second:
        A2, X2 = A, X
    K = len(FOLD_LIST); M = len(FOLD_COUNTS)
    mp = _lib.MatchParams(0, A.shape[1], FOLD_RATIO, True)
    seeds = np.asarray(FOLD_SEEDS, np.uint32); prs = np.ascontiguousarray(FOLD_LIST, np.int32)
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))          # noqa: E731
    rc = entry(*head, C.byref(mp), A.ctypes.data, A2.ctypes.data, o.ctypes.data_as(lp), M, o.ctypes.data_as(lp), M, X.ctypes.data_as(dp),
               X2.ctypes.data_as(dp), 2, ptr(prs), K, *[C.byref(p) for p in prms], ptr(seeds), 0, *[ptr(a) for a in outs], *[ptr(a) for a in optional])
    assert rc == 0, _lib.lib().mi_degensac_last_error()


@pytest.mark.parametrize("model", ["F", "H"])
def test_pair_list_host_form_with_and_without_its_optional_outputs(model):
    """mi_degensac_match_verify_pairs on stores whose first offsets are above zero, with one entry short for both models and one that
    only H can take: model / match / inlier are the same bytes with stats and counts given, with both NULL, and with the store passed
    as two distinct equal copies (both sides uploaded), and they are the bytes of the _dev form"""
    import torch
    xy, desc = _fold_scene(); K = len(FOLD_LIST)
    tk, td = _t(xy), _t(desc)
    want = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, FOLD_COUNTS, FOLD_COUNTS, FOLD_LIST, model=model, ratio=FOLD_RATIO, mutual=True,
                                                     max_iters=2000, seeds=FOLD_SEEDS)
    torch.cuda.synchronize()
    cnt = want[4]; n = int(want[5][-1])
    assert list(cnt) == [30, 1, 7, 30] and n == 41 + 40 + 41 + 39
    assert list(want[3][:, MI_ST_SAMPLES].cpu().numpy() > 0) == [True, False, model == "H", True]
    prm = matcher.estimator_params(model, max_iters=2000)
    first = None
    for optional, second in ((True, False), (False, False), (True, True)):
        Mh = np.zeros((K, 9)); mh = np.full(n, -7, np.int32); ih = np.full(n, 7, np.uint8)
        opt = [np.zeros((K, 16), np.int32), np.zeros(K, np.int32)] if optional else [None, None]
        _fold_pairs_host(_lib.lib().mi_degensac_match_verify_pairs, (int(model == "H"),), [prm], [Mh, mh, ih], opt, second)
        if first is None:
            first = (Mh, mh, ih)
            Mu = _t(Mh).view(K, 3, 3)
            Mu = tensor_api._h_user_form(Mu) if model == "H" else Mu
            assert torch.equal(Mu.view(torch.int64), want[0].contiguous().view(torch.int64))
            assert np.array_equal(mh, want[1].cpu().numpy()) and np.array_equal(ih.astype(bool), want[2].cpu().numpy()) and ih.max() <= 1
        for a, b in zip(first, (Mh, mh, ih)):
            assert a.tobytes() == b.tobytes(), (optional, second)
        if optional:
            assert np.array_equal(opt[0][:, DET], want[3].cpu().numpy()[:, DET]) and np.array_equal(opt[1], cnt), second
