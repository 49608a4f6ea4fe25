"""GPU: the uint8 L2 norm (norm "l2_u8", MI_DEGENSAC_NORM_L2_U8) through every layer — the int8 matrix-core tile body of the dense
matcher (mi_matcher_u8.h) behind the single-pair and the batched kernel, the guided stage's integer distance, the decisions and the
match-and-verify pipeline.  Every comparison is equality, of indices and of distance bit patterns: for dim <= 256 the squared distance
is an integer below 2^24, so the device must reproduce the float32 oracle (oracle/matcher_np.py) on the cast rows and this library's
own float32 path (tests/test_matcher_u8l2_cpu.py shows that the oracle itself meets that claim on the same inputs).

Run time of this file on one MI355X: a few seconds (the numpy oracle's n1 x n2 matrices are most of it)."""
import ctypes as C

import numpy as np
import pytest

import pydegensac_amd as pd
from oracle import matcher_np as mo
from pydegensac_amd import _lib, matcher, synthetic as syn, tensor_api
from tests import matcher_u8_ref as ur

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _f32(x):
    return np.asarray(x).astype(np.float32)


def _same(got, want, what):
    assert np.array_equal(np.asarray(got[0]), want[0]), (what, np.flatnonzero((np.asarray(got[0]) != want[0]).any(1))[:5])
    assert ur.same_bits(got, want), what


# ---- dense, single pair --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ur.FAMILIES)
def test_single_pair_equals_the_oracle_and_the_float32_path(family):
    """row counts 0 .. 1000 around the 64-query / 32-row / 128-row steps, dims 4 .. 256 around the 32-byte k-steps (1, 2, 4 and 8
    of them: the three kernel instances), and the unpadded dims 5 and 130 through the numpy API"""
    for n1, n2, dim in ur.shapes() + [(65, 129, d) for d in ur.UNPADDED_DIMS]:
        a, b = ur.descs(family, n1, n2, dim, 2)
        got = matcher.knn_match(a, b, "l2_u8")
        assert got[0].shape == (n1, 2) and got[1].dtype == np.float32
        _same(got, mo.knn2(_f32(a), _f32(b), "l2"), (family, n1, n2, dim, "oracle"))
        _same(got, matcher.knn_match(_f32(a), _f32(b), "l2"), (family, n1, n2, dim, "float32 path"))


@pytest.mark.parametrize("n1,n2,dim,split", [(5, 20000, 128, True), (70, 20000, 36, True), (300, 60, 128, False), (33000, 100, 32, False)])
def test_with_and_without_train_splits(n1, n2, dim, split):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    qtiles, ttiles = (n1 + 63) // 64, (n2 + 63) // 64
    assert (min((2 * cus + qtiles - 1) // qtiles, ttiles) > 1) == split            # the launch rule of mi_degensac_match_knn2_dev
    for family in ("uniform", "sift"):
        a, b = ur.descs(family, n1, n2, dim, 3)
        got = tensor_api.knn_match_tensors(_t(a), _t(b), norm="l2_u8")
        got = (got[0].cpu().numpy(), got[1].cpu().numpy())
        _same(got, mo.knn2(_f32(a), _f32(b), "l2"), (family, "oracle"))
        _same(got, matcher.knn_match(_f32(a), _f32(b), "l2"), (family, "float32 path"))


@pytest.mark.parametrize("dim", [64, 128, 36])
def test_tensor_view_at_an_odd_byte_offset(dim):
    import torch
    a, b = ur.descs("uniform", 130, 257, dim, 4)
    buf = torch.zeros(a.size + b.size + 8, dtype=torch.uint8, device=_dev())
    va = buf[1:1 + a.size].view(130, dim); vb = buf[3 + a.size:3 + a.size + b.size].view(257, dim)
    va.copy_(_t(a)); vb.copy_(_t(b))
    assert va.data_ptr() % 4 and vb.is_contiguous()
    idx, dist = tensor_api.knn_match_tensors(va, vb, norm="l2_u8")
    _same((idx.cpu().numpy(), dist.cpu().numpy()), mo.knn2(_f32(a), _f32(b), "l2"), dim)
    # word-aligned but not 16-byte aligned rows: the kernel's word-wise loads
    wa = buf[4:4 + a.size].view(130, dim); wa.copy_(_t(a))
    assert wa.data_ptr() % 16 == 4
    idx, dist = tensor_api.knn_match_tensors(wa, _t(b), norm="l2_u8")
    _same((idx.cpu().numpy(), dist.cpu().numpy()), mo.knn2(_f32(a), _f32(b), "l2"), dim)


def test_norm_keyword_keeps_the_dtype_rule():
    a, b = ur.descs("uniform", 70, 90, 32, 5)
    hi, hd = tensor_api.knn_match_tensors(_t(a), _t(b))
    _same((hi.cpu().numpy(), hd.cpu().numpy()), mo.knn2(a, b, "hamming"), "uint8 without a norm is Hamming")
    hi, hd = tensor_api.knn_match_tensors(_t(a), _t(b), norm="hamming")
    _same((hi.cpu().numpy(), hd.cpu().numpy()), mo.knn2(a, b, "hamming"), "hamming")
    with pytest.raises(ValueError):
        tensor_api.knn_match_tensors(_t(a), _t(b), norm="l2")
    with pytest.raises(ValueError):
        tensor_api.knn_match_tensors(_t(_f32(a)), _t(_f32(b)), norm="l2_u8")


# ---- batched -------------------------------------------------------------------------------------------------------------------
_SIZES = [(0, 50), (40, 0), (70, 1), (1, 3), (130, 2), (3, 0), (64, 64), (65, 200), (300, 280), (129, 127), (40, 2100)]


def _ragged(family, dim, seed, sizes=_SIZES):
    D1, D2 = [], []
    for i, (n1, n2) in enumerate(sizes):
        a, b = ur.descs(family, n1, n2, dim, seed + i)
        D1.append(a); D2.append(b)
    return D1, D2


@pytest.mark.parametrize("family,dim", [("uniform", 128), ("sift", 128), ("uniform", 60), ("extremes", 256), ("sift", 8)])
def test_batched_equals_the_single_pair_call(family, dim):
    D1, D2 = _ragged(family, dim, 10)
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    idx, dist = tensor_api.knn_match_batch_tensors(_t(np.concatenate(D1)), _t(np.concatenate(D2)), c1, c2, norm="l2_u8")
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy()
    o = 0
    for p, (a, b) in enumerate(zip(D1, D2)):
        n1 = len(a)
        si, sd = tensor_api.knn_match_tensors(_t(a), _t(b), norm="l2_u8")
        _same((idx[o:o + n1], dist[o:o + n1]), (si.cpu().numpy(), sd.cpu().numpy()), (p, "single pair"))
        _same((idx[o:o + n1], dist[o:o + n1]), mo.knn2(_f32(a), _f32(b), "l2"), (p, "oracle"))
        o += n1


def test_batched_without_train_splits():
    """enough query tiles to cover the device twice: the batched kernel writes the final answer itself"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K = (2 * cus + 2) // 3 + 1
    sizes = [(130 + (p % 3), 150 + (p % 5)) for p in range(K)]                          # three query tiles per pair
    assert sum((n1 + 63) // 64 for n1, _ in sizes) >= 2 * cus
    D1, D2 = _ragged("uniform", 128, 20, sizes)
    idx, dist = tensor_api.knn_match_batch_tensors(_t(np.concatenate(D1)), _t(np.concatenate(D2)), [s[0] for s in sizes], [s[1] for s in sizes],
                                                   norm="l2_u8")
    fi, fd = tensor_api.knn_match_batch_tensors(_t(_f32(np.concatenate(D1))), _t(_f32(np.concatenate(D2))), [s[0] for s in sizes],
                                                [s[1] for s in sizes])
    _same((idx.cpu().numpy(), dist.cpu().numpy()), (fi.cpu().numpy(), fd.cpu().numpy()), "float32 path")
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy()
    o = 0
    for p in range(0, K, 37):
        o = sum(s[0] for s in sizes[:p]); n1 = sizes[p][0]
        _same((idx[o:o + n1], dist[o:o + n1]), mo.knn2(_f32(D1[p]), _f32(D2[p]), "l2"), p)


def test_sub_batch_with_non_zero_first_offsets():
    """the C entry point on pairs 3 .. 8 of a larger batch: rows outside the sub-batch stay untouched"""
    import torch
    D1, D2 = _ragged("uniform", 68, 30)
    A = _t(np.concatenate(D1)); B = _t(np.concatenate(D2))
    o1 = np.zeros(len(D1) + 1, np.int64); o1[1:] = np.cumsum([len(x) for x in D1])
    o2 = np.zeros(len(D2) + 1, np.int64); o2[1:] = np.cumsum([len(x) for x in D2])
    lo, hi = 3, 9
    s1 = np.ascontiguousarray(o1[lo:hi + 1]); s2 = np.ascontiguousarray(o2[lo:hi + 1])
    assert s1[0] > 0 and s2[0] > 0
    idx = torch.full((A.shape[0], 2), -7, dtype=torch.int32, device=_dev()); dist = torch.full((A.shape[0], 2), -7.0, device=_dev())
    lp = C.POINTER(C.c_int64)
    rc = _lib.lib().mi_degensac_match_knn2_batch_dev(4, A.data_ptr(), B.data_ptr(), s1.ctypes.data_as(lp), s2.ctypes.data_as(lp), hi - lo, 68, 0,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream), idx.data_ptr(), dist.data_ptr())
    assert rc == 0, _lib.lib().mi_degensac_match_last_error()
    torch.cuda.synchronize()
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy()
    assert (idx[:o1[lo]] == -7).all() and (idx[o1[hi]:] == -7).all() and (dist[:o1[lo]] == -7).all() and (dist[o1[hi]:] == -7).all()
    for p in range(lo, hi):
        _same((idx[o1[p]:o1[p + 1]], dist[o1[p]:o1[p + 1]]), mo.knn2(_f32(D1[p]), _f32(D2[p]), "l2"), p)      # (3, 0): -1 / inf


# ---- decisions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("family,n1,n2,dim", [("uniform", 300, 280, 128), ("sift", 129, 200, 128), ("uniform", 64, 1, 32), ("uniform", 50, 0, 8)])
def test_match_snn_equals_the_oracle(family, n1, n2, dim, mutual):
    a, b = ur.descs(family, n1, n2, dim, 6)
    e = np.zeros(0, np.int64)                                          # (no train rows: nothing passes, and the oracle's mutual check needs one)
    want = mo.match_snn(_f32(a), _f32(b), 0.9, mutual, "l2") if n2 else (e, e, np.zeros(0, np.float32))
    got = matcher.match_snn(a, b, 0.9, mutual, norm="l2_u8")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    tq, tt, td = tensor_api.match_snn_tensors(_t(a), _t(b), 0.9, mutual, norm="l2_u8")
    assert np.array_equal(tq.cpu().numpy(), want[0]) and np.array_equal(tt.cpu().numpy(), want[1])
    assert np.array_equal(td.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
    if n1 == 300:
        assert len(want[0]) > 50                                       # the near copies are found


# ---- pipeline ------------------------------------------------------------------------------------------------------------------
def _scene_batch(model, sizes, seed, dim=128):
    """geometric pairs with uint8 descriptors: true matches are byte-noisy copies, image 2 permuted"""
    rng = np.random.default_rng(seed)
    K1, K2, D1, D2, M = [], [], [], [], []
    for i, n in enumerate(sizes):
        if model == "F":
            p1, p2, lab, Mt = syn.two_view_fundamental(max(n, 50), 0.5, 0.1, seed=seed * 1000 + i)
        else:
            p1, p2, lab, Mt = syn.homography_pairs(max(n, 50), 0.5, 0.3, seed=seed * 1000 + i)
        p1, p2, lab = p1[:n], p2[:n], lab[:n]
        d1 = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        d2 = np.clip(d1.astype(np.int64) + rng.integers(-12, 13, d1.shape), 0, 255).astype(np.uint8)
        d2[~lab] = rng.integers(0, 256, (int((~lab).sum()), dim), dtype=np.uint8)
        perm = rng.permutation(n)
        K1.append(p1); K2.append(p2[perm]); D1.append(d1); D2.append(d2[perm]); M.append(Mt)
    return K1, K2, D1, D2, np.stack(M)


def _eq_lists(x, y):
    return len(x) == len(y) and all(np.array_equal(a, b) for a, b in zip(x, y))


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("model", ["F", "H"])
def test_match_and_verify_equals_the_float32_call(model, guided):
    sizes = [300, 3, 150, 0, 420, 6]                                   # pairs 1, 3 and 5 stay below the 8 / 4 tentatives
    K1, K2, D1, D2, _ = _scene_batch(model, sizes, 7)
    F1 = [_f32(x) for x in D1]; F2 = [_f32(x) for x in D2]
    kw = dict(model=model, ratio=0.85, mutual=True, max_iters=2000, guided=guided)
    got = matcher.match_and_verify_batch(K1, K2, D1, D2, norm="l2_u8", **kw); st_u = pd.last_stats()
    want = matcher.match_and_verify_batch(K1, K2, F1, F2, **kw); st_f = pd.last_stats()
    assert np.array_equal(got[0], want[0])
    for k in range(1, len(want)):
        assert _eq_lists(got[k], want[k]), k
    timers = ("ticks_best", "ticks_total")                             # device clock readings: the only entries that differ between two runs
    assert [{k: v for k, v in d.items() if k not in timers} for d in st_u] == [{k: v for k, v in d.items() if k not in timers} for d in st_f]
    assert [s["tentatives"] for s in st_u][1] < 4 and st_u[0]["tentatives"] >= 8 and not got[0][1].any() and got[0][0].any()
    assert sum(int(x.sum()) for x in got[2]) > 100                     # inliers were found at all
    # the tensor form
    c = sizes
    args = (_t(np.concatenate(K1)), _t(np.concatenate(K2)))
    tu = tensor_api.match_and_verify_batch_tensors(*args, _t(np.concatenate(D1)), _t(np.concatenate(D2)), c, c, norm="l2_u8", **kw)
    tf = tensor_api.match_and_verify_batch_tensors(*args, _t(np.concatenate(F1)), _t(np.concatenate(F2)), c, c, **kw)
    assert len(tu) == len(tf) == (6 if guided else 5)
    for k, (x, y) in enumerate(zip(tu, tf)):
        x = x if isinstance(x, np.ndarray) else x.cpu().numpy(); y = y if isinstance(y, np.ndarray) else y.cpu().numpy()
        if k == 3:                                                     # stats [K, 16]: columns 12 and 13 are the timers
            x = np.delete(x, [12, 13], axis=1); y = np.delete(y, [12, 13], axis=1)
        assert np.array_equal(x, y), k
    assert np.array_equal(tu[1].cpu().numpy(), np.concatenate(got[1])) and np.array_equal(tu[2].cpu().numpy(), np.concatenate(got[2]))
    if model == "F":                                                   # (H is inverted by numpy in one form and by torch in the other)
        assert np.array_equal(tu[0].cpu().numpy(), got[0])


def test_match_and_verify_pads_unpadded_rows():
    K1, K2, D1, D2, _ = _scene_batch("F", [200, 90], 8, dim=61)
    got = matcher.match_and_verify_batch(K1, K2, D1, D2, norm="l2_u8", max_iters=1000)
    want = matcher.match_and_verify_batch(K1, K2, [_f32(x) for x in D1], [_f32(x) for x in D2], max_iters=1000)
    assert np.array_equal(got[0], want[0]) and _eq_lists(got[1], want[1]) and _eq_lists(got[2], want[2])


# ---- guided alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model,px_th", [("F", 0.5), ("H", 1.0), ("F", 1e100), ("H", 1e100)])
def test_guided_equals_the_float32_call(model, px_th, mutual):
    """px_th 1e100 opens the gate: every query's candidate list (up to 420 rows) crosses the 64-row flush several times"""
    sizes = [300, 1, 150, 0, 420, 70]
    K1, K2, D1, D2, M = _scene_batch(model, sizes, 9, dim=132)
    D2[0][5] = D2[0][3]; D2[0][7] = D2[0][3]; K2[0][5] = K2[0][3]; K2[0][7] = K2[0][3]             # ties among the candidates
    M[2] = 0                                                           # a failed pair: no matches
    F1 = [_f32(x) for x in D1]; F2 = [_f32(x) for x in D2]
    kw = dict(model=model, ratio=0.9, mutual=mutual, px_th=px_th)
    got = matcher.guided_match_batch(K1, K2, D1, D2, M, norm="l2_u8", **kw)
    want = matcher.guided_match_batch(K1, K2, F1, F2, M, **kw)
    for p, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(g[2].view(np.uint32), w[2].view(np.uint32)), p
    assert len(got[2][0]) == 0 and len(got[0][0]) > 20
    c = sizes
    args = (_t(np.concatenate(K1)), _t(np.concatenate(K2)))
    tu = tensor_api.guided_match_batch_tensors(*args, _t(np.concatenate(D1)), _t(np.concatenate(D2)), c, c, _t(M), norm="l2_u8", **kw)
    tf = tensor_api.guided_match_batch_tensors(*args, _t(np.concatenate(F1)), _t(np.concatenate(F2)), c, c, _t(M), **kw)
    for k, (x, y) in enumerate(zip(tu, tf)):
        x = x.cpu().numpy(); y = y.cpu().numpy()
        assert np.array_equal(x, y) if x.dtype != np.float32 else np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
    if px_th > 1e6:                                                    # gate wide open: the guided 2-NN is the dense 2-NN
        di, dd = tensor_api.knn_match_batch_tensors(_t(np.concatenate(D1)), _t(np.concatenate(D2)), c, c, norm="l2_u8")
        gi = tu[1].cpu().numpy(); o = np.cumsum([0] + sizes)
        keep = np.r_[0:o[2], o[3]:o[6]]                                 # all pairs but the zero model's
        assert np.array_equal(gi[keep], di.cpu().numpy()[keep])
        assert np.array_equal(tu[2].cpu().numpy()[keep].view(np.uint32), dd.cpu().numpy()[keep].view(np.uint32))
