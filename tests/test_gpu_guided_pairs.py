"""GPU: guided matching over a pair list (include/mi_degensac.h mi_degensac_match_guided_*_pairs*; tensor_api.guided_match_pairs_tensors,
matcher.guided_match_pairs): descriptors and keypoints stored once per image, a list of (i, j) image indices, one model per list entry.
Equality only.  Every result is compared bit for bit with BOTH
  (a) tests/guided_ref.oracle per list entry on the entry's store slices under the entry's model (the CPU restatement: the oracle's own
      residuals, `<=`, the numpy matcher's distances), and
  (b) guided_match_batch_tensors on the expansion of tests/pairs_ref.py (entry p's rows copied out of the stores) with the same models.
The shapes are the smallest at which the row tables can go wrong: query images on both sides of the 16-query tile, train images around
the 64-row step and the 1024-row LDS chunk, lists with empty query images at the start, at the end and in runs, empty train images, self
pairs, repeats with other models, both orders, shared train images under the mutual check, unused images, two stores."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, tensor_api
from tests import guided_ref as gr, pairs_ref as pr

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _name(model, et):
    return gr.ERROR_NAMES[model][et]


def _px(model, et):
    return 12.0 if (model == "H" and et in (2, 4)) else 6.0


def _store(sizes, dim, norm, seed):
    """images that see one bank of scene points: image i holds sizes[i] of them (keypoints in [0, 200]^2 with a little noise, descriptors
    as noisy copies), so entries have true matches under a model near the identity; rows 3 and 5 of an image are exact duplicates (ties)"""
    rng = np.random.default_rng([seed, dim, len(sizes)])
    B = max(max(sizes), 8) + 16
    bank_k = rng.uniform(0, 200, (B, 2))
    bank_d = rng.normal(size=(B, dim)).astype(np.float32) if norm == "l2" else rng.integers(0, 256, (B, dim), dtype=np.uint8)
    ks, ds = [], []
    for n in sizes:
        sel = rng.permutation(B)[:n]
        k = bank_k[sel] + 0.3 * rng.normal(size=(n, 2))
        if norm == "l2":
            d = bank_d[sel] + 0.1 * rng.normal(size=(n, dim)).astype(np.float32)
        else:
            d = bank_d[sel] ^ (rng.random((n, dim)) < 0.05).astype(np.uint8)
        if n > 8:
            d[5] = d[3]; k[5] = k[3]
        ks.append(k); ds.append(d)
    return np.concatenate(ks), np.concatenate(ds), list(sizes)


def _models(model, K, seed, zero=(), nan=()):
    """one driver-form model per list entry, each another one: H = a translation by small whole numbers (H_c = inv(H)^T), F = the model whose
    band is the query's image row shifted by s (x2^T F x1 = y1 - y2 + s); entries in `zero` get nine zeros, those in `nan` one NaN"""
    rng = np.random.default_rng([seed, K])
    M = np.zeros((K, 3, 3))
    for p in range(K):
        a, b = rng.integers(-3, 4, 2)
        M[p] = [[1, 0, 0], [0, 1, 0], [-a, -b, 1]] if model == "H" else [[0, 0, 0], [0, 0, -1], [0, 1, a]]
    for p in zero:
        M[p] = 0.0
    for p in nan:
        M[p, 1, 1] = np.nan
    return M


def _split(po, *arrs):
    return [tuple(a[po[p]:po[p + 1]] for a in arrs) for p in range(len(po) - 1)]


def _both(P, s1, s2, pairs, M, model, et, px, norm, ratio=0.9, mutual=False, kps_for_oracle=None, **kw):
    """the pair-list call on the stores s1 / s2 = (kps, desc, counts) (s2 is s1: one store, the same tensors on both sides) against (b) the
    batched call on the expansion and (a) the restatement per entry; M in the driver's form.  Returns per entry (match, idx, dist)."""
    import torch
    k1, d1, c1 = s1; k2, d2, c2 = s2
    tk1, td1 = _t(k1), _t(d1)
    tk2, td2 = (tk1, td1) if s2 is s1 else (_t(k2), _t(d2))
    tM = _t(M)
    name = _name(model, et)
    got = tensor_api.guided_match_pairs_tensors(tk1, tk2, td1, td2, c1, c2, pairs, tM, model=model, ratio=ratio, mutual=mutual, px_th=px,
                                                error_type=name, norm=norm, driver_form=True, **kw)
    (ek1, ed1), (ek2, ed2), e1, e2, want_po = pr.expand((k1, d1), c1, (k2, d2), c2, pairs)
    want = tensor_api.guided_match_batch_tensors(_t(ek1), _t(ek2), _t(ed1), _t(ed2), e1, e2, tM, model=model, ratio=ratio, mutual=mutual, px_th=px,
                                                 error_type=name, norm=norm, driver_form=True)
    torch.cuda.synchronize()
    match, idx, dist, po = got
    assert isinstance(po, np.ndarray) and po.dtype == np.int64 and np.array_equal(po, want_po)
    assert match.shape == want[0].shape and idx.shape == want[1].shape and dist.shape == want[2].shape
    assert torch.equal(match, want[0]) and torch.equal(idx, want[1]) and torch.equal(dist.view(torch.int32), want[2].view(torch.int32))
    res = _split(po, match.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy())
    x1, x2 = kps_for_oracle or (k1, k2)
    o1, o2 = pr.offsets(c1), pr.offsets(c2)
    onorm = "hamming" if norm == "hamming" else "l2"
    for p, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        q, t = d1[o1[i]:o1[i + 1]], d2[o2[j]:o2[j + 1]]
        if norm == "l2_u8":                                              # uint8 rows under L2: the float32 path on the same values is exact
            q, t = q.astype(np.float32), t.astype(np.float32)
        oi, od, om = gr.oracle(P, model, et, px, M[p], x1[o1[i]:o1[i + 1], :2], x2[o2[j]:o2[j + 1], :2], q, t, onorm, ratio, mutual)
        gm, gi, gd = res[p]
        assert gi.shape == (c1[i], 2), p
        assert np.array_equal(gi, oi), (p, i, j, np.flatnonzero((gi != oi).any(1))[:5])
        assert np.array_equal(_bits(gd), _bits(od)), (p, i, j)
        assert np.array_equal(gm, om), (p, i, j)
        assert ((gi >= -1) & (gi < max(c2[j], 1))).all(), p              # indices are local to image j
    return res


def _found(res):
    return sum(int((g[1][:, 0] >= 0).sum()) for g in res), sum(int((g[0] >= 0).sum()) for g in res)


# ---- query images around the 16-query tile x train images around the 64-row step and the 1024-row chunk; two stores ----
Q_SIZES = [0, 1, 15, 16, 17, 33, 65]
T_SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]
EDGE_PAIRS = [(i, j) for i in range(len(Q_SIZES)) for j in range(len(T_SIZES))]


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model,et,norm,dim", [("F", 0, "l2", 5), ("H", 0, "hamming", 8), ("H", 2, "l2_u8", 4)])
def test_query_and_train_edges_over_two_stores(oracle_port, model, et, norm, dim, mutual):
    s1 = _store(Q_SIZES, dim, norm, 1); s2 = _store(T_SIZES, dim, norm, 2)
    K = len(EDGE_PAIRS)
    M = _models(model, K, 3, zero=(5, 40), nan=(17,))
    res = _both(oracle_port, s1, s2, EDGE_PAIRS, M, model, et, _px(model, et), norm, mutual=mutual)
    cand, kept = _found(res)
    assert cand > 300 and kept > 30, (cand, kept)
    assert all((res[p][1] == -1).all() for p in (5, 17, 40))             # zero and NaN models pass nothing


# ---- an all-pass gate: every 64-row step fills the list exactly, the rest is carried to the end; and a gate that carries 63 ----
def test_all_pass_gate_fills_the_lists_exactly(oracle_port):
    import torch
    sizes = [17, 63, 64, 127, 128, 191, 1087, 0]
    pairs = [(0, j) for j in range(8)] + [(j, 0) for j in range(8)] + [(3, 3), (6, 5)]
    k, d, c = s = _store(sizes, 3, "l2", 4)
    rng = np.random.default_rng(5)
    M = rng.normal(size=(len(pairs), 3, 3))                              # any model: every residual is below 1e200
    for model, et in (("F", 0), ("H", 1)):
        for mutual in (False, True):
            res = _both(oracle_port, s, s, pairs, M, model, et, 1e100, "l2", mutual=mutual)
            # all-pass: the guided 2-NN is the unguided 2-NN of the pair list
            ui, ud, po = tensor_api.knn_match_pairs_tensors(_t(d), _t(d), c, c, pairs)
            torch.cuda.synchronize()
            for g, (wi, wd) in zip(res, _split(po, ui.cpu().numpy(), ud.cpu().numpy())):
                assert np.array_equal(g[1], wi) and np.array_equal(_bits(g[2]), _bits(wd))


def test_a_list_of_63_pending_rows_takes_a_full_step(oracle_port):
    """train rows 0 .. 62 and 64 .. 191 lie on query 0's image row, row 63 does not: 63 pending + a 64-row step = 127 in the list, a flush
    that leaves 63, another step; the entry is the second user of its train image and sits behind an empty query image"""
    sizes = [0, 3, 192, 20]
    rng = np.random.default_rng(6)
    k = rng.uniform(1000, 2000, (sum(sizes), 2)); d = rng.normal(size=(sum(sizes), 7)).astype(np.float32)
    o = pr.offsets(sizes)
    k[o[1]] = (50.0, 70.0)
    k[o[2]:o[3], 1] = 70.0; k[o[2] + 63, 1] = 500.0
    M = np.stack([np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])] * 4)
    pairs = [(0, 2), (3, 2), (1, 2), (2, 1)]
    gate = gr.gate_matrix(oracle_port, "F", 0, 1.0, M[2], k[o[1]:o[2]], k[o[2]:o[3]])
    assert list(np.flatnonzero(gate[0])) == [r for r in range(192) if r != 63] and not gate[1:].any()
    for mutual in (False, True):
        _both(oracle_port, (k, d, sizes), (k, d, sizes), pairs, M, "F", 0, 1.0, "l2", mutual=mutual)


# ---- the lists: empty query images at the start, at the end and in runs; the model belongs to the entry ----
# image 0, 2, 5 are empty, image 7 takes part in no pair
L_SIZES = [0, 40, 0, 17, 70, 0, 33, 9]
L_PAIRS = [(0, 1), (2, 4), (0, 0),                                       # starts with a run of empty query images (and an empty-empty pair)
           (1, 4), (3, 4), (6, 4), (4, 4),                               # one train image, four entries: each needs its own back block
           (5, 3), (2, 2), (0, 6),                                       # a run of empty query images in the middle
           (4, 1), (1, 4),                                               # the other order; the repeat of entry 3 under ANOTHER model
           (1, 0), (6, 2),                                               # empty train images
           (3, 3), (1, 1), (6, 3), (3, 6),                               # self pairs, both orders
           (4, 6), (5, 5), (2, 1)]                                       # ends with empty query images
L_ZERO, L_NAN = (4, 16), (14,)


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model,et", gr.KINDS)
def test_lists_with_empty_images_repeats_and_shared_train_images(oracle_port, model, et, mutual):
    s = _store(L_SIZES, 33, "l2", 7)
    K = len(L_PAIRS)
    M = _models(model, K, 8, zero=L_ZERO, nan=L_NAN)
    M[11] = M[3]; M[11][2, 0 if model == "H" else 2] += 5.0              # entry 11 = entry 3's images under a model shifted by 5
    res = _both(oracle_port, s, s, L_PAIRS, M, model, et, _px(model, et), "l2", mutual=mutual)
    cand, kept = _found(res)
    assert cand > 100 and kept > 20, (cand, kept)
    assert not np.array_equal(res[3][1], res[11][1]) and (res[3][1][:, 0] >= 0).any() and (res[11][1][:, 0] >= 0).any()
    for p in L_ZERO + L_NAN + (12, 13):                                  # zero model, NaN model, empty train image
        assert (res[p][0] == -1).all() and (res[p][1] == -1).all() and np.isposinf(res[p][2]).all(), p
    for p in (0, 1, 2, 7, 8, 9, 19, 20):
        assert res[p][1].shape == (0, 2)


def test_a_repeat_under_the_same_model_repeats_the_result_and_order_does_not_matter(oracle_port):
    s = _store(L_SIZES, 16, "l2", 9)
    M = _models("H", len(L_PAIRS), 10)
    M[11] = M[3]
    res = _both(oracle_port, s, s, L_PAIRS, M, "H", 0, 6.0, "l2", mutual=True)
    assert all(np.array_equal(a, b) for a, b in zip(res[3], res[11]))
    perm = np.random.default_rng(11).permutation(len(L_PAIRS))
    res2 = _both(oracle_port, s, s, [L_PAIRS[p] for p in perm], M[perm], "H", 0, 6.0, "l2", mutual=True)
    for n, p in enumerate(perm):
        assert all(np.array_equal(a, b) for a, b in zip(res2[n], res[p])), (n, p)
    one = _both(oracle_port, s, s, [L_PAIRS[4]], M[4:5], "H", 0, 6.0, "l2", mutual=True)                     # K = 1
    assert all(np.array_equal(a, b) for a, b in zip(one[0], res[4]))


# ---- norms and row widths: 1, 64 and 65 words; uint8 L2 at 4 / 128 / 256 bytes ----
WIDTHS = [("l2", 1), ("l2", 64), ("l2", 65), ("hamming", 4), ("hamming", 256), ("hamming", 260), ("l2_u8", 4), ("l2_u8", 128), ("l2_u8", 256)]


@pytest.mark.parametrize("norm,dim", WIDTHS)
def test_norms_and_widths(oracle_port, norm, dim):
    s = _store(L_SIZES, dim, norm, 12)
    M = _models("H", len(L_PAIRS), 13, zero=L_ZERO)
    res = _both(oracle_port, s, s, L_PAIRS, M, "H", 0, 6.0, norm, mutual=True)
    assert _found(res)[0] > 100


# ---- keypoint layouts, and H in the user's and in the driver's form ----
@pytest.mark.parametrize("form", ["xy", "laf6", "kpts4"])
@pytest.mark.parametrize("model", ["F", "H"])
def test_keypoint_layouts(oracle_port, model, form):
    k, d, c = _store(L_SIZES, 20, "l2", 14)
    rng = np.random.default_rng(15)
    N = len(k)
    if form == "laf6":
        kps = np.c_[k, rng.normal(size=(N, 4))]; xy = kps
    elif form == "kpts4":
        kps = np.c_[k, rng.uniform(2, 9, N), rng.uniform(0, 360, N)].astype(np.float32); xy = kps[:, :2].astype(np.float64)
    else:
        kps = xy = k
    M = _models(model, len(L_PAIRS), 16, zero=L_ZERO)
    s = (kps, d, c)
    res = _both(oracle_port, s, s, L_PAIRS, M, model, 0, 6.0, "l2", mutual=True, kps_for_oracle=(xy, xy))
    assert _found(res)[0] > 100


def test_user_form_h_is_converted_on_the_device(oracle_port):
    """translations by whole numbers invert exactly in any algorithm, so the user-form call must equal the driver-form call on inv(H)^T bit
    for bit; zero models stay zero"""
    import torch
    k, d, c = s = _store(L_SIZES, 20, "l2", 17)
    K = len(L_PAIRS)
    Md = _models("H", K, 18, zero=L_ZERO)
    Hu = np.zeros_like(Md)
    for p in range(K):
        if Md[p].any():
            Hu[p] = np.linalg.inv(Md[p].T)
            assert np.array_equal(np.linalg.inv(Hu[p]).T, Md[p])
    res = _both(oracle_port, s, s, L_PAIRS, Md, "H", 1, 6.0, "l2", mutual=True)
    tk, td = _t(k), _t(d)
    match, idx, dist, po = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, c, c, L_PAIRS, _t(Hu), model="H", mutual=True, px_th=6.0,
                                                                 error_type="symm_sq_max")
    torch.cuda.synchronize()
    for g, w in zip(_split(po, match.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), res):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(_bits(g[2]), _bits(w[2]))


# ---- the numpy entry point, one store and two ----
def _tuples(res):
    out = []
    for m, i, d in res:
        q = np.flatnonzero(m >= 0)
        out.append((q, m[q], d[q, 0]))
    return out


@pytest.mark.parametrize("norm,dim", [("l2", 20), ("hamming", 6), ("l2_u8", 6)])
def test_numpy_entry_point(oracle_port, norm, dim):
    """uint8 rows of 6 bytes: the numpy entry point pads them to whole words, the tensor call takes padded rows"""
    k, d, c = _store(L_SIZES, dim, norm, 19)
    o = pr.offsets(c)
    kl = [k[o[i]:o[i + 1]] for i in range(len(c))]; dl = [d[o[i]:o[i + 1]] for i in range(len(c))]
    dpad = d if norm == "l2" else np.c_[d, np.zeros((len(d), 2), np.uint8)]
    M = _models("F", len(L_PAIRS), 20, zero=L_ZERO)
    kept = 0
    for mutual in (False, True):
        res = _both(oracle_port, (k, dpad, c), (k, dpad, c), L_PAIRS, M, "F", 1, 4.0, norm, mutual=mutual)
        got = matcher.guided_match_pairs(kl, dl, L_PAIRS, M, model="F", mutual=mutual, px_th=4.0, error_type="symm_epipolar", norm=norm)
        twice = matcher.guided_match_pairs(kl, dl, L_PAIRS, M, model="F", mutual=mutual, px_th=4.0, error_type="symm_epipolar", norm=norm,
                                           kps2_list=kl, desc2_list=dl)                                  # the same store given again
        assert len(got) == len(L_PAIRS)
        for g, g2, w in zip(got, twice, _tuples(res)):
            assert g[0].dtype == np.int64 and g[1].dtype == np.int64
            assert all(np.array_equal(a, b) for a, b in zip(g, w)) and np.array_equal(_bits(g[2]), _bits(w[2]))
            assert all(np.array_equal(a, b) for a, b in zip(g2, w))
            kept += len(g[0])
    assert kept > 20
    # two stores of different size: images 1, 3, 4 as the database
    k2 = np.concatenate([kl[1], kl[3], kl[4]]); d2 = np.concatenate([dl[1], dl[3], dl[4]]); c2 = [c[1], c[3], c[4]]
    d2pad = d2 if norm == "l2" else np.c_[d2, np.zeros((len(d2), 2), np.uint8)]
    pairs2 = [(0, 2), (4, 0), (1, 2), (6, 1), (3, 1), (7, 2), (2, 0)]
    M2 = _models("F", len(pairs2), 21)
    res = _both(oracle_port, (k, dpad, c), (k2, d2pad, c2), pairs2, M2, "F", 0, 4.0, norm, mutual=True)
    got = matcher.guided_match_pairs(kl, dl, pairs2, M2, model="F", mutual=True, px_th=4.0, norm=norm, kps2_list=[kl[1], kl[3], kl[4]],
                                     desc2_list=[dl[1], dl[3], dl[4]])
    for g, w in zip(got, _tuples(res)):
        assert all(np.array_equal(a, b) for a, b in zip(g, w))
    assert sum(len(g[0]) for g in got) > 10


def test_numpy_entry_point_takes_user_form_h_and_kpts4(oracle_port):
    k, d, c = _store(L_SIZES, 20, "l2", 22)
    rng = np.random.default_rng(23)
    k4 = np.c_[k, rng.uniform(2, 9, len(k)), rng.uniform(0, 360, len(k))].astype(np.float32)
    o = pr.offsets(c)
    kl = [k4[o[i]:o[i + 1]] for i in range(len(c))]; dl = [d[o[i]:o[i + 1]] for i in range(len(c))]
    Md = _models("H", len(L_PAIRS), 24, zero=L_ZERO)
    Hu = np.stack([np.linalg.inv(m.T) if m.any() else m for m in Md])
    xy = k4[:, :2].astype(np.float64)
    res = _both(oracle_port, (k4, d, c), (k4, d, c), L_PAIRS, Md, "H", 3, 6.0, "l2", mutual=True, kps_for_oracle=(xy, xy))
    got = matcher.guided_match_pairs(kl, dl, L_PAIRS, Hu, model="H", mutual=True, px_th=6.0, error_type="symm_sq_sum")
    drv = matcher.guided_match_pairs(kl, dl, L_PAIRS, Md, model="H", mutual=True, px_th=6.0, error_type="symm_sq_sum", driver_form=True)
    for g, g2, w in zip(got, drv, _tuples(res)):
        assert all(np.array_equal(a, b) for a, b in zip(g, w)) and all(np.array_equal(a, b) for a, b in zip(g2, w))


# ---- a second stream ----
def test_second_stream_without_host_synchronisation(oracle_port):
    import torch
    k, d, c = s = _store(L_SIZES, 33, "l2", 25)
    M = _models("F", len(L_PAIRS), 26, zero=L_ZERO)
    want = _both(oracle_port, s, s, L_PAIRS, M, "F", 0, 6.0, "l2", mutual=True)
    tk, td, tM = _t(k), _t(d), _t(M)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(st):
        match, idx, dist, po = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, c, c, L_PAIRS, tM, model="F", mutual=True, px_th=6.0,
                                                                     driver_form=True)
    st.synchronize()
    for g, w in zip(_split(po, match.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(_bits(g[2]), _bits(w[2]))


# ---- the C ABI: stores entered at a non-zero first offset, all three entry points ----
def _p(x, t):
    return x.ctypes.data_as(C.POINTER(t))


@pytest.mark.parametrize("model,et,norm,dim,kd", [("F", 0, "l2", 37, 2), ("H", 1, "hamming", 32, 6), ("H", 0, "l2_u8", 8, 2)])
def test_stores_whose_first_offset_is_above_zero(oracle_port, model, et, norm, dim, kd):
    import torch
    code = {"l2": 0, "hamming": 1, "l2_u8": 4}[norm]
    k, d, c = s = _store(L_SIZES, dim, norm, 27)
    K = len(L_PAIRS)
    M = _models(model, K, 28, zero=L_ZERO)
    want = _both(oracle_port, s, s, L_PAIRS, M, model, et, 6.0, norm, mutual=True)
    wm = np.concatenate([w[0] for w in want]); wi = np.concatenate([w[1] for w in want]); wd = np.concatenate([w[2] for w in want])
    rng = np.random.default_rng(29)
    if kd == 6:
        k = np.c_[k, rng.normal(size=(len(k), 4))]
    jk1 = rng.uniform(0, 200, (5, kd)); jk2 = rng.uniform(0, 200, (12, kd))
    jd1 = _store([5], dim, norm, 30)[1]; jd2 = _store([12], dim, norm, 31)[1]
    A = np.ascontiguousarray(np.concatenate([jd1, d])); B = np.ascontiguousarray(np.concatenate([jd2, d, jd1]))
    X1 = np.ascontiguousarray(np.concatenate([jk1, k])); X2 = np.ascontiguousarray(np.concatenate([jk2, k, jk1]))
    o1 = pr.offsets(c) + 5; o2 = pr.offsets(c) + 12
    prs = np.ascontiguousarray(L_PAIRS, np.int32); Mh = np.ascontiguousarray(M.reshape(K, 9))
    n = len(wm); m = len(c)
    mp = _lib.MatchParams(code, dim, 0.9, True); gp = _lib.GuideParams(model == "H", et, 6.0)
    L = _lib.lib()
    # host pointers
    idx = np.full((n, 2), -7, np.int32); dist = np.full((n, 2), -7, np.float32); match = np.full(n, -7, np.int32); cnt = np.zeros(K, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_pairs(C.byref(mp), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), _p(o1, C.c_int64), m,
                     _p(o2, C.c_int64), m, _p(prs, C.c_int32), K, _lib.dptr(X1), _lib.dptr(X2), kd, _lib.dptr(Mh), C.byref(gp), 0,
                     _p(idx, C.c_int32), _p(dist, C.c_float), _p(match, C.c_int32), _p(cnt, C.c_int32)))
    assert np.array_equal(idx, wi) and np.array_equal(_bits(dist), _bits(wd)) and np.array_equal(match, wm)
    assert list(cnt) == [int((w[0] >= 0).sum()) for w in want]
    # host pointers without the one optional output, counts
    i0 = np.full((n, 2), -7, np.int32); d0 = np.full((n, 2), -7, np.float32); m0 = np.full(n, -7, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_pairs(C.byref(mp), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), _p(o1, C.c_int64), m,
                     _p(o2, C.c_int64), m, _p(prs, C.c_int32), K, _lib.dptr(X1), _lib.dptr(X2), kd, _lib.dptr(Mh), C.byref(gp), 0,
                     _p(i0, C.c_int32), _p(d0, C.c_float), _p(m0, C.c_int32), None))
    assert np.array_equal(i0, idx) and np.array_equal(_bits(d0), _bits(dist)) and np.array_equal(m0, match)
    # device pointers: the guided 2-NN + decision (device counts and host counts), then the guided 2-NN alone
    dA, dB, dX1, dX2, dM = _t(A), _t(B), _t(X1), _t(X2), _t(Mh)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    di = torch.full((n, 2), -7, dtype=torch.int32, device=_dev()); dd = torch.full((n, 2), -7.0, dtype=torch.float32, device=_dev())
    dm = torch.full((n,), -7, dtype=torch.int32, device=_dev()); dc = torch.full((K,), -7, dtype=torch.int32, device=_dev())
    hc = np.zeros(K, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_pairs_dev(C.byref(mp), dA.data_ptr(), dB.data_ptr(), _p(o1, C.c_int64), m, _p(o2, C.c_int64), m,
                     _p(prs, C.c_int32), K, dX1.data_ptr(), dX2.data_ptr(), kd, dM.data_ptr(), C.byref(gp), 0, st, di.data_ptr(), dd.data_ptr(),
                     dm.data_ptr(), dc.data_ptr(), _p(hc, C.c_int32)))
    assert list(hc) == list(cnt)                                         # host counts are valid on return
    assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(_bits(dd.cpu().numpy()), _bits(wd)) and np.array_equal(dm.cpu().numpy(), wm)
    assert list(dc.cpu().numpy()) == list(cnt)
    di.fill_(-7); dd.fill_(-7.0)
    _lib.check_match(L.mi_degensac_match_guided_knn2_pairs_dev(code, dA.data_ptr(), dB.data_ptr(), _p(o1, C.c_int64), m, _p(o2, C.c_int64), m,
                     _p(prs, C.c_int32), K, dim, dX1.data_ptr(), dX2.data_ptr(), kd, dM.data_ptr(), C.byref(gp), 0, st, di.data_ptr(), dd.data_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(_bits(dd.cpu().numpy()), _bits(wd))


# ---- the pipeline: pair list -> models -> guided matches, every image stored once ----
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model", ["F", "H"])
def test_chain_from_match_and_verify_pairs(oracle_port, model, mutual):
    """match_and_verify_pairs_tensors, then guided_match_pairs_tensors on the models it returned (F as it is, H in the user's form),
    against match_and_verify_batch_tensors(guided=True) on the expansion with the same seeds; and against the restatement under the
    driver-form models"""
    import torch
    from tests.test_gpu_match_pairs import SCENE_PAIRS, SEEDS, _scene
    xy, k4, k6, desc, counts = _scene(model)
    tk, td = _t(xy), _t(desc)
    kw = dict(model=model, mutual=mutual, max_iters=2000, seeds=SEEDS)
    Mu, match, inl, stats, cnt, po = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, **kw)
    gm, gi, gd, gpo = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, Mu, model=model, mutual=mutual)
    (ek1, ed1), (ek2, ed2), c1, c2, want_po = pr.expand((xy, desc), counts, (xy, desc), counts, SCENE_PAIRS)
    want = tensor_api.match_and_verify_batch_tensors(_t(ek1), _t(ek2), _t(ed1), _t(ed2), c1, c2, guided=True, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(gpo, want_po) and np.array_equal(po, want_po)
    assert torch.equal(Mu.contiguous().view(torch.int64), want[0].contiguous().view(torch.int64))
    assert torch.equal(gm, want[5])
    gm = gm.cpu().numpy()
    need = 8 if model == "F" else 4
    assert cnt[3] < need and (gm[po[3]:po[4]] == -1).all()              # the short pair: zero model, no guided matches
    for p in (0, 1, 2):
        assert (gm[po[p]:po[p + 1]] >= 0).sum() >= 20, p
    # (a): the restatement under the models in the driver's form (for H: inv(H)^T of the user form, as the call converts it)
    Md = Mu if model == "F" else tensor_api._h_driver_form(Mu)
    px = 0.5 if model == "F" else 1.0
    res = _both(oracle_port, (xy, desc, counts), (xy, desc, counts), SCENE_PAIRS, Md.cpu().numpy(), model, 0, px, "l2", mutual=mutual)
    assert np.array_equal(np.concatenate([r[0] for r in res]), gm)
