"""GPU: FGINN inside the gate of guided matching (include/mi_degensac.h mi_degensac_match_guided_fginn_*; fginn_th= of
tensor_api.guided_match_batch_tensors / guided_match_pairs_tensors and matcher.guided_match / _batch / _pairs; guided_fginn_th= of
match_and_verify_batch[_tensors]).  Equality only, bit for bit: every result against tests/guided_fginn_ref.oracle per entry (the CPU
oracle's residuals, `<=`, the numpy matcher's distances, the exclusion rule of tests/fginn_ref.py), and every pair-list result also
against the batched new call on the expansion of tests/pairs_ref.py.  The shapes are the edges of the rescan kernel, not a workload:
query images around the 16-query tile, train images around the 64-row step and the 1024-row LDS chunk, needy counts around the tile and
the wave, candidate lists at their flush edges, the radius at equality and one ulp beside it."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, tensor_api
from tests import guided_fginn_ref as gf, guided_ref as gr, pairs_ref as pr

pytestmark = pytest.mark.gpu
R = 10.0
CODE = {"l2": 0, "hamming": 1, "l2_u8": 4}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _px(model, et):
    return 12.0 if (model == "H" and et in (2, 4)) else 6.0


def _split(po, *arrs):
    return [tuple(a[po[p]:po[p + 1]] for a in arrs) for p in range(len(po) - 1)]


def _store(sizes, dim, norm, seed):
    """images that see one bank of scene points (keypoints in [0, 200]^2, a little noise; descriptors noisy copies), so entries have true
    matches under a model near the identity and a few gated strangers.  The last third of an image's rows are TWINS of its first rows: 1.5 px
    beside them with a near-equal descriptor.  Rows 3 and 5 are exact duplicates (ties)."""
    rng = np.random.default_rng([seed, dim, len(sizes)])
    B = max(max(sizes), 8) + 16
    bank_k = rng.uniform(0, 200, (B, 2))
    bank_d = rng.normal(size=(B, dim)).astype(np.float32) if norm == "l2" else rng.integers(0, 256, (B, dim), dtype=np.uint8)
    ks, ds = [], []
    for n in sizes:
        base = n - n // 3
        sel = rng.permutation(B)[:base]
        sel = np.r_[sel, sel[:n - base]]
        k = bank_k[sel] + 0.3 * rng.normal(size=(n, 2))
        k[base:, 0] += 1.5
        if norm == "l2":
            d = bank_d[sel] + 0.1 * rng.normal(size=(n, dim)).astype(np.float32)
            d[base:] = d[:n - base] + 0.002 * rng.normal(size=(n - base, dim)).astype(np.float32)
        else:
            d = bank_d[sel] ^ (rng.random((n, dim)) < 0.05).astype(np.uint8)
            d[base:] = d[:n - base]; d[base:, 0] ^= 1
        if n > 8:
            d[5] = d[3]; k[5] = k[3]
        ks.append(k); ds.append(d)
    return np.concatenate(ks), np.concatenate(ds), list(sizes)


def _models(model, K, seed, zero=(), nan=()):
    """one driver-form model per list entry, each another one (tests/test_gpu_guided_pairs.py): translations by small whole numbers"""
    rng = np.random.default_rng([seed, K])
    M = np.zeros((K, 3, 3))
    for p in range(K):
        a, b = rng.integers(-3, 4, 2)
        M[p] = gf.shift_model(model, a, b if model == "H" else a)
    for p in zero:
        M[p] = 0.0
    for p in nan:
        M[p, 1, 1] = np.nan
    return M


def _both(P, s1, s2, pairs, M, model, et, px, norm, r=R, ratio=0.9, mutual=False, kps_for_oracle=None):
    """guided_match_pairs_tensors(fginn_th=r) on the stores s1 / s2 = (kps, desc, counts) (s2 is s1: one store) against the batched new call
    on the expansion and the restatement per entry; slot 0 also against the plain guided call.  Returns (per entry (match, idx, dist), needy
    count per entry by the restatement)."""
    import torch
    k1, d1, c1 = s1; k2, d2, c2 = s2
    tk1, td1 = _t(k1), _t(d1)
    tk2, td2 = (tk1, td1) if s2 is s1 else (_t(k2), _t(d2))
    tM = _t(M)
    kw = dict(model=model, ratio=ratio, mutual=mutual, px_th=px, error_type=gr.ERROR_NAMES[model][et], norm=norm, driver_form=True)
    got = tensor_api.guided_match_pairs_tensors(tk1, tk2, td1, td2, c1, c2, pairs, tM, fginn_th=r, **kw)
    plain = tensor_api.guided_match_pairs_tensors(tk1, tk2, td1, td2, c1, c2, pairs, tM, **kw)
    (ek1, ed1), (ek2, ed2), e1, e2, want_po = pr.expand((k1, d1), c1, (k2, d2), c2, pairs)
    want = tensor_api.guided_match_batch_tensors(_t(ek1), _t(ek2), _t(ed1), _t(ed2), e1, e2, tM, fginn_th=r, **kw)
    torch.cuda.synchronize()
    match, idx, dist, po = got
    assert np.array_equal(po, want_po)
    assert torch.equal(match, want[0]) and torch.equal(idx, want[1]) and torch.equal(dist.view(torch.int32), want[2].view(torch.int32))
    assert torch.equal(idx[:, 0], plain[1][:, 0]) and torch.equal(dist[:, 0].view(torch.int32), plain[2][:, 0].view(torch.int32))
    res = _split(po, match.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy())
    x1, x2 = kps_for_oracle or (k1, k2)
    o1, o2 = pr.offsets(c1), pr.offsets(c2)
    needy = []
    for p, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        oi, od, om, on = gf.oracle(P, model, et, px, M[p], x1[o1[i]:o1[i + 1], :2], x2[o2[j]:o2[j + 1], :2], d1[o1[i]:o1[i + 1]],
                                   d2[o2[j]:o2[j + 1]], norm, r, ratio, mutual)
        gm, gi, gd = res[p]
        assert gi.shape == (c1[i], 2), p
        assert np.array_equal(gi, oi), (p, i, j, np.flatnonzero((gi != oi).any(1))[:5])
        assert np.array_equal(_bits(gd), _bits(od)), (p, i, j)
        assert np.array_equal(gm, om), (p, i, j)
        needy.append(int(on.sum()))
    return res, needy


def _stores_of(scenes):
    """entries (k1, k2, a, b, M, ...) -> two stores with image p = scene p, the identity list and the models"""
    s1 = (np.concatenate([s[0] for s in scenes]), np.concatenate([s[2] for s in scenes]), [len(s[0]) for s in scenes])
    s2 = (np.concatenate([s[1] for s in scenes]), np.concatenate([s[3] for s in scenes]), [len(s[1]) for s in scenes])
    return s1, s2, [(p, p) for p in range(len(scenes))], np.stack([s[4] for s in scenes])


# ---- query images around the 16-query tile x train images around the 64-row step and the 1024-row chunk; zero and NaN models ----
Q_SIZES = [0, 1, 15, 16, 17, 33, 65]
T_SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025]
EDGE_PAIRS = [(i, j) for i in range(len(Q_SIZES)) for j in range(len(T_SIZES))]


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model,et,norm,dim", [("F", 0, "l2", 5), ("H", 0, "hamming", 8), ("H", 2, "l2_u8", 4)])
def test_query_and_train_edges_over_two_stores(oracle_port, model, et, norm, dim, mutual):
    s1 = _store(Q_SIZES, dim, norm, 1); s2 = _store(T_SIZES, dim, norm, 2)
    M = _models(model, len(EDGE_PAIRS), 3, zero=(5, 40), nan=(17,))
    res, needy = _both(oracle_port, s1, s2, EDGE_PAIRS, M, model, et, _px(model, et), norm, mutual=mutual)
    assert sum(needy) > 20, needy
    assert all((res[p][1] == -1).all() for p in (5, 17, 40))             # zero and NaN models pass nothing


# ---- exact needy counts around the tile and the wave; an entry whose every query is needy; runs of empty entries around a needy one ----
NEEDY = [0, 1, 15, 16, 17, 63, 64, 65]


@pytest.mark.parametrize("model,norm,width", [("H", "l2", 8), ("F", "l2", 8), ("H", "hamming", 32), ("F", "l2_u8", 32)])
def test_exact_needy_counts(oracle_port, model, norm, width):
    empty = gf.twin_scene(0, 0, 0, width, norm, 0, model)
    scenes, want = [empty, empty], [0, 0]
    for n in NEEDY:
        scenes += [gf.twin_scene(4, n, 90 + n, width, norm, n, model), gf.twin_scene(5, n + 9, 90 + n, width, norm, n, model), empty]
        want += [n, n, 0]
    scenes += [empty]; want += [0]
    s1, s2, pairs, M = _stores_of(scenes)
    res, needy = _both(oracle_port, s1, s2, pairs, M, model, 0, 3.0, norm, mutual=False)
    assert needy == want
    for (m, i, d), n in zip(res, want):                                   # every twinned query is a match
        assert (m[:n] >= 0).all()
        if model == "H":                                                   # the keep rule: the twin was the only companion
            assert (i[:n, 1] == -1).all() and np.isposinf(d[:n, 1]).all()


# ---- the rescan's candidate lists at their flush edges, ties across a flush, anchor and twin in two chunks ----
@pytest.mark.parametrize("n_q", [1, 17])
def test_candidate_lists_at_their_edges(oracle_port, n_q):
    kinds = ["exact64", "carry63", "excluded", "chunks", "tie_lo", "tie_hi", "offband"]
    scenes = [gf.flush_scene(k, n_q) for k in kinds[:-1]] + [gf.offband_scene(n_q)]
    s1, s2, pairs, M = _stores_of(scenes)
    res, needy = _both(oracle_port, s1, s2, pairs, M, "F", 0, 1.0, "l2")
    assert needy == [n_q] * len(kinds)
    for (m, i, d), s, k in zip(res, scenes, kinds):
        assert (i[:, 0] == s[5]).all() and (i[:, 1] == s[6]).all(), k


# ---- the radius: dx dx + dy dy == r r competes, one ulp beside it does not ----
def test_radius_edge(oracle_port):
    s1, s2, pairs, M = _stores_of([gf.radius_scene(), gf.radius_scene(below=True)])
    for r, want in ((10.0, [2, 3]), (float(np.nextafter(10.0, 11.0)), [3, 3]), (float(np.nextafter(10.0, 0.0)), [2, 2])):
        res, needy = _both(oracle_port, s1, s2, pairs, M, "H", 0, 1e100, "l2", r=r)
        assert needy == [3, 3] and [int(g[1][0, 1]) for g in res] == want, r


# ---- r = 0 and fginn_th=None are the plain guided call, bit for bit; an all-pass gate is the unguided FGINN 2-NN ----
L_SIZES = [0, 40, 0, 17, 70, 0, 33, 9]
L_PAIRS = [(7, 1), (0, 1), (2, 4), (0, 0), (1, 4), (3, 4), (6, 4), (4, 4), (5, 3), (2, 2), (0, 6), (4, 1), (1, 4), (1, 0), (6, 2), (3, 3), (1, 1),
           (6, 3), (3, 6), (4, 6), (5, 5), (2, 1)]                       # the last image first; self pairs, repeats, both orders, empty images
L_ZERO, L_NAN = (5, 17), (15,)


@pytest.mark.parametrize("norm,dim", [("l2", 9), ("hamming", 8), ("l2_u8", 8)])
def test_radius_zero_is_the_plain_guided_call(oracle_port, norm, dim):
    import torch
    k, d, c = _store(L_SIZES, dim, norm, 6)
    tk, td, tM = _t(k), _t(d), _t(_models("H", len(L_PAIRS), 7, zero=L_ZERO))
    for mutual in (False, True):
        kw = dict(model="H", mutual=mutual, px_th=6.0, norm=norm, driver_form=True)
        zero = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, c, c, L_PAIRS, tM, fginn_th=0.0, **kw)
        plain = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, c, c, L_PAIRS, tM, **kw)
        none = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, c, c, L_PAIRS, tM, fginn_th=None, **kw)
        torch.cuda.synchronize()
        for g in (zero, none):
            assert torch.equal(g[0], plain[0]) and torch.equal(g[1], plain[1]) and torch.equal(g[2].view(torch.int32), plain[2].view(torch.int32))
        assert int((plain[0] >= 0).sum()) > 20


def test_all_pass_gate_is_the_unguided_fginn_2nn(oracle_port):
    import torch
    sizes = [17, 63, 64, 127, 191, 1087, 0]
    pairs = [(0, j) for j in range(7)] + [(j, 0) for j in range(7)] + [(3, 3), (5, 4)]
    k, d, c = s = _store(sizes, 3, "l2", 8)
    M = np.random.default_rng(9).normal(size=(len(pairs), 3, 3))
    res, needy = _both(oracle_port, s, s, pairs, M, "F", 0, 1e100, "l2", mutual=True)
    assert sum(needy) > 50
    ui, ud, po = tensor_api.knn_match_fginn_pairs_tensors(_t(d), _t(d), _t(k), c, c, pairs, spatial_th=R)
    torch.cuda.synchronize()
    for g, (wi, wd) in zip(res, _split(po, ui.cpu().numpy(), ud.cpu().numpy())):
        assert np.array_equal(g[1], wi) and np.array_equal(_bits(g[2]), _bits(wd))


# ---- every error type, mutual on and off; the same (i, j) under two models; a shared train image ----
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model,et", gr.KINDS)
def test_error_types_and_lists(oracle_port, model, et, mutual):
    s = _store(L_SIZES, 33, "l2", 10)
    M = _models(model, len(L_PAIRS), 11, zero=L_ZERO, nan=L_NAN)
    M[12] = M[4]; M[12][2, 0 if model == "H" else 2] += 5.0              # entry 12 = entry 4's images under a model shifted by 5
    res, needy = _both(oracle_port, s, s, L_PAIRS, M, model, et, _px(model, et), "l2", mutual=mutual)
    assert sum(needy) > 10 and not np.array_equal(res[4][1], res[12][1])
    for p in L_ZERO + L_NAN:
        assert (res[p][0] == -1).all() and (res[p][1] == -1).all()


# ---- norms and row widths: 1, 64 and 65 words; every uint8 L2 class ----
WIDTHS = [("l2", 1), ("l2", 64), ("l2", 65), ("hamming", 4), ("hamming", 256), ("hamming", 260), ("l2_u8", 4), ("l2_u8", 64), ("l2_u8", 68),
          ("l2_u8", 128), ("l2_u8", 132), ("l2_u8", 256)]


@pytest.mark.parametrize("norm,dim", WIDTHS)
def test_norms_and_widths(oracle_port, norm, dim):
    s = _store(L_SIZES, dim, norm, 12)
    M = _models("H", len(L_PAIRS), 13, zero=L_ZERO)
    res, needy = _both(oracle_port, s, s, L_PAIRS, M, "H", 0, 6.0, norm, mutual=True)
    assert sum(needy) > 10 or dim == 1                                    # (one float: descriptors hardly tell rows apart)


# ---- non-finite keypoints and descriptor rows ----
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_keypoints_and_descriptors(oracle_port, bad):
    k, d, c = _store(L_SIZES, 6, "l2", 14)
    k = k.copy(); d = d.copy()
    o = pr.offsets(c)
    k[o[4] + 2, 0] = bad; k[o[4] + 50, 1] = bad; k[o[1] + 30] = bad; d[o[4] + 7, 2] = bad; d[o[3] + 1, 0] = bad; d[o[1] + 28] = bad
    M = _models("H", len(L_PAIRS), 15)
    _both(oracle_port, (k, d, c), (k, d, c), L_PAIRS, M, "H", 0, 6.0, "l2", mutual=True)
    _both(oracle_port, (k, d, c), (k, d, c), L_PAIRS, M, "F", 1, 1e100, "l2")


# ---- keypoint layouts ----
@pytest.mark.parametrize("form", ["laf6", "kpts4"])
def test_keypoint_layouts(oracle_port, form):
    k, d, c = _store(L_SIZES, 20, "l2", 16)
    rng = np.random.default_rng(17)
    if form == "laf6":
        kps = np.c_[k, rng.normal(size=(len(k), 4))]; xy = kps
    else:
        kps = np.c_[k, rng.uniform(2, 9, len(k)), rng.uniform(0, 360, len(k))].astype(np.float32); xy = kps[:, :2].astype(np.float64)
    M = _models("F", len(L_PAIRS), 18, zero=L_ZERO)
    res, needy = _both(oracle_port, (kps, d, c), (kps, d, c), L_PAIRS, M, "F", 0, 6.0, "l2", mutual=True, kps_for_oracle=(xy, xy))
    assert sum(needy) > 10


# ---- the numpy entry points (one store and two, the batch, one pair) and a second stream ----
def _tuples(res):
    return [(np.flatnonzero(m >= 0), m[m >= 0], d[m >= 0, 0]) for m, i, d in res]


@pytest.mark.parametrize("norm,dim", [("l2", 20), ("l2_u8", 6)])
def test_numpy_entry_points(oracle_port, norm, dim):
    k, d, c = _store(L_SIZES, dim, norm, 19)
    o = pr.offsets(c)
    kl = [k[o[i]:o[i + 1]] for i in range(len(c))]; dl = [d[o[i]:o[i + 1]] for i in range(len(c))]
    dpad = d if norm == "l2" else np.c_[d, np.zeros((len(d), 2), np.uint8)]
    M = _models("F", len(L_PAIRS), 20, zero=L_ZERO)
    res, needy = _both(oracle_port, (k, dpad, c), (k, dpad, c), L_PAIRS, M, "F", 1, 4.0, norm, mutual=True)
    kw = dict(model="F", mutual=True, px_th=4.0, error_type="symm_epipolar", norm=norm, fginn_th=R)
    got = matcher.guided_match_pairs(kl, dl, L_PAIRS, M, **kw)
    two = matcher.guided_match_pairs(kl, dl, L_PAIRS, M, kps2_list=kl, desc2_list=dl, **kw)
    bat = matcher.guided_match_batch([kl[i] for i, j in L_PAIRS], [kl[j] for i, j in L_PAIRS], [dl[i] for i, j in L_PAIRS],
                                     [dl[j] for i, j in L_PAIRS], M, **kw)
    one = matcher.guided_match(kl[4], kl[1], dl[4], dl[1], M[11], **kw)
    plain = matcher.guided_match_pairs(kl, dl, L_PAIRS, M, **dict(kw, fginn_th=None))
    w = _tuples(res)
    for g in (got, two, bat):
        assert all(np.array_equal(a, b) for gp, wp in zip(g, w) for a, b in zip(gp, wp))
    assert all(np.array_equal(a, b) for a, b in zip(one, w[11]))
    assert sum(len(g[0]) for g in got) > sum(len(g[0]) for g in plain) > 20


def test_second_stream_without_host_synchronisation(oracle_port):
    import torch
    k, d, c = s = _store(L_SIZES, 33, "l2", 21)
    M = _models("F", len(L_PAIRS), 22, zero=L_ZERO)
    want, _ = _both(oracle_port, s, s, L_PAIRS, M, "F", 0, 6.0, "l2", mutual=True)
    tk, td, tM = _t(k), _t(d), _t(M)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(st):
        match, idx, dist, po = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, c, c, L_PAIRS, tM, model="F", mutual=True, px_th=6.0,
                                                                     driver_form=True, fginn_th=R)
    st.synchronize()
    for g, w in zip(_split(po, match.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(_bits(g[2]), _bits(w[2]))


# ---- the C ABI: stores entered at a non-zero first offset, all six entry points; a short struct_size is the plain call ----
def _p(x, t):
    return x.ctypes.data_as(C.POINTER(t))


@pytest.mark.parametrize("model,et,norm,dim,kd", [("F", 0, "l2", 37, 2), ("H", 1, "hamming", 32, 6), ("H", 0, "l2_u8", 8, 2)])
def test_stores_whose_first_offset_is_above_zero(oracle_port, model, et, norm, dim, kd):
    import torch
    code = CODE[norm]
    k, d, c = s = _store(L_SIZES, dim, norm, 23)
    K = len(L_PAIRS)
    M = _models(model, K, 24, zero=L_ZERO)
    want, needy = _both(oracle_port, s, s, L_PAIRS, M, model, et, 6.0, norm, mutual=True)
    assert sum(needy) > 10
    wm = np.concatenate([w[0] for w in want]); wi = np.concatenate([w[1] for w in want]); wd = np.concatenate([w[2] for w in want])
    rng = np.random.default_rng(25)
    if kd == 6:
        k = np.c_[k, rng.normal(size=(len(k), 4))]
    A = np.ascontiguousarray(np.concatenate([d[:5], d])); B = np.ascontiguousarray(np.concatenate([d[:12], d, d[:5]]))
    X1 = np.ascontiguousarray(np.concatenate([k[:5], k])); X2 = np.ascontiguousarray(np.concatenate([k[:12], k, k[:5]]))
    o1 = pr.offsets(c) + 5; o2 = pr.offsets(c) + 12
    prs = np.ascontiguousarray(L_PAIRS, np.int32); Mh = np.ascontiguousarray(M.reshape(K, 9))
    n = len(wm); m = len(c)
    mp = _lib.MatchParams(code, dim, 0.9, True, R); gp = _lib.GuideParams(model == "H", et, 6.0)
    L = _lib.lib()
    i64, i32, f32 = C.c_int64, C.c_int32, C.c_float
    idx = np.full((n, 2), -7, np.int32); dist = np.full((n, 2), -7, np.float32); match = np.full(n, -7, np.int32); cnt = np.zeros(K, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_fginn_pairs(C.byref(mp), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), _p(o1, i64), m,
                     _p(o2, i64), m, _p(prs, i32), K, _lib.dptr(X1), _lib.dptr(X2), kd, _lib.dptr(Mh), C.byref(gp), 0, _p(idx, i32), _p(dist, f32),
                     _p(match, i32), _p(cnt, i32)))
    assert np.array_equal(idx, wi) and np.array_equal(_bits(dist), _bits(wd)) and np.array_equal(match, wm)
    assert list(cnt) == [int((w[0] >= 0).sum()) for w in want]
    # a struct_size that does not cover spatial_th: the plain guided call
    short = _lib.MatchParams(code, dim, 0.9, True, R); short.struct_size = _lib.MatchParams.spatial_th.offset
    pi = np.full((n, 2), -7, np.int32); pd = np.full((n, 2), -7, np.float32); pm = np.full(n, -7, np.int32)
    si, sd, sm = pi.copy(), pd.copy(), pm.copy()
    args = lambda a, b, e: (A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), _p(o1, i64), m, _p(o2, i64), m, _p(prs, i32), K, _lib.dptr(X1),
                            _lib.dptr(X2), kd, _lib.dptr(Mh), C.byref(gp), 0, _p(a, i32), _p(b, f32), _p(e, i32), None)
    _lib.check_match(L.mi_degensac_match_guided_pairs(C.byref(mp), *args(pi, pd, pm)))
    _lib.check_match(L.mi_degensac_match_guided_fginn_pairs(C.byref(short), *args(si, sd, sm)))
    assert np.array_equal(si, pi) and np.array_equal(_bits(sd), _bits(pd)) and np.array_equal(sm, pm) and not np.array_equal(pi, wi)
    # device pointers, pair list
    dA, dB, dX1, dX2, dM = _t(A), _t(B), _t(X1), _t(X2), _t(Mh)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    new = lambda shape, dt: torch.full(shape, -7, dtype=dt, device=_dev())
    di, dd, dm, dc = new((n, 2), torch.int32), new((n, 2), torch.float32), new((n,), torch.int32), new((K,), torch.int32)
    hc = np.zeros(K, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_fginn_pairs_dev(C.byref(mp), dA.data_ptr(), dB.data_ptr(), _p(o1, i64), m, _p(o2, i64), m, _p(prs, i32),
                     K, dX1.data_ptr(), dX2.data_ptr(), kd, dM.data_ptr(), C.byref(gp), 0, st, di.data_ptr(), dd.data_ptr(), dm.data_ptr(),
                     dc.data_ptr(), _p(hc, i32)))
    assert list(hc) == list(cnt)
    assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(_bits(dd.cpu().numpy()), _bits(wd)) and np.array_equal(dm.cpu().numpy(), wm)
    assert list(dc.cpu().numpy()) == list(cnt)
    di.fill_(-7); dd.fill_(-7.0)
    _lib.check_match(L.mi_degensac_match_guided_fginn_knn2_pairs_dev(code, dA.data_ptr(), dB.data_ptr(), _p(o1, i64), m, _p(o2, i64), m, _p(prs, i32), K,
                     dim, dX1.data_ptr(), dX2.data_ptr(), kd, dM.data_ptr(), C.byref(gp), R, 0, st, di.data_ptr(), dd.data_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy(), wi) and np.array_equal(_bits(dd.cpu().numpy()), _bits(wd))
    # the ragged batch at a non-zero first offset: the expansion behind 5 / 12 foreign rows, results at rows 5 ..
    (ek1, ed1), (ek2, ed2), e1, e2, po = pr.expand((k, d), c, (k, d), c, L_PAIRS)
    A = np.ascontiguousarray(np.concatenate([d[:5], ed1])); B = np.ascontiguousarray(np.concatenate([d[:12], ed2]))
    X1 = np.ascontiguousarray(np.concatenate([k[:5], ek1])); X2 = np.ascontiguousarray(np.concatenate([k[:12], ek2]))
    b1 = pr.offsets(e1) + 5; b2 = pr.offsets(e2) + 12
    idx = np.full((n + 5, 2), -7, np.int32); dist = np.full((n + 5, 2), -7, np.float32); match = np.full(n + 5, -7, np.int32)
    _lib.check_match(L.mi_degensac_match_guided_fginn_batch(C.byref(mp), A.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), _p(b1, i64),
                     _p(b2, i64), _lib.dptr(X1), _lib.dptr(X2), kd, K, _lib.dptr(Mh), C.byref(gp), 0, _p(idx, i32), _p(dist, f32), _p(match, i32),
                     _p(cnt, i32)))
    assert np.array_equal(idx[5:], wi) and np.array_equal(_bits(dist[5:]), _bits(wd)) and np.array_equal(match[5:], wm) and (idx[:5] == -7).all()
    dA, dB, dX1, dX2 = _t(A), _t(B), _t(X1), _t(X2)
    di, dd, dm = new((n + 5, 2), torch.int32), new((n + 5, 2), torch.float32), new((n + 5,), torch.int32)
    _lib.check_match(L.mi_degensac_match_guided_fginn_batch_dev(C.byref(mp), dA.data_ptr(), dB.data_ptr(), _p(b1, i64), _p(b2, i64), dX1.data_ptr(),
                     dX2.data_ptr(), kd, K, dM.data_ptr(), C.byref(gp), 0, st, di.data_ptr(), dd.data_ptr(), dm.data_ptr(), None, _p(hc, i32)))
    assert list(hc) == list(cnt)
    assert np.array_equal(di.cpu().numpy()[5:], wi) and np.array_equal(_bits(dd.cpu().numpy()[5:]), _bits(wd))
    assert np.array_equal(dm.cpu().numpy()[5:], wm) and (dm.cpu().numpy()[:5] == -7).all()
    di.fill_(-7); dd.fill_(-7.0)
    _lib.check_match(L.mi_degensac_match_guided_fginn_knn2_batch_dev(code, dA.data_ptr(), dB.data_ptr(), _p(b1, i64), _p(b2, i64), K, dim,
                     dX1.data_ptr(), dX2.data_ptr(), kd, dM.data_ptr(), C.byref(gp), R, 0, st, di.data_ptr(), dd.data_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy()[5:], wi) and np.array_equal(_bits(dd.cpu().numpy()[5:]), _bits(wd)) and (di.cpu().numpy()[:5] == -7).all()


# ---- the chains ----
@pytest.mark.parametrize("model", ["F", "H"])
def test_chains_from_match_and_verify(oracle_port, model):
    """match_and_verify_batch_tensors(guided=True, guided_fginn_th=r) = that call without the keyword, then guided_match_batch_tensors(
    fginn_th=r) on its models; match_and_verify_fginn_pairs_tensors -> guided_match_pairs_tensors(fginn_th=r) gives the same rows and
    equals the restatement under the driver-form models"""
    import torch
    from tests.test_gpu_match_pairs import SCENE_PAIRS, SEEDS, _scene
    xy, k4, k6, desc, counts = _scene(model)
    tk, td = _t(xy), _t(desc)
    kw = dict(model=model, mutual=True, max_iters=2000, seeds=SEEDS)
    Mu, match, inl, stats, cnt, po = tensor_api.match_and_verify_fginn_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, R, **kw)
    gm, gi, gd, gpo = tensor_api.guided_match_pairs_tensors(tk, tk, td, td, counts, counts, SCENE_PAIRS, Mu, model=model, mutual=True, fginn_th=R)
    (ek1, ed1), (ek2, ed2), c1, c2, want_po = pr.expand((xy, desc), counts, (xy, desc), counts, SCENE_PAIRS)
    te = [_t(x) for x in (ek1, ek2, ed1, ed2)]
    chain = tensor_api.match_and_verify_batch_tensors(*te, c1, c2, guided=True, fginn_th=R, guided_fginn_th=R, **kw)
    base = tensor_api.match_and_verify_batch_tensors(*te, c1, c2, guided=True, fginn_th=R, **kw)
    step = tensor_api.guided_match_batch_tensors(*te, c1, c2, base[0], model=model, mutual=True, fginn_th=R)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(chain[1:3], base[1:3])) and np.array_equal(chain[4], base[4])
    assert torch.equal(chain[0].contiguous().view(torch.int64), base[0].contiguous().view(torch.int64))
    assert torch.equal(chain[5], step[0]) and torch.equal(chain[5], gm)
    assert torch.equal(Mu.contiguous().view(torch.int64), base[0].contiguous().view(torch.int64))
    Md = Mu if model == "F" else tensor_api._h_driver_form(Mu)
    res, needy = _both(oracle_port, (xy, desc, counts), (xy, desc, counts), SCENE_PAIRS, Md.cpu().numpy(), model, 0, 0.5 if model == "F" else 1.0,
                       "l2", mutual=True)
    assert np.array_equal(np.concatenate([r[0] for r in res]), gm.cpu().numpy())
    host = matcher.match_and_verify_batch([ek1[want_po[p]:want_po[p + 1]] for p in range(len(c1))],
                                          [ek2[pr.offsets(c2)[p]:pr.offsets(c2)[p + 1]] for p in range(len(c1))],
                                          [ed1[want_po[p]:want_po[p + 1]] for p in range(len(c1))],
                                          [ed2[pr.offsets(c2)[p]:pr.offsets(c2)[p + 1]] for p in range(len(c1))], guided=True, fginn_th=R,
                                          guided_fginn_th=R, **kw)
    assert np.array_equal(np.concatenate(host[3]), gm.cpu().numpy())


# ---- the twin scene end to end: what the feature is for ----
@pytest.mark.parametrize("model", ["F", "H"])
def test_twin_scene_end_to_end(oracle_port, model):
    n_tw = 40
    k1, k2, a, b, M = gf.twin_scene(7, 150, 200, 32, "l2", n_tw, model)
    kw = dict(model=model, px_th=3.0, driver_form=True)
    plain = matcher.guided_match(k1, k2, a, b, M, **kw)
    new = matcher.guided_match(k1, k2, a, b, M, fginn_th=R, **kw)
    oi, od, om, on = gf.oracle(oracle_port, model, 0, 3.0, M, k1, k2, a, b, "l2", R, 0.9, False)
    gi, gd, gm = gr.oracle(oracle_port, model, 0, 3.0, M, k1, k2, a, b, "l2", 0.9, False)
    assert int(on.sum()) == n_tw and int((om >= 0).sum()) - int((gm >= 0).sum()) == n_tw
    assert len(new[0]) - len(plain[0]) == n_tw
    assert np.array_equal(new[0], np.flatnonzero(om >= 0)) and np.array_equal(new[1], om[om >= 0])
    assert not np.isin(np.arange(n_tw), plain[0]).any() and np.isin(np.arange(n_tw), new[0]).all()
