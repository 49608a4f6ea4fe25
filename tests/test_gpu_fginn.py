"""GPU: the FGINN second neighbour (mi_fginn.h; tensor_api.knn_match_fginn_batch_tensors, matcher.match_fginn, fginn_th= of the
match-and-verify calls).  Every case compares idx with equality and dist by bits against the restatement of tests/fginn_ref.py,
for the three norms: train / query / needy counts around the 64-row tiles, empty pairs, widths around the 64-word chunk and the
uint8 instances, the radius edge, r = 0, ties across a tile and a split boundary, duplicates, non-finite keypoints and descriptors,
[n, 6] keypoints, an unsplit and a split launch, the pipeline, the single pair and a second stream."""
import numpy as np
import pytest

import pydegensac_amd as pd
from pydegensac_amd import matcher, parallel, synthetic as syn, tensor_api
from tests import fginn_ref as fr, matcher_ref as mr

pytestmark = pytest.mark.gpu

NORMS = list(fr.NORMS)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _cat(xs, width, dtype):
    return np.concatenate(xs) if len(xs) else np.zeros((0, width), dtype)


def _run(D1, D2, K2, r, norm):
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    idx, dist = tensor_api.knn_match_fginn_batch_tensors(_t(np.concatenate(D1)), _t(np.concatenate(D2)), _t(np.concatenate(K2)), c1, c2, r, norm)
    idx = idx.cpu().numpy(); dist = dist.cpu().numpy()
    o = np.r_[0, np.cumsum(c1)]
    return [(idx[o[p]:o[p + 1]], dist[o[p]:o[p + 1]]) for p in range(len(c1))]


def _check(D1, D2, K2, r, norm, got=None):
    """the device against the restatement, pair by pair; returns the needy count of every pair (from the restatement)"""
    got = got or _run(D1, D2, K2, r, norm)
    needy = []
    for p, (gi, gd) in enumerate(got):
        oi, od, nd, _ = fr.fginn(D1[p], D2[p], K2[p][:, :2], r, norm)
        assert np.array_equal(gi, oi), (p, np.flatnonzero((gi != oi).any(1))[:5], gi[(gi != oi).any(1)][:3], oi[(gi != oi).any(1)][:3])
        assert np.array_equal(_bits(gd), _bits(od)), (p, np.flatnonzero((_bits(gd) != _bits(od)).any(1))[:5])
        needy.append(int(nd.sum()))
    return needy


def _twins(seed, sizes, width, norm):
    """one twin scene per (n1, n2, needy)"""
    S = [fr.twin_scene(seed + i, n1, n2, width, norm, m) for i, (n1, n2, m) in enumerate(sizes)]
    return [s[0] for s in S], [s[1] for s in S], [s[2] for s in S]


def _w(norm):
    return 33 if norm == "l2" else 36


TRAIN_ROWS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129]
QUERY_ROWS = [0, 1, 64, 65]


@pytest.mark.parametrize("norm", NORMS)
def test_train_and_query_counts_and_empty_pairs(norm):
    """train rows 0 .. 129 and queries 0 .. 65 per pair in one ragged batch: every pair but the first has non-zero offsets, and the
    pairs without queries / without train rows lie between ordinary ones"""
    sizes = [(5, n2, min(5, n2 // 2)) for n2 in TRAIN_ROWS] + [(n1, 70, min(n1, 20)) for n1 in QUERY_ROWS] + [(7, 30, 3)]
    D1, D2, K2 = _twins(10, sizes, _w(norm), norm)
    needy = _check(D1, D2, K2, 10.0, norm)
    assert needy[4] == 5 and needy[-1] == 3 and needy[0] == 0 and needy[len(TRAIN_ROWS) + 3] >= 20


@pytest.mark.parametrize("norm", NORMS)
def test_needy_counts_around_the_tile(norm):
    want = [0, 1, 63, 64, 65]
    D1, D2, K2 = _twins(20, [(130, 200, m) for m in want], _w(norm), norm)
    assert _check(D1, D2, K2, 10.0, norm) == want


@pytest.mark.parametrize("norm,width", [("l2", w) for w in (1, 64, 65, 132)] + [("l2_u8", w) for w in (4, 64, 68, 128, 132, 256)]
                         + [("hamming", w) for w in (4, 64, 68, 128, 132, 256, 260, 528)])
def test_widths(norm, width):
    D1, D2, K2 = _twins(30, [(7, 30, 3), (70, 130, 20), (66, 65, 9)], width, norm)
    needy = _check(D1, D2, K2, 10.0, norm)
    assert sum(needy) > 0


# ---- placed distances: train row t at distance level[t] from the one query ---------------------------------------------------
def _levels(norm, lv, n1=1):
    lv = np.asarray(lv)
    if norm == "l2":
        b = np.zeros((len(lv), 3), np.float32); b[:, 0] = lv
        return np.zeros((n1, 3), np.float32), b
    b = (np.arange(8)[None, :] < lv[:, None]).astype(np.uint8)
    return np.zeros((n1, 8), np.uint8), b


@pytest.mark.parametrize("norm", NORMS)
def test_radius_edge_on_integer_keypoints(norm):
    a, b = _levels(norm, [0, 1, 2, 3])
    kp2 = np.array([[0.0, 0], [3, 4], [100, 100], [0.5, 0]])
    for r, second in ((5.0, 1), (np.nextafter(5.0, 6.0), 2), (0.0, 1), (4.0, 1)):
        (gi, _), = _run([a], [b], [kp2], r, norm)
        _check([a], [b], [kp2], r, norm, [(gi, _)])
        assert list(gi[0]) == [0, second], r


@pytest.mark.parametrize("norm", NORMS)
def test_radius_zero_equals_the_plain_batched_2nn(norm):
    sizes = [(5, n2, min(5, n2 // 2)) for n2 in TRAIN_ROWS] + [(n1, 70, min(n1, 20)) for n1 in QUERY_ROWS]
    D1, D2, K2 = _twins(40, sizes, _w(norm), norm)
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    pi, pdist = tensor_api.knn_match_batch_tensors(_t(np.concatenate(D1)), _t(np.concatenate(D2)), c1, c2, norm)
    got = _run(D1, D2, K2, 0.0, norm)
    assert np.array_equal(np.concatenate([g[0] for g in got]), pi.cpu().numpy())
    assert np.array_equal(_bits(np.concatenate([g[1] for g in got])), _bits(pdist.cpu().numpy()))
    assert _check(D1, D2, K2, 0.0, norm, got) == [0] * len(sizes)


@pytest.mark.parametrize("norm", NORMS)
def test_every_train_keypoint_inside_the_radius(norm):
    D1, D2, K2 = _twins(50, [(7, 30, 3), (70, 130, 20), (5, 70, 2)], _w(norm), norm)
    K2[1] = np.random.default_rng(1).uniform(0, 3, K2[1].shape)
    got = _run(D1, D2, K2, 10.0, norm)
    _check(D1, D2, K2, 10.0, norm, got)
    gi, gd = got[1]
    assert (gi[:, 0] >= 0).all() and (gi[:, 1] == -1).all() and np.isposinf(gd[:, 1]).all()
    keep = tensor_api.match_filter_tensors(_t(gi), _t(gd), 0.9)
    assert int(keep.sum()) == 0


def _tie_pair(norm, n2, rows, n1=2):
    """row 0 nearest, row 1 its twin (inside the radius), the two `rows` tie as the nearest competing rows, the rest farther"""
    lv = np.full(n2, 5); lv[0] = 0; lv[1] = 1; lv[list(rows)] = 2
    a, b = _levels(norm, lv, n1)
    kp2 = np.c_[100.0 * (1 + np.arange(n2)), np.zeros(n2)]; kp2[1] = kp2[0] + [1.0, 0.0]
    return a, b, kp2


@pytest.mark.parametrize("norm", NORMS)
def test_ties_across_a_tile_and_a_split_boundary_and_a_short_last_split(norm):
    """equal distances on both sides of the 64-row tile boundary (an unsplit pair) and of the split boundary (rows t_chunk - 1 and
    t_chunk of a pair whose train set is split, the last split short): the lower index wins"""
    c1, c2 = [3, 2, 3], [70, 20000, 70]
    t_chunk, splits = mr.batch_split(c1, c2)
    rows = mr.split_rows(c2[1], t_chunk, splits)
    assert splits > 1 and t_chunk == 128 and mr.split_case(rows) == "short" and rows[-1] == 32
    a0, b0, k0 = _tie_pair(norm, 70, (63, 64), 3)
    a1, b1, k1 = _tie_pair(norm, 20000, (t_chunk - 1, t_chunk))
    a2, b2, k2 = _tie_pair(norm, 70, (64, 69), 3)
    got = _run([a0, a1, a2], [b0, b1, b2], [k0, k1, k2], 10.0, norm)
    assert _check([a0, a1, a2], [b0, b1, b2], [k0, k1, k2], 10.0, norm, got) == [3, 2, 3]
    assert [list(g[0][0]) for g in got] == [[0, 63], [0, t_chunk - 1], [0, 64]]
    # the same tie in a batch that is not split: 600 pairs cover the device twice
    many = [_tie_pair(norm, 70, (63, 64), 1)] * 600
    assert mr.batch_split([1] * 600, [70] * 600)[1] == 1
    got = _run([m[0] for m in many], [m[1] for m in many], [m[2] for m in many], 10.0, norm)
    assert all(list(g[0][0]) == [0, 63] for g in got)


@pytest.mark.parametrize("norm", NORMS)
def test_duplicate_descriptors_inside_the_radius(norm):
    lv = np.array([0, 0, 0, 3, 3, 4] + [6] * 70)
    a, b = _levels(norm, lv, 2)
    kp2 = np.c_[100.0 * np.arange(len(lv)), np.zeros(len(lv))]; kp2[1] = [0.5, 0]; kp2[2] = [0, 0.5]
    got = _run([a], [b], [kp2], 10.0, norm)
    assert _check([a], [b], [kp2], 10.0, norm, got) == [2]
    assert list(got[0][0][0]) == [0, 3]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_keypoints(norm, bad):
    lv = np.array([0, 1, 2, 3, 4] + [6] * 70)
    a, b = _levels(norm, lv, 2)
    n2 = len(lv)
    base = np.c_[100.0 * np.arange(n2), 50.0 + np.zeros(n2)]; base[1] = base[0] + [1, 0]
    ka = base.copy(); ka[0, 0] = bad                                  # the anchor
    kc = base.copy(); kc[2, 1] = bad; kc[3] = bad                     # competing rows
    kb = base.copy(); kb[0] = bad; kb[2] = bad                        # both sides: inf - inf is NaN
    got = _run([a, a, a], [b, b, b], [ka, kc, kb], 10.0, norm)
    _check([a, a, a], [b, b, b], [ka, kc, kb], 10.0, norm, got)
    if np.isnan(bad):
        assert list(got[0][0][0]) == [0, -1] and list(got[1][0][0]) == [0, 4]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_descriptor_rows(bad):
    D1, D2, K2 = _twins(60, [(7, 30, 3), (70, 130, 20)], 33, "l2")
    D2[1][3, 5] = bad; D2[1][120:, 0] = bad                           # a twinned train row and half of the twins
    D1[1][9, 2] = bad
    needy = _check(D1, D2, K2, 10.0, "l2")
    assert needy[1] > 0


@pytest.mark.parametrize("norm", NORMS)
def test_six_column_keypoints(norm):
    D1, D2, K2 = _twins(70, [(7, 30, 3), (70, 130, 20)], _w(norm), norm)
    rng = np.random.default_rng(2)
    K6 = [np.c_[k, rng.normal(size=(len(k), 4))] for k in K2]
    got6 = _run(D1, D2, K6, 10.0, norm)
    assert min(_check(D1, D2, K6, 10.0, norm, got6)) > 0


@pytest.mark.parametrize("norm", NORMS)
def test_unsplit_batch_of_many_small_pairs(norm):
    import torch
    K = 600
    D1, D2, K2 = _twins(80, [(8, 70, 4)] * K, 8, norm)
    assert mr.batch_split([8] * K, [70] * K, torch.cuda.get_device_properties(0).multi_processor_count)[1] == 1
    assert sum(_check(D1, D2, K2, 10.0, norm)) >= K


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
def _scene_pairs(model, sizes, seed, dim=32):
    """two-view pairs with descriptors; a third of the train keypoints get a twin 1.5 px away with a near-equal descriptor"""
    rng = np.random.default_rng(seed)
    K1, K2, D1, D2 = [], [], [], []
    for i, n in enumerate(sizes):
        if model == "F":
            p1, p2, lab, _ = syn.two_view_fundamental(max(n, 50), 0.5, 0.1, seed=seed * 100 + i)
        else:
            p1, p2, lab, _ = syn.homography_pairs(max(n, 50), 0.5, 0.3, seed=seed * 100 + i)
        p1, p2, lab = p1[:n, :2], p2[:n, :2], lab[:n]
        d1 = rng.normal(size=(n, dim)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32)
        d2[~lab] = rng.normal(size=((~lab).sum(), dim)).astype(np.float32)
        tw = rng.permutation(n)[:n // 3]
        p2 = np.r_[p2, p2[tw] + [1.5, 0.0]]; d2 = np.r_[d2, d2[tw] + 0.002 * rng.normal(size=(len(tw), dim)).astype(np.float32)]
        perm = rng.permutation(len(p2))
        K1.append(np.ascontiguousarray(p1)); K2.append(np.ascontiguousarray(p2[perm])); D1.append(d1); D2.append(d2[perm])
    return K1, K2, D1, D2


def _pipeline(K1, K2, D1, D2, **kw):
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    out = tensor_api.match_and_verify_batch_tensors(_t(np.concatenate(K1)), _t(np.concatenate(K2)), _t(np.concatenate(D1)), _t(np.concatenate(D2)),
                                                    c1, c2, **kw)
    return [x.cpu().numpy() if hasattr(x, "cpu") else x for x in out]


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("model", ["F", "H"])
def test_pipeline_equals_the_composed_calls(model, mutual, guided):
    sizes = [400, 6, 250, 0, 300]
    K1, K2, D1, D2 = _scene_pairs(model, sizes, 3)
    K = len(sizes); seeds = parallel.pair_seeds(7, 7 + K); r = 10.0
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    o1 = np.r_[0, np.cumsum(c1)]; o2 = np.r_[0, np.cumsum(c2)]
    kw = dict(model=model, ratio=0.9, mutual=mutual, seeds=seeds, guided=guided, max_iters=20000)
    res = _pipeline(K1, K2, D1, D2, fginn_th=r, **kw)
    M, match, inl, st, cnt = res[:5]
    # composed: the FGINN 2-NN, the filter per pair, the batch estimator on the tentatives
    a, b = _t(np.concatenate(D1)), _t(np.concatenate(D2))
    idx, dist = tensor_api.knn_match_fginn_batch_tensors(a, b, _t(np.concatenate(K2)), c1, c2, r)
    back = tensor_api.knn_match_batch_tensors(b, a, c2, c1)[0] if mutual else None
    A, B, elig = [], [], []
    for p in range(K):
        bk = back[o2[p]:o2[p + 1]] if mutual and c2[p] > 0 else None
        keep = tensor_api.match_filter_tensors(idx[o1[p]:o1[p + 1]], dist[o1[p]:o1[p + 1]], 0.9, bk).cpu().numpy().astype(bool)
        ip = idx[o1[p]:o1[p + 1]].cpu().numpy()
        want = np.where(keep, ip[:, 0], -1)
        assert np.array_equal(match[o1[p]:o1[p + 1]], want) and cnt[p] == keep.sum(), p
        if keep.sum() >= (8 if model == "F" else 4):
            elig.append(p); A.append(K1[p][keep]); B.append(K2[p][want[keep]])
    assert len(elig) >= 3
    if model == "F":
        Mh, mh = pd.findFundamentalMatrixBatch(A, B, max_iters=20000, seeds=[seeds[p] for p in elig])
    else:
        Mh, mh = pd.findHomographyBatch(A, B, max_iters=20000, seeds=[seeds[p] for p in elig])
    for e, p in enumerate(elig):
        q = match[o1[p]:o1[p + 1]] >= 0
        assert np.array_equal(inl[o1[p]:o1[p + 1]][q], mh[e]), p
        if model == "F":
            assert np.array_equal(M[p], Mh[e]), p
        else:                      # inv() runs in numpy on the host path and in torch.linalg on the device path: same to rounding
            assert np.linalg.norm(M[p] - Mh[e]) <= 1e-9 * max(np.linalg.norm(Mh[e]), 1e-300), p
    # FGINN changes the tentatives of this scene, and None is the call without the keyword
    plain = _pipeline(K1, K2, D1, D2, **kw)
    none = _pipeline(K1, K2, D1, D2, fginn_th=None, **kw)
    cols = [0, 1, 3]                                                   # samples, LO runs, I: the other stats columns hold device ticks
    for k, (x, y) in enumerate(zip(plain, none)):
        assert np.array_equal(x[:, cols], y[:, cols]) if k == 3 else np.array_equal(x, y), k
    assert cnt.sum() > plain[4].sum()
    if guided and model == "F":                                         # the guided stage keeps its own gate and decision
        import torch
        gm = tensor_api.guided_match_batch_tensors(_t(np.concatenate(K1)), _t(np.concatenate(K2)), a, b, c1, c2, torch.from_numpy(M).to(a.device),
                                                   model="F", ratio=0.9, mutual=mutual)[0]
        assert np.array_equal(res[5], gm.cpu().numpy())


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("mutual", [False, True])
def test_single_pair_equals_the_batch_of_one(norm, mutual):
    a, b, kp2 = fr.twin_scene(90, 70, 130, _w(norm), norm, 20)
    q, t, d = matcher.match_fginn(a, b, kp2, 0.9, 10.0, mutual, norm)
    (gi, gd), = _run([a], [b], [kp2], 10.0, norm)
    keep = fr.keep(gi, gd, 0.9)
    if mutual:
        back = tensor_api.knn_match_tensors(_t(b), _t(a), norm)[0].cpu().numpy()
        keep &= back[np.clip(gi[:, 0], 0, None), 0] == np.arange(len(gi))
    assert np.array_equal(q, np.flatnonzero(keep)) and np.array_equal(t, gi[keep, 0]) and np.array_equal(_bits(d), _bits(gd[keep, 0]))
    assert len(q) >= 20


@pytest.mark.parametrize("norm", NORMS)
def test_second_stream_gives_the_same_bits(norm):
    import torch
    D1, D2, K2 = _twins(95, [(7, 30, 3), (130, 200, 65), (5, 70, 2)], _w(norm), norm)
    ref = _run(D1, D2, K2, 10.0, norm)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _run(D1, D2, K2, 10.0, norm)
    s.synchronize()
    for (ri, rd), (gi, gd) in zip(ref, got):
        assert np.array_equal(ri, gi) and np.array_equal(_bits(rd), _bits(gd))
