"""GPU: tracks = the connected components of exported matches (include/mi_degensac.h mi_degensac_tracks_dev / mi_degensac_tracks;
tensor_api.tracks_tensors, matcher.tracks).  Equality only: every output array is compared at full length, fills included, with
tests/tracks_ref.py, and the C entry point writes into slices of larger tensors whose guard elements must stay.  The shapes are the
smallest at which the passes can go wrong: node and edge counts around a wave, a workgroup's 256 threads and TRACK_ROWS positions, one
store that takes a second and third step of the boundary scan, long chains, one contended root, and the largest possible track count."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, tensor_api
from tests import tracks_ref as tr

pytestmark = pytest.mark.gpu
T, S = _lib.TRACK_ROWS, _lib.TRACK_SCAN
G, GUARD = 8, -77                                                       # guard elements on both sides of every output


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _sizes(R):
    import torch
    i32, i64 = torch.int32, torch.int64
    return dict(label=(R, i32), track=(R, i32), n_tracks=(1, i64), n_obs=(1, i64), track_offsets=(R // 2 + 1, i64), obs=(R, i32), obs_image=(R, i32),
                track_images=(R // 2, i32))


def _buffers(R):
    import torch
    return {k: torch.full((n + 2 * G,), GUARD, dtype=dt, device=_dev()) for k, (n, dt) in _sizes(R).items()}


def _raw(off, rows_t, M, total_t=None, nulls=(), bufs=None):
    """mi_degensac_tracks_dev on the current stream, every output a slice [G : G + n] of a tensor of n + 2 G guard values; returns the
    tensors"""
    import torch
    off = np.ascontiguousarray(off, np.int64)
    R = int(off[-1] - off[0])
    bufs = _buffers(R) if bufs is None else bufs
    p = {k: None if k in nulls else bufs[k].data_ptr() + G * bufs[k].element_size() for k in _sizes(R)}      # (also where n == 0)
    stream = torch.cuda.current_stream(_dev())
    rc = _lib.lib().mi_degensac_tracks_dev(off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1, None if rows_t is None else rows_t.data_ptr(), M,
                                           None if total_t is None else total_t.data_ptr(), 0, C.c_void_p(stream.cuda_stream), p["label"], p["track"],
                                           p["n_tracks"], p["n_obs"], p["track_offsets"], p["obs"], p["obs_image"], p["track_images"])
    _lib.check_match(rc)
    return bufs


def _read(bufs, R, nulls=()):
    """the outputs as numpy (None for those in nulls), after the guards were found untouched"""
    import torch
    torch.cuda.synchronize()
    out = {}
    for k, (n, _) in _sizes(R).items():
        a = bufs[k].cpu().numpy()
        assert (a[:G] == GUARD).all() and (a[G + n:] == GUARD).all(), k
        if k in nulls:
            assert (a == GUARD).all(), k
            out[k] = None
        else:
            out[k] = a[G:G + n]
    out["n_tracks"] = int(out["n_tracks"][0]); out["n_obs"] = int(out["n_obs"][0])
    return out


def _check(rows, off, total=None, nulls=(), rows_t=None, bufs=None):
    """the C entry point against the restatement; returns the restatement's result"""
    import torch
    rows = np.asarray(rows, np.int32).reshape(-1, 2)
    off = np.asarray(off, np.int64)
    R = int(off[-1] - off[0]); M = len(rows)
    if rows_t is None and M:
        rows_t = _t(rows)
    tt = None if total is None else torch.tensor([total], dtype=torch.int64, device=_dev())
    got = _read(_raw(off, rows_t, M, tt, nulls, bufs), R, nulls)
    want = tr.tracks(rows, off, total)
    assert tr.equal(got, want, [k for k in tr.NAMES if k not in nulls])
    return want


def _split(R, parts, rng):
    """R rows over `parts` images, some of them empty"""
    cuts = np.sort(rng.integers(0, R + 1, parts - 1)) if R else np.zeros(parts - 1, np.int64)
    c = np.diff(np.concatenate([[0], cuts, [R]])).astype(np.int64)
    if parts > 3:
        c[-1] += c[1]; c[1] = 0                                          # one image that is surely empty
    return c


def _random_edges(R, M, rng):
    return rng.integers(0, max(R, 1), (M, 2)).astype(np.int32)


# ---- node and edge counts ----
@pytest.mark.parametrize("R", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1])
def test_node_counts_at_the_edges_of_wave_workgroup_and_tile(R):
    rng = np.random.default_rng([1, R])
    off = tr.offsets(_split(R, 6, rng))
    want = _check(_random_edges(R, max(R // 3, 2), rng), off)
    if R >= 63:
        assert 0 < want["n_tracks"] and want["n_obs"] < R                 # tracks and nodes without one
    _check(np.zeros((0, 2), np.int32), off)                              # no edge at all


def test_a_store_that_takes_a_second_step_of_the_boundary_scan():
    """more than S workgroups with track starts in every one of them: pairs (2 i, 2 i + 1) over the whole store, every pair a track"""
    R = S * T + 2 * T + 3
    rng = np.random.default_rng(2)
    off = tr.offsets(_split(R, 40, rng))
    rows = np.arange(R - 1, dtype=np.int32).reshape(-1, 2)
    want = _check(rows[rng.permutation(len(rows))], off)
    assert want["n_tracks"] == R // 2 and want["n_obs"] == R - 1 and want["track"][-1] == -1


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1])
def test_edge_counts_at_the_edges_of_wave_and_workgroup(M):
    rng = np.random.default_rng([3, M])
    R = 700
    _check(_random_edges(R, M, rng), tr.offsets(_split(R, 5, rng)))


def test_more_edges_than_the_link_grid_has_threads():
    """the grid-stride loop of the link: 2048 workgroups of 256 threads and one more edge, over few nodes"""
    rng = np.random.default_rng(4)
    R = 900
    rows = rng.integers(0, R, (2048 * 256 + 1, 2)).astype(np.int32)
    rows[:, 1] = np.where(rng.random(len(rows)) < 0.999, rows[:, 0], rows[:, 1])    # nearly all self edges: many small tracks survive
    rows[-1] = (R - 2, R - 1)
    want = _check(rows, tr.offsets([400, 500]))
    assert want["label"][R - 1] <= R - 2 and 1 < want["n_tracks"]


# ---- contention and depth ----
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_path_over_4097_nodes(order):
    R = 4097
    rows = np.stack([np.arange(R - 1), np.arange(1, R)], axis=1).astype(np.int32)
    if order == "descending":
        rows = rows[::-1]                                                # builds the longest chains
    elif order == "shuffled":
        rows = rows[np.random.default_rng(5).permutation(R - 1)]
    want = _check(rows, tr.offsets([1000, 2000, 1097]))
    assert want["n_tracks"] == 1 and want["n_obs"] == R and want["track_images"][0] == 3 and (want["label"] == 0).all()


@pytest.mark.parametrize("centre", [0, 4096])
def test_a_star_with_4096_leaves(centre):
    """every edge hooks onto, or is hooked from, one word"""
    leaves = np.setdiff1d(np.arange(4097), [centre])
    rows = np.stack([np.full(4096, centre), leaves], axis=1).astype(np.int32)
    want = _check(rows, tr.offsets([4097]))
    assert want["n_tracks"] == 1 and (want["label"] == 0).all()
    _check(rows[:, ::-1], tr.offsets([2000, 0, 2097]))


def test_a_complete_bipartite_graph():
    a, b = np.meshgrid(np.arange(64), 64 + np.arange(64), indexing="ij")
    rows = np.stack([a.ravel(), b.ravel()], axis=1).astype(np.int32)
    want = _check(rows[np.random.default_rng(6).permutation(len(rows))], tr.offsets([64, 64]))
    assert want["n_tracks"] == 1 and want["n_obs"] == 128 and want["track_images"][0] == 2


def test_disjoint_pairs_fill_the_track_table():
    """n_tracks = R / 2, the bound of track_offsets and track_images"""
    R = 4096
    rng = np.random.default_rng(7)
    rows = np.stack([np.arange(2048), 2048 + rng.permutation(2048)], axis=1).astype(np.int32)
    want = _check(rows[rng.permutation(2048)], tr.offsets([2048, 2048]))
    assert want["n_tracks"] == R // 2 and (want["track_images"] == 2).all() and want["track_offsets"][-1] == R
    want = _check(rows[:, ::-1], tr.offsets([4095]))                     # odd R: node 4095 is no row, one pair fewer
    assert want["n_tracks"] == 2047 == 4095 // 2


def test_one_component_covers_everything_and_two_halves_meet_at_the_last_edge():
    rng = np.random.default_rng(8)
    R = 3000
    tree = np.stack([np.arange(1, R), [rng.integers(0, k) for k in range(1, R)]], axis=1)      # a random spanning tree
    rows = np.concatenate([tree, rng.integers(0, R, (R, 2))]).astype(np.int32)
    off = tr.offsets(_split(R, 7, rng))
    want = _check(rows[rng.permutation(len(rows))], off)
    assert want["n_tracks"] == 1 and want["n_obs"] == R
    h = R // 2
    left = np.stack([np.arange(1, h), [rng.integers(0, k) for k in range(1, h)]], axis=1)
    halves = np.concatenate([left, left + h])
    halves = halves[rng.permutation(len(halves))]
    want = _check(halves, off)
    assert want["n_tracks"] == 2 and want["track_offsets"][:3].tolist() == [0, h, R]
    want = _check(np.concatenate([halves, [[R - 1, 7]]]), off)
    assert want["n_tracks"] == 1 and (want["label"] == 0).all()


# ---- selection ----
def _mixed(seed, R=500, M=400):
    rng = np.random.default_rng(seed)
    return _random_edges(R, M, rng), tr.offsets(_split(R, 6, rng)), rng


def test_total_selects_a_prefix():
    rows, off, rng = _mixed(9)
    full = _check(rows, off)                                             # total None
    for total in (len(rows), len(rows) + 1, 1 << 40):
        assert tr.equal(_check(rows, off, total=total), full)
    cut = _check(rows, off, total=150)                                   # in-range edges behind total are not read as edges
    assert not tr.equal(cut, full) and tr.equal(cut, _check(rows[:150], off))
    for total in (0, -1, -(1 << 40)):
        assert _check(rows, off, total=total)["n_tracks"] == 0


def test_minus_one_and_rows_outside_the_store_drop_their_edge():
    rows, off, rng = _mixed(10)
    off = off + 1000                                                     # the store's first row is 1000
    rows = rows + 1000
    bad = rng.choice(np.array([-1, 0, 999, 1500, 1501, 0x7fffffff, -0x80000000], np.int64), len(rows)).astype(np.int32)
    where = rng.random(len(rows))
    rows[:, 0] = np.where(where < 0.2, bad, rows[:, 0])
    rows[:, 1] = np.where(where > 0.8, bad, rows[:, 1])
    rows[:7] = -1                                                        # the export's fill
    want = _check(rows, off)
    assert 0 < want["n_tracks"] and want["obs"][0] >= 1000
    assert tr.equal(want, tr.tracks(rows[((rows >= 1000) & (rows < 1500)).all(axis=1)], off))


def test_self_edges_repeats_and_column_order_change_nothing():
    rows, off, rng = _mixed(11)
    want = _check(rows, off)
    nodes = np.arange(500, dtype=np.int32)
    assert tr.equal(_check(np.concatenate([np.stack([nodes, nodes], axis=1), rows]), off), want)
    assert tr.equal(_check(np.repeat(rows, 3, axis=0), off), want)
    assert tr.equal(_check(np.tile(rows, (3, 1)), off), want)
    assert tr.equal(_check(rows[:, ::-1], off), want)
    only_self = _check(np.stack([nodes, nodes], axis=1), off)
    assert only_self["n_tracks"] == 0 and (only_self["track"] == -1).all()


# ---- store layout ----
@pytest.mark.parametrize("first", [1, 5, 1027, 0x7fffffff - 700])
def test_a_store_whose_first_row_is_not_zero(first):
    rows, off, rng = _mixed(12, R=700, M=500)
    want = _check(rows.astype(np.int64) + first, off + first)
    base = tr.tracks(rows, off)
    assert np.array_equal(want["label"], base["label"]) and np.array_equal(want["obs_image"], base["obs_image"])
    assert np.array_equal(want["obs"][:want["n_obs"]].astype(np.int64), base["obs"][:base["n_obs"]].astype(np.int64) + first)


def test_empty_images_at_the_start_at_the_end_and_in_runs():
    counts = [0, 0, 7, 0, 0, 0, 1, 5, 0, 1, 0, 0]
    off = tr.offsets(counts)
    rng = np.random.default_rng(13)
    want = _check(_random_edges(14, 9, rng), off)
    n = want["n_obs"]
    assert n > 4 and set(want["obs_image"][:n].tolist()) <= {2, 6, 7, 9}
    assert np.array_equal(want["obs_image"][:n], tr.image_of(off, want["obs"][:n]))
    _check(np.array([[6, 7], [7, 12], [12, 13]], np.int32), off)         # one track over the images 2, 6, 7, 9 in one row each


def test_two_keypoints_of_one_image_in_a_track():
    off = tr.offsets([4, 4, 4])
    want = _check(np.array([[0, 4], [4, 8], [8, 1], [2, 6], [5, 9]], np.int32), off)
    assert want["n_tracks"] == 3
    length = np.diff(want["track_offsets"][:4])
    assert length.tolist() == [4, 2, 2] and want["track_images"][:3].tolist() == [3, 2, 2]       # track 0 holds rows 0 and 1 of image 0


def test_rows_that_are_4_byte_but_not_8_byte_aligned():
    import torch
    rows, off, rng = _mixed(14, R=1500, M=1300)
    flat = torch.zeros(2 * len(rows) + 1, dtype=torch.int32, device=_dev())
    flat[1:] = _t(rows).reshape(-1)
    view = flat[1:].view(len(rows), 2)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    want = _check(rows, off, rows_t=view)
    out = tensor_api.tracks_tensors(view, np.diff(off), with_label=True)
    assert np.array_equal(out[-1].cpu().numpy(), want["label"]) and np.array_equal(out[3].cpu().numpy(), want["obs"])


# ---- calling forms ----
def _as_dict(out):
    track, nt, to, obs, oi, ti, no, label = (x.cpu().numpy() for x in out)
    return {"label": label, "track": track, "n_tracks": int(nt[0]), "n_obs": int(no[0]), "track_offsets": to, "obs": obs, "obs_image": oi,
            "track_images": ti}


def test_tensor_entry_point_and_a_second_stream():
    import torch
    rows, off, rng = _mixed(15, R=2 * T + 5, M=2000)
    counts = np.diff(off)
    want = tr.tracks(rows, off)
    tr_rows = _t(rows)
    assert tr.equal(_as_dict(tensor_api.tracks_tensors(tr_rows, counts, with_label=True)), want)
    assert len(tensor_api.tracks_tensors(tr_rows, counts)) == 7
    total = torch.tensor([700], dtype=torch.int64, device=_dev())
    s = torch.cuda.Stream(device=_dev())
    s.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(s):
        out = tensor_api.tracks_tensors(tr_rows, counts, total=total, with_label=True)
        again = tensor_api.tracks_tensors(tr_rows, counts, with_label=True)
    s.synchronize()
    assert tr.equal(_as_dict(out), tr.tracks(rows, off, total=700)) and tr.equal(_as_dict(again), want)
    empty = tensor_api.tracks_tensors(torch.zeros((0, 2), dtype=torch.int32, device=_dev()), counts, with_label=True)
    assert tr.equal(_as_dict(empty), tr.tracks(rows[:0], off))
    none = tensor_api.tracks_tensors(tr_rows, [0, 0], with_label=True)
    assert tr.equal(_as_dict(none), tr.tracks(rows, [0, 0, 0]))


def test_numpy_entry_point():
    rows, off, rng = _mixed(16, R=T + 300, M=900)
    counts = np.diff(off)
    want = tr.tracks(rows, off)
    nt, no = want["n_tracks"], want["n_obs"]
    for total, w in ((None, want), (-1, want), (300, tr.tracks(rows, off, total=300))):
        got = matcher.tracks(rows, counts, total=total)
        nt, no = w["n_tracks"], w["n_obs"]
        assert (got["n_tracks"], got["n_obs"]) == (nt, no)
        assert np.array_equal(got["label"], w["label"]) and np.array_equal(got["track"], w["track"])
        assert np.array_equal(got["track_offsets"], w["track_offsets"][:nt + 1]) and np.array_equal(got["obs"], w["obs"][:no])
        assert np.array_equal(got["obs_image"], w["obs_image"][:no]) and np.array_equal(got["track_images"], w["track_images"][:nt])
    got = matcher.tracks(np.zeros((0, 2), np.int32), counts)
    assert got["n_tracks"] == 0 and len(got["obs"]) == 0 and got["track_offsets"].tolist() == [0]
    got = matcher.tracks(rows, [])
    assert got["n_tracks"] == 0 and len(got["label"]) == 0 and got["track_offsets"].tolist() == [0]


def test_host_form_without_optional_outputs_equals_the_device_form():
    """mi_degensac_tracks with label, obs, obs_image and track_images NULL, on 3 images with one empty: what it writes is what the device
    form writes on the same inputs, bit for bit (fills included), and the device form itself equals the restatement"""
    off = np.array([0, 4, 4, 9], np.int64)
    rows = np.array([[0, 5], [5, 8], [1, 6], [3, 3], [2, -1]], np.int32)
    R, M, nulls = 9, 5, ("label", "obs", "obs_image", "track_images")
    dev = _read(_raw(off, _t(rows), M, None, nulls), R, nulls)
    assert tr.equal(dev, tr.tracks(rows, off), [k for k in tr.NAMES if k not in nulls]) and dev["n_tracks"] == 2
    track = np.full(R, GUARD, np.int32); to = np.full(R // 2 + 1, GUARD, np.int64); n = np.full(2, GUARD, np.int64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)          # noqa: E731
    _lib.check_match(_lib.lib().mi_degensac_tracks(off.ctypes.data_as(C.POINTER(C.c_int64)), 3, vp(rows), M, -1, 0, None, vp(track), vp(n[0:]),
                                                   vp(n[1:]), vp(to), None, None, None))
    assert (int(n[0]), int(n[1])) == (dev["n_tracks"], dev["n_obs"])
    assert np.array_equal(track, dev["track"]) and np.array_equal(to, dev["track_offsets"])


def test_reused_output_buffers_are_overwritten_down_to_the_fills():
    rows, off, rng = _mixed(17, R=1200, M=500)
    R = 1200
    bufs = _buffers(R)
    many = _check(rows, off, bufs=bufs)
    few = _check(rows[:40], off, bufs=bufs)                              # the same tensors: fewer tracks, longer tails
    assert few["n_obs"] < many["n_obs"] and few["n_tracks"] < many["n_tracks"]
    _check(rows[:0], off, bufs=bufs)
    assert tr.equal(_check(rows, off, bufs=bufs), many)


@pytest.mark.parametrize("nulls", [("label",), ("obs_image",), ("track_images",), ("obs_image", "track_images"),
                                   ("label", "obs", "obs_image", "track_images")], ids=repr)
def test_nullable_outputs_given_as_null(nulls):
    rows, off, rng = _mixed(18, R=T + 77, M=800)
    _check(rows, off, nulls=nulls)
    _check(rows, off, total=100, nulls=nulls)


# ---- end to end ----
def _pipeline(kps, descs, pairs):
    """match and verify (F), export the inliers as store rows, build the tracks: no host synchronisation in between"""
    counts = [len(d) for d in descs]
    tk, td = _t(np.concatenate(kps)), _t(np.concatenate(descs))
    F, match, inlier, stats, nten, po = tensor_api.match_and_verify_pairs_tensors(tk, tk, td, td, counts, counts, pairs, model="F")
    rows, co, total = tensor_api.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inlier, store_rows=True)[:3]
    out = tensor_api.tracks_tensors(rows, counts, total=total, with_label=True)
    return counts, rows.cpu().numpy(), int(total[0]), _as_dict(out)


def test_a_collection_from_descriptors_to_tracks():
    from pydegensac_amd import synthetic
    kps, descs = synthetic.image_collection(6, 300, 0.6, 0.1, 32, seed=0)
    counts, rows, total, got = _pipeline(kps, descs, matcher.exhaustive_pairs(6))
    assert total > 500 and (rows[total:] == -1).all()
    want = tr.tracks(rows, tr.offsets(counts), total)                    # the restatement on the device's own rows
    assert tr.equal(got, want) and want["n_tracks"] > 100
    assert tr.equal(got, tr.tracks(rows, tr.offsets(counts)))            # the -1 fill behind total is no edge either
    lengths = np.diff(want["track_offsets"][:want["n_tracks"] + 1])
    assert lengths.min() >= 2 and lengths.max() >= 4


def test_a_scene_where_every_point_is_seen_in_every_image():
    """exact projections and identical descriptors: the tracks are the points.  The point of a keypoint is read from its descriptor (the
    row of image 0 with the same bytes), not from any matching code."""
    from pydegensac_amd import synthetic
    m, n = 4, 120
    kps, descs = synthetic.image_collection(m, n, 1.0, 0.0, 32, seed=3, desc_sigma=0.0)
    counts, rows, total, got = _pipeline(kps, descs, matcher.exhaustive_pairs(m))
    row_of = {descs[0][r].tobytes(): r for r in range(n)}
    point = np.array([[row_of[descs[i][r].tobytes()] for r in range(n)] for i in range(m)])     # [image, row] -> its row in image 0
    assert got["n_tracks"] == n and got["n_obs"] == m * n and (got["track_images"][:n] == m).all()
    assert np.array_equal(got["track"], point.reshape(-1))               # tracks are numbered by their smallest row = the row in image 0
    assert np.array_equal(got["track_offsets"][:n + 1], m * np.arange(n + 1))
    members = got["obs"][:m * n].reshape(n, m)
    for t in (0, 1, n // 2, n - 1):
        assert members[t].tolist() == [i * n + int(np.flatnonzero(point[i] == t)[0]) for i in range(m)]
    assert tr.equal(got, tr.tracks(rows, tr.offsets(counts), total))


# ---- determinism ----
def test_twenty_calls_give_identical_bytes():
    import torch
    R = 4097
    rng = np.random.default_rng(19)
    path = np.stack([np.arange(R - 1), np.arange(1, R)], axis=1).astype(np.int32)[rng.permutation(R - 1)]
    star = np.stack([np.full(R - 1, R - 1), np.arange(R - 1)], axis=1).astype(np.int32)
    counts = [1000, 2000, 1097]
    for rows in (path, star):
        t = _t(rows)
        want = tr.tracks(rows, tr.offsets(counts))
        outs = [tensor_api.tracks_tensors(t, counts, with_label=True) for _ in range(20)]
        torch.cuda.synchronize()
        first = [x.cpu().numpy().tobytes() for x in outs[0]]
        assert tr.equal(_as_dict(outs[0]), want)
        for out in outs[1:]:
            assert [x.cpu().numpy().tobytes() for x in out] == first
