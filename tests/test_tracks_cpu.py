"""The tracks call without a device (include/mi_degensac.h mi_degensac_tracks_dev / mi_degensac_tracks, matcher.tracks,
tensor_api.tracks_tensors): every refusal of both C entry points with its message and in its order (each comes back as EINVAL, not
ENODEV, on a machine without a device: it came before a device was looked for), the Python keyword and shape checks, and the restatement
tests/tracks_ref.py on tables written by hand, which also reject three broken restatements."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import tracks_ref as tr

EINVAL = -1
NAMES = ("tracks_dev", "tracks")
OUTS = ("label", "track", "n_tracks", "n_obs", "track_offsets", "obs", "obs_image", "track_images")


def _abi(which, off=(0, 3, 3, 5, 9), n_images=None, n_edges=4, null=(), misalign=0):
    """(rc, message) of one entry point.  Data pointers hold an address (never read: every call here is refused first) unless named in
    `null`; misalign is added to the address of rows."""
    L = _lib.lib(); lp = C.POINTER(C.c_int64)
    o = np.asarray(off, np.int64)
    buf = np.zeros(64); addr = buf.ctypes.data
    P = lambda name: None if name in null else addr          # noqa: E731
    rows = None if "rows" in null else addr + misalign
    outs = tuple(P(n) for n in OUTS)
    op = None if "offsets" in null else o.ctypes.data_as(lp)
    n = len(o) - 1 if n_images is None else n_images
    if which == "tracks_dev":
        rc = L.mi_degensac_tracks_dev(op, n, rows, n_edges, P("total"), 0, None, *outs)
    else:
        rc = L.mi_degensac_tracks(op, n, rows, n_edges, -1, 0, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(msg_part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and msg_part in msg, (which, rc, msg)


def test_the_tile_constants_are_mirrored():
    L = _lib.lib()
    assert L.mi_degensac_tracks_tile(0) == _lib.TRACK_ROWS and L.mi_degensac_tracks_tile(1) == _lib.TRACK_SCAN
    assert L.mi_degensac_tracks_tile(2) == -1


# ---- the refusals, one by one ----
def test_negative_n_images():
    _refused(b"n_images", n_images=-1)
    _refused(b"n_images", n_images=-(1 << 31))


def test_null_offsets():
    _refused(b"NULL argument: offsets", null=("offsets",))
    _refused(b"NULL argument: offsets", null=("offsets",), n_images=0)


@pytest.mark.parametrize("off", [(0, 6, 4), (-1, 3, 7), (-5, -2), (3, 2), (0, 5, 5, 4)], ids=repr)
def test_decreasing_or_negative_offsets(off):
    _refused(b"non-decreasing", off=off)


@pytest.mark.parametrize("off", [(0, 0x80000000), (0x7ffffff0, 0x7ffffff8, 0x80000008), (0x80000000,)], ids=repr)
def test_offsets_beyond_int32(off):
    _refused(b"int32", off=off)


def test_the_last_int32_row_is_accepted_as_an_offset():
    _refused(b"always written", off=(0x7ffffff0, 0x7fffffff), null=("track",))      # a valid store as far as the pointer check


@pytest.mark.parametrize("n_edges", [-1, 0x40000000, -(1 << 40), 1 << 40])
def test_edge_counts_out_of_range(n_edges):
    _refused(b"n_edges", n_edges=n_edges)


def test_null_rows_only_with_edges():
    _refused(b"rows of a list", null=("rows",))
    _refused(b"always written", null=("rows", "n_obs"), n_edges=0)     # no edges: rows may be NULL, the next defect answers


@pytest.mark.parametrize("name", ["track", "n_tracks", "n_obs", "track_offsets"])
def test_the_four_outputs_that_are_always_written(name):
    _refused(b"always written", null=(name,))


def test_optional_outputs():
    _refused(b"need obs", null=("obs",))
    _refused(b"need obs", null=("obs", "obs_image"))
    _refused(b"need obs", null=("obs", "track_images"))
    # label, total, and all three grouped outputs together are optional: the next defect answers
    _refused(b"aligned", null=("label", "total", "obs", "obs_image", "track_images"), misalign=2)
    _refused(b"aligned", null=("obs_image",), misalign=1)
    _refused(b"aligned", null=("track_images",), misalign=3)


@pytest.mark.parametrize("misalign", [1, 2, 3, 5, 6, 7])
def test_rows_must_be_4_byte_aligned(misalign):
    _refused(b"aligned", misalign=misalign)


# ---- the order: of two defects the earlier one answers ----
@pytest.mark.parametrize("first,kw", [
    (b"n_images", dict(n_images=-1, null=("offsets",))),
    (b"NULL argument: offsets", dict(null=("offsets",), n_edges=-1)),
    (b"non-decreasing", dict(off=(0, 6, 4), n_edges=-1)),
    (b"non-decreasing", dict(off=(0, 0x80000000, 4))),
    (b"int32", dict(off=(0, 0x80000000), n_edges=0x40000000)),
    (b"n_edges", dict(n_edges=-1, null=("rows",))),
    (b"rows of a list", dict(null=("rows", "track"))),
    (b"always written", dict(null=("n_tracks", "obs"))),
    (b"need obs", dict(null=("obs",), misalign=2)),
], ids=lambda x: x.decode() if isinstance(x, bytes) else "")
def test_the_order_of_the_refusals(first, kw):
    _refused(first, **kw)


# ---- the Python keyword and shape checks ----
COUNTS = [3, 0, 2, 4]                                                  # offsets 0 3 3 5 9: image 1 is empty
OFF = tr.offsets(COUNTS)


def test_good_arguments():
    off, R, M = matcher.check_tracks_args((5, 2), np.int32, COUNTS)
    assert off.tolist() == [0, 3, 3, 5, 9] and off.dtype == np.int64 and (R, M) == (9, 5)
    assert matcher.check_tracks_args((0, 2), "torch.int32", [], None)[1:] == (0, 0)
    assert matcher.check_tracks_args((1, 2), np.int32, np.zeros(3, np.int64), total=-1)[1:] == (0, 1)


@pytest.mark.parametrize("kw,msg", [
    (dict(rows_shape=(5,)), "rows"), (dict(rows_shape=(5, 3)), "rows"), (dict(rows_shape=(2, 5)), "rows"), (dict(rows_shape=(5, 2, 1)), "rows"),
    (dict(rows_dtype=np.int64), "rows"), (dict(rows_dtype=np.uint32), "rows"), (dict(rows_dtype=np.float32), "rows"),
    (dict(rows_shape=(0x40000000, 2)), "too many edges"),
    (dict(counts=[3, -1]), "counts"), (dict(counts=[[3, 0], [2, 4]]), "counts"), (dict(counts=[3.0, 1.0]), "counts"), (dict(counts=7), "counts"),
    (dict(counts=[0x7fffffff, 1]), "too many rows"),
    (dict(total=2.0), "total"), (dict(total=True), "total"), (dict(total="3"), "total"),
], ids=repr)
def test_keyword_defects(kw, msg):
    a = dict(rows_shape=(5, 2), rows_dtype=np.int32, counts=COUNTS)
    a.update(kw)
    with pytest.raises(ValueError, match=msg):
        matcher.check_tracks_args(**a)


def test_numpy_entry_point_checks_before_the_device():
    rows = np.zeros((4, 2), np.int32)
    with pytest.raises(ValueError, match="rows"):
        matcher.tracks(rows.astype(np.int64), COUNTS)
    with pytest.raises(ValueError, match="rows"):
        matcher.tracks(rows.reshape(-1), COUNTS)
    with pytest.raises(ValueError, match="counts"):
        matcher.tracks(rows, [3, -1])
    with pytest.raises(ValueError, match="total"):
        matcher.tracks(rows, COUNTS, total=1.5)


def test_tensor_form_checks_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    rows = torch.zeros((4, 2), dtype=torch.int32)
    call = tensor_api.tracks_tensors
    with pytest.raises(ValueError, match="torch tensors"):
        call(rows.numpy(), COUNTS)
    with pytest.raises(ValueError, match="torch tensors"):
        call(rows, COUNTS, total=4)
    with pytest.raises(ValueError, match="rows"):
        call(rows.long(), COUNTS)
    with pytest.raises(ValueError, match="rows"):
        call(rows.reshape(-1), COUNTS)
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros((4, 4), dtype=torch.int32)[:, :2], COUNTS)
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros((2, 4), dtype=torch.int32).t()[:, :2], COUNTS)
    with pytest.raises(ValueError, match="counts"):
        call(rows, [3, -1])
    with pytest.raises(ValueError, match="total"):
        call(rows, COUNTS, total=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="total"):
        call(rows, COUNTS, total=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="ROCm device"):                # valid arguments, but not on a ROCm device
        call(rows, COUNTS, total=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError):
        call(rows, COUNTS, None, False, 0)                              # no fifth argument


# ---- the restatement on tables written by hand: R = 9 nodes, R / 2 = 4 ----
F = -1
ID = list(range(9))
TABLES = {
    # a path 0 - 1 - 2 - 3 across images 0 and 2, its edges out of order
    "path": dict(rows=[(2, 3), (0, 1), (1, 2)], label=[0, 0, 0, 0, 4, 5, 6, 7, 8], track=[0, 0, 0, 0, F, F, F, F, F], n_tracks=1, n_obs=4,
                 track_offsets=[0, 4, 4, 4, 4], obs=[0, 1, 2, 3, F, F, F, F, F], obs_image=[0, 0, 0, 2, F, F, F, F, F], track_images=[2, F, F, F]),
    # a star around 5 with leaves 1, 8, 3: images 0, 2, 3, 3
    "star": dict(rows=[(5, 1), (8, 5), (5, 3)], label=[0, 1, 2, 1, 4, 1, 6, 7, 1], track=[F, 0, F, 0, F, 0, F, F, 0], n_tracks=1, n_obs=4,
                 track_offsets=[0, 4, 4, 4, 4], obs=[1, 3, 5, 8, F, F, F, F, F], obs_image=[0, 2, 3, 3, F, F, F, F, F], track_images=[3, F, F, F]),
    # {0, 4} and {2, 7} and {6, 8}; the last edge merges the first two
    "merge": dict(rows=[(4, 0), (7, 2), (6, 8), (4, 7)], label=[0, 1, 0, 3, 0, 5, 6, 0, 6], track=[0, F, 0, F, 0, F, 1, 0, 1], n_tracks=2, n_obs=6,
                  track_offsets=[0, 4, 6, 6, 6], obs=[0, 2, 4, 7, 6, 8, F, F, F], obs_image=[0, 0, 2, 3, 3, 3, F, F, F], track_images=[3, 1, F, F]),
    "unmerged": dict(rows=[(4, 0), (7, 2), (6, 8)], label=[0, 1, 2, 3, 0, 5, 6, 2, 6], track=[0, F, 1, F, 0, F, 2, 1, 2], n_tracks=3, n_obs=6,
                     track_offsets=[0, 2, 4, 6, 6], obs=[0, 4, 2, 7, 6, 8, F, F, F], obs_image=[0, 2, 0, 3, 3, 3, F, F, F], track_images=[2, 2, 1, F]),
    "self": dict(rows=[(3, 3), (0, 0), (8, 8)], label=ID, track=[F] * 9, n_tracks=0, n_obs=0, track_offsets=[0] * 5, obs=[F] * 9, obs_image=[F] * 9,
                 track_images=[F] * 4),
    "duplicates": dict(rows=[(1, 2), (1, 2), (2, 1), (1, 2)], label=[0, 1, 1, 3, 4, 5, 6, 7, 8], track=[F, 0, 0, F, F, F, F, F, F], n_tracks=1, n_obs=2,
                       track_offsets=[0, 2, 2, 2, 2], obs=[1, 2, F, F, F, F, F, F, F], obs_image=[0, 0, F, F, F, F, F, F, F], track_images=[1, F, F, F]),
    "minus_one": dict(rows=[(-1, 2), (3, -1), (5, 4), (-1, -1)], label=[0, 1, 2, 3, 4, 4, 6, 7, 8], track=[F, F, F, F, 0, 0, F, F, F], n_tracks=1, n_obs=2,
                      track_offsets=[0, 2, 2, 2, 2], obs=[4, 5, F, F, F, F, F, F, F], obs_image=[2, 3, F, F, F, F, F, F, F], track_images=[2, F, F, F]),
    # 9 = offsets[n_images] is no row
    "the_end": dict(rows=[(9, 0), (0, 9), (7, 8), (1 << 30, 3)], label=[0, 1, 2, 3, 4, 5, 6, 7, 7], track=[F, F, F, F, F, F, F, 0, 0], n_tracks=1, n_obs=2,
                    track_offsets=[0, 2, 2, 2, 2], obs=[7, 8, F, F, F, F, F, F, F], obs_image=[3, 3, F, F, F, F, F, F, F], track_images=[1, F, F, F]),
    "empty": dict(rows=[], label=ID, track=[F] * 9, n_tracks=0, n_obs=0, track_offsets=[0] * 5, obs=[F] * 9, obs_image=[F] * 9, track_images=[F] * 4),
}


def _rows(t):
    return np.asarray(t["rows"], np.int32).reshape(-1, 2)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_restatement_on_the_tables(name):
    t = TABLES[name]
    got = tr.tracks(_rows(t), OFF)
    assert tr.equal(got, t), got
    assert got["label"].dtype == np.int32 and got["track_offsets"].dtype == np.int64 and got["obs"].dtype == np.int32


def test_restatement_total_cuts_the_list():
    t = TABLES["merge"]
    assert tr.equal(tr.tracks(_rows(t), OFF, total=3), TABLES["unmerged"])
    assert tr.equal(tr.tracks(_rows(t), OFF, total=4), t) and tr.equal(tr.tracks(_rows(t), OFF, total=99), t)
    assert tr.equal(tr.tracks(_rows(t), OFF, total=0), TABLES["empty"]) and tr.equal(tr.tracks(_rows(t), OFF, total=-2), TABLES["empty"])


def test_restatement_with_a_first_offset():
    """node k is row offsets[0] + k: the tables shifted by 2, with the rows below the store ignored like those beyond it"""
    off = OFF + 2
    t = TABLES["merge"]
    rows = np.concatenate([_rows(t) + 2, [[1, 4], [0, 1], [11, 3]]]).astype(np.int32)
    got = tr.tracks(rows, off)
    assert got["obs"][:6].tolist() == [2, 4, 6, 9, 8, 10] and got["label"].tolist() == t["label"] and got["obs_image"].tolist() == t["obs_image"]
    assert got["track"].tolist() == t["track"] and got["track_images"].tolist() == t["track_images"]


def test_restatement_on_no_nodes():
    got = tr.tracks(np.zeros((2, 2), np.int32), np.array([5, 5, 5], np.int64))
    assert got["n_tracks"] == 0 and got["n_obs"] == 0 and got["track_offsets"].tolist() == [0]
    assert all(len(got[k]) == 0 for k in ("label", "track", "obs", "obs_image", "track_images"))


def test_image_of_skips_empty_images():
    off = np.array([0, 0, 0, 2, 2, 5, 5], np.int64)                    # images 2 and 4 own the rows
    assert tr.image_of(off, [0, 1, 2, 3, 4]).tolist() == [2, 2, 4, 4, 4]


@pytest.mark.parametrize("seed", range(5))
def test_restatement_does_not_depend_on_edge_order_or_column_order(seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 12, 9)
    off = tr.offsets(counts, first=int(rng.integers(0, 4)))
    R = int(off[-1] - off[0])
    rows = rng.integers(off[0] - 1, off[-1] + 1, (R // 2, 2)).astype(np.int32)
    want = tr.tracks(rows, off)
    assert 0 < want["n_tracks"] and want["n_obs"] < R
    shuffled = rows[rng.permutation(len(rows))]
    swap = rng.random(len(rows)) < 0.5
    shuffled[swap] = shuffled[swap][:, ::-1]
    assert tr.equal(tr.tracks(shuffled, off), want)
    assert tr.equal(tr.tracks(rows[:, ::-1], off), want)


# ---- three broken restatements, each rejected by the tables ----
def _broken_root_is_max(rows, off):
    label = tr.labels(rows, off)
    top = np.zeros(len(label), np.int32)
    np.maximum.at(top, label, np.arange(len(label), dtype=np.int32))
    return tr.group(top[label], off)


def _broken_members_unsorted(rows, off):
    got = tr.tracks(rows, off)
    for t in range(got["n_tracks"]):
        a, b = got["track_offsets"][t], got["track_offsets"][t] + np.count_nonzero(got["track"] == t)
        got["obs"][a:b] = got["obs"][a:b][::-1]
        got["obs_image"][a:b] = got["obs_image"][a:b][::-1]
    return got


def _broken_singletons_are_tracks(rows, off):
    got = tr.tracks(rows, off)
    roots = np.flatnonzero(got["label"] == np.arange(len(got["label"])))
    number = np.zeros(len(got["label"]), np.int32); number[roots] = np.arange(len(roots))
    got["track"] = number[got["label"]]
    got["n_tracks"] = len(roots); got["n_obs"] = len(got["label"])
    return got


@pytest.mark.parametrize("broken", [_broken_root_is_max, _broken_members_unsorted, _broken_singletons_are_tracks])
@pytest.mark.parametrize("name", ["path", "star", "merge", "duplicates", "minus_one", "the_end"])
def test_broken_restatements_are_rejected_by_the_tables(broken, name):
    t = TABLES[name]
    assert not tr.equal(broken(_rows(t), OFF), t)
