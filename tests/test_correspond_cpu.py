"""The correspondence export without a device (include/mi_degensac.h mi_degensac_correspondences_*, matcher.correspondences_pairs / _batch,
tensor_api.correspondences_*_tensors): every refusal of the four C entry points with its message and in its order (each comes back as
EINVAL, not ENODEV, on a machine without a device: it came before a device was looked for), n_pairs == 0, the Python keyword checks, and
the numpy restatement tests/correspond_ref.py on hand-written tables, which also reject three broken restatements."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import correspond_ref as cr

EINVAL = -1
NAMES = ("pairs_dev", "batch_dev", "pairs", "batch")


def _abi(which, pairs=((0, 1),), off1=(0, 4, 10), off2=(0, 3, 7), n_pairs=None, flags=0, kp_dim=2, gp="default", capacity=8, m1=None, m2=None,
         null=(), want=("rows",)):
    """(rc, message) of one entry point.  Data pointers hold an address (never read: every call here is refused first) unless named in
    `null`; of the optional outputs only those in `want` are given.  The batch forms take off1 / off2 as their [K + 1] offsets."""
    L = _lib.lib(); lp = C.POINTER(C.c_int64); ip = C.POINTER(C.c_int32)
    o1 = np.asarray(off1, np.int64); o2 = np.asarray(off2, np.int64); pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    buf = np.zeros(64); addr = buf.ctypes.data

    def P(name, optional=False):
        if name in null or (optional and name not in want):
            return None
        return addr
    if gp == "default":
        gp = _lib.GuideParams(0, 0, 0.5)
    gpp = None if gp is None else C.byref(gp)
    if which.startswith("pairs"):
        n = len(pr) if n_pairs is None else n_pairs
        lay = (o1.ctypes.data_as(lp), len(o1) - 1 if m1 is None else m1, o2.ctypes.data_as(lp), len(o2) - 1 if m2 is None else m2,
               pr.ctypes.data_as(ip), n)
    else:
        n = len(o1) - 1 if n_pairs is None else n_pairs
        lay = (o1.ctypes.data_as(lp) if "off1" not in null else None, o2.ctypes.data_as(lp) if "off2" not in null else None, n)
    mid = (P("match"), P("keep", True), flags, P("kp1"), P("kp2"), kp_dim, P("models"), gpp, capacity, 0)
    outs = (P("corr_offsets"), P("total"), P("rows"), P("entry", True), P("pts", True), P("resid", True))
    f = getattr(L, f"mi_degensac_correspondences_{which}")
    rc = f(*lay, *mid, None, *outs) if which.endswith("_dev") else f(*lay, *mid, *outs)
    return rc, L.mi_degensac_match_last_error()


def _refused(msg_part, **kw):
    for which in NAMES:
        rc, msg = _abi(which, **kw)
        assert rc == EINVAL and msg_part in msg, (which, rc, msg)


def test_the_tile_constants_are_mirrored():
    L = _lib.lib()
    assert L.mi_degensac_correspondences_tile(0) == _lib.CORR_ROWS and L.mi_degensac_correspondences_tile(1) == _lib.CORR_SCAN
    assert L.mi_degensac_correspondences_tile(2) == -1
    assert _lib.CORR_ROWS % 256 == 0 and _lib.CORR_SCAN % 64 == 0


# ---- the refusals, one by one ----
@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xfffffffe])
def test_unknown_flag_bits(flags):
    _refused(b"flags", flags=flags)
    _refused(b"flags", flags=flags, n_pairs=0)


@pytest.mark.parametrize("kp_dim", [0, 3, 4, -2])
@pytest.mark.parametrize("want", [("pts",), ("resid",), ("pts", "resid")])
def test_keypoint_width_when_points_or_residuals_are_asked_for(kp_dim, want):
    _refused(b"keypoint rows", kp_dim=kp_dim, want=want)
    _refused(b"keypoint rows", kp_dim=kp_dim, want=want, n_pairs=0)


def test_keypoint_width_is_not_read_without_points_and_residuals():
    _refused(b"NULL", kp_dim=3, null=("match",))                       # a valid call as far as the pointer check


def test_residuals_need_models_and_guide_params():
    _refused(b"models", want=("resid",), null=("models",))
    _refused(b"guide params", want=("resid",), gp=None)
    _refused(b"NULL", gp=None, null=("models", "match"))               # neither is needed without resid
    gp = _lib.GuideParams(0, 0, 0.5); gp.struct_size = 8
    _refused(b"struct_size", want=("resid",), gp=gp)
    gp = _lib.GuideParams(0, 0, 0.5); gp.homography = 2
    _refused(b"homography", want=("resid",), gp=gp)
    for g in (_lib.GuideParams(0, 2, 0.5), _lib.GuideParams(0, -1, 0.5), _lib.GuideParams(1, 5, 0.5), _lib.GuideParams(1, -1, 0.5)):
        _refused(b"error_type", want=("resid",), gp=g)
        _refused(b"error_type", want=("resid",), gp=g, n_pairs=0)


@pytest.mark.parametrize("px", [-1.0, float("nan"), float("inf")])
def test_px_th_is_not_read(px):
    _refused(b"NULL", want=("resid",), gp=_lib.GuideParams(1, 3, px), null=("match",))


def test_negative_capacity_and_negative_n_pairs():
    _refused(b"capacity", capacity=-1)
    _refused(b"capacity", capacity=-(1 << 40), n_pairs=0)
    _refused(b"n_pairs", n_pairs=-1)


@pytest.mark.parametrize("case", [
    dict(pairs=[(0, 2)]), dict(pairs=[(2, 0)]), dict(pairs=[(0, 1), (-1, 0)]), dict(pairs=[(0, -1)]), dict(pairs=[(0, 0)], m1=0),
    dict(off1=(0, 6, 4)), dict(off2=(0, 8, 7)), dict(off2=(-1, 3, 7)), dict(off1=(-2, 4, 10)),
    dict(off1=(0, 0x3fffffff), off2=(0, 1), pairs=[(0, 0), (0, 0)]),
    dict(off1=(0, 1), off2=(0, 0x3fffffff), pairs=[(0, 0), (0, 0)]),
], ids=repr)
def test_pair_lists_the_layout_refuses(case):
    for which in ("pairs_dev", "pairs"):
        rc, msg = _abi(which, **case)
        assert rc == EINVAL and msg, which


@pytest.mark.parametrize("case", [
    dict(off1=(0, 6, 4)), dict(off2=(0, 8, 7)), dict(off2=(-1, 3, 7)), dict(off1=(-2, 4, 10)), dict(null=("off1",)), dict(null=("off2",)),
    dict(off1=(0, 0x40000000, 0x40000001)), dict(off2=(5, 5, 0x40000006)),
], ids=repr)
def test_batches_the_layout_refuses(case):
    for which in ("batch_dev", "batch"):
        rc, msg = _abi(which, **case)
        assert rc == EINVAL and (b"offsets" in msg or b"too many" in msg), which


def test_store_rows_must_fit_int32():
    far = (0x7ffffff0, 0x7ffffff8, 0x80000008)                         # 24 rows whose last store row is beyond int32
    _refused(b"int32", flags=1, off1=far)
    _refused(b"int32", flags=1, off2=far)
    _refused(b"NULL", flags=0, off1=far, off2=far, null=("match",))    # local rows: only the flag makes it a defect
    _refused(b"NULL", flags=1, off1=(0x7fffffe8, 0x7ffffff0, 0x7fffffff), null=("match",))


def test_null_pointers_on_a_valid_layout_are_refused_not_read():
    for name in ("match", "corr_offsets", "total", "rows"):
        _refused(b"NULL", null=(name,))
    for name in ("kp1", "kp2"):
        _refused(b"NULL", null=(name,), want=("pts",))
        _refused(b"NULL", null=(name,), want=("resid",))
    # rows may be NULL when nothing can be written
    for which in NAMES:
        rc, msg = _abi(which, capacity=0, null=("rows", "match"))
        assert rc == EINVAL and b"NULL" in msg                         # (match is the defect)


# ---- the order: of two defects the earlier one answers ----
@pytest.mark.parametrize("first,kw", [
    (b"flags", dict(flags=2, kp_dim=3, want=("pts",))),
    (b"keypoint rows", dict(kp_dim=3, want=("resid",), null=("models",))),
    (b"models", dict(want=("resid",), null=("models",), capacity=-1)),
    (b"error_type", dict(want=("resid",), gp=_lib.GuideParams(0, 3, 0.5), capacity=-1)),
    (b"capacity", dict(capacity=-1, n_pairs=-1)),
    (b"n_pairs", dict(n_pairs=-1, off1=(0, 6, 4))),
    (b"int32", dict(flags=1, off1=(0x7ffffff0, 0x7ffffff8, 0x80000008), null=("match", "total"))),
], ids=lambda x: x.decode() if isinstance(x, bytes) else "")
def test_the_order_of_the_refusals(first, kw):
    _refused(first, **kw)


def test_the_layout_is_judged_before_the_store_rows_and_the_pointers():
    for which in ("pairs_dev", "pairs"):
        rc, msg = _abi(which, flags=1, pairs=[(0, 2)], off1=(0x7ffffff0, 0x7ffffff8, 0x80000008), null=("match",))
        assert rc == EINVAL and b"image index" in msg
    for which in ("batch_dev", "batch"):
        rc, msg = _abi(which, flags=1, off1=(0x7ffffff8, 0x7ffffff0, 0x80000008), null=("match",))
        assert rc == EINVAL and b"non-decreasing" in msg


# ---- n_pairs == 0 ----
def test_empty_list_on_host_pointers_writes_total_and_the_first_offset_without_a_device():
    L = _lib.lib(); lp = C.POINTER(C.c_int64)
    for which in ("pairs", "batch"):
        co = np.full(3, 77, np.int64); total = np.full(1, 77, np.int64)
        lay = (None, 0, None, 0, None, 0) if which == "pairs" else (None, None, 0)
        rc = getattr(L, f"mi_degensac_correspondences_{which}")(*lay, None, None, 0, None, None, 0, None, None, 0, 0, co.ctypes.data_as(lp),
                                                                total.ctypes.data_as(lp), None, None, None, None)
        assert rc == 0 and total[0] == 0 and co.tolist() == [0, 77, 77]


def test_empty_list_looks_at_nothing_but_its_two_outputs():
    """the list, the offsets and the data pointers of an empty list are not judged: the one defect left is a missing output"""
    for which in NAMES:
        rc, msg = _abi(which, n_pairs=0, pairs=[(9, 9)], off1=(7, 3), off2=(-1,), null=("match", "rows", "kp1", "kp2", "total"))
        assert rc == EINVAL and b"NULL" in msg, which
        rc, msg = _abi(which, n_pairs=0, null=("corr_offsets",))
        assert rc == EINVAL and b"NULL" in msg, which


# ---- the Python keyword checks ----
COUNTS = [3, 0, 2, 4]
PAIRS = [(1, 0), (0, 2), (1, 1), (3, 0), (2, 3), (1, 2)]              # empty entries at the start, in the middle and at the end
N = 9
MATCH = np.array([1, 2, 0, 2, -1, 0, 1, 3, 3], np.int32)                # row 1: match = nt of its entry; row 4: -1
KEEP = np.array([1, 1, 0, 1, 1, 255, 0, 1, 1], np.uint8)
KPS = np.stack([10.0 * np.arange(9), 10.0 * np.arange(9) + 1], axis=1)  # store row r has the keypoint (10 r, 10 r + 1)


def _chk(**kw):
    a = dict(match_shape=(N,), match_dtype=np.int32, counts1=COUNTS, counts2=COUNTS, pairs=PAIRS)
    a.update(kw)
    return matcher.check_correspond_args(**a)


def test_good_arguments():
    o1, o2, pr, po, kind, et, cap = _chk()
    assert po.tolist() == [0, 0, 3, 3, 7, 9, 9] and kind is None and cap == N and pr.dtype == np.int32
    assert _chk(capacity=4)[-1] == 4 and _chk(capacity=0)[-1] == 0
    assert _chk(kps1=((9, 6), np.float64), kps2=((9, 6), np.float64), models=((6, 3, 3), np.float64), model="H", error_type="symm_sum")[4:6] == ("xy", 4)
    assert _chk(pairs=None, match_shape=(9,))[3].tolist() == [0, 3, 3, 5, 9]


@pytest.mark.parametrize("kw,msg", [
    (dict(models=((6, 3, 3), np.float64)), "need kps1"),                                       # residuals without keypoints
    (dict(kps1=((9, 2), np.float64)), "go together"),
    (dict(kps2=((9, 2), np.float64)), "go together"),
    (dict(match_shape=(8,)), "match"), (dict(match_shape=(9, 1)), "match"), (dict(match_dtype=np.int64), "match"),
    (dict(match_dtype=np.float32), "match"),
    (dict(keep=((8,), np.uint8)), "keep"), (dict(keep=((9,), np.int32)), "keep"), (dict(keep=((9,), np.float32)), "keep"),
    (dict(kps1=((8, 2), np.float64), kps2=((9, 2), np.float64)), "keypoint rows"),
    (dict(kps1=((9, 2), np.float64), kps2=((9, 6), np.float64)), "same layout"),
    (dict(kps1=((9, 3), np.float64), kps2=((9, 3), np.float64)), "keypoints"),
    (dict(kps1=((9, 2), np.float32), kps2=((9, 2), np.float32)), "keypoints"),
    (dict(kps1=((9, 2), np.float64), kps2=((9, 2), np.float64), models=((5, 3, 3), np.float64)), "models"),
    (dict(kps1=((9, 2), np.float64), kps2=((9, 2), np.float64), models=((6, 9), np.float64)), "models"),
    (dict(kps1=((9, 2), np.float64), kps2=((9, 2), np.float64), models=((6, 3, 3), np.float32)), "models"),
    (dict(model="E"), "model"), (dict(error_type="symm_max"), "Error type"), (dict(model="H", error_type="symm_epipolar"), "Error type"),
    (dict(capacity=-1), "capacity"), (dict(capacity=2.5), "capacity"), (dict(capacity=True), "capacity"),
    (dict(counts1=[3, 0, 2, -4]), "counts"), (dict(counts1=[[3, 0], [2, 4]]), "counts"), (dict(counts2=[3.0, 0, 2, 4]), "counts"),
    (dict(pairs=[0, 1]), "pairs"), (dict(pairs=np.zeros((0, 2), np.int64)), "at least one pair"), (dict(pairs=[(0, 4)]), "image index"),
    (dict(pairs=[(-1, 0)]), "image index"), (dict(pairs=[(0.0, 1.0)]), "pairs"),
    (dict(pairs=None, counts2=[3, 0, 2]), "one entry per pair"),
], ids=repr)
def test_keyword_defects(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _chk(**kw)


def test_numpy_entry_points_check_before_the_device():
    with pytest.raises(ValueError, match="match"):
        matcher.correspondences_pairs(MATCH[:-1], COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="need kps1"):
        matcher.correspondences_pairs(MATCH, COUNTS, COUNTS, PAIRS, models=np.zeros((6, 3, 3)))
    with pytest.raises(ValueError, match="keep"):
        matcher.correspondences_pairs(MATCH, COUNTS, COUNTS, PAIRS, keep=KEEP.astype(np.int32))
    with pytest.raises(ValueError, match="pairs"):
        matcher.correspondences_pairs(MATCH, COUNTS, COUNTS, None)
    with pytest.raises(ValueError, match="go together"):
        matcher.correspondences_batch(MATCH, COUNTS, COUNTS, kps1_list=[KPS[:3], KPS[3:3], KPS[3:5], KPS[5:]])
    with pytest.raises(ValueError, match="kps_list"):
        matcher.correspondences_pairs(MATCH, COUNTS, COUNTS, PAIRS, kps2_list=[KPS])
    with pytest.raises(ValueError, match="keypoint rows"):
        matcher.correspondences_pairs(MATCH, COUNTS, COUNTS, PAIRS, kps_list=[KPS[:3], KPS[3:3], KPS[3:5], KPS[5:8]])


def test_tensor_forms_check_before_the_device():
    torch = pytest.importorskip("torch")
    from pydegensac_amd import tensor_api
    m = torch.from_numpy(MATCH); k = torch.from_numpy(KPS); M = torch.zeros((6, 3, 3), dtype=torch.float64)
    call = tensor_api.correspondences_pairs_tensors
    with pytest.raises(ValueError, match="need kps1"):
        call(m, COUNTS, COUNTS, PAIRS, models=M)
    with pytest.raises(ValueError, match="match"):
        call(m.long(), COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="match"):
        call(m[:-1], COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="keep"):
        call(m, COUNTS, COUNTS, PAIRS, keep=torch.zeros(9))
    with pytest.raises(ValueError, match="models"):
        call(m, COUNTS, COUNTS, PAIRS, kps1=k, kps2=k, models=M[:-1])
    with pytest.raises(ValueError, match="capacity"):
        call(m, COUNTS, COUNTS, PAIRS, capacity=-3)
    with pytest.raises(ValueError, match="pairs"):
        call(m, COUNTS, COUNTS, None)
    with pytest.raises(ValueError, match="torch tensors"):
        call(MATCH, COUNTS, COUNTS, PAIRS)
    with pytest.raises(ValueError, match="ROCm device"):                # valid arguments, but not on a ROCm device
        call(m, COUNTS, COUNTS, PAIRS, keep=torch.from_numpy(KEEP), kps1=k, kps2=k, models=M)
    with pytest.raises(ValueError, match="one entry per pair"):
        tensor_api.correspondences_batch_tensors(m, COUNTS, COUNTS[:-1])
    with pytest.raises(ValueError, match="ROCm device"):
        tensor_api.correspondences_batch_tensors(m, COUNTS, COUNTS)


# ---- the restatement on hand-written tables ----
# with KEEP: rows 0, 3, 5, 7, 8 survive (row 1: match = nt; row 2, 6: keep = 0; row 4: match = -1)
WANT_KEEP = dict(rows=[(0, 1), (0, 2), (2, 0), (0, 3), (1, 3)], entry=[1, 3, 3, 4, 4], corr_offsets=[0, 0, 1, 1, 3, 5, 5], total=5,
                 store=[(0, 4), (5, 2), (7, 0), (3, 8), (4, 8)],
                 pts=[(0, 1, 40, 41), (50, 51, 20, 21), (70, 71, 0, 1), (30, 31, 80, 81), (40, 41, 80, 81)])
# without keep: rows 0, 2, 3, 5, 6, 7, 8
WANT_ALL = dict(rows=[(0, 1), (2, 0), (0, 2), (2, 0), (3, 1), (0, 3), (1, 3)], entry=[1, 1, 3, 3, 3, 4, 4], corr_offsets=[0, 0, 2, 2, 5, 7, 7],
                total=7)


def _equal(got, want, store=False):
    return (got["rows"].tolist() == [list(r) for r in want["store" if store else "rows"]] and got["entry"].tolist() == want["entry"]
            and got["corr_offsets"].tolist() == want["corr_offsets"] and got["total"] == want["total"])


def test_restatement_on_the_tables():
    assert _equal(cr.export(MATCH, COUNTS, COUNTS, PAIRS, keep=KEEP), WANT_KEEP)
    assert _equal(cr.export(MATCH, COUNTS, COUNTS, PAIRS, keep=KEEP != 0), WANT_KEEP)
    assert _equal(cr.export(MATCH, COUNTS, COUNTS, PAIRS), WANT_ALL)
    got = cr.export(MATCH, COUNTS, COUNTS, PAIRS, keep=KEEP, store_rows=True, kps1=KPS, kps2=KPS)
    assert _equal(got, WANT_KEEP, store=True) and got["pts"].tolist() == [list(map(float, p)) for p in WANT_KEEP["pts"]]
    assert got["rows"].dtype == np.int32 and got["corr_offsets"].dtype == np.int64


@pytest.mark.parametrize("cap,n", [(5, 5), (4, 4), (1, 1), (0, 0), (None, 5), (100, 5)])
def test_restatement_capacity_cuts_the_arrays_and_nothing_else(cap, n):
    got = cr.export(MATCH, COUNTS, COUNTS, PAIRS, keep=KEEP, capacity=cap, kps1=KPS, kps2=KPS)
    assert got["rows"].tolist() == [list(r) for r in WANT_KEEP["rows"][:n]] and got["entry"].tolist() == WANT_KEEP["entry"][:n]
    assert len(got["pts"]) == n and got["corr_offsets"].tolist() == WANT_KEEP["corr_offsets"] and got["total"] == 5


def test_restatement_two_stores_and_the_identity_list():
    c2 = [2, 5]                                                        # a second store: the train images
    pairs = [(3, 1), (0, 0), (3, 1)]
    match = np.array([4, 5, 0, -7, 1, 2, 0, 0, 1, 2, 3], np.int32)     # entry 0: nt = 5; entry 1: nt = 2; entry 2: nt = 5
    got = cr.export(match, COUNTS, c2, pairs, store_rows=True)
    assert got["rows"].tolist() == [[5, 6], [7, 2], [3 - 3, 1], [2, 0], [5, 2], [6, 3], [7, 4], [8, 5]]
    assert got["corr_offsets"].tolist() == [0, 2, 4, 8]
    b = cr.export(MATCH, COUNTS, COUNTS, cr.identity_pairs(4))
    assert b["corr_offsets"].tolist() == [0, 3, 3, 3, 7]                 # nt = the entry's own rows: 3, 0, 2, 4
    assert b["rows"].tolist() == [[0, 1], [1, 2], [2, 0], [0, 0], [1, 1], [2, 3], [3, 3]]


def test_restatement_residuals_are_the_oracles(oracle_port):
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 50, (6, 4)); entry = np.array([0, 0, 2, 2, 2, 3], np.int32)
    M = rng.normal(size=(4, 9))
    from tests import guided_ref as gr
    for model, et in gr.KINDS:
        d = cr.resid(oracle_port, model, et, M, entry, pts)
        for i in range(6):
            w = gr.resid(oracle_port, model, et, M[entry[i]], pts[i:i + 1, 0:2], pts[i:i + 1, 2:4])[0, 0]
            assert d[i].tobytes() == np.float64(w).tobytes(), (model, et, i)
    assert cr.same_bits_or_nan([1.0, np.nan], [1.0, np.nan]) and not cr.same_bits_or_nan([0.0], [-0.0])
    assert not cr.same_bits_or_nan([1.0], [np.nan]) and cr.same_bits_or_nan([np.nan], [np.nan])


# ---- three broken restatements, each rejected by the tables ----
def _broken_ignores_keep(match, counts1, counts2, pairs, keep):
    return cr.export(match, counts1, counts2, pairs, keep=None)


def _broken_offsets_skip_empty_entries(match, counts1, counts2, pairs, keep):
    got = cr.export(match, counts1, counts2, pairs, keep=keep)
    o1, _, pr, out = cr.layout(counts1, counts2, pairs)
    owns = np.diff(out) > 0
    got["corr_offsets"] = np.concatenate([got["corr_offsets"][:-1][owns], got["corr_offsets"][-1:]])
    return got


def _broken_sorts_by_train_row(match, counts1, counts2, pairs, keep):
    got = cr.export(match, counts1, counts2, pairs, keep=keep)
    order = np.lexsort((got["rows"][:, 1], got["entry"]))
    got["rows"] = got["rows"][order]
    return got


@pytest.mark.parametrize("broken", [_broken_ignores_keep, _broken_offsets_skip_empty_entries, _broken_sorts_by_train_row])
def test_broken_restatements_are_rejected_by_the_tables(broken):
    assert not _equal(broken(MATCH, COUNTS, COUNTS, PAIRS, KEEP), WANT_KEEP)
