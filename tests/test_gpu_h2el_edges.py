"""GPU: ransacH2el (dg_kernel_h2el.h, launch_h2el) where the suite did not reach: a workgroup that runs a second pair, row counts on both
sides of every tile and pass step, the device entry mi_degensac_ransac_h2el_batch_dev (absolute offsets, d_stats = NULL, a second stream,
refusals) and the fit limit at the length of a list.  Every pair is compared with the CPU restatement (tests/h2el_ref.py: counters equal,
mask byte for byte, model to 1e-6); two device runs of one pair are compared byte for byte (model, mask, stats words 0-11; 12-13 are
clocks).  tests/test_h2el_edges_cpu.py proves on the CPU that the scenes take the branches they are here for."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib
from tests import h2el_ref as hr

pytestmark = pytest.mark.gpu
G = 8                                                                     # guard elements on both sides of every output
GUARD_H, GUARD_M, GUARD_S = -77.0, 0xB5, -77
EINVAL = -1                                                               # MI_DEGENSAC_EINVAL
_LP = C.POINTER(C.c_int64)


def _prm(do_lo, lim, th=None, conf=None, max_iters=None):
    return _lib.H2elParams(hr.CALL["th"] if th is None else th, hr.CALL["conf"] if conf is None else conf,
                           hr.CALL["max_iters"] if max_iters is None else max_iters, int(bool(do_lo)), int(lim), 0)


def _offsets(U):
    return np.concatenate([[0], np.cumsum([len(u) for u in U])]).astype(np.int64)


def _host(U, seeds, do_lo, lim, th=None):
    """mi_degensac_ransac_h2el_batch: per pair (H [3, 3] raw, mask bytes, stats words)"""
    off = _offsets(U); P = len(U)
    cat = np.ascontiguousarray(np.concatenate(U, 0)); sd = np.ascontiguousarray(seeds, dtype=np.uint32)
    H = np.zeros((P, 9)); mask = np.full(int(off[-1]), GUARD_M, np.uint8); st = np.zeros((P, 16), np.int32)
    prm = _prm(do_lo, lim, th)
    rc = _lib.lib().mi_degensac_ransac_h2el_batch(_lib.dptr(cat), off.ctypes.data_as(_LP), P, C.byref(prm), sd.ctypes.data_as(C.POINTER(C.c_uint32)), 0,
                                                  _lib.dptr(H), mask.ctypes.data_as(C.POINTER(C.c_uint8)), st.ctypes.data_as(C.POINTER(C.c_int32)))
    _lib.check(rc)
    return [(H[p].reshape(3, 3), mask[off[p]:off[p + 1]], st[p]) for p in range(P)]


def _same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2][:12].tobytes() == b[2][:12].tobytes()


# ---- 1: more pairs than workgroups -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("do_lo,lim", hr.REUSE_SETTINGS)
def test_more_pairs_than_workgroups_run_a_second_pair(oracle_port, do_lo, lim):
    """2 CUs + 3 pairs on a grid of one persistent workgroup per CU: every workgroup runs at least two pairs, every seventh pair has 2500
    rows, and pairs that never get a model (errs[3] unwritten), that start the run after the loop from the unwritten errs[4], and of 2 and
    3 rows lie between ordinary ones.  Against the restatement, against the same pair run alone, and against the batch in reversed order."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    U, seeds, kinds = hr.reuse_batch(cus)
    P = len(U)
    assert P > cus and P == 2 * cus + 3
    print(f"CUs = {cus}, pairs = {P}")
    got = _host(U, seeds, do_lo, lim)
    bad = [i for i in range(P) if not hr.agrees(got[i], hr.oracle(oracle_port, ("reuse", i), U[i], seeds[i], do_lo, lim))]
    assert not bad, (bad[:10], [kinds[i] for i in bad[:10]])
    for i, k in enumerate(kinds):
        if k in "ab":
            assert hr.never_a_model(got[i]) and (got[i][1] == 1).all(), (i, k)
    rev = _host(U[::-1], seeds[::-1], do_lo, lim)[::-1]
    bad = [i for i in range(P) if not _same_bytes(got[i], rev[i])]
    assert not bad, ("reversed order", bad[:10], [kinds[i] for i in bad[:10]])
    for i in hr.reuse_sample(kinds):
        assert _same_bytes(got[i], _host([U[i]], [seeds[i]], do_lo, lim)[0]), ("alone", i, kinds[i])


# ---- 2: row counts ---------------------------------------------------------------------------------------------------------------------
_rows = {}


def _row_results(lim, desc):
    if (lim, desc) not in _rows:
        U, seeds, keys = hr.row_batch(desc)
        _rows[lim, desc] = dict(zip(keys, _host(U, seeds, True, lim)))
    return _rows[lim, desc]


@pytest.mark.parametrize("n", hr.ROW_NS)
def test_row_counts_at_the_pass_edges(oracle_port, n):
    """n on both sides of the wave tile (256 rows), the pass step (2048 rows at 512 threads, four tiles per step) and twice that, two scenes
    each, all counts of one setting in ONE ragged batch (ascending and descending: ragged offsets, a workspace sized by the largest pair)"""
    th = hr.CALL["th"]
    for lim in hr.ROW_LIMITS:
        for j in (0, 1):
            u, seed = hr.row_scene(n, j)
            want = hr.oracle(oracle_port, ("row", n, j), u, seed, True, lim)
            up, down = _row_results(lim, False)[n, j], _row_results(lim, True)[n, j]
            assert hr.agrees(up, want), (n, j, lim, up[2][:5], want[2])
            assert _same_bytes(up, down), (n, j, lim)
            if up[0].any():
                # the driver's last loop: mask[j] = HDs(returned model) <= th, in float64 numpy from the raw model
                m, close = hr.mask_from_model(up[0], u, th)
                assert close.sum() <= 0.01 * n, (n, j, lim, int(close.sum()))
                assert np.array_equal(m[~close], up[1][~close].astype(bool)), (n, j, lim)
            assert set(np.unique(up[1]).tolist()) <= {0, 1}


# ---- 3: the device entry ---------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _buffers(P, rows):
    import torch
    return dict(H=torch.full((P * 9 + 2 * G,), GUARD_H, dtype=torch.float64, device=_dev()),
                mask=torch.full((rows + 2 * G,), GUARD_M, dtype=torch.uint8, device=_dev()),
                stats=torch.full((P * 16 + 2 * G,), GUARD_S, dtype=torch.int32, device=_dev()))


def _raw(u_t, off_t, off_host, P, prm, seeds_t, bufs, nulls=(), skip=0, host_null=False):
    """mi_degensac_ransac_h2el_batch_dev on the current stream; every output is the slice [G : G + n] of its tensor.  skip: the call's
    offsets start at entry `skip` of off_t / off_host; d_u10 and d_mask stay the bases of the whole store.  Returns the return code."""
    import torch
    p = {k: None if k in nulls else bufs[k].data_ptr() + G * bufs[k].element_size() for k in bufs}
    stream = torch.cuda.current_stream(_dev())
    return _lib.lib().mi_degensac_ransac_h2el_batch_dev(u_t.data_ptr(), off_t.data_ptr() + 8 * skip, None if host_null else off_host[skip:].ctypes.data_as(_LP), P,
                                                        None if prm is None else C.byref(prm), seeds_t.data_ptr(), 0, C.c_void_p(stream.cuda_stream),
                                                        p["H"], p["mask"], p["stats"])


def _read(bufs, P, off):
    """per pair (H, mask, stats) after the guards were found untouched; off: the host offsets of the P pairs, absolute into the mask tensor;
    mask bytes in front of off[0] and behind off[P] count as guards"""
    import torch
    torch.cuda.synchronize()
    H, m, st = (bufs[k].cpu().numpy() for k in ("H", "mask", "stats"))
    assert (H[:G] == GUARD_H).all() and (H[G + 9 * P:] == GUARD_H).all()
    assert (m[:G + int(off[0])] == GUARD_M).all() and (m[G + int(off[P]):] == GUARD_M).all()
    assert (st[:G] == GUARD_S).all() and (st[G + 16 * P:] == GUARD_S).all()
    return [(H[G + 9 * p:G + 9 * p + 9].reshape(3, 3), m[G + int(off[p]):G + int(off[p + 1])], st[G + 16 * p:G + 16 * p + 16]) for p in range(P)]


def _untouched(bufs):
    import torch
    torch.cuda.synchronize()
    return all(bool((bufs[k] == v).all()) for k, v in (("H", GUARD_H), ("mask", GUARD_M), ("stats", GUARD_S)))


@pytest.fixture(scope="module")
def dev_case():
    U, seeds = hr.dev_batch()
    off = _offsets(U)
    return dict(U=U, seeds=seeds, off=off, u_t=_t(np.concatenate(U, 0)), off_t=_t(off), seeds_t=_t(np.asarray(seeds, np.uint32).view(np.int32)),
                host={s: _host(U, seeds, *s) for s in ((True, 0), (True, 16))})


def test_device_entry_equals_the_host_entry(oracle_port, dev_case):
    d = dev_case; P = len(d["U"])
    for (do_lo, lim), host in d["host"].items():
        bufs = _buffers(P, int(d["off"][-1]))
        assert _raw(d["u_t"], d["off_t"], d["off"], P, _prm(do_lo, lim), d["seeds_t"], bufs) == 0
        got = _read(bufs, P, d["off"])
        for p in range(P):
            assert _same_bytes(got[p], host[p]), (do_lo, lim, p)
            assert hr.agrees(got[p], hr.oracle(oracle_port, ("row", len(d["U"][p]), 0), d["U"][p], d["seeds"][p], do_lo, lim)), (do_lo, lim, p)


def test_device_entry_without_stats(dev_case):
    d = dev_case; P = len(d["U"]); host = d["host"][True, 0]
    bufs = _buffers(P, int(d["off"][-1]))
    assert _raw(d["u_t"], d["off_t"], d["off"], P, _prm(True, 0), d["seeds_t"], bufs, nulls=("stats",)) == 0
    got = _read(bufs, P, d["off"])
    assert bool((bufs["stats"] == GUARD_S).all())
    for p in range(P):
        assert got[p][0].tobytes() == host[p][0].tobytes() and got[p][1].tobytes() == host[p][1].tobytes(), p


def test_device_entry_offsets_that_start_above_zero(oracle_port, dev_case):
    """the middle pairs of a longer store through `offsets + 2`: d_u10 and d_mask stay the bases of the store (the offsets are absolute row
    numbers), d_H / d_stats / d_seeds belong to the call.  The rows of the other pairs are NaN and their mask bytes guards: a read of them
    would show in the model, a write in the guards."""
    d = dev_case; off = d["off"]; host = d["host"][True, 16]
    cat = np.concatenate(d["U"], 0)
    cat[:off[2]] = np.nan; cat[off[4]:] = np.inf
    bufs = _buffers(2, int(off[-1]))
    assert _raw(_t(cat), d["off_t"], off, 2, _prm(True, 16), d["seeds_t"][2:4].contiguous(), bufs, skip=2) == 0
    got = _read(bufs, 2, off[2:5])
    for q in range(2):
        assert _same_bytes(got[q], host[2 + q]), q
        assert hr.agrees(got[q], hr.oracle(oracle_port, ("row", len(d["U"][2 + q]), 0), d["U"][2 + q], d["seeds"][2 + q], True, 16)), q


def test_device_entry_on_a_second_stream(dev_case):
    import torch
    d = dev_case; P = len(d["U"]); host = d["host"][True, 0]
    a, b = _buffers(P, int(d["off"][-1])), _buffers(P, int(d["off"][-1]))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(s):
        for bufs in (a, b):                                               # back to back: the second call reuses the stream's workspace
            assert _raw(d["u_t"], d["off_t"], d["off"], P, _prm(True, 0), d["seeds_t"], bufs) == 0
    s.synchronize()
    for bufs in (a, b):
        got = _read(bufs, P, d["off"])
        assert all(_same_bytes(got[p], host[p]) for p in range(P))
    assert _lib.lib().mi_degensac_release_scratch(0, C.c_void_p(s.cuda_stream)) == 0


def test_device_entry_refusals(dev_case):
    d = dev_case; P = len(d["U"]); off = d["off"]
    bufs = _buffers(P, int(off[-1]))
    call = lambda prm, **kw: _raw(d["u_t"], d["off_t"], kw.pop("off", off), kw.pop("P", P), prm, d["seeds_t"], bufs, **kw)
    short = off.copy(); short[3] = short[2] + 1                            # pair 2 with one row
    cases = [("prm", call(None)), ("offsets_host", call(_prm(True, 0), host_null=True)), ("one row", call(_prm(True, 0), off=short)),
             ("d_H", call(_prm(True, 0), nulls=("H",))), ("d_mask", call(_prm(True, 0), nulls=("mask",)))]
    cases += [(f"inl_limit {k}", call(_prm(True, k))) for k in (1, 2, 3)]
    cases += [(f"th {v}", call(_prm(True, 0, th=v))) for v in (0.0, -1.0)]
    cases += [(f"conf {v}", call(_prm(True, 0, conf=v))) for v in (0.0, 1.0, -0.5, 1.5)]
    cases += [(f"max_iters {v}", call(_prm(True, 0, max_iters=v))) for v in (0, -3)]
    assert [(k, rc) for k, rc in cases if rc != EINVAL] == []
    assert _untouched(bufs)
    assert call(_prm(True, 0), P=0) == 0 and _untouched(bufs)


# ---- 4: the fit limit at the length of a list --------------------------------------------------------------------------------------------
def test_inl_limit_equal_to_and_one_below_the_list_length(oracle_port):
    """a list of L rows under the limits L - 1 (one draw: a random L - 1 of them are fitted), L, L + 1 and 0 (no draw)"""
    u, _ = hr.limit_scene()
    L = hr.LIMIT_L
    got = {lim: _host([u], [hr.LIMIT_SEED], True, lim, th=hr.LIMIT_TH)[0] for lim in (L - 1, L, L + 1, 0)}
    for lim, g in got.items():
        assert hr.agrees(g, hr.oracle(oracle_port, "limit", u, hr.LIMIT_SEED, True, lim, th=hr.LIMIT_TH)), (lim, g[2][:5])
    assert _same_bytes(got[L], got[0]) and _same_bytes(got[L + 1], got[0])
    assert not _same_bytes(got[L - 1], got[L])


# ---- 5: samples of two identical rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("do_lo,lim", hr.REUSE_SETTINGS)
def test_samples_of_two_identical_rows_are_turned_down(oracle_port, do_lo, lim):
    u = hr.duplicate_scene()
    two = np.ascontiguousarray(np.repeat(u[:1], 2, axis=0))
    got = _host([u, two], [hr.DUP_SEED, hr.DUP_SEED], do_lo, lim)
    assert hr.agrees(got[0], hr.oracle(oracle_port, "dup", u, hr.DUP_SEED, do_lo, lim)), got[0][2][:5]
    assert hr.agrees(got[1], hr.oracle(oracle_port, "dup-two", two, hr.DUP_SEED, do_lo, lim)), got[1][2][:5]
