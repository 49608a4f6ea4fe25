"""GPU: the asynchronous device-pointer entries of the two RANSAC kernels, mi_degensac_find_fundamental_batch_dev[_ex] and
mi_degensac_find_homography_batch_dev[_ex] (include/mi_degensac.h), called directly through ctypes: what one call reads and writes.
Every output lies between guard elements and is filled with sentinels (tests/estimator_dev_ref.py: model -7.0, mask 7, stats -5); after
every call the guards, the mask bytes of unowned rows and, with d_stats = NULL, the stats buffer must be untouched and every owned mask
byte 0 or 1.  Per pair the CPU restatement decides (counters equal, mask bit for bit, model to 1e-6 relative Frobenius, nine zeros and a
zero mask where it has no model), and the bytes of model and mask and the stats words 0 .. 11 equal the host-pointer call on the same pair
and seed (12 and 13 are device clock ticks).  Row counts sit at the edges of a wave, of the 256-point wave tile and of one pass step.
tests/test_estimator_dev_entry_cpu.py shows on the CPU that the scenes have the models they are here for and that the guard check bites."""
import ctypes as C

import numpy as np
import pytest

import pydegensac_amd as pd
from pydegensac_amd import _lib
from tests import estimator_dev_ref as R

pytestmark = pytest.mark.gpu
KINDS = ("F", "H")
_LP = C.POINTER(C.c_int64)
# find_homography_batch_tensors against numpy's inverse of the same 3 x 3 (relative Frobenius); test_tensor_forms prints the worst value
H_INV_BOUND = 1e-12


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _params(scenes, tuning=0, error_type=0):
    px, conf, mi, lc = R.call_params(scenes)
    return _lib.make_params(px, conf, mi, error_type, True, lc, True, 0, tuning)


def _upload(torch, store):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    return dict(pts1=t(store["pts1"]), pts2=t(store["pts2"]), offsets=t(store["off"]), seeds=t(store["seeds"].view(np.int32)))


def _raw(torch, kind, d, host_off, P, dim, prm, outs, stream=None, nulls=(), ex=None, host_null=False, device=0):
    """the C entry on `stream` (default: the current one); every output pointer is the first body element of its guarded tensor.  nulls:
    the pointers passed as NULL; ex: None = the plain entry, "null" = *_dev_ex with diag = NULL, "empty" = with a diag of NULL pointers.
    Returns the return code; nothing is synchronised."""
    s = torch.cuda.current_stream() if stream is None else stream
    i = lambda k: None if k in nulls else d[k].data_ptr()                   # noqa: E731
    o = lambda k: None if k in nulls else outs[k].data_ptr() + R.G * R.PER[k] * outs[k].element_size()          # noqa: E731
    name = "mi_degensac_find_" + ("fundamental" if kind == "F" else "homography") + "_batch_dev" + ("_ex" if ex else "")
    args = [i("pts1"), i("pts2"), i("offsets"), None if host_null else np.ascontiguousarray(host_off).ctypes.data_as(_LP), P, dim, C.byref(prm),
            i("seeds"), device, C.c_void_p(s.cuda_stream), o("model"), o("mask"), o("stats")]
    if ex:
        diag = _lib.Diag()
        assert diag.struct_size == C.sizeof(_lib.Diag) and not (diag.d_resids or diag.d_hist or diag.d_screen)
        args.append(None if ex == "null" else C.byref(diag))
    return getattr(_lib.lib(), name)(*args)


def _call(torch, kind, scenes, first_row=0, tail=0, nulls=(), ex=None, stream=None, tuning=0, outs=None):
    """one call on the pairs, at rows first_row ... of a store with `tail` unowned rows behind them, into sentinel-filled guarded outputs
    (outs: the device buffers of an earlier call, used as they are).  Synchronises the stream, checks everything the call does not own
    (R.read) and returns (per pair (model [9], mask bytes, stats [16] or None), outs)."""
    store = R.build_store(scenes, first_row, tail); P = len(scenes)
    d = _upload(torch, store)
    if outs is None:
        outs = {k: torch.from_numpy(v).cuda() for k, v in R.new_outputs(P, store["rows"]).items()}
    s = torch.cuda.current_stream() if stream is None else stream
    _lib.check(_raw(torch, kind, d, store["off"], P, store["pts1"].shape[1], _params(scenes, tuning), outs, s, nulls, ex))
    s.synchronize()
    return R.read({k: v.cpu().numpy() for k, v in outs.items()}, store["off"], P, stats_null="stats" in nulls), outs


_host = {}


def _host_call(sc):
    """the host-pointer call on the pair alone, once per process: (model [9], mask bytes, stats words 0 .. 11)"""
    key = (sc["kind"], sc["key"])
    if key not in _host:
        px, conf, mi, lc = R.call_params([sc])
        if sc["kind"] == "F":
            M, m = pd.findFundamentalMatrix_(sc["p1"], sc["p2"], px, conf, mi, 0, True, lc, True, seed=sc["seed"])
        else:
            M, m = pd.findHomography_(sc["p1"], sc["p2"], px, conf, mi, 0, True, lc, seed=sc["seed"])
        st = pd.last_stats()
        assert not st["discarded"] and not st["rerun"]
        _host[key] = (np.ascontiguousarray(M).ravel().copy(), np.asarray(m, np.uint8), np.array([st[k] for k in _lib.STAT_NAMES[:12]], np.int32))
    return _host[key]


def _check(port, scenes, got):
    """every pair against the restatement and, byte for byte, against the host-pointer call"""
    for p, sc in enumerate(scenes):
        ref = R.oracle(port, sc)
        why = R.agrees(sc["kind"], got[p], ref)
        assert why == "", (sc["kind"], p, len(sc["p1"]), why)
        assert R.same_bytes(got[p], _host_call(sc), stats=got[p][2] is not None), (sc["kind"], p, len(sc["p1"]), "differs from the host-pointer call")


_base = {}


def _zero_based(torch, kind, name):
    """the plain call on the batch `name` of R.all_batches, zero-based, default stream, fresh outputs: once per process"""
    if (kind, name) not in _base:
        _base[kind, name] = _call(torch, kind, R.all_batches(kind)[name])[0]
    return _base[kind, name]


def _same(a, b):
    return [p for p in range(len(a)) if not R.same_bytes(a[p], b[p], stats=a[p][2] is not None and b[p][2] is not None)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "laf"])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_equals_oracle_inside_guards(torch, oracle_port, kind, name):
    """one ragged batch of every row count (F: 8, 63 .. 65, 255 .. 257, 513; H: also 4 and 5), and one pair of [257, 6] rows under the LAF
    check, whose row stride is another"""
    scenes = R.all_batches(kind)[name]
    got = _zero_based(torch, kind, name)
    assert len(got) == len(scenes) and [len(g[1]) for g in got] == [len(s["p1"]) for s in scenes]
    _check(oracle_port, scenes, got)
    assert all(g[0].any() and g[1].sum() >= R.MIN_ROWS[kind] for g in got)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_row", R.FIRST_ROWS)
@pytest.mark.parametrize("name", ["ragged", "laf"])
@pytest.mark.parametrize("kind", KINDS)
def test_store_whose_first_row_is_not_zero(torch, kind, name, first_row):
    """the same pairs at rows 5 ... / 12 ... of a store with 9 rows behind them: d_pts1, d_pts2 and d_mask stay the bases of the store, the
    unowned rows are NaN (a read of one shows in the model) and their mask bytes must keep the sentinel (R.read), the model, the stats
    and the seeds are indexed by pair from 0"""
    got, _ = _call(torch, kind, R.all_batches(kind)[name], first_row=first_row, tail=R.TAIL_ROWS)
    assert _same(got, _zero_based(torch, kind, name)) == []


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_null_stats_and_diag_forms(torch, kind):
    scenes = R.ragged_batch(kind); base = _zero_based(torch, kind, "ragged")
    got, _ = _call(torch, kind, scenes, nulls=("stats",))
    assert all(g[2] is None for g in got) and _same(got, base) == []
    for ex in ("null", "empty"):
        got, _ = _call(torch, kind, scenes, ex=ex)
        assert all(g[2] is not None for g in got) and _same(got, base) == [], ex


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_outputs_reused_and_ten_identical_calls(torch, oracle_port, kind):
    """nine pairs, then three into the same buffers as the first call left them (the guards behind the shorter bodies re-armed): the pair
    without a model lands on the model and the mask bytes of pairs that had one.  Then ten calls with identical bytes."""
    first, second = R.reuse_batches(kind)
    got, outs = _call(torch, kind, first)
    _check(oracle_port, first, got)
    assert got[0][0].any() and got[0][1].any() and got[1][1].any()
    R.rearm(outs, len(second), R.build_store(second)["off"])
    got, _ = _call(torch, kind, second, outs=outs)
    _check(oracle_port, second, got)
    assert R.no_model(got[0], R.oracle(oracle_port, second[0])[2]["I"]) and got[1][0].any() and got[2][0].any()
    for _ in range(9):
        again, _ = _call(torch, kind, second, outs=outs)
        assert _same(again, got) == []


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_no_model_pairs_are_zeroed_between_found_ones(torch, oracle_port, kind):
    """[found, no model, found, no model] into sentinel-filled outputs.  The pairs without a model are the all-outlier case of
    tests/test_gpu_parity_*.py (n = 300 / 200, inlier ratio 0, max_iters = 3000 / 2000) with image 2 collapsed to one point: the case
    itself always has a model in the restatement (tests/estimator_dev_ref.no_model_scene).  MI_ST_I of such a pair is the restatement's:
    0 for H, and for F the score I = 8 that the driver starts from and returns when it accepted nothing."""
    scenes = R.mixed_batch(kind)
    refs = [R.oracle(oracle_port, sc) for sc in scenes]
    assert [bool(np.asarray(r[0]).any()) for r in refs] == [True, False, True, False]          # the precondition
    got = _zero_based(torch, kind, "mixed")
    _check(oracle_port, scenes, got)
    for p in (1, 3):
        assert got[p][0].tobytes() == bytes(72) and got[p][1].tobytes() == bytes(len(scenes[p]["p1"])), p
        assert got[p][2][_lib.STAT_NAMES.index("I")] == refs[p][2]["I"] == (0 if kind == "H" else 8) and not got[p][2][15] & (1 << 10), p
    for p in (0, 2):
        assert got[p][0].any() and got[p][1].sum() >= R.MIN_ROWS[kind], p


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_same_bytes_in_any_order_and_on_two_workgroups(torch, kind):
    """the ragged batch in reverse order (seeds travel with their pairs), and on a grid capped at two workgroups, each of which takes
    several pairs in a row"""
    scenes = R.ragged_batch(kind); base = _zero_based(torch, kind, "ragged")
    rev, _ = _call(torch, kind, scenes[::-1])
    assert _same(rev[::-1], base) == []
    two, _ = _call(torch, kind, scenes, tuning=_lib.TUNE_GRID_CAP(2))
    assert _same(two, base) == []
    assert all(t[2][14] == b[2][14] for t, b in zip(two, base))          # the same kernel variant


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_second_stream(torch, kind):
    base = _zero_based(torch, kind, "ragged")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = _call(torch, kind, R.ragged_batch(kind), stream=s)
    assert _same(got, base) == []
    assert _lib.lib().mi_degensac_release_scratch(0, C.c_void_p(s.cuda_stream)) == 0


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def _refuse(torch, kind, case, outs):
    scenes = R.refusal_batch(kind, case)
    store = R.build_store(scenes)
    prm = _params(scenes, error_type=case["error_type"][kind] if "error_type" in case else 0)
    rc = _raw(torch, kind, _upload(torch, store), store["off"], case.get("n_pairs", len(scenes)), case.get("dim", 2), prm, outs,
              nulls=(case["null"],) if "null" in case else (), host_null=case.get("host_null", False), device=case.get("device", 0))
    torch.cuda.synchronize()
    return rc, all(bool((outs[k] == R.FILL[k]).all()) for k in outs)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_launch_nothing(torch, kind):
    """every refused call returns its code and leaves every output byte, body and guards alike, as it was.  The NULL-pointer cases are
    host-side checks: a library without them would launch on the pointer, so the probe first shows that the loaded library has them (a
    call with a NULL d_pts1 AND an error type no library accepts: no library launches it, and the message says which check refused it)."""
    good = R.build_store(R.refusal_batch(kind, {}))
    outs = {k: torch.from_numpy(v).cuda() for k, v in R.new_outputs(2, good["rows"]).items()}
    rc, clean = _refuse(torch, kind, R.REFUSAL_PROBE, outs)
    assert rc == _lib.EINVAL and clean
    assert _lib.lib().mi_degensac_last_error().decode().startswith(R.REFUSAL_PROBE_MESSAGE), "this library does not check its device pointers"
    for case in R.REFUSALS:
        rc, clean = _refuse(torch, kind, case, outs)
        assert rc == getattr(_lib, case["code"]) and (rc != 0 or case.get("n_pairs") == 0), (case["name"], rc)
        assert clean, case["name"]
    # ... and the buffers, the store and the parameters of these cases are good ones
    got, _ = _call(torch, kind, R.refusal_batch(kind, {}), outs=outs)
    assert _same(got[:1], [_host_call(R.row_scene(kind, R.REFUSAL_ROWS))]) == [] and _same(got[1:], got[:1]) == []


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_tensor_forms(torch, oracle_port, kind):
    """find_fundamental_batch_tensors / find_homography_batch_tensors on [found, no model, found, no model] and on the LAF pair, from
    non-contiguous views (the columns [:, :2] of a [total, 5] tensor, [:, :6] of a [total, 9] one; NaN beside them) under the seeds 0, 1,
    2^31 - 1, 2^31 and 2^32 - 1, which travel as int32 bit patterns.  The user-facing H is inv(H_c^T) of the C entry's model, compared with
    numpy's inverse of the same 3 x 3 to 1e-12 relative Frobenius: the worst distance measured on these scenes is 1.8e-16 (printed below)."""
    from pydegensac_amd import tensor_api as T
    worst = 0.0
    for scenes in R.tensor_batches(kind):
        store = R.build_store(scenes); P = len(scenes); dim = store["pts1"].shape[1]
        wide = [torch.full((store["rows"], 5 if dim == 2 else 9), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
        v1, v2 = wide[0][:, :dim], wide[1][:, :dim]
        v1.copy_(torch.from_numpy(store["pts1"])); v2.copy_(torch.from_numpy(store["pts2"]))
        assert not v1.is_contiguous() and not v2.is_contiguous()
        counts = [len(s["p1"]) for s in scenes]; seeds = [s["seed"] for s in scenes]
        px, conf, mi, lc = R.call_params(scenes)
        raw = T._run(kind, v1, v2, counts, _params(scenes), seeds, R.MIN_ROWS[kind])          # the C entry's own model
        if kind == "F":
            res = T.find_fundamental_batch_tensors(v1, v2, counts, px, conf, mi, lc if lc > 0 else -1.0, "sampson", True, True, seeds=seeds)
        else:
            res = T.find_homography_batch_tensors(v1, v2, counts, px, conf, mi, lc if lc > 0 else -1.0, "sampson", True, seeds=seeds)
        for r in (raw, res):
            assert r[0].is_cuda and r[0].shape == (P, 3, 3) and r[0].dtype == torch.float64 and r[1].dtype == torch.bool and r[1].shape == (store["rows"],)
            assert r[2].shape == (P, 16) and r[2].dtype == torch.int32 and np.array_equal(r[3], store["off"]) and np.array_equal(r[3][1:], np.cumsum(counts))
        Mr, mr, sr = (x.cpu().numpy() for x in raw[:3]); Mu, mu, su = (x.cpu().numpy() for x in res[:3])
        off = store["off"]
        got = [(Mr[p].ravel(), mr[off[p]:off[p + 1]].astype(np.uint8), sr[p]) for p in range(P)]
        _check(oracle_port, scenes, got)
        assert np.array_equal(mu, mr) and np.array_equal(su[:, :12], sr[:, :12])
        for p, sc in enumerate(scenes):
            Hc = _host_call(sc)[0].reshape(3, 3)
            assert bool(Hc.any()) == (not R.is_no_model_scene(sc)), p
            if kind == "F":
                assert Mu[p].tobytes() == Hc.tobytes(), p
            elif not Hc.any():
                assert Mu[p].tobytes() == bytes(72), p
            else:
                want = np.linalg.inv(Hc.T)
                worst = max(worst, float(np.linalg.norm(Mu[p] - want) / np.linalg.norm(want)))
    print(f"{kind}: worst relative distance of the tensor form's inverse from numpy's: {worst:.3e}")
    assert worst <= H_INV_BOUND, worst
    # refusals of the tensor form
    fn = T.find_fundamental_batch_tensors if kind == "F" else T.find_homography_batch_tensors
    sc = R.row_scene(kind, 64); n = 64
    a = torch.from_numpy(sc["p1"]).cuda(); b = torch.from_numpy(sc["p2"]).cuda()
    short = R.MIN_ROWS[kind] - 1
    for args in ((a.float(), b.float(), [n]), (a, b, [n - 1]), (a, b, [n + 1]), (a, b, [n - short, short]), (a.cpu(), b.cpu(), [n]), (a, b.cpu(), [n])):
        with pytest.raises(ValueError):
            fn(*args, seeds=list(range(len(args[2]))))
