"""No GPU: what tests/test_gpu_estimator_dev_entry.py rests on.  Every scene it runs has a model in the CPU restatement (at least 8 / 4
inliers) except the scenes built to have none; the store builder and the guard check of tests/estimator_dev_ref.py hold for
a numpy "kernel" that writes its owned ranges only and catch those that write one element too far; the refusal table names error codes
that exist."""
import numpy as np
import pytest

from pydegensac_amd import _lib
from tests import estimator_dev_ref as R

KINDS = ("F", "H")


@pytest.mark.parametrize("kind", KINDS)
def test_every_scene_has_a_model_and_the_no_model_scenes_have_none(oracle_port, kind):
    """no scene of estimator_shapes had to be replaced: every one has a model under its own data seed"""
    seen = 0
    for name, batch in R.all_batches(kind).items():
        assert 1 <= len(batch) <= 12 and max(len(s["p1"]) for s in batch) <= 513, name
        R.call_params(batch)
        for p, sc in enumerate(batch):
            M, m, st = R.oracle(oracle_port, sc)
            if R.is_no_model_scene(sc):
                # H: every sample is turned down before scoring (the run after the loop scores its fits and accepts none), I = 0.  F: no sample
                # yields a model to score, and the driver returns the score it started from, I = 8, with the mask of its unwritten
                # residuals (all ones; the device's contract is all zero)
                assert not M.any() and st["samples"] == R.call_params(batch)[2], (name, p, st)
                assert (st["rejected"] == st["samples"] and st["I"] == 0 and not m.any()) if kind == "H" else (st["models"] == 0 and st["I"] == 8), (name, p, st)
            else:
                assert M.any() and st["I"] >= R.MIN_ROWS[kind] and int(m.sum()) >= R.MIN_ROWS[kind], (name, p, st)
                assert len(sc["p1"]) >= R.MIN_ROWS[kind]
            seen += 1
    assert seen == (32 if kind == "H" else 30)
    mixed = R.mixed_batch(kind)
    assert [R.is_no_model_scene(s) for s in mixed] == [False, True, False, True]
    assert [R.is_no_model_scene(s) for s in R.tensor_batches(kind)[0]] == [False, True, False, True]
    assert sorted(len(s["p1"]) for s in R.ragged_batch(kind)) == list(R.ROWS[kind])
    assert R.laf_batch(kind)[0]["p1"].shape == (R.LAF_N, 6) and R.laf_batch(kind)[0]["laf_coef"] > 0
    assert [s["seed"] for b in R.tensor_batches(kind) for s in b] == list(R.TENSOR_SEEDS)


# ---- the store and the guard check, with numpy kernels ------------------------------------------------------------------------------------
def _fake_kernel(store, outs, P, stats=True, mask_shift=0, mask_extra=0, model_extra=0, stats_extra=0):
    """what a correct entry writes, through pointers at the bodies' first elements: pair p's mask bytes at the absolute rows off[p] ..
    off[p + 1], its model and stats at p.  The keyword faults are the ones the guards are there for: mask_shift moves every mask write
    (off - off[0] instead of off is mask_shift = -off[0]), *_extra write that many elements behind the last pair."""
    off = store["off"]
    model = outs["model"][R.G * 9:]; mask = outs["mask"][R.G:]; st = outs["stats"][R.G * 16:]
    for p in range(P):
        b, e = int(off[p]) + mask_shift, int(off[p + 1]) + mask_shift
        assert not np.isnan(store["pts1"][off[p]:off[p + 1]]).any() and not np.isnan(store["pts2"][off[p]:off[p + 1]]).any()
        mask[b:e] = (np.arange(e - b) + p) % 2
        model[9 * p:9 * p + 9] = p + 1.0
        if stats:
            st[16 * p:16 * p + 16] = np.arange(16) + 100 * p
    mask[int(off[P]) + mask_shift:int(off[P]) + mask_shift + mask_extra] = 1
    model[9 * P:9 * P + model_extra] = 0.0
    st[16 * P:16 * P + stats_extra] = 0


@pytest.mark.parametrize("first_row,tail", [(0, 0), (5, R.TAIL_ROWS), (12, R.TAIL_ROWS)])
def test_guard_check_passes_a_kernel_that_writes_what_it_owns(first_row, tail):
    scenes = R.ragged_batch("H"); P = len(scenes)
    store = R.build_store(scenes, first_row, tail)
    assert store["off"][0] == first_row and store["rows"] == store["off"][-1] + tail and store["seeds"].dtype == np.uint32
    owned = np.zeros(store["rows"], bool)
    for p, s in enumerate(scenes):
        b, e = store["off"][p], store["off"][p + 1]
        assert np.array_equal(store["pts1"][b:e], s["p1"]) and np.array_equal(store["pts2"][b:e], s["p2"]) and store["seeds"][p] == s["seed"]
        owned[b:e] = True
    assert np.isnan(store["pts1"][~owned]).all() and np.isnan(store["pts2"][~owned]).all() and (~owned).sum() == first_row + tail
    outs = R.new_outputs(P, store["rows"])
    assert R.untouched(outs) and all(len(outs[k]) == (2 * R.G + (store["rows"] if k == "mask" else P)) * R.PER[k] for k in R.PER)
    _fake_kernel(store, outs, P)
    got = R.read(outs, store["off"], P)
    assert not R.untouched(outs)
    for p in range(P):
        assert (got[p][0] == p + 1.0).all() and len(got[p][1]) == len(scenes[p]["p1"]) and got[p][2][3] == 3 + 100 * p
    assert (outs["mask"][R.G:R.G + first_row] == R.FILL["mask"]).all()
    # stats = NULL: nothing of the stats buffer may change
    outs = R.new_outputs(P, store["rows"])
    _fake_kernel(store, outs, P, stats=False)
    assert all(g[2] is None for g in R.read(outs, store["off"], P, stats_null=True))
    with pytest.raises(AssertionError, match="although NULL"):
        _fake_kernel(store, outs, P, stats=True); R.read(outs, store["off"], P, stats_null=True)


@pytest.mark.parametrize("fault,match", [(dict(mask_extra=1), "behind the last owned row"), (dict(model_extra=1), "model: a guard element behind"),
                                         (dict(stats_extra=1), "stats: a guard element behind"), (dict(mask_shift=-5), "in front of the first owned row"),
                                         (dict(mask_shift=-1), "in front of the first owned row"), (dict(mask_shift=1), "behind the last owned row")])
def test_guard_check_catches_one_element_too_far(fault, match):
    scenes = R.ragged_batch("F"); P = len(scenes)
    store = R.build_store(scenes, 5, R.TAIL_ROWS)
    outs = R.new_outputs(P, store["rows"])
    _fake_kernel(store, outs, P, **fault)
    with pytest.raises(AssertionError, match=match):
        R.read(outs, store["off"], P)


def test_guard_check_catches_a_byte_that_is_no_mask_value_and_rearm_restores_the_guards():
    scenes = R.ragged_batch("F"); P = len(scenes)
    store = R.build_store(scenes)
    outs = R.new_outputs(P, store["rows"])
    _fake_kernel(store, outs, P)
    outs["mask"][R.G + 70] = 2
    with pytest.raises(AssertionError, match="neither 0 nor 1"):
        R.read(outs, store["off"], P)
    outs["mask"][R.G + 70] = 1
    short = R.build_store(scenes[:3])
    with pytest.raises(AssertionError):                                   # the longer call's bytes lie where the shorter call has guards
        R.read(outs, short["off"], 3)
    R.rearm(outs, 3, short["off"])
    got = R.read(outs, short["off"], 3)
    assert (got[2][0] == 3.0).all() and len(outs["model"]) == (2 * R.G + P) * 9          # the bodies keep what the first call left


def test_comparisons_tell_a_wrong_pair_from_a_right_one(oracle_port):
    sc = R.row_scene("F", 64); ref = R.oracle(oracle_port, sc)
    st = np.zeros(16, np.int32)
    for k in R.KEYS["F"]:
        st[_lib.STAT_NAMES.index(k)] = ref[2][k]
    good = (np.asarray(ref[0], float).ravel().copy(), np.asarray(ref[1], np.uint8), st)
    assert R.agrees("F", good, ref) == "" and not R.no_model(good)
    flipped = good[1].copy(); flipped[0] ^= 1
    assert "mask" in R.agrees("F", (good[0], flipped, st), ref)
    assert "model" in R.agrees("F", (good[0] * (1 + 1e-4 * np.arange(9)), good[1], st), ref)
    assert R.agrees("F", (good[0] * (1 + 1e-9 * np.arange(9)), good[1], st), ref) == ""
    assert "zero model" in R.agrees("F", (np.zeros(9), good[1], st), ref)
    st2 = st.copy(); st2[0] += 1
    assert "counters" in R.agrees("F", (good[0], good[1], st2), ref)
    st3 = st.copy(); st3[15] |= 1024
    assert R.agrees("F", (good[0], good[1], st3), ref) == "discarded"
    none = R.oracle(oracle_port, R.no_model_scene("F", 0)); n = len(none[1])
    zs = np.zeros(16, np.int32)
    for k in R.KEYS["F"]:
        zs[_lib.STAT_NAMES.index(k)] = none[2][k]
    assert R.agrees("F", (np.zeros(9), np.zeros(n, np.uint8), zs), none) == "" and R.no_model((np.zeros(9), np.zeros(n, np.uint8), zs), 8)
    assert R.agrees("F", (np.full(9, -0.0), np.zeros(n, np.uint8), zs), none) != ""          # nine zeros means every byte
    left = np.zeros(n, np.uint8); left[5] = 1
    assert R.agrees("F", (np.zeros(9), left, zs), none) != "" and not R.no_model((np.zeros(9), left, zs), 8)
    assert not R.same_bytes(good, (good[0], good[1], st2)) and R.same_bytes(good, (good[0], good[1], st2), stats=False)
    st4 = st.copy(); st4[12:14] += 7
    assert R.same_bytes(good, (good[0].copy(), good[1].copy(), st4))


def test_refusal_table_names_existing_error_codes():
    names = [c["name"] for c in R.REFUSALS]
    assert len(set(names)) == len(names) == 12
    for case in R.REFUSALS + (R.REFUSAL_PROBE,):
        code = getattr(_lib, case["code"])
        assert isinstance(code, int) and code in (_lib.OK, _lib.EINVAL, _lib.ENODEV, _lib.EHIP, _lib.ENOMEM), case
        assert set(case) - {"name", "code"} <= {"n_pairs", "rows", "dim", "host_null", "error_type", "device", "null"}, case
        assert (code == 0) == (case.get("n_pairs") == 0), case             # only the call with nothing to do succeeds
    assert (_lib.OK, _lib.EINVAL, _lib.ENODEV, _lib.EHIP, _lib.ENOMEM) == (0, -1, -2, -3, -4)          # include/mi_degensac.h
    assert sorted(c["null"] for c in R.REFUSALS if "null" in c) == ["mask", "model", "offsets", "pts1", "pts2", "seeds"]
    for kind in KINDS:
        for case in R.REFUSALS:
            a, b = R.refusal_batch(kind, case)
            assert len(a["p1"]) == R.REFUSAL_ROWS and len(b["p1"]) == (case["rows"][kind] if "rows" in case else R.REFUSAL_ROWS)
        assert R.REFUSALS[1]["rows"][kind] == R.MIN_ROWS[kind] - 1
