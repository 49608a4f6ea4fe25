"""Descriptor quantisation (mi_degensac_desc_quantize*, matcher.quantize_descriptors) without a device: every refusal of the two C
entry points with its message (all before the library looks for a device: this machine has none, so reaching that step would answer
ENODEV), the Python checks, presets and overrides, and the restatement the GPU tests compare with (tests/quantize_ref.py) against the
plain numpy formula, against exactly summed norms, against five deliberately wrong restatements and on rows written by hand."""
import ctypes as C
import math

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher
from tests import quantize_ref as qr

EINVAL = -1


# ---- C refusals ----------------------------------------------------------------------------------------------------------------
def _call(entry, qp, n=3, dim=8, inp=True, out=True):
    l = _lib.lib()
    a = np.zeros((max(n, 1), max(dim, 1)), np.float32); o = np.zeros((max(n, 1), 256), np.uint8)
    pa = a.ctypes.data_as(C.c_void_p) if inp else None
    po = o.ctypes.data_as(C.c_void_p) if out else None
    q = C.byref(qp) if qp is not None else None
    if entry == "dev":
        rc = l.mi_degensac_desc_quantize_dev(q, pa, n, dim, 0, None, po, None)
    else:
        rc = l.mi_degensac_desc_quantize(q, pa, n, dim, 0, po, None)
    return rc, l.mi_degensac_match_last_error().decode()


def _qp(normalize=1, scale=512.0, offset=0, struct_size=None):
    qp = _lib.QuantParams(normalize, scale, offset)
    if struct_size is not None:
        qp.struct_size = struct_size
    return qp


REFUSALS = [
    ("dim 0", dict(qp=_qp(), dim=0), "dim should be 1 .. 256"),
    ("dim -1", dict(qp=_qp(), dim=-1), "dim should be 1 .. 256"),
    ("dim 257", dict(qp=_qp(), dim=257), "dim should be 1 .. 256"),
    ("n < 0", dict(qp=_qp(), n=-1), "n < 0"),
    ("NULL qp", dict(qp=None), "quant params are NULL"),
    ("NULL input", dict(qp=_qp(), inp=False), "NULL argument"),
    ("NULL output", dict(qp=_qp(), out=False), "NULL argument"),
    ("normalize -1", dict(qp=_qp(normalize=-1)), "normalize should be 0"),
    ("normalize 3", dict(qp=_qp(normalize=3)), "normalize should be 0"),
    ("scale 0", dict(qp=_qp(scale=0.0)), "scale should be finite and > 0"),
    ("scale < 0", dict(qp=_qp(scale=-1.0)), "scale should be finite and > 0"),
    ("scale inf", dict(qp=_qp(scale=float("inf"))), "scale should be finite and > 0"),
    ("scale nan", dict(qp=_qp(scale=float("nan"))), "scale should be finite and > 0"),
    ("offset -1", dict(qp=_qp(offset=-1)), "offset should be 0 .. 255"),
    ("offset 256", dict(qp=_qp(offset=256)), "offset should be 0 .. 255"),
    ("struct_size 0", dict(qp=_qp(struct_size=0)), "struct_size does not cover offset"),
    ("struct_size 16", dict(qp=_qp(struct_size=16)), "struct_size does not cover offset"),
    ("struct_size 19", dict(qp=_qp(struct_size=19)), "struct_size does not cover offset"),
]


@pytest.mark.parametrize("entry", ["dev", "host"])
@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_c_refusals_come_before_the_device(entry, what, kw, msg):
    rc, err = _call(entry, **kw)
    assert rc == EINVAL and msg in err, (what, rc, err)


def test_c_misaligned_device_pointers_are_refused():
    l = _lib.lib()
    buf = np.zeros(256, np.uint8); base = buf.ctypes.data
    qp = _qp()
    for din, dout, dcl in ((base + 1, base + 64, None), (base, base + 66, None), (base, base + 64, base + 130)):
        rc = l.mi_degensac_desc_quantize_dev(C.byref(qp), din, 1, 4, 0, None, dout, dcl)
        assert rc == EINVAL and "4-byte aligned" in l.mi_degensac_match_last_error().decode()


@pytest.mark.parametrize("entry", ["dev", "host"])
def test_c_empty_call_succeeds_without_a_device(entry):
    assert _call(entry, _qp(), n=0)[0] == 0
    assert _call(entry, None, n=0, inp=False, out=False)[0] == 0           # touches nothing: nothing has to be there
    assert _call(entry, _qp(struct_size=20), n=0)[0] == 0                   # a struct_size that just covers offset
    rc, err = _call(entry, _qp(offset=300), n=0)                            # ... but what is given is still checked
    assert rc == EINVAL and "offset" in err


def test_pass_rows_follow_the_width():
    f = _lib.lib().mi_degensac_desc_quantize_pass_rows
    assert [f(d) for d in (0, 257)] == [0, 0]
    assert f(1) == f(64) == 2048 * 16 and f(65) == f(128) == 2048 * 8 and f(129) == f(256) == 2048 * 4


def test_struct_layout():
    assert C.sizeof(_lib.QuantParams) == 24 and _lib.QuantParams.offset.offset == 16 and _lib.QuantParams.scale.offset == 8


# ---- Python checks, presets, overrides -------------------------------------------------------------------------------------------
def test_presets():
    assert matcher.QUANT_PRESETS == {"sift": ("l2", 512.0, 0), "rootsift": ("l1root", 512.0, 0), "unit": ("l2", 256.0, 128)}
    assert matcher.quant_params("sift") == (1, 512.0, 0)
    assert matcher.quant_params("rootsift") == (2, 512.0, 0) == matcher.quant_params()
    assert matcher.quant_params("unit") == (1, 256.0, 128)
    assert {k: (matcher._QUANT_NORMALIZE[v[0]], v[1], v[2]) for k, v in matcher.QUANT_PRESETS.items()} == qr.PRESETS


def test_keywords_override_the_preset():
    assert matcher.quant_params("sift", normalize="none") == (0, 512.0, 0)
    assert matcher.quant_params("sift", normalize="l1root", scale=300) == (2, 300.0, 0)
    assert matcher.quant_params("unit", offset=0) == (1, 256.0, 0)
    assert matcher.quant_params("unit", scale=127.5, offset=np.int64(127)) == (1, 127.5, 127)
    assert matcher.quant_params("rootsift", normalize=1) == (1, 512.0, 0)


@pytest.mark.parametrize("kw,msg", [(dict(preset="hardnet"), "preset"), (dict(normalize="l1"), "normalize"), (dict(normalize=3), "normalize"),
                                    (dict(normalize=True), "normalize"), (dict(scale=0), "scale"), (dict(scale=-2.0), "scale"),
                                    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"), (dict(scale="big"), "scale"),
                                    (dict(offset=-1), "offset"), (dict(offset=256), "offset"), (dict(offset=1.5), "offset"),
                                    (dict(offset=True), "offset")])
def test_python_refuses_bad_parameters(kw, msg):
    with pytest.raises(ValueError, match=msg):
        matcher.quant_params(**kw)
    with pytest.raises(ValueError, match=msg):
        matcher.quantize_descriptors(np.zeros((2, 8), np.float32), **kw)


@pytest.mark.parametrize("desc", [np.zeros((2, 8), np.float64), np.zeros((2, 8), np.uint8), np.zeros((2, 8), np.float16), np.zeros(8, np.float32),
                                  np.zeros((2, 2, 4), np.float32), np.zeros((2, 0), np.float32), np.zeros((2, 257), np.float32)],
                         ids=["float64", "uint8", "float16", "1-D", "3-D", "dim 0", "dim 257"])
def test_python_refuses_dtype_shape_and_dim_before_the_library(desc, monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was called"))
    with pytest.raises(ValueError, match="descriptors to quantise"):
        matcher.quantize_descriptors(desc)


def test_tensor_form_refuses_before_the_library(monkeypatch):
    import torch
    from pydegensac_amd import tensor_api
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was called"))
    with pytest.raises(ValueError, match="ROCm device"):
        tensor_api.quantize_descriptors_tensors(torch.zeros((2, 8)))
    with pytest.raises(ValueError, match="ROCm device"):
        tensor_api.quantize_descriptors_tensors(np.zeros((2, 8), np.float32))


# ---- the restatement against the plain formula: integer-valued rows, whose sums are exact in any order ----------------------------
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 252, 255, 256])
def test_restatement_equals_the_plain_formula_on_integer_rows(dim):
    x = qr.sift_like(40, dim, dim)
    q, cl = qr.quantize(x, qr.L1ROOT, 512.0, 0)
    assert np.array_equal(q[:, :dim], qr.plain_rootsift(x).astype(np.uint8)) and not q[:, dim:].any()
    q2, cl2 = qr.quantize(x, qr.L2, 512.0, 0)
    assert np.array_equal(q2[:, :dim], qr.plain_l2(x).astype(np.uint8)) and not q2[:, dim:].any()
    assert (cl >= 0).all() and (cl2 >= 0).all()
    if dim == 1:                                       # 512 * 1 leaves the byte: the one column clips
        assert (q[:, 0] == 255).all() and (cl == 1).all() and (cl2 == 1).all()


def test_documented_sum_order_is_what_row_sums_runs():
    """lane sums in ascending column order, then the xor butterfly: spelled out once more with Python floats on one row"""
    x = qr.float_rows(1, 203, 9)[0].astype(np.float64)
    lanes = []
    for i in range(64):
        s = 0.0
        for k in range(4 * i, min(4 * i + 4, 203)):
            s = s + x[k] * x[k]
        lanes.append(s)
    for m in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[i] + lanes[i ^ m] for i in range(64)]
    assert len(set(lanes)) == 1
    assert qr.row_sums((x * x)[None])[0] == lanes[0]


# ---- random float rows against exactly summed norms --------------------------------------------------------------------------------
def _clamp(v):
    return np.minimum(255.0, np.maximum(0.0, v))


@pytest.mark.parametrize("name", ["sift", "rootsift", "unit"])
@pytest.mark.parametrize("dim", [5, 128, 255])
def test_restatement_within_the_rounding_bound_of_exact_norms(name, dim):
    """delta = (dim + 8) 2^-53: dim - 1 additions, square root, division, square root and multiplication, each within one rounding
    (the exact side's own square root, division and multiplication fit in the same allowance)"""
    nz, scale, offset = qr.PRESETS[name]
    x = qr.float_rows(60, dim, dim + len(name), signed=(name == "unit"))
    q, _ = qr.quantize(x, nz, scale, offset)
    xd = x.astype(np.float64)
    delta = (dim + 8) * 2.0 ** -53
    for i in range(x.shape[0]):
        if nz == qr.L2:
            v = scale * (xd[i] / math.sqrt(math.fsum(xd[i] * xd[i])))
        else:
            v = scale * np.copysign(np.sqrt(np.abs(xd[i]) / math.fsum(np.abs(xd[i]))), xd[i])
        lo = _clamp(np.rint(v * (1 - delta)) + offset); hi = _clamp(np.rint(v * (1 + delta)) + offset)
        got = q[i, :dim].astype(np.float64)
        assert ((got == lo) | (got == hi)).all(), (name, dim, i)


# ---- wrong restatements are told apart ---------------------------------------------------------------------------------------------
def test_round_half_up_is_rejected():
    x = np.array([[1, 3, 5]], np.float32)                     # 0.5, 1.5, 2.5 -> 0, 2, 2 (half to even), not 1, 2, 3
    good = qr.quantize(x, qr.NONE, 0.5, 0)[0]
    assert good[0].tolist() == [0, 2, 2, 0]
    assert not np.array_equal(good, qr.quantize(x, qr.NONE, 0.5, 0, "half_up")[0])


def test_truncation_is_rejected():
    x = np.array([[1.6, 2.7, 3.5, 0.9]], np.float32)
    good = qr.quantize(x, qr.NONE, 1.0, 0)[0]
    assert good[0].tolist() == [2, 3, 4, 1]
    assert not np.array_equal(good, qr.quantize(x, qr.NONE, 1.0, 0, "truncate")[0])


def test_missing_clamp_is_rejected():
    x = np.array([[300, -3, 255, 256]], np.float32)
    good, cl = qr.quantize(x, qr.NONE, 1.0, 0)
    assert good[0].tolist() == [255, 0, 255, 255] and cl[0] == 3
    assert not np.array_equal(good, qr.quantize(x, qr.NONE, 1.0, 0, "no_clamp")[0])


def test_l2_norm_where_l1_is_meant_is_rejected():
    x = np.array([[9, 16, 0, 0]], np.float32)                 # L1: 100 sqrt(9/25), 100 sqrt(16/25)
    good = qr.quantize(x, qr.L1ROOT, 100.0, 0)[0]
    assert good[0].tolist() == [60, 80, 0, 0]
    assert not np.array_equal(good, qr.quantize(x, qr.L1ROOT, 100.0, 0, "l2_for_l1")[0])


def test_dead_row_leaking_zero_is_rejected():
    x = np.array([[1, np.nan, 2, 3], [0, 0, 0, 0]], np.float32)
    good, cl = qr.quantize(x, qr.L2, 256.0, 128)
    assert good.tolist() == [[128] * 4] * 2 and cl.tolist() == [-1, -1]
    assert not np.array_equal(good, qr.quantize(x, qr.L2, 256.0, 128, "nan_to_zero")[0])


# ---- rows written by hand ----------------------------------------------------------------------------------------------------------
def test_hand_written_clip_counts_dead_rows_and_pad():
    inf = np.inf
    x = np.array([[0.0, 255.0, 255.4, 255.6, -0.4, -0.6, 1e30],      # v = 0, 255, 255, 256, -0, -1, 1e30: three leave the byte
                  [1, 2, 3, 4, 5, 6, 7],
                  [inf, 0, 0, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0, 0, -inf],
                  [0, 0, 0, np.nan, 0, 0, 0],
                  [0, 0, 0, 0, 0, 0, 0]], np.float32)
    q, cl = qr.quantize(x, qr.NONE, 1.0, 0)
    assert q.shape == (6, 8) and not q[:, 7].any()
    assert q[0].tolist() == [0, 255, 255, 255, 0, 0, 255, 0] and q[1].tolist() == [1, 2, 3, 4, 5, 6, 7, 0]
    assert cl.tolist() == [3, 0, -1, -1, -1, 0]                 # without a norm an all-zero row is a live row of zeros
    assert not q[2:].any()
    q, cl = qr.quantize(x, qr.NONE, 1.0, 7)
    assert q[2].tolist() == q[3].tolist() == q[4].tolist() == [7] * 7 + [0] and q[5].tolist() == [7] * 7 + [0]
    assert cl.tolist() == [4, 0, -1, -1, -1, 0] and q[0].tolist() == [7, 255, 255, 255, 7, 6, 255, 0]
    for nz in (qr.L2, qr.L1ROOT):
        q, cl = qr.quantize(x, nz, 256.0, 128)
        assert cl[2:].tolist() == [-1] * 4 and (q[2:, :7] == 128).all() and not q[:, 7].any()
        assert cl[0] == 1 and q[0, 6] == 255                     # 1e30 takes the whole norm: 128 + 256 clips
        assert cl[1] == {qr.L2: 2, qr.L1ROOT: 1}[nz]             # 128 + 256 * 6 / sqrt(140) and 7 / sqrt(140); 128 + 256 sqrt(7 / 28) = 256
    one = np.array([[2.0]], np.float32)
    assert qr.quantize(one, qr.L2, 256.0, 128)[0].tolist() == [[255, 0, 0, 0]]
    assert qr.quantize(-one, qr.L2, 100.0, 128)[0].tolist() == [[28, 0, 0, 0]]
    assert qr.quantize(-one, qr.L1ROOT, 100.0, 128)[0].tolist() == [[28, 0, 0, 0]]
