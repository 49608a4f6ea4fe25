"""GPU: descriptor quantisation (mi_degensac_desc_quantize[_dev], matcher.quantize_descriptors, tensor_api.quantize_descriptors_tensors).
Every comparison is equality of bytes and clip counts with the numpy restatement tests/quantize_ref.py (tests/test_quantize_cpu.py
checks that restatement by itself); integer-valued rows are compared with the plain numpy formula as well.

Run time of this file on one MI355X: a few seconds."""
import ctypes as C

import numpy as np
import pytest

from pydegensac_amd import _lib, matcher, tensor_api
from tests import matcher_u8_ref as ur
from tests import quantize_ref as qr

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 252, 255, 256]      # scalar and float4 loads, a partly used last lane, every pad 0 .. 3
COUNTS = [0, 1, 3, 4, 5, 255, 256, 257]
NORMALIZE = [qr.NONE, qr.L2, qr.L1ROOT]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _gpu(x, **kw):
    """the device form with the clip counts -> numpy (q [n, out_dim], clipped [n])"""
    q, cl = tensor_api.quantize_descriptors_tensors(_t(x), return_clipped=True, **kw)
    return q.cpu().numpy(), cl.cpu().numpy()


def _same(got, want, what):
    assert got[0].shape == want[0].shape and got[0].dtype == np.uint8 and got[1].dtype == np.int32, what
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1] != want[1]))
    assert bad.size == 0, (what, bad[:5], got[0][bad[:2]], want[0][bad[:2]], got[1][bad[:5]], want[1][bad[:5]])


def _mixed_rows(n, dim, seed):
    """float rows of both signs over several orders of magnitude, with a few integer-valued rows among them"""
    x = qr.float_rows(n, dim, seed)
    x[::7] = qr.sift_like(len(x[::7]), dim, seed + 1)
    return x


# ---- widths, row counts, parameters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", WIDTHS)
def test_every_width_and_row_count(dim):
    for n in COUNTS:
        x = _mixed_rows(n, dim, 100 * dim + n)
        for nz in NORMALIZE:
            for offset in (0, 128):
                scale = 512.0 if offset == 0 else 200.0
                _same(_gpu(x, normalize=nz, scale=scale, offset=offset), qr.quantize(x, nz, scale, offset), (dim, n, nz, offset))


@pytest.mark.parametrize("name", ["sift", "rootsift", "unit"])
@pytest.mark.parametrize("dim", [5, 64, 128, 129, 256])
def test_presets(name, dim):
    x = _mixed_rows(257, dim, dim + len(name))
    if name != "unit":
        x = np.abs(x)
    _same(_gpu(x, preset=name), qr.preset(x, name), (name, dim))


@pytest.mark.parametrize("dim", WIDTHS)
def test_integer_rows_equal_the_plain_formula(dim):
    x = qr.sift_like(130, dim, dim)
    q = _gpu(x, preset="rootsift")[0]
    assert np.array_equal(q[:, :dim], qr.plain_rootsift(x).astype(np.uint8)) and not q[:, dim:].any()
    q = _gpu(x, preset="sift")[0]
    assert np.array_equal(q[:, :dim], qr.plain_l2(x).astype(np.uint8)) and not q[:, dim:].any()


@pytest.mark.parametrize("dim", [5, 68, 130])
def test_second_step_of_the_grid_stride_loop(dim):
    """one row more than a pass of the launched grid covers (the library states that count per width: 16, 8 or 4 rows per workgroup)"""
    n = int(_lib.lib().mi_degensac_desc_quantize_pass_rows(dim)) + 1
    assert n == 2048 * {5: 16, 68: 8, 130: 4}[dim] + 1
    x = _mixed_rows(n, dim, dim)
    x[-1] = np.arange(1, dim + 1)
    _same(_gpu(x, preset="unit"), qr.preset(x, "unit"), dim)


# ---- rounding and clamping ---------------------------------------------------------------------------------------------------------
def test_ties_round_to_even_and_the_ends_clamp():
    x = np.array([[-1, 1, 3, 5, 509, 511],                          # scale 0.5: -0.5, 0.5, 1.5, 2.5, 254.5, 255.5
                  [-2e30, -300, -1, 256, 1e6, 3e38]], np.float32)
    q, cl = _gpu(x, normalize="none", scale=0.5, offset=0)
    assert q[0].tolist() == [0, 0, 2, 2, 254, 255, 0, 0] and cl[0] == 1          # only 255.5 -> 256 leaves the byte (-0.5 -> -0)
    q, cl = _gpu(x, normalize="none", scale=1.0, offset=0)
    assert q[1].tolist() == [0, 0, 0, 255, 255, 255, 0, 0] and cl[1] == 6
    q, cl = _gpu(x, normalize="none", scale=1.0, offset=1)
    assert q[1].tolist() == [0, 0, 0, 255, 255, 255, 0, 0] and cl[1] == 5        # -1 + 1 = 0 stays inside
    for scale, offset in ((0.5, 0), (1.0, 0), (1.0, 1), (0.5, 128)):
        _same(_gpu(x, normalize="none", scale=scale, offset=offset), qr.quantize(x, qr.NONE, scale, offset), (scale, offset))


# ---- dead rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [7, 128, 200])          # 16, 8 and 4 rows per workgroup
@pytest.mark.parametrize("kind", ["nan", "+inf", "-inf", "zero"])
def test_dead_rows_leave_their_neighbours_alone(dim, kind):
    rpb = int(_lib.lib().mi_degensac_desc_quantize_pass_rows(dim)) // 2048
    n = 3 * rpb + 2
    x = _mixed_rows(n, dim, dim)
    clean = {nz: _gpu(x, normalize=nz, scale=256.0, offset=128) for nz in NORMALIZE}
    rows = [rpb, rpb + rpb // 2, 2 * rpb - 1, n - 1]          # first, middle and last row of a workgroup, the last row overall
    y = x.copy()
    for i, r in enumerate(rows):
        if kind == "zero":
            y[r] = 0
        else:
            y[r, (i * 37) % dim] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    for nz in NORMALIZE:
        q, cl = _gpu(y, normalize=nz, scale=256.0, offset=128)
        _same((q, cl), qr.quantize(y, nz, 256.0, 128), (dim, kind, nz))
        live = np.setdiff1d(np.arange(n), rows)
        assert np.array_equal(q[live], clean[nz][0][live]) and np.array_equal(cl[live], clean[nz][1][live])
        if kind == "zero" and nz == qr.NONE:
            assert (cl[rows] == 0).all()                   # without a norm a row of zeros is a live row
        else:
            assert (cl[rows] == -1).all()
        assert (q[rows][:, :dim] == 128).all() and not q[rows][:, dim:].any()


def test_extreme_magnitudes():
    tiny = np.float32(1.401298464324817e-45)                # the smallest denormal: its square is a normal float64
    x = np.zeros((4, 6), np.float32)
    x[0, 2] = tiny; x[1] = 3e38; x[2, :3] = [tiny, -tiny, 3e38]; x[3, 1] = -3e38
    for nz in (qr.L2, qr.L1ROOT):
        got = _gpu(x, normalize=nz, scale=100.0, offset=100)
        _same(got, qr.quantize(x, nz, 100.0, 100), nz)
        assert (got[1] == 0).all()                          # nothing overflowed, nothing died
        assert got[0][0].tolist() == [100, 100, 200, 100, 100, 100, 0, 0] and got[0][3].tolist() == [100, 0, 100, 100, 100, 100, 0, 0]
    assert _gpu(x, normalize=qr.L2, scale=100.0, offset=100)[0][1].tolist() == [141] * 6 + [0, 0]           # 100 / sqrt(6) = 40.8


# ---- pad bytes, optional output ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 5, 126, 127, 253])
def test_pad_bytes_are_written_as_zero(dim):
    import torch
    x = _mixed_rows(37, dim, dim)
    out = torch.full((37, (dim + 3) & ~3), 0xFF, dtype=torch.uint8, device=_dev())
    got = tensor_api.quantize_descriptors_tensors(_t(x), "unit", out=out)                 # no clipped output
    assert got is out
    assert np.array_equal(out.cpu().numpy(), qr.preset(x, "unit")[0])
    assert not out[:, dim:].any()


def test_out_is_checked():
    import torch
    x = _t(np.ones((4, 6), np.float32))
    for bad in (torch.zeros((4, 6), dtype=torch.uint8, device=_dev()), torch.zeros((4, 8), dtype=torch.int8, device=_dev()),
                torch.zeros((8, 8), dtype=torch.uint8, device=_dev())[::2], torch.zeros((4, 8), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out should be"):
            tensor_api.quantize_descriptors_tensors(x, out=bad)


# ---- entry points ------------------------------------------------------------------------------------------------------------------
def test_device_form_on_a_second_stream():
    import torch
    x = _mixed_rows(1000, 128, 5)
    s = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(s):
        q, cl = tensor_api.quantize_descriptors_tensors(_t(x), "sift", return_clipped=True)
    s.synchronize()
    _same((q.cpu().numpy(), cl.cpu().numpy()), qr.preset(x, "sift"), "second stream")


@pytest.mark.parametrize("dim,shift", [(5, 0), (127, 0), (129, 0), (128, 1), (128, 2), (64, 3), (128, 0)])
def test_store_inside_a_larger_allocation(dim, shift):
    """rows 3 .. of a larger store, for odd dim at a row base that is not 16-byte aligned, and (shift) whole-word rows moved 1 .. 3
    floats off the allocation's alignment: single floats are read there, with the same result"""
    import torch
    x = _mixed_rows(70, dim, dim + shift)
    flat = torch.zeros(70 * dim + 8, dtype=torch.float32, device=_dev())
    flat[shift:shift + 70 * dim] = _t(x).flatten()
    view = flat[shift:shift + 70 * dim].view(70, dim)[3:]
    assert view.is_contiguous() and view.data_ptr() != flat.data_ptr()
    assert (view.data_ptr() % 16 != 0) == (shift != 0 or dim in (5, 127, 129))
    q, cl = tensor_api.quantize_descriptors_tensors(view, "unit", return_clipped=True)
    _same((q.cpu().numpy(), cl.cpu().numpy()), qr.preset(x[3:], "unit"), (dim, shift))


def test_host_c_entry_point():
    x = _mixed_rows(301, 130, 8)
    out = np.full((301, 132), 0xFF, np.uint8); cl = np.full(301, 77, np.int32)
    qp = _lib.QuantParams(qr.L1ROOT, 300.0, 20)
    l = _lib.lib()
    rc = l.mi_degensac_desc_quantize(C.byref(qp), x.ctypes.data_as(C.c_void_p), 301, 130, 0, out.ctypes.data_as(C.c_void_p),
                                     cl.ctypes.data_as(C.c_void_p))
    assert rc == 0, l.mi_degensac_match_last_error().decode()
    _same((out, cl), qr.quantize(x, qr.L1ROOT, 300.0, 20), "host, clipped")
    out2 = np.full((301, 132), 0xFF, np.uint8)
    assert l.mi_degensac_desc_quantize(C.byref(qp), x.ctypes.data_as(C.c_void_p), 301, 130, 0, out2.ctypes.data_as(C.c_void_p), None) == 0
    assert np.array_equal(out2, out)


def test_numpy_call_trims_the_pad():
    x = np.abs(_mixed_rows(90, 130, 3))
    want = qr.preset(x, "rootsift")
    q = matcher.quantize_descriptors(x)
    assert q.shape == (90, 130) and q.dtype == np.uint8 and q.flags.c_contiguous and np.array_equal(q, want[0][:, :130])
    q, cl = matcher.quantize_descriptors(x, "sift", scale=300, offset=3, return_clipped=True)
    want = qr.quantize(x, qr.L2, 300.0, 3)
    assert np.array_equal(q, want[0][:, :130]) and np.array_equal(cl, want[1]) and cl.dtype == np.int32
    assert matcher.quantize_descriptors(np.zeros((0, 7), np.float32)).shape == (0, 7)


# ---- the chain into the matcher ------------------------------------------------------------------------------------------------------
def test_quantised_store_enters_the_pair_list_matcher():
    """5 images of 0 .. 129 rows, dim 126 (two pad bytes): quantise on the device, match every pair under "l2_u8", and compare with
    the float32 matcher on the same bytes cast to float32, bit for bit"""
    counts = [129, 0, 64, 65, 1]
    x = qr.float_rows(sum(counts), 126, 11)
    q = tensor_api.quantize_descriptors_tensors(_t(x), "unit")
    assert tuple(q.shape) == (sum(counts), 128)
    pairs = matcher.exhaustive_pairs(5)
    got = tensor_api.knn_match_pairs_tensors(q, q, counts, counts, pairs, norm="l2_u8")
    want = tensor_api.knn_match_pairs_tensors(q.float(), q.float(), counts, counts, pairs, norm="l2")
    got = (got[0].cpu().numpy(), got[1].cpu().numpy()); want = (want[0].cpu().numpy(), want[1].cpu().numpy())
    assert np.array_equal(got[0], want[0]) and ur.same_bits(got, want)
    assert (got[0][:, 0] >= 0).sum() > 0
    assert np.array_equal(q.cpu().numpy(), qr.preset(x, "unit")[0])
