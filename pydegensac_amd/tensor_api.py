"""Device-resident batch API: correspondences and results stay in HBM.

The natural caller of a robust estimator is a matching pipeline that already holds its tentative
correspondences on the GPU.  These functions take `torch` tensors on a ROCm device (anything exposing
`data_ptr()`, float64, C-contiguous), run the same persistent kernels through the `*_batch_dev` entry points
of include/mi_degensac.h on the tensor's current stream, and return tensors — no host staging, no
synchronisation.  Marshalling rules follow bindings.cpp:126-198 (rows are [x, y] or [x, y, a11, a12, a21,
a22]); seeds follow pydegensac_amd.parallel.pair_seeds unless given (any uint32 value is allowed).
"""
import ctypes as C

import numpy as np

from . import _lib
from .api import error_type_dict_fundamental, error_type_dict_homography
from .matcher import _sd


# ---- the plumbing every call shares: the two tensor refusals, pointers, the stream, keeping inputs alive, result fills ----
def _require(names, tensors, device=None):
    """The two tensor refusals of a call, under the names its texts use.  device None: every argument is a torch tensor.  "same": they
    live on one device; "cuda": and it is a ROCm one (where "same" leaves that to _desc_pair, whose text differs)."""
    import torch
    if device is None:
        if not all(isinstance(t, torch.Tensor) for t in tensors):
            raise ValueError(f"{names} must be torch tensors on a ROCm device")
    elif any(t.device != tensors[0].device for t in tensors) or (device == "cuda" and tensors[0].device.type != "cuda"):
        raise ValueError(f"{names} must live on the same ROCm device")


def _p(t, empty_none=False):
    """the device pointer of a tensor; None stays None (a nullable argument), and with empty_none so does a tensor without elements"""
    return None if t is None or (empty_none and t.numel() == 0) else t.data_ptr()


def _stream(dev):
    """(device index, current stream, its handle as the entry points take it)"""
    import torch
    stream = torch.cuda.current_stream(dev)
    return dev.index or 0, stream, C.c_void_p(stream.cuda_stream)


def _keep_alive(stream, *tensors):
    """the kernels read their inputs asynchronously: keep them alive until the stream reaches this point"""
    for t in tensors:
        if t is not None:
            t.record_stream(stream)


def _knn_out(n, dev, with_match=False):
    """the 2-NN result tensors of n query rows with their fills: idx -1, dist inf, and with with_match match -1 (else None)"""
    import torch
    return (torch.full((n, 2), -1, dtype=torch.int32, device=dev), torch.full((n, 2), float("inf"), dtype=torch.float32, device=dev),
            torch.full((n,), -1, dtype=torch.int32, device=dev) if with_match else None)


def _store_kps(kind, kps1, kps2, per_store):
    """the keypoints of the two sides as float64 rows; per_store: a store named on both sides is converted once"""
    conv = kpts_to_xyA_tensors if kind == "kpts" else (lambda k: k.contiguous())
    k1 = conv(kps1)
    return k1, k1 if per_store and kps2 is kps1 else conv(kps2)


def _driver_models(models, model, driver_form, K):
    """the models of a call as the library takes them: contiguous float64 [K, 9], the user-facing H converted on the device"""
    M = models.contiguous()
    if model == "H" and not driver_form:
        M = _h_driver_form(M)
    return M.reshape(K, 9).contiguous()


def _cam_index(pairs, n1, n2):
    """matcher._cam_index on a device tensor, without a host round trip"""
    import torch
    wide = pairs.to(torch.int64)
    if n2 is not None:                                                # an image of store 1 must not reach into store 2's rows
        a = torch.where((wide[:, 0] < 0) | (wide[:, 0] >= n1), -1, wide[:, 0])
        b = torch.where(wide[:, 1] < 0, -1, wide[:, 1] + n1)
        wide = torch.stack([a, b], 1)
    return wide.clamp(-1, 0x7fffffff).to(torch.int32).contiguous()


def _cameras(cams1, cams2, pairs, K, n1, n2):
    """the camera table of the pose calls -> (cams, n_cams, cam_idx int32 [K, 2] or None = two rows per entry)"""
    import torch
    if pairs is None:
        return cams1.contiguous(), 2 * K, None
    return cams1.contiguous() if cams2 is None else torch.cat([cams1, cams2]), n1 + (n2 or 0), _cam_index(pairs, n1, n2)


def _prep(pts1, pts2, counts):
    import torch
    if not (isinstance(pts1, torch.Tensor) and isinstance(pts2, torch.Tensor)):
        raise ValueError("pts1/pts2 must be torch tensors on the GPU")
    if pts1.device.type != "cuda" or pts2.device != pts1.device:
        raise ValueError("pts1/pts2 must live on the same ROCm device")
    if pts1.dtype != torch.float64 or pts2.dtype != torch.float64:
        raise ValueError("correspondences must be float64 (the path is fp64 end to end)")
    if pts1.dim() != 2 or pts1.shape != pts2.shape or pts1.shape[1] not in (2, 6):
        raise ValueError("expected two [total, 2] or [total, 6] tensors of equal shape")
    counts = np.asarray(counts, dtype=np.int64).ravel()
    offs = np.zeros(len(counts) + 1, dtype=np.int64); np.cumsum(counts, out=offs[1:])
    if offs[-1] != pts1.shape[0]:
        raise ValueError("counts do not add up to the number of rows")
    return pts1.contiguous(), pts2.contiguous(), offs


def _run(which, pts1, pts2, counts, prm, seeds, min_n):
    import torch
    from . import parallel
    pts1, pts2, offs = _prep(pts1, pts2, counts)
    P = len(offs) - 1
    if P == 0 or (np.diff(offs) < min_n).any():
        raise ValueError(f"every pair needs at least {min_n} correspondences")
    dev = pts1.device
    if seeds is None:
        seeds = parallel.pair_seeds(0, P)
    # uint32 seeds travel as their int32 bit pattern (torch has no uint32 arithmetic; the kernel reads them as unsigned)
    d_seeds = torch.from_numpy((np.asarray(seeds, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    model = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    mask = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)
    stats = torch.zeros((P, 16), dtype=torch.int32, device=dev)
    di, stream, sp = _stream(dev)
    fn = _lib.lib().mi_degensac_find_fundamental_batch_dev if which == "F" else _lib.lib().mi_degensac_find_homography_batch_dev
    rc = fn(_p(pts1), _p(pts2), _p(d_off), _lib.ptr(offs), P, int(pts1.shape[1]), C.byref(prm), _p(d_seeds), di, sp, _p(model), _p(mask), _p(stats))
    _lib.check(rc)
    _keep_alive(stream, d_off, d_seeds, pts1, pts2)
    return model.view(P, 3, 3), mask.to(torch.bool), stats, offs


def find_fundamental_batch_tensors(pts1, pts2, counts, px_th=0.5, conf=0.9999, max_iters=100000,
                                   laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True,
                                   enable_degeneracy_check=True, seeds=None):
    """P independent pairs, rows of pair p = pts[offs[p]:offs[p+1]] with offs = cumsum(counts).
    Returns (F [P,3,3] float64, mask [total] bool, stats [P,16] int32, offsets) — all but offsets on the device.
    stats columns = include/mi_degensac.h MI_ST_* (column 15: placement in bits 0-7, bit 8 = the pair was set aside once)."""
    et = error_type_dict_fundamental[error_type.lower()]
    prm = _lib.make_params(px_th, conf, max_iters, et, symmetric_error_check, max(0.0, laf_consistensy_coef), enable_degeneracy_check)
    return _run("F", pts1, pts2, counts, prm, seeds, 8)


def find_homography_batch_tensors(pts1, pts2, counts, px_th=1.0, conf=0.999, max_iters=50000, laf_consistensy_coef=-1.0,
                                  error_type="sampson", symmetric_error_check=True, seeds=None):
    """As above for homographies.  Returns the reference's user-facing H = inv(H_c^T) (utils.py:108), zeros when no
    model was found (the inversion runs on the device with torch.linalg)."""
    import torch
    et = error_type_dict_homography[error_type.lower()]
    prm = _lib.make_params(px_th, conf, max_iters, et, symmetric_error_check, max(0.0, laf_consistensy_coef), True)
    Hc, mask, stats, offs = _run("H", pts1, pts2, counts, prm, seeds, 4)
    found = Hc.abs().sum(dim=(1, 2)) != 0
    out = torch.zeros_like(Hc)
    if bool(found.any()):
        out[found] = torch.linalg.inv(Hc[found].transpose(1, 2))
    return out, mask, stats, offs


# ---- the stage in front of the estimators on the device: matcher and keypoint conversion -------------
def knn_match_tensors(desc1, desc2, norm=None):
    """cv2 `BFMatcher().knnMatch(descs1, descs2, k=2)` (examples/simple-example.py:46-47) on device tensors: float32
    descriptors [n, dim] -> L2, uint8 [n, dim] (dim % 4 == 0) -> Hamming; norm="l2_u8" takes uint8 rows (dim % 4 == 0, dim <= 256)
    under L2, bit-identical to the float32 path on the same values (norm None / "l2" / "hamming": the dtype's norm, as before).
    Returns (idx [n1, 2] int32, dist [n1, 2] float32) on the device, asynchronous on the current stream."""
    import torch
    if not (isinstance(desc1, torch.Tensor) and isinstance(desc2, torch.Tensor)) or desc1.device.type != "cuda" or desc2.device != desc1.device:
        raise ValueError("descriptors must be torch tensors on the same ROCm device")
    if desc1.dim() != 2 or desc2.dim() != 2 or desc1.shape[1] != desc2.shape[1] or desc1.dtype != desc2.dtype:
        raise ValueError("descriptors should be [n1, dim] and [n2, dim] tensors of one dtype")
    if norm not in (None, "l2", "hamming", "l2_u8"):
        raise ValueError("norm should be None, 'l2', 'hamming' or 'l2_u8'")
    if desc1.dtype == torch.float32 and norm in (None, "l2"):
        norm = 0
    elif desc1.dtype == torch.uint8 and desc1.shape[1] % 4 == 0 and norm in (None, "hamming"):
        norm = 1
    elif desc1.dtype == torch.uint8 and desc1.shape[1] % 4 == 0 and norm == "l2_u8":
        if desc1.shape[1] > 256:
            raise ValueError("norm 'l2_u8' takes dim <= 256: use float32 descriptors with norm 'l2' beyond that")
        norm = 4
    else:
        raise ValueError("float32 descriptors (L2) or uint8 descriptors with dim % 4 == 0 (Hamming, or L2 with norm='l2_u8')")
    a = desc1.contiguous(); b = desc2.contiguous(); dev = a.device
    # the kernel reads descriptor rows as 32-bit words: a contiguous view into a packed buffer may start at any byte
    if a.data_ptr() % 4: a = a.clone()
    if b.data_ptr() % 4: b = b.clone()
    n1, n2, dim = a.shape[0], b.shape[0], a.shape[1]
    idx, dist, _ = _knn_out(n1, dev)
    di, stream, sp = _stream(dev)
    _lib.check_match(_lib.lib().mi_degensac_match_knn2_dev(norm, _p(a), n1, _p(b), n2, dim, di, sp, _p(idx), _p(dist)), value_error=False)
    _keep_alive(stream, a, b)
    return idx, dist


def match_filter_tensors(idx, dist, ratio=0.9, back=None):
    """The ratio test `dist[:, 0] < ratio * dist[:, 1]` (a query without a second neighbour is not kept) on a 2-NN result, and with
    back (the idx of the reverse search) the mutual check; returns keep [n1] uint8 on the device, asynchronous on the current stream."""
    import torch
    dev = idx.device; n1 = idx.shape[0]
    keep = torch.zeros(n1, dtype=torch.uint8, device=dev)
    di, stream, sp = _stream(dev)
    _lib.check_match(_lib.lib().mi_degensac_match_filter_dev(_p(idx), _p(dist), n1, float(ratio), _p(back), di, sp, _p(keep)))
    _keep_alive(stream, idx, dist, back)
    return keep


def match_decide_tensors(idx, dist, ratio=0.9, back=None, back_dist=None, max_dist=None, back_ratio=False):
    """match_filter_tensors under the decision rule (include/mi_degensac.h mi_degensac_match_decide_dev): ratio=None drops the ratio test
    (a query with a nearest neighbour is kept, a second train row is not needed), back (the idx of the reverse search) adds the mutual
    check, back_ratio=True (with back and back_dist, the reverse search's idx and dist) the ratio test at the train row's own reverse
    search, max_dist the threshold dist[:, 0] <= max_dist.  Returns keep [n1] uint8 on the device, asynchronous on the current stream."""
    import torch
    from . import matcher
    if back_ratio and (back is None or back_dist is None):
        raise ValueError("back_ratio=True needs back and back_dist, the idx and dist of the reverse search")
    rule = matcher.check_rule(ratio, "ratio" if back_ratio else back is not None, max_dist)
    dev = idx.device; n1 = idx.shape[0]
    keep = torch.zeros(n1, dtype=torch.uint8, device=dev)
    di, stream, sp = _stream(dev)
    mp = _lib.MatchParamsEx(0, 0, rule.ratio, rule.mutual, None, rule.decide, rule.max_dist)
    _lib.check_match(_lib.lib().mi_degensac_match_decide_dev(C.byref(mp), _p(idx), _p(dist), n1, _p(back), _p(back_dist), di, sp, _p(keep)))
    _keep_alive(stream, idx, dist, back, back_dist)
    return keep


def match_snn_tensors(desc1, desc2, ratio=0.9, mutual=False, norm=None, *, max_dist=None):
    """The ratio test of the example (`m.distance < ratio * n.distance`, simple-example.py:49-53), optionally restricted to
    mutual nearest neighbours, on the device: (query indices, train indices, distances) of the tentative correspondences.
    norm as for knn_match_tensors.  The only host synchronisation is the final boolean selection (the number of survivors sizes the
    outputs).  ratio=None, mutual="ratio" and max_dist: the decision rule of matcher.check_rule, through match_decide_tensors."""
    import torch
    from . import matcher
    rule = matcher.check_rule(ratio, mutual, max_dist)
    idx, dist = knn_match_tensors(desc1, desc2, norm)
    if rule.decide:
        back, bdist = knn_match_tensors(desc2, desc1, norm) if rule.mutual and desc2.shape[0] > 0 else (None, None)
        if rule.mutual and back is None:                     # no train row: nothing to keep, and no reverse search to read
            keep = torch.zeros(idx.shape[0], dtype=torch.uint8, device=idx.device)
        else:
            keep = match_decide_tensors(idx, dist, ratio, back, bdist, max_dist, bool(rule.decide & _lib.DECIDE_BACK_RATIO))
    else:
        keep = match_filter_tensors(idx, dist, ratio, knn_match_tensors(desc2, desc1, norm)[0] if mutual and desc2.shape[0] > 0 else None)
    sel = torch.nonzero(keep, as_tuple=False).flatten()
    return sel, idx[sel, 0].to(torch.int64), dist[sel, 0]


def kpts_to_xyA_tensors(kpts):
    """utils.py:24-41 `convert_cv2_kpts_to_xyA` on the device: [n, 4] float32 (x, y, size, angle in degrees) -> [n, 6] float64"""
    import torch
    if not isinstance(kpts, torch.Tensor) or kpts.device.type != "cuda" or kpts.dtype != torch.float32 or kpts.dim() != 2 or kpts.shape[1] != 4:
        raise ValueError("keypoints should be a float32 tensor [n, 4] = (x, y, size, angle) on a ROCm device")
    k = kpts.contiguous(); dev = k.device
    out = torch.zeros((k.shape[0], 6), dtype=torch.float64, device=dev)
    di, stream, sp = _stream(dev)
    _lib.check_match(_lib.lib().mi_degensac_kpts_to_xyA_dev(_p(k), k.shape[0], di, sp, _p(out)), value_error=False)
    _keep_alive(stream, k)
    return out


def quantize_descriptors_tensors(desc, preset="rootsift", *, normalize=None, scale=None, offset=None, out=None, return_clipped=False):
    """matcher.quantize_descriptors on a device tensor (include/mi_degensac.h mi_degensac_desc_quantize_dev): float32 [n, dim] with
    dim <= 256 -> uint8 [n, out_dim], out_dim = dim rounded up to a multiple of 4 with zero pad bytes: the width the norm="l2_u8"
    tensor calls take.  preset / normalize / scale / offset as there.  out: None, or a contiguous uint8 tensor [n, out_dim] on the same
    device to write into.  return_clipped=True adds clipped [n] int32 (-1 for a dead row).  Asynchronous on the current stream; an
    "l2_u8" distance between quantised rows is about scale x the float distance of the normalised rows."""
    import torch
    from . import matcher
    if not isinstance(desc, torch.Tensor) or desc.device.type != "cuda":
        raise ValueError("descriptors must be a torch tensor on a ROCm device")
    matcher.check_quantize_input(tuple(desc.shape), desc.dtype)
    nz, sc, of = matcher.quant_params(preset, normalize, scale, offset)
    a = desc.contiguous(); dev = a.device
    n, dim = a.shape; out_dim = (dim + 3) & ~3
    if out is None:
        out = torch.empty((n, out_dim), dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (n, out_dim)
              and out.is_contiguous() and out.data_ptr() % 4 == 0):
        raise ValueError(f"out should be a contiguous, 4-byte aligned uint8 tensor [{n}, {out_dim}] on the descriptors' device")
    clipped = torch.empty(n, dtype=torch.int32, device=dev) if return_clipped else None
    di, stream, sp = _stream(dev)
    qp = _lib.QuantParams(nz, sc, of)
    _lib.check_match(_lib.lib().mi_degensac_desc_quantize_dev(C.byref(qp), _p(a), n, dim, di, sp, _p(out), _p(clipped)))
    _keep_alive(stream, a)
    return (out, clipped) if return_clipped else out


# ---- many image pairs: descriptors + keypoints -> tentatives -> F / H on the device (include/mi_degensac.h mi_degensac_match_*_batch*) ----
def _word_aligned(t):
    # the kernels read descriptor rows as 32-bit words: a contiguous view into a packed buffer may start at any byte
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 4 else t


def _desc_pair(desc1, desc2):
    import torch
    if not (isinstance(desc1, torch.Tensor) and isinstance(desc2, torch.Tensor)) or desc1.device.type != "cuda" or desc2.device != desc1.device:
        raise ValueError("descriptors must be torch tensors on the same ROCm device")
    if desc1.dtype == torch.uint8 and desc1.shape[1] % 4:
        raise ValueError("uint8 descriptors (Hamming, L2 with norm='l2_u8') need dim % 4 == 0: pad with zero bytes")
    return _word_aligned(desc1), _word_aligned(desc2)


def knn_match_batch_tensors(desc1, desc2, counts1, counts2, norm=None):
    """knn_match_tensors for K image pairs in one launch: pair p's queries are the next counts1[p] rows of desc1, its train set the
    next counts2[p] rows of desc2.  Returns (idx [N1, 2] int32 with indices LOCAL to the pair, dist [N1, 2] float32) on the device,
    per pair bit-identical to knn_match_tensors on that pair; asynchronous on the current stream.  norm: None = the dtype's norm
    (float32 L2, uint8 Hamming), or "l2" / "hamming" / "l2_u8" (uint8 rows under L2, dim <= 256)."""
    from . import matcher
    _require("descriptors", (desc1, desc2))
    code, _, o1, o2 = matcher.check_match_verify_args("F", 1.0, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape), desc2.dtype,
                                                      (desc1.shape[0], 2), np.float64, (desc2.shape[0], 2), np.float64, counts1, counts2)
    return _knn2_dev(matcher.layout(o1, o2), code, *_desc_pair(desc1, desc2), value_error=False)


def _knn2_dev(L, code, a, b, k2=None, r=None, value_error=True):
    """mi_degensac_match_knn2_* (k2 and r given: mi_degensac_match_fginn_knn2_*, the FGINN second neighbour at radius r on the keypoints
    k2) of the checked layout L on prepared device tensors, asynchronous on the current stream.  Returns (idx [n, 2], dist [n, 2])."""
    from . import matcher
    dev = a.device
    idx, dist, _ = _knn_out(L.n, dev)
    di, stream, sp = _stream(dev)
    fginn = () if k2 is None else (_p(k2), int(k2.shape[1]), r)
    entry = getattr(_lib.lib(), f"mi_degensac_match_{'' if k2 is None else 'fginn_'}knn2_{L.name}_dev")
    _lib.check_match(entry(code, _p(a), _p(b), *matcher.knn_layout(L, int(a.shape[1])), *fginn, di, sp, _p(idx), _p(dist)), value_error)
    _keep_alive(stream, a, b, k2)
    return idx, dist


def _fginn_knn2_args(desc1, desc2, kps2, spatial_th):
    """the checks of the two FGINN knn2 calls in front of their layout check -> the checked radius"""
    from . import matcher
    import torch
    _require("desc1, desc2 and kps2", (desc1, desc2, kps2))
    r = matcher.check_fginn_th(spatial_th, "spatial_th")
    if kps2.dim() != 2 or kps2.dtype != torch.float64 or kps2.shape[1] not in (2, 6):
        raise ValueError("keypoints should be float64 [n, 2] / [n, 6] rows")
    return r


def knn_match_fginn_batch_tensors(desc1, desc2, kps2, counts1, counts2, spatial_th=10.0, norm=None):
    """knn_match_batch_tensors with the FGINN rule for the second neighbour (include/mi_degensac.h
    mi_degensac_match_fginn_knn2_batch_dev): slot 0 is the nearest train row as before; slot 1 is the nearest train row of the pair
    whose keypoint (kps2: float64 [N2, 2] / [N2, 6] on the device, only x, y are read) lies at least spatial_th from the keypoint of
    slot 0 (dx*dx + dy*dy >= spatial_th**2 in float64; NaN never competes), -1 / inf when there is none.  spatial_th=0 with finite
    keypoints gives knn_match_batch_tensors bit for bit.  Returns (idx [N1, 2] int32, dist [N1, 2] float32) on the device,
    asynchronous on the current stream (no host synchronisation)."""
    from . import matcher
    r = _fginn_knn2_args(desc1, desc2, kps2, spatial_th)
    code, _, o1, o2 = matcher.check_match_verify_args("F", 1.0, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape), desc2.dtype,
                                                      (desc1.shape[0], kps2.shape[1]), np.float64, tuple(kps2.shape), kps2.dtype, counts1, counts2)
    _require("desc1, desc2 and kps2", (desc1, kps2), "same")
    return _knn2_dev(matcher.layout(o1, o2), code, *_desc_pair(desc1, desc2), kps2.contiguous(), r)


def _guided_dev(L, code, a, b, k1, k2, Md, model, rule, px, et, fginn_r=None):
    """mi_degensac_match_guided_{batch,pairs}_dev (fginn_r, a checked radius: mi_degensac_match_guided_fginn_*_dev) of the checked layout
    L on prepared device tensors (Md: [K, 9] driver-form models), asynchronous on the current stream.  Returns (match [n] int32,
    idx [n, 2] int32, dist [n, 2] float32)."""
    from . import matcher
    dev = a.device
    idx, dist, match = _knn_out(L.n, dev, True)
    mp = _lib.match_params(code, a.shape[1], rule, fginn_r); gp = _lib.GuideParams(model == "H", et, px)
    di, stream, sp = _stream(dev)
    rc = matcher.guided_entry(f"{L.name}_dev", fginn_r)(C.byref(mp), _p(a), _p(b), *matcher.guided_layout(L, _p(k1), _p(k2), int(k1.shape[1])),
                                                        _p(Md), C.byref(gp), di, sp, _p(idx), _p(dist), _p(match), None, None)
    _lib.check_match(rc)
    _keep_alive(stream, a, b, k1, k2, Md)
    return match, idx, dist


def _h_driver_form(M):
    """the user-facing H [K, 3, 3] -> the driver's H_c = inv(H)^T where the model is not zero, without a host round trip (inv_ex: no error
    check, no sync); zero models stay zero"""
    import torch
    K = M.shape[0]
    found = (M.abs().sum(dim=(1, 2)) != 0).view(K, 1, 1)
    eye = torch.eye(3, dtype=M.dtype, device=M.device).expand(K, 3, 3)
    return torch.where(found, torch.linalg.inv_ex(torch.where(found, M, eye)).inverse.transpose(1, 2), torch.zeros_like(M))


def guided_match_batch_tensors(kps1, kps2, desc1, desc2, counts1, counts2, models, model="F", ratio=0.9, mutual=False, px_th=None,
                               error_type="sampson", norm=None, driver_form=False, fginn_th=None, *, max_dist=None):
    """Guided matching on the device (include/mi_degensac.h mi_degensac_match_guided_batch_dev): per pair the 2-NN search of
    knn_match_batch_tensors restricted to the train keypoints that are inliers of the pair's model under the estimator's own residual
    for error_type and its threshold from px_th (None = the model's default: 0.5 for F, 1.0 for H), then the ratio test (and, with
    mutual, the reverse guided search).  A query with a single gated train row passes the ratio test (nothing competes with it); a
    zero model gives its pair no matches.  models: [K, 3, 3] float64 on the device — F, or the user-facing H (converted here to the
    driver's form H_c = inv(H)^T without a host round trip); driver_form=True takes them as the *_batch_dev entry points write them.
    Keypoints and descriptors as for match_and_verify_batch_tensors.  Cost follows the rows that pass the gate; a gate that passes
    everything (a huge px_th) is correct but slower than the unguided matcher.  Returns (match [N1] int32 = pair-local train row or -1,
    idx [N1, 2] int32, dist [N1, 2] float32) on the device, asynchronous on the current stream (no host synchronisation).
    fginn_th: None = this call through mi_degensac_match_guided_batch_dev; a number (pixels of kps2, finite and >= 0) goes to
    mi_degensac_match_guided_fginn_batch_dev: slot 1 of idx / dist becomes the nearest GATED train row whose keypoint lies at least that
    far from the keypoint of slot 0 (FGINN inside the gate), so a keypoint's own twin inside the band (a second orientation, a
    neighbouring scale) no longer fails the ratio test.  A query whose only gated companions lie inside the radius has dist1 = inf and
    is KEPT (nothing competes with it) — not the rule of knn_match_fginn_batch_tensors, which needs a second row.  The reverse search
    of mutual stays the plain one.
    ratio=None, mutual="ratio" and max_dist: the rule of matcher.check_rule in its guided form (a missing slot 1 has dist = inf and passes
    either ratio test)."""
    from . import matcher
    rule = matcher.check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    ts = (kps1, kps2, desc1, desc2, models)
    _require(_GUIDED_NAMES, ts)
    code, kind, o1, o2 = matcher.check_match_verify_args(model, ratio, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape), desc2.dtype,
                                                         tuple(kps1.shape), kps1.dtype, tuple(kps2.shape), kps2.dtype, counts1, counts2)
    return _guided_tensors(matcher.layout(o1, o2), code, kind, ts, model, rule, px_th, error_type, driver_form, fginn_th, False)


_GUIDED_NAMES = "kps1, kps2, desc1, desc2 and models"


def _guided_tensors(L, code, kind, ts, model, rule, px_th, error_type, driver_form, fginn_th, per_store):
    """the two guided calls after their layout check: the guided stage's own checks, the device refusal, the conversions, the call"""
    from . import matcher
    kps1, kps2, desc1, desc2, models = ts
    px, et = matcher.check_guided_args(model, px_th, error_type, tuple(models.shape), models.dtype, L.K)
    fr = None if fginn_th is None else matcher.check_fginn_th(fginn_th)
    _require(_GUIDED_NAMES, ts, "cuda")
    a, b = _desc_pair(desc1, desc2)
    k1, k2 = _store_kps(kind, kps1, kps2, per_store)
    return _guided_dev(L, code, a, b, k1, k2, _driver_models(models, model, driver_form, L.K), model, rule, px, et, fr)


def _h_user_form(M):
    """the driver's H_c [K, 3, 3] -> the user-facing inv(H_c^T) where a model was found, without a host round trip: short / failed
    pairs invert the identity and stay zero"""
    import torch
    K = M.shape[0]
    found = (M.abs().sum(dim=(1, 2)) != 0).view(K, 1, 1)
    eye = torch.eye(3, dtype=M.dtype, device=M.device).expand(K, 3, 3)
    inv = torch.linalg.inv_ex(torch.where(found, M.transpose(1, 2), eye)).inverse      # inv_ex: no error check, no sync
    return torch.where(found, inv, torch.zeros_like(M))


def _verify_in(L, sd, dev):
    """what every match-and-verify call has once: (seeds on the device, match [n] filled with -1, the host counts [K])"""
    import torch
    # pinned + non_blocking: a pageable copy would wait for the stream (the call's one synchronisation is the count read)
    d_seeds = torch.from_numpy(sd.view(np.int32)).pin_memory().to(dev, non_blocking=True)
    return d_seeds, torch.full((L.n,), -1, dtype=torch.int32, device=dev), np.zeros(L.K, np.int32)


def _verify_out(L, dev):
    """the outputs of one estimator over a layout with their fills: (model [K, 9], inlier [n] uint8, stats [K, 16])"""
    import torch
    return (torch.zeros((L.K, 9), dtype=torch.float64, device=dev), torch.zeros(L.n, dtype=torch.uint8, device=dev),
            torch.zeros((L.K, 16), dtype=torch.int32, device=dev))


def _match_verify_dev(entry, L, model, mp, prm, a, b, k1, k2, sd, guide=None):
    """The match-and-verify call of both layouts after the argument checks: entry = the *_dev entry point of the checked layout L, sd =
    uint32 seeds [K].  guide (nullable) gets the driver-form models [K, 9] as the library wrote them, on the same stream.  Returns
    (model [K, 3, 3] — H as the user-facing form —, match [n], inlier [n] bool, stats [K, 16], n_tentatives [K] numpy int64, what guide
    returned)."""
    import torch
    from . import matcher
    dev = a.device
    d_seeds, match, cnt = _verify_in(L, sd, dev)
    M, inlier, stats = _verify_out(L, dev)
    di, stream, sp = _stream(dev)
    rc = entry(1 if model == "H" else 0, C.byref(mp), _p(a), _p(b), *matcher.verify_layout(L, _p(k1), _p(k2), int(k1.shape[1])), C.byref(prm),
               _p(d_seeds), di, sp, _p(M), _p(match), _p(inlier), _p(stats), _lib.ptr(cnt))
    _lib.check(rc)
    _keep_alive(stream, a, b, k1, k2, d_seeds)
    gm = guide(M) if guide else None
    M = M.view(L.K, 3, 3)
    return _h_user_form(M) if model == "H" else M, match, inlier.to(torch.bool), stats, cnt.astype(np.int64), gm


def match_and_verify_batch_tensors(kps1, kps2, desc1, desc2, counts1, counts2, model="F", ratio=0.9, mutual=False, px_th=None, conf=None,
                                   max_iters=None, laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True,
                                   enable_degeneracy_check=True, seeds=None, guided=False, norm=None, fginn_th=None, guided_fginn_th=None, *,
                                   max_dist=None):
    """K image pairs from descriptors to models with ONE host synchronisation (the read of the per-pair tentative counts): per pair
    the 2-NN ratio test (`m.distance < ratio * n.distance`, optionally mutual) of match_snn_tensors, then the estimator of
    find_fundamental_batch_tensors (model "F") / find_homography_batch_tensors ("H") on its tentatives in query order.
    kps: float64 [N, 2] / [N, 6] rows, or float32 [N, 4] keypoints (x, y, size, angle) that go through kpts_to_xyA_tensors;
    descriptors float32 (L2) or uint8 with dim % 4 == 0 (Hamming; L2 with norm="l2_u8" and dim <= 256).
    Defaults are findFundamentalMatrix's / findHomography's; seeds
    default to parallel.pair_seeds(0, K) and belong to the pair, whatever else is in the batch.  A pair with fewer than 8 (F) / 4 (H)
    tentatives is not estimated: zero model, zero stats row, no inliers.
    Returns (model [K, 3, 3] float64 — H as the user-facing inv(H_c^T), zeros where none was found —, match [N1] int32 = pair-local
    train row or -1, inlier [N1] bool, stats [K, 16] int32, n_tentatives [K] numpy int64); all but the last on the device.
    guided=True then runs guided_match_batch_tensors on the same stream with the estimator's driver-form models straight from device
    memory (no conversion) and this call's px_th / error_type / ratio / mutual, and appends its match [N1] int32 (the guided match of
    every query or -1); the call still synchronises exactly once.
    fginn_th: None = the plain ratio test; a number switches it to the FGINN ratio test (knn_match_fginn_batch_tensors at that radius
    on kps2's x, y).  Only the tentatives in front of the estimator change: the guided stage keeps its own gate and decision.
    guided_fginn_th: None, or the radius of guided_match_batch_tensors(fginn_th=) for the guided stage (FGINN inside the gate; a query
    whose only gated companions lie inside the radius is kept).  It is passed on only with guided=True and is a ValueError without it.
    ratio=None, mutual="ratio" and max_dist: the rule of matcher.check_rule, for the tentatives and (guided form) the guided stage."""
    from . import matcher
    gfr = matcher.check_guided_fginn_th(guided, guided_fginn_th)
    rule = matcher.check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    if gfr is not None:
        matcher.check_rule(ratio, mutual, max_dist, fginn=True)
    ts = (kps1, kps2, desc1, desc2)
    _require(_VERIFY_NAMES, ts)
    code, kind, o1, o2 = matcher.check_match_verify_args(model, ratio, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape), desc2.dtype,
                                                         tuple(kps1.shape), kps1.dtype, tuple(kps2.shape), kps2.dtype, counts1, counts2, fginn_th)
    _require(_VERIFY_NAMES, ts, "same")
    prm = matcher.estimator_params(model, px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check)
    a, b = _desc_pair(desc1, desc2)
    k1, k2 = _store_kps(kind, kps1, kps2, False)
    L = matcher.layout(o1, o2)
    sd = matcher._seeds_u32(None if seeds is None else np.asarray(seeds).ravel(), L.K)
    guide = (lambda M: _guided_dev(L, code, a, b, k1, k2, M, model, rule, prm.px_th, prm.error_type, gfr)[0]) if guided else None
    res = _match_verify_dev(_lib.lib().mi_degensac_match_verify_batch_dev, L, model, _lib.match_params(code, a.shape[1], rule, fginn_th), prm,
                            a, b, k1, k2, sd, guide)
    return res if guided else res[:5]


_VERIFY_NAMES = "kps1, kps2, desc1 and desc2"


# ---- the pair-list form: image stores + (i, j) image indices (include/mi_degensac.h mi_degensac_match_*_pairs*) ----
def knn_match_pairs_tensors(desc1, desc2, counts1, counts2, pairs, norm=None):
    """knn_match_batch_tensors over a pair list.  desc1 / desc2 are image stores: image i of store 1 is the next counts1[i] rows of desc1,
    image j of store 2 the next counts2[j] rows of desc2 (the same tensor may be passed twice: a collection against itself).  pairs:
    integer array [K, 2]; entry p = (i, j) runs image i's rows as queries against image j's rows.  Any list is fine: self pairs,
    repeats, both orders, any order; images may be empty or unused.  No descriptor row is copied.  Returns (idx [N, 2] int32 with
    indices LOCAL to image j, dist [N, 2] float32, pair_offsets [K + 1] host int64): pair p owns the rows pair_offsets[p] ..
    pair_offsets[p + 1], counts1[pairs[p, 0]] of them, and they are bit for bit what knn_match_batch_tensors returns for the pair's
    copied rows.  Asynchronous on the current stream."""
    from . import matcher
    _require("descriptors", (desc1, desc2))
    code, _, o1, o2, pr, po, _ = matcher.check_match_pairs_args("F", 1.0, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape), desc2.dtype,
                                                                (desc1.shape[0], 2), np.float64, (desc2.shape[0], 2), np.float64, counts1, counts2,
                                                                pairs)
    return _knn2_dev(matcher.layout(o1, o2, pr, po), code, *_desc_pair(desc1, desc2)) + (po,)


def knn_match_fginn_pairs_tensors(desc1, desc2, kps2, counts1, counts2, pairs, spatial_th=10.0, norm=None):
    """knn_match_pairs_tensors with the FGINN rule of knn_match_fginn_batch_tensors for the second neighbour (include/mi_degensac.h
    mi_degensac_match_fginn_knn2_pairs_dev).  kps2 is the keypoint store of side 2: float64 [N2, 2] / [N2, 6] on the device, one row
    per row of desc2 (only x, y are read).  For entry p = (i, j) slot 1 is the nearest row of image j whose keypoint lies at least
    spatial_th from the keypoint of slot 0.  Stores, list and layout as for knn_match_pairs_tensors: no descriptor or keypoint row is
    copied, and per entry the rows are bit for bit what knn_match_fginn_batch_tensors returns for the entry's copied rows.  Returns
    (idx [N, 2] int32 with indices LOCAL to image j, dist [N, 2] float32, pair_offsets [K + 1] host int64); asynchronous on the current
    stream (no host synchronisation)."""
    from . import matcher
    r = _fginn_knn2_args(desc1, desc2, kps2, spatial_th)
    code, _, o1, o2, pr, po, _ = matcher.check_match_pairs_args("F", 1.0, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape), desc2.dtype,
                                                                (desc1.shape[0], kps2.shape[1]), np.float64, tuple(kps2.shape), kps2.dtype,
                                                                counts1, counts2, pairs)
    _require("desc1, desc2 and kps2", (desc1, kps2), "same")
    return _knn2_dev(matcher.layout(o1, o2, pr, po), code, *_desc_pair(desc1, desc2), kps2.contiguous(), r) + (po,)


def match_and_verify_pairs_tensors(kps1, kps2, desc1, desc2, counts1, counts2, pairs, model="F", ratio=0.9, mutual=False, px_th=None, conf=None,
                                   max_iters=None, laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True,
                                   enable_degeneracy_check=True, seeds=None, guided=False, norm=None, fginn_th=None, *, max_dist=None):
    """match_and_verify_batch_tensors over a pair list: kps / desc are image stores (counts1 / counts2 rows per image, as for
    knn_match_pairs_tensors; pass the same tensors on both sides for a collection matched against itself) and pairs [K, 2] lists the
    (i, j) to run, e.g. matcher.exhaustive_pairs(M).  Descriptors and keypoints stay where they are: the device holds M images' rows,
    not 2 K.  float32 [N, 4] keypoints go through kpts_to_xyA_tensors once per store.  seeds: one per list entry, default
    parallel.pair_seeds(0, K).  Per pair every output is bit for bit that of match_and_verify_batch_tensors on the pair's copied rows
    with the same seeds; the call synchronises exactly once (the read of the tentative counts).
    Returns (model [K, 3, 3], match [N] int32 = train row local to image j or -1, inlier [N] bool, stats [K, 16], n_tentatives [K]
    numpy int64, pair_offsets [K + 1] host int64) with N = pair_offsets[K]: the per-query outputs lie pair after pair in list order.
    guided=True and fginn_th are not part of this call (ValueError): guided matching over the list is guided_match_pairs_tensors, which
    takes the models returned here as they are; the FGINN ratio test over a list is match_and_verify_fginn_pairs_tensors."""
    return _match_verify_pairs_tensors(None, kps1, kps2, desc1, desc2, counts1, counts2, pairs, model, ratio, mutual, px_th, conf, max_iters,
                                       laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check, seeds, guided, norm, fginn_th,
                                       max_dist)


def match_and_verify_fginn_pairs_tensors(kps1, kps2, desc1, desc2, counts1, counts2, pairs, fginn_th, model="F", ratio=0.9, mutual=False, px_th=None,
                                         conf=None, max_iters=None, laf_consistensy_coef=-1.0, error_type="sampson", symmetric_error_check=True,
                                         enable_degeneracy_check=True, seeds=None, guided=False, norm=None, *, max_dist=None):
    """match_and_verify_pairs_tensors with the FGINN ratio test in front of the estimator (include/mi_degensac.h
    mi_degensac_match_verify_fginn_pairs_dev): fginn_th is the radius in pixels of kps2 (knn_match_fginn_pairs_tensors at that radius on
    the x, y of store 2's keypoints), a finite number >= 0.  Stores, list, seeds, the returned tuple and the single synchronisation are
    those of match_and_verify_pairs_tensors; per entry every output is bit for bit that of match_and_verify_batch_tensors(fginn_th=) on
    the entry's copied rows with the same seeds.  guided=True is refused here as well: guided_match_pairs_tensors takes the returned
    models as they are."""
    from . import matcher
    r = matcher.check_fginn_th(fginn_th)
    return _match_verify_pairs_tensors(r, kps1, kps2, desc1, desc2, counts1, counts2, pairs, model, ratio, mutual, px_th, conf, max_iters,
                                       laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check, seeds, guided, norm, None,
                                       max_dist)


def _match_verify_pairs_tensors(fginn_r, kps1, kps2, desc1, desc2, counts1, counts2, pairs, model, ratio, mutual, px_th, conf, max_iters,
                                laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check, seeds, guided, norm, fginn_th,
                                max_dist=None):
    """the body of the two pair-list match-and-verify calls: fginn_r None = the plain call (which refuses fginn_th), a checked radius =
    the FGINN call and its entry point; ratio / mutual / max_dist: the rule of matcher.check_rule"""
    from . import matcher
    rule = matcher.check_rule(ratio, mutual, max_dist, fginn=fginn_r is not None)
    ts = (kps1, kps2, desc1, desc2)
    _require(_VERIFY_NAMES, ts)
    code, kind, o1, o2, pr, po, sd = matcher.check_match_pairs_args(model, ratio, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape),
                                                                    desc2.dtype, tuple(kps1.shape), kps1.dtype, tuple(kps2.shape), kps2.dtype,
                                                                    counts1, counts2, pairs, seeds, guided, fginn_th)
    _require(_VERIFY_NAMES, ts, "same")
    prm = matcher.estimator_params(model, px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check, enable_degeneracy_check)
    a, b = _desc_pair(desc1, desc2)
    L = matcher.layout(o1, o2, pr, po)
    k1, k2 = _store_kps(kind, kps1, kps2, True)          # once per store, not per pair
    if sd is None:
        sd = matcher._seeds_u32(None, L.K)
    entry = _lib.lib().mi_degensac_match_verify_pairs_dev if fginn_r is None else _lib.lib().mi_degensac_match_verify_fginn_pairs_dev
    return _match_verify_dev(entry, L, model, _lib.match_params(code, a.shape[1], rule, fginn_r), prm, a, b, k1, k2, sd)[:5] + (po,)


# ---- match once, verify F and H (include/mi_degensac.h mi_degensac_match_verify_fh_*) ----
def _match_verify_fh_dev(L, code, kind, ts, rule, fginn_r, prm_f, prm_h, sd, per_store):
    """The two-model call of both layouts after the argument checks: the device refusal, the conversions, then one call with both
    estimators on the same tentatives.  Returns (F [K, 3, 3], H [K, 3, 3] user-facing, match [n], inlier_f [n] bool, inlier_h [n] bool,
    stats_f [K, 16], stats_h [K, 16], summary [K, 4], n_tentatives [K] numpy int64)."""
    import torch
    from . import matcher
    kps1, kps2, desc1, desc2 = ts
    _require(_VERIFY_NAMES, ts, "same")
    a, b = _desc_pair(desc1, desc2)
    k1, k2 = _store_kps(kind, kps1, kps2, per_store)
    dev = a.device; K = L.K
    d_seeds, match, cnt = _verify_in(L, sd, dev)
    MF, inf, stf = _verify_out(L, dev); MH, inh, sth = _verify_out(L, dev)
    summ = torch.zeros((K, 4), dtype=torch.int32, device=dev)
    mp = _lib.match_params(code, a.shape[1], rule, fginn_r)
    di, stream, sp = _stream(dev)
    rc = getattr(_lib.lib(), f"mi_degensac_match_verify_fh_{L.name}_dev")(
        C.byref(mp), _p(a), _p(b), *matcher.verify_layout(L, _p(k1), _p(k2), int(k1.shape[1])), C.byref(prm_f), C.byref(prm_h), _p(d_seeds), di, sp,
        _p(MF), _p(MH), _p(match), _p(inf), _p(inh), _p(stf), _p(sth), _p(summ), _lib.ptr(cnt))
    _lib.check(rc)
    _keep_alive(stream, a, b, k1, k2, d_seeds)
    return MF.view(K, 3, 3), _h_user_form(MH.view(K, 3, 3)), match, inf.to(torch.bool), inh.to(torch.bool), stf, sth, summ, cnt.astype(np.int64)


def match_and_verify_fh_batch_tensors(kps1, kps2, desc1, desc2, counts1, counts2, ratio=0.9, mutual=False, norm=None, fginn_th=None, seeds=None,
                                      f_params=None, h_params=None, *, max_dist=None):
    """match_and_verify_batch_tensors with BOTH models on the same tentatives (include/mi_degensac.h mi_degensac_match_verify_fh_batch_dev):
    the 2-NN search, the FGINN step, the reverse search of mutual and the ratio test run ONCE, the tentative counts are read ONCE (the
    call's one host synchronisation), then the fundamental-matrix and the homography estimator run one after the other on every pair's
    tentatives, both seeded with the pair's seed.  A pipeline that has to decide per pair between a general scene, a planar / panoramic
    one and a rejected pair gets both models, both inlier sets and their overlap for about the price of one matching phase less than two
    match_and_verify_batch_tensors calls.  Tensors, ratio, mutual, norm, fginn_th and seeds as there.  f_params / h_params: None or a dict
    of estimator keywords (px_th, conf, max_iters, laf_consistensy_coef, error_type, symmetric_error_check, and for F
    enable_degeneracy_check); missing keys take findFundamentalMatrix's / findHomography's defaults, an unknown key is a ValueError.
    Per pair F / inlier_f / stats_f are bit for bit those of match_and_verify_batch_tensors(model="F", **f_params), H / inlier_h / stats_h
    those of model="H" with h_params, match and n_tentatives those of either.  A pair with 4 .. 7 tentatives has an H and a zero F; below
    4 both are zero.
    Returns (F [K, 3, 3], H [K, 3, 3] — the user-facing inv(H_c^T) —, match [N1] int32, inlier_f [N1] bool, inlier_h [N1] bool,
    stats_f [K, 16], stats_h [K, 16], summary [K, 4] int32 = per pair (tentatives, nF, nH, nFH): its tentatives and its queries that are
    inliers of F, of H, of both; n_tentatives [K] numpy int64); all but the last on the device.  matcher.two_view_config(summary)
    classifies the pairs.
    The guided stage is not part of this call (there is no guided= keyword): guided_match_batch_tensors / guided_match_pairs_tensors take
    either returned model as it is.  ratio=None, mutual="ratio" and max_dist: the rule of matcher.check_rule."""
    from . import matcher
    rule = matcher.check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    ts = (kps1, kps2, desc1, desc2)
    _require(_VERIFY_NAMES, ts)
    code, kind, o1, o2 = matcher.check_match_verify_args("H", ratio, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape), desc2.dtype,
                                                         tuple(kps1.shape), kps1.dtype, tuple(kps2.shape), kps2.dtype, counts1, counts2, fginn_th)
    L = matcher.layout(o1, o2)
    sd = matcher._seeds_u32(None if seeds is None else np.asarray(seeds).ravel(), L.K)
    prm_f, prm_h = matcher.two_view_params(f_params, h_params)
    return _match_verify_fh_dev(L, code, kind, ts, rule, fginn_th, prm_f, prm_h, sd, False)


def match_and_verify_fh_pairs_tensors(kps1, kps2, desc1, desc2, counts1, counts2, pairs, ratio=0.9, mutual=False, norm=None, fginn_th=None,
                                      seeds=None, f_params=None, h_params=None, *, max_dist=None):
    """match_and_verify_fh_batch_tensors over a pair list (include/mi_degensac.h mi_degensac_match_verify_fh_pairs_dev): kps / desc are
    image stores (counts1 / counts2 rows per image; pass the same tensors on both sides for a collection matched against itself) and
    pairs [K, 2] lists the (i, j) to run, as for match_and_verify_pairs_tensors.  fginn_th IS part of this call (None = the plain ratio
    test, a number = the FGINN ratio test of match_and_verify_fginn_pairs_tensors): there is no separate FGINN form.  seeds: one per list
    entry, for both estimators.  Per entry F / inlier_f / stats_f are bit for bit those of match_and_verify_pairs_tensors (with fginn_th:
    match_and_verify_fginn_pairs_tensors) with model="F" and f_params, H / inlier_h / stats_h those with model="H" and h_params; the call
    synchronises exactly once.
    Returns (F [K, 3, 3], H [K, 3, 3] user-facing, match [N] int32 = train row local to image j or -1, inlier_f [N] bool, inlier_h [N]
    bool, stats_f [K, 16], stats_h [K, 16], summary [K, 4] int32 = (tentatives, nF, nH, nFH), n_tentatives [K] numpy int64,
    pair_offsets [K + 1] host int64) with N = pair_offsets[K].
    The guided stage is not part of this call (there is no guided= keyword): guided_match_pairs_tensors / guided_match_batch_tensors take
    either returned model as it is."""
    from . import matcher
    rule = matcher.check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    ts = (kps1, kps2, desc1, desc2)
    _require(_VERIFY_NAMES, ts)
    fr = None if fginn_th is None else matcher.check_fginn_th(fginn_th)
    code, kind, o1, o2, pr, po, sd = matcher.check_match_pairs_args("H", ratio, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape),
                                                                    desc2.dtype, tuple(kps1.shape), kps1.dtype, tuple(kps2.shape), kps2.dtype,
                                                                    counts1, counts2, pairs, seeds)
    prm_f, prm_h = matcher.two_view_params(f_params, h_params)
    if sd is None:
        sd = matcher._seeds_u32(None, len(pr))
    return _match_verify_fh_dev(matcher.layout(o1, o2, pr, po), code, kind, ts, rule, fr, prm_f, prm_h, sd, True) + (po,)


def guided_match_pairs_tensors(kps1, kps2, desc1, desc2, counts1, counts2, pairs, models, model="F", ratio=0.9, mutual=False, px_th=None,
                               error_type="sampson", norm=None, driver_form=False, fginn_th=None, *, max_dist=None):
    """guided_match_batch_tensors over a pair list (include/mi_degensac.h mi_degensac_match_guided_pairs_dev): kps / desc are image stores
    (counts1 / counts2 rows per image; pass the same tensors on both sides for a collection matched against itself), pairs [K, 2] lists
    the (i, j) to run and models [K, 3, 3] float64 on the device holds one model per LIST ENTRY — what match_and_verify_pairs_tensors
    returned for the same list goes in as it is: F, or the user-facing H (converted here on the device; driver_form=True takes
    H_c = inv(H)^T).  The same (i, j) may appear twice with two models.  Descriptors and keypoints stay where they are: no row is copied
    per pair, float32 [N, 4] keypoints go through kpts_to_xyA_tensors once per store, and with mutual the reverse search takes 16 bytes
    per train row of the list.  Gate, decision and the zero-model rule as in guided_match_batch_tensors; per entry every output is bit for
    bit what that call returns on the entry's copied rows.  Returns (match [N] int32 = train row local to image j or -1, idx [N, 2]
    int32, dist [N, 2] float32, pair_offsets [K + 1] host int64) with N = pair_offsets[K]: entry p owns the rows pair_offsets[p] ..
    pair_offsets[p + 1].  Asynchronous on the current stream (no host synchronisation).
    fginn_th as in guided_match_batch_tensors, through mi_degensac_match_guided_fginn_pairs_dev: anchors and competitors are the
    keypoints of the entry's train image in store 2; a needy query is rescanned through its image's rows in store 1 and answered at
    its output row (two different rows in a list), nothing is copied.  A query whose only gated companions lie inside the radius is kept.
    ratio=None, mutual="ratio" and max_dist as in guided_match_batch_tensors."""
    from . import matcher
    rule = matcher.check_rule(ratio, mutual, max_dist, fginn=fginn_th is not None)
    ts = (kps1, kps2, desc1, desc2, models)
    _require(_GUIDED_NAMES, ts)
    code, kind, o1, o2, pr, po, _ = matcher.check_match_pairs_args(model, ratio, norm, tuple(desc1.shape), desc1.dtype, tuple(desc2.shape),
                                                                   desc2.dtype, tuple(kps1.shape), kps1.dtype, tuple(kps2.shape), kps2.dtype,
                                                                   counts1, counts2, pairs)
    # once per store, not per pair
    return _guided_tensors(matcher.layout(o1, o2, pr, po), code, kind, ts, model, rule, px_th, error_type, driver_form, fginn_th, True) + (po,)


def _correspondences_tensors(match, counts1, counts2, pairs, keep, kps1, kps2, models, model, error_type, driver_form, store_rows, with_entry,
                             capacity):
    import torch
    from . import matcher
    names = "match, keep, kps1, kps2 and models"
    ts = [t for t in (match, keep, kps1, kps2, models) if t is not None]
    _require(names, ts)
    o1, o2, pr, po, kind, et, cap = matcher.check_correspond_args(tuple(match.shape), match.dtype, counts1, counts2, pairs, _sd(keep), _sd(kps1),
                                                                  _sd(kps2), _sd(models), model, error_type, capacity)
    _require(names, ts, "cuda")
    name, layout, K = matcher.correspond_layout(o1, o2, pr)
    dev = match.device
    m = match.contiguous()
    kp = None if keep is None else keep.contiguous().view(torch.uint8)
    k1, k2 = (None, None) if kps1 is None else _store_kps(kind, kps1, kps2, True)
    M = None if models is None else _driver_models(models, model, driver_form, K)
    rows = torch.full((cap, 2), -1, dtype=torch.int32, device=dev)
    co = torch.empty(K + 1, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    entry = torch.full((cap,), -1, dtype=torch.int32, device=dev) if with_entry else None
    pts = None if k1 is None else torch.full((cap, 4), float("nan"), dtype=torch.float64, device=dev)
    resid = None if M is None else torch.full((cap,), float("nan"), dtype=torch.float64, device=dev)
    gp = _lib.GuideParams(model == "H", et, 0.0)
    di, stream, sp = _stream(dev)
    p = _p
    rc = getattr(_lib.lib(), f"mi_degensac_correspondences_{name}_dev")(*layout, p(m), p(kp), _lib.CORR_STORE_ROWS if store_rows else 0, p(k1), p(k2),
                                                                       0 if k1 is None else int(k1.shape[1]), p(M), C.byref(gp), cap, di, sp,
                                                                       p(co), p(total), p(rows), p(entry), p(pts), p(resid))
    _lib.check_match(rc)
    _keep_alive(stream, m, kp, k1, k2, M)
    return rows, co, total, entry, pts, resid


def correspondences_pairs_tensors(match, counts1, counts2, pairs, keep=None, kps1=None, kps2=None, models=None, model="F", error_type="sampson",
                                  driver_form=False, store_rows=False, with_entry=False, capacity=None):
    """The verified matches of a pair list as compact per-entry lists, on the device and without a host synchronisation (include/mi_degensac.h
    mi_degensac_correspondences_pairs_dev): what a two-view database, triangulation or a track builder takes.  match [N] int32 (train row
    local to image j, or -1) with N the output rows of the list, counts1 / counts2 the rows per image of the two stores, pairs [K, 2].
    What goes in as it is: `match` and `keep=inlier` of match_and_verify_pairs_tensors (and of the batch form, with
    correspondences_batch_tensors); `match` of guided_match_pairs_tensors with keep=None; `keep = inlier_f & inlier_h` of
    match_and_verify_fh_pairs_tensors.  A row is selected when 0 <= match < rows(image j) and (keep is None or keep != 0, bool or uint8);
    any other match value means "not selected".  kps1 / kps2 (the stores' keypoints, [n, 2] / [n, 6] float64, or [n, 4] float32 through
    kpts_to_xyA_tensors) add pts; models [K, 3, 3] float64 (what the verify calls return: F, or the user-facing H, converted on the device;
    driver_form=True takes H_c = inv(H)^T) add resid = the estimator's own residual of error_type on every exported correspondence, the
    function the gate of guided matching calls (so resid <= th holds for every correspondence of a guided call with that threshold).
    Returns (rows [cap, 2] int32, corr_offsets [K + 1] int64 on the device, total [1] int64 on the device, entry [cap] int32 or None,
    pts [cap, 4] float64 = x1, y1, x2, y2 or None, resid [cap] float64 or None).  The selected rows stand in list order, query order
    inside an entry; entry p owns the positions corr_offsets[p] .. corr_offsets[p + 1].  rows = (query row in image i, train row in image
    j), with store_rows=True (row of store 1, row of store 2).  cap = capacity, or N when capacity is None; positions >= total keep their
    fill (rows / entry -1, pts / resid NaN).  corr_offsets and total are exact whatever capacity is: total > cap says that the tail was
    dropped.  capacity=int(n_tentatives.sum()) is a safe bound after a verify call (inliers are tentatives) and saves the memory of
    the rows that were never matched."""
    if pairs is None:
        raise ValueError("pairs should be an integer array [K, 2] of (image of store 1, image of store 2)")
    return _correspondences_tensors(match, counts1, counts2, pairs, keep, kps1, kps2, models, model, error_type, driver_form, store_rows, with_entry,
                                    capacity)


def correspondences_batch_tensors(match, counts1, counts2, keep=None, kps1=None, kps2=None, models=None, model="F", error_type="sampson",
                                  driver_form=False, store_rows=False, with_entry=False, capacity=None):
    """correspondences_pairs_tensors on the ragged batch (mi_degensac_correspondences_batch_dev): entry p is pair p with counts1[p] query rows
    and counts2[p] train rows; match [sum(counts1)] and keep are `match` / `inlier` of match_and_verify_batch_tensors (or `match` of
    guided_match_batch_tensors), kps1 / kps2 that call's keypoints.  The same result as the pair-list call on the identity list."""
    return _correspondences_tensors(match, counts1, counts2, None, keep, kps1, kps2, models, model, error_type, driver_form, store_rows, with_entry,
                                    capacity)


def tracks_tensors(rows, counts, total=None, with_label=False):
    """Tracks = the connected components of verified matches over one image store, on the device and without a host synchronisation
    (include/mi_degensac.h mi_degensac_tracks_dev).  rows [M, 2] int32 and total [1] int64 are what
    correspondences_pairs_tensors(..., store_rows=True) returned for a collection matched against itself (the same tensors on both sides),
    counts the rows per image of that store.  Only the first min(total, M) edges count (total=None: all M); an edge with an end outside
    the store (the -1 fill of the export) is ignored, self edges and repeated edges change nothing.
    Returns (track [R] int32 = the keypoint's track or -1, n_tracks [1] int64, track_offsets [R // 2 + 1] int64, obs [R] int32,
    obs_image [R] int32, track_images [R // 2] int32, n_obs [1] int64[, label [R] int32 with with_label=True]), all on the device, R the
    rows of the store.  A track is a component of at least two keypoints; tracks are numbered in ascending order of their smallest store
    row (label).  Track t owns obs[track_offsets[t] : track_offsets[t + 1]], store rows in ascending order, obs_image their images;
    track_images[t] is the number of distinct images, so the track is consistent (one keypoint per image at most) iff it equals the
    track's length.  Tails: track_offsets beyond [n_tracks] repeat n_obs, obs / obs_image beyond n_obs and track_images beyond n_tracks
    hold -1.  Every output is a pure function of the input: the same bits on every call.  Asynchronous on the current stream."""
    import torch
    from . import matcher
    ts = [rows] + ([] if total is None else [total])
    _require("rows (and total)", ts)
    off, R, M = matcher.check_tracks_args(tuple(rows.shape), rows.dtype, counts)
    if not rows.is_contiguous():
        raise ValueError("rows should be a contiguous int32 [M, 2] tensor")
    if total is not None and (tuple(total.shape) != (1,) or total.dtype != torch.int64):
        raise ValueError("total should be int64 [1] on the device, as the correspondence export returns it")
    _require("rows and total", ts, "cuda")
    dev = rows.device
    half = R // 2
    i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)          # noqa: E731  (an address also where n == 0)
    track, obs, oi, ti = i32(R), i32(R), i32(R), i32(half)
    label = i32(R) if with_label else None
    to = torch.empty(half + 1, dtype=torch.int64, device=dev)
    nt = torch.empty(1, dtype=torch.int64, device=dev); no = torch.empty(1, dtype=torch.int64, device=dev)
    di, stream, sp = _stream(dev)
    p = _p
    rc = _lib.lib().mi_degensac_tracks_dev(_lib.ptr(off), len(off) - 1, p(rows) if M else None, M, p(total), di, sp, p(label), p(track), p(nt), p(no),
                                           p(to), p(obs), p(oi), p(ti))
    _lib.check_match(rc)
    _keep_alive(stream, rows, total)
    out = (track[:R], nt, to, obs[:R], oi[:R], ti[:half], no)
    return out + (label[:R],) if with_label else out


def refit_correspondences_tensors(pts, corr_offsets, models, model="F", px_th=None, error_type="sampson", driver_form=False, max_fits=4,
                                  with_resid=False):
    """Refit F / H on exported correspondence lists, on the device and without a host synchronisation (include/mi_degensac.h
    mi_degensac_refit_lists_dev): the model of a verify call has never seen the matches the guided stage brought back, nor matches that
    come from elsewhere.  pts [cap, 4] float64 and corr_offsets [K + 1] int64 are what correspondences_pairs_tensors / _batch_tensors
    returned (kps1 / kps2 given), models [K, 3, 3] float64 what any verify call returned: F, or the user-facing H (converted on the device
    in both directions; driver_form=True takes and returns H_c = inv(H)^T).  Per entry: the members of its model (resid <= th, the
    estimator's own residual of error_type and its threshold from px_th, None = the model's default, as in the guided calls), then at
    most max_fits rounds of the reference's non-minimal fit on the members followed by the members of the fit; a round that loses members
    is dropped, a round that keeps the set ends the entry.  The kernel reads the entries' lengths from corr_offsets itself, so nothing
    is read back.  An entry that a truncated export (total > capacity) cut keeps its model and flags nothing (status _lib.REFIT_TRUNCATED).
    Returns (models [K, 3, 3], inlier [cap] bool, info [K, 4] int32 = (members of the start model, members at the end, fits run,
    _lib.REFIT_* status)[, resid [cap] under the returned model]) on the device, asynchronous on the current stream.  `inlier` goes into
    correspondences_pairs_tensors as it is only after a scatter to output rows; on the exported list itself it is the mask of the rows."""
    import torch
    from . import matcher
    ts = (pts, corr_offsets, models)
    _require("pts, corr_offsets and models", ts)
    K, cap, px, et, mf = matcher.check_refit_args(tuple(pts.shape), pts.dtype, tuple(corr_offsets.shape), corr_offsets.dtype, tuple(models.shape),
                                                  models.dtype, model, px_th, error_type, max_fits)
    _require("pts, corr_offsets and models", ts, "cuda")
    dev = pts.device
    P = pts.contiguous(); o = corr_offsets.contiguous()
    M = _driver_models(models, model, driver_form, K)
    out = torch.empty((K, 9), dtype=torch.float64, device=dev)
    user = torch.empty((K, 9), dtype=torch.float64, device=dev) if (model == "H" and not driver_form) else None
    inl = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)          # (an address also where cap == 0)
    info = torch.empty((K, 4), dtype=torch.int32, device=dev)
    resid = torch.empty(max(cap, 1), dtype=torch.float64, device=dev) if with_resid else None
    gp = _lib.GuideParams(model == "H", et, px)
    di, stream, sp = _stream(dev)
    p = _p
    rc = _lib.lib().mi_degensac_refit_lists_dev(p(P), p(o), p(M), K, cap, C.byref(gp), mf, di, sp, p(out), p(inl), p(user), p(info), p(resid))
    _lib.check_match(rc)
    _keep_alive(stream, P, o, M)
    res = ((out if user is None else user).view(K, 3, 3), inl[:cap].view(torch.bool), info)
    return res + (resid[:cap],) if with_resid else res


def _pose_lists_tensors(from_h, pts, corr_offsets, models, cams1, pairs, cams2, keep, min_parallax_deg, with_points, with_candidates, rotation_eps=None,
                        driver_form=False):
    """the tensor body of relative_pose_tensors (from_h False) and homography_pose_tensors (True: rotation_eps and driver_form, normal and
    t_over_d behind info, cand_normal between cand and cand_front)"""
    import torch
    from . import matcher
    opt = [t for t in (pairs, cams2, keep) if t is not None]
    names = "pts, corr_offsets, models, cams1 (and pairs, cams2, keep)"
    ts = [pts, corr_offsets, models, cams1] + opt
    _require(names, ts)
    shapes = (tuple(pts.shape), pts.dtype, tuple(corr_offsets.shape), corr_offsets.dtype, tuple(models.shape), models.dtype, tuple(cams1.shape),
              cams1.dtype, _sd(pairs), _sd(cams2), _sd(keep), min_parallax_deg)
    if from_h:
        K, cap, n1, n2, cos_min, eps = matcher.check_pose_h_args(*shapes, rotation_eps)
    else:
        K, cap, n1, n2, cos_min = matcher.check_pose_args(*shapes)
    _require(names, ts, "cuda")
    dev = pts.device
    P = pts.contiguous(); o = corr_offsets.contiguous()
    M = (_h_user_form(models.contiguous()) if from_h and driver_form else models).contiguous()
    cams, n_cams, idx = _cameras(cams1, cams2, pairs, K, n1, n2)
    kp = None if keep is None else keep.contiguous().view(torch.uint8)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)          # noqa: E731
    rows = max(cap, 1)                                                # (an address also where cap == 0)
    pose = f64(K, 12); front = torch.empty(rows, dtype=torch.uint8, device=dev); info = torch.empty((K, 5), dtype=torch.int32, device=dev)
    plane = (f64(K, 3), f64(K)) if from_h else ()                     # normal, t_over_d
    pts3 = (f64(rows, 3), f64(rows, 2), f64(rows)) if with_points else (None,) * 3          # X, depth, cosang
    cand = f64(K, 4, 12) if with_candidates else None
    cn = (f64(K, 4, 3) if with_candidates else None,) if from_h else ()
    cf = torch.empty((K, 4), dtype=torch.int32, device=dev) if with_candidates else None
    di, stream, sp = _stream(dev)
    p = _p
    entry = _lib.lib().mi_degensac_pose_h_lists_dev if from_h else _lib.lib().mi_degensac_pose_lists_dev
    rc = entry(p(P), p(o), p(kp), p(M), p(cams), n_cams, p(idx), K, cap, cos_min, *((eps,) if from_h else ()), di, sp, p(pose), p(front), p(info),
               *map(p, plane), *map(p, pts3), p(cand), *map(p, cn), p(cf))
    _lib.check_match(rc)
    _keep_alive(stream, P, o, M, cams, idx, kp)
    res = (pose[:, :9].reshape(K, 3, 3), pose[:, 9:], front[:cap].view(torch.bool), info) + plane
    if with_points:
        res += tuple(x[:cap] for x in pts3)
    return res + (cand,) + cn + (cf,) if with_candidates else res


def relative_pose_tensors(pts, corr_offsets, models, cams1, pairs=None, cams2=None, keep=None, min_parallax_deg=1.5, with_points=False,
                          with_candidates=False):
    """Relative pose and triangulation on exported correspondence lists, on the device and without a host synchronisation
    (include/mi_degensac.h mi_degensac_pose_lists_dev): what a structure-from-motion front end stores per pair besides F.  pts [cap, 4]
    float64 and corr_offsets [K + 1] int64 are what correspondences_pairs_tensors / _batch_tensors returned (kps1 / kps2 given), models
    [K, 3, 3] float64 the fundamental matrices of a verify call or of the refit (x2^T F x1 = 0).  Cameras are pinhole (fx, fy, cx, cy),
    float64: with pairs=None cams1 is [K, 8], the two cameras of every entry; with pairs [K, 2] (the pair list, int32 or int64) cams1 is
    [n_images, 4] per image of store 1 and cams2 likewise for store 2 (None = cams1).  keep [cap] bool / uint8: only rows with keep != 0
    are used, so the refit's `inlier` goes in as it is.  Per entry: E = K2^T F K1, its four (R, t) candidates (X2 = R X1 + t, |t| = 1),
    and the candidate under which most used rows lie in front of both cameras (closed-form midpoint of the two rays; ties go to the first
    candidate).  A front row is wide when the angle between its rays is at least min_parallax_deg (COLMAP's minimum triangulation angle).
    The kernel reads the entries' lengths from corr_offsets itself, so nothing is read back.
    Returns (R [K, 3, 3], t [K, 3], front [cap] bool, info [K, 5] int32 = (rows used, front rows of the chosen candidate, the largest
    front count of the other three, wide rows, _lib.POSE_* status)[, X [cap, 3] in the frame of camera 1, depth [cap, 2] along the two
    rays, cosang [cap]][, cand [K, 4, 12], cand_front [K, 4]]) on the device, asynchronous on the current stream.  Rows that are not
    used, and rows of an entry without a pose (status != POSE_OK: R and t are zeros), keep front = False and NaN."""
    return _pose_lists_tensors(False, pts, corr_offsets, models, cams1, pairs, cams2, keep, min_parallax_deg, with_points, with_candidates)


def homography_pose_tensors(pts, corr_offsets, models, cams1, pairs=None, cams2=None, keep=None, min_parallax_deg=1.5, rotation_eps=1e-3,
                            driver_form=False, with_points=False, with_candidates=False):
    """Relative pose from a homography on exported correspondence lists, on the device and without a host synchronisation
    (include/mi_degensac.h mi_degensac_pose_h_lists_dev): the pose of a pair that matcher.two_view_config put into class 2, planar or
    panoramic, on which the F of relative_pose_tensors is degenerate.  pts, corr_offsets, cameras, pairs and keep exactly as
    relative_pose_tensors takes them; models [K, 3, 3] float64 are the homographies of a verify, F + H or refit call in the caller's form
    (x2 ~ H x1), or with driver_form=True in the driver's.  Per entry G = K2^-1 H K1 is decomposed into its four solutions G = R + (t / d)
    n^T; the one under which most used rows triangulate in front of both cameras and see the plane from its visible side is chosen (ties
    go to the first).  A G whose singular values differ by no more than rotation_eps times the middle one is a pure rotation: status
    _lib.POSE_ROTATION, R the rotation, t = 0.  The kernel reads the entries' lengths from corr_offsets itself, so nothing is read back.
    Returns (R [K, 3, 3], t [K, 3], front [cap] bool, info [K, 5] int32 = (rows used, front rows of the chosen candidate, the largest
    front count of the other three, wide rows, _lib.POSE_* status), normal [K, 3] = the unit plane normal in the frame of camera 1 (zeros
    when there is none), t_over_d [K] = baseline over plane distance[, X [cap, 3], depth [cap, 2], cosang [cap]][, cand [K, 4, 12],
    cand_normal [K, 4, 3], cand_front [K, 4]]) on the device, asynchronous on the current stream.  The meaning is the pose call's: X2 = R
    X1 + t, |t| = 1; R, t, front and info go into refine_pose_tensors and average_rotations_tensors as its results do."""
    return _pose_lists_tensors(True, pts, corr_offsets, models, cams1, pairs, cams2, keep, min_parallax_deg, with_points, with_candidates, rotation_eps,
                               driver_form)


def select_pose_tensors(cls, pose_f, pose_h, corr_offsets=None):
    """matcher.select_pose on device tensors, as plain `where` expressions without a host read: per pair pose_h's R, t, front and info
    where cls [K] (the classes of matcher.two_view_config as an integer tensor on the device) says 2 and pose_h's status is POSE_OK or
    POSE_ROTATION, else pose_f's.  pose_f and pose_h are the results of relative_pose_tensors and homography_pose_tensors on the same
    lists.  front is chosen per row by the row's pair, which takes the lists' corr_offsets [K + 1] (non-decreasing; a binary search on
    the device); without it front is None.  Returns (R [K, 3, 3], t [K, 3], front [cap] bool or None, info [K, 5], use_h [K] bool,
    edge_keep [K] bool = the pairs whose R is valid, for average_rotations_tensors: status POSE_OK or POSE_ROTATION of the selected pose;
    a ROTATION pair has a valid R although its t is zero and refine_pose_tensors answers it with REFINE_BAD_POSE)."""
    import torch
    from . import matcher
    Rf, tf, ff, inf = pose_f[:4]; Rh, th, fh, inh = pose_h[:4]
    ts = [cls, Rf, tf, ff, inf, Rh, th, fh, inh] + ([] if corr_offsets is None else [corr_offsets])
    names = "cls, pose_f, pose_h (and corr_offsets)"
    _require(names, ts)
    K = matcher.check_select_args(tuple(cls.shape), inf.shape[0], inh.shape[0])
    _require(names, ts, "same")
    sh = inh[:, 4]
    use_h = (cls == 2) & ((sh == _lib.POSE_OK) | (sh == _lib.POSE_ROTATION))
    R = torch.where(use_h[:, None, None], Rh, Rf); t = torch.where(use_h[:, None], th, tf); info = torch.where(use_h[:, None], inh, inf)
    front = None
    if corr_offsets is not None:
        if tuple(corr_offsets.shape) != (K + 1,) or ff.shape != fh.shape:
            raise ValueError("corr_offsets should be [K + 1], the offsets of the lists both pose calls ran on")
        cap = ff.shape[0]
        if K == 0 or cap == 0:
            front = ff.clone()
        else:
            entry = torch.searchsorted(corr_offsets[1:].contiguous(), torch.arange(cap, device=ff.device), right=True).clamp(max=K - 1)
            front = torch.where(use_h[entry], fh, ff)
    st = info[:, 4]
    return R, t, front, info, use_h, (st == _lib.POSE_OK) | (st == _lib.POSE_ROTATION)


def refine_pose_tensors(pts, corr_offsets, R, t, cams1, pairs=None, cams2=None, keep=None, max_trials=20, ftol=1e-12, with_resid=False,
                        with_F=False, **unknown):
    """Refine relative poses on exported correspondence lists, on the device and without a host synchronisation (include/mi_degensac.h
    mi_degensac_pose_refine_lists_dev): the non-linear step that follows the decomposition of relative_pose_tensors.  pts [cap, 4]
    float64, corr_offsets [K + 1] int64, cameras, pairs and keep exactly as relative_pose_tensors takes them (its `front` goes in as
    keep as it is); R [K, 3, 3] and t [K, 3] float64 are what it returned.  Per entry a Levenberg-Marquardt run over the five degrees of
    freedom of (R, t / |t|) on the Sampson distance, in pixels, of the used rows: at most max_trials trial steps, an accepted step that
    lowers the cost by no more than ftol times the cost ends the run.  The kernel reads the entries' lengths from corr_offsets itself, so
    nothing is read back.
    Returns (R [K, 3, 3], t [K, 3], cost [K, 2] = (start, end), info [K, 4] int32 = (rows used, trials, trials accepted, _lib.REFINE_*
    status)[, resid [cap]: the signed Sampson distance of the used rows under the final pose, NaN elsewhere][, F [K, 3, 3] = K2^-T [t]x R
    K1^-1 of the final pose, x2^T F x1 = 0, which guided_match_pairs_tensors, correspondences_pairs_tensors(models=) and
    relative_pose_tensors take as it is]) on the device, asynchronous on the current stream.  An entry without a usable start (status
    REFINE_SHORT, NOT_FINITE, BAD_CAMERA, TRUNCATED) keeps its pose and has NaN costs; REFINE_BAD_POSE (the zeros of a failed pose entry)
    gives zeros."""
    import torch
    from . import matcher
    if unknown:
        raise ValueError(f"refine_pose_tensors: unknown keyword {sorted(unknown)[0]!r}")
    opt = [x for x in (pairs, cams2, keep) if x is not None]
    names = "pts, corr_offsets, R, t, cams1 (and pairs, cams2, keep)"
    ts = [pts, corr_offsets, R, t, cams1] + opt
    _require(names, ts)
    K, cap, n1, n2, mt, ft = matcher.check_refine_args(tuple(pts.shape), pts.dtype, tuple(corr_offsets.shape), corr_offsets.dtype, tuple(R.shape), R.dtype,
                                                       tuple(t.shape), t.dtype, tuple(cams1.shape), cams1.dtype, _sd(pairs), _sd(cams2), _sd(keep),
                                                       max_trials, ftol)
    _require(names, ts, "cuda")
    dev = pts.device
    P = pts.contiguous(); o = corr_offsets.contiguous()
    pose = torch.cat([R.reshape(K, 9), t], 1).contiguous()
    cams, n_cams, idx = _cameras(cams1, cams2, pairs, K, n1, n2)
    kp = None if keep is None else keep.contiguous().view(torch.uint8)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)          # noqa: E731
    out = f64(K, 12); cost = f64(K, 2); info = torch.empty((K, 4), dtype=torch.int32, device=dev)
    resid = f64(max(cap, 1)) if with_resid else None                  # (an address also where cap == 0)
    F = f64(K, 9) if with_F else None
    di, stream, sp = _stream(dev)
    p = _p
    rc = _lib.lib().mi_degensac_pose_refine_lists_dev(p(P), p(o), p(kp), p(pose), p(cams), n_cams, p(idx), K, cap, mt, ft, di, sp, p(out), p(cost),
                                                      p(info), p(resid), p(F))
    _lib.check_match(rc)
    _keep_alive(stream, P, o, pose, cams, idx, kp)
    res = (out[:, :9].reshape(K, 3, 3), out[:, 9:], cost, info)
    if with_resid:
        res += (resid[:cap],)
    return res + (F.view(K, 3, 3),) if with_F else res


def triangulate_tracks_tensors(track_offsets, obs, obs_image, kps, cams, R, t, n_tracks=None, min_angle_deg=1.5, max_reproj_px=4.0, max_iters=10,
                               ftol=1e-12, with_obs=False, **unknown):
    """Triangulate tracks under known camera poses, on the device and without a host synchronisation (include/mi_degensac.h
    mi_degensac_triangulate_tracks_dev): the step after tracks_tensors when poses come from elsewhere (a previous reconstruction, a SLAM
    front end, a rig).  track_offsets [T + 1] int64, obs [M] int32, obs_image [M] int32 and n_tracks [1] int64 go in exactly as
    tracks_tensors returned them, fills included (n_tracks=None: all T tracks); kps [rows, >= 2] float64 holds x, y per row of the store
    the tracks were built on, cams [n_images, 4] float64 = fx, fy, cx, cy, R [n_images, 3, 3] and t [n_images, 3] float64 the
    world-to-camera poses X_cam = R X + t (the convention of synthetic.collection_cameras).  Per track: the N-view midpoint of its used
    observations, then at most max_iters Gauss-Newton steps on the reprojection error in pixels (a step is kept iff it lowers the cost;
    one that lowers it by no more than ftol times the cost ends the run).  An observation with an index out of range or with a keypoint,
    pose or focal length that is not finite is skipped.  The kernel reads the ranges and n_tracks itself, so nothing is read back.
    Returns (X [T, 3] in the world frame, info [T, 5] int32 = (observations used, observations in front and within max_reproj_px at the
    final point, accepted steps, trial steps, _lib.TRI_* status), cost [T, 2] = the summed squared reprojection error at the linear and
    at the final point, cosang [T] = the smallest cosine between two rays of the track[, err [M] in px, ok [M] bool, depth [M] per used
    observation, NaN / False elsewhere]) on the device, asynchronous on the current stream.  TRI_NARROW (no two rays min_angle_deg apart)
    still has its point; TRI_DEGENERATE, TRI_SHORT, TRI_TRUNCATED and the tracks beyond n_tracks have NaN."""
    import torch
    from . import matcher
    if unknown:
        raise ValueError(f"triangulate_tracks_tensors: unknown keyword {sorted(unknown)[0]!r}")
    ts = [track_offsets, obs, obs_image, kps, cams, R, t] + ([] if n_tracks is None else [n_tracks])
    names = "track_offsets, obs, obs_image, kps, cams, R, t (and n_tracks)"
    _require(names, ts)
    T, M, rows, n, ang, px, mi, ft = matcher.check_triangulate_args(tuple(track_offsets.shape), track_offsets.dtype, tuple(obs.shape), obs.dtype,
                                                                    tuple(obs_image.shape), obs_image.dtype, tuple(kps.shape), kps.dtype, tuple(cams.shape),
                                                                    cams.dtype, tuple(R.shape), R.dtype, tuple(t.shape), t.dtype, _sd(n_tracks),
                                                                    min_angle_deg, max_reproj_px, max_iters, ftol)
    _require(names, ts, "cuda")
    dev = obs.device
    o = track_offsets.contiguous(); ob = obs.contiguous(); oi = obs_image.contiguous(); cm = cams.contiguous()
    xy = kps[:, :2].contiguous()
    poses = torch.cat([R.reshape(n, 9), t], 1).contiguous()
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)          # noqa: E731
    X = f64(max(T, 1), 3); cost = f64(max(T, 1), 2); cosang = f64(max(T, 1))          # (an address also where T == 0)
    info = torch.empty((max(T, 1), 5), dtype=torch.int32, device=dev)
    err = f64(max(M, 1)) if with_obs else None
    depth = f64(max(M, 1)) if with_obs else None
    ok = torch.empty(max(M, 1), dtype=torch.uint8, device=dev) if with_obs else None
    di, stream, sp = _stream(dev)
    p = lambda x: _p(x, empty_none=True)          # noqa: E731
    rc = _lib.lib().mi_degensac_triangulate_tracks_dev(p(o), p(ob), p(oi), p(n_tracks), p(xy), rows, p(cm), p(poses), n, T, M, ang, px, mi, ft, di, sp,
                                                       p(X), p(info), p(cost), p(cosang), p(err), p(ok), p(depth))
    _lib.check_match(rc)
    _keep_alive(stream, o, ob, oi, n_tracks, xy, cm, poses)
    res = (X[:T], info[:T], cost[:T], cosang[:T])
    return res + (err[:M], ok[:M].view(torch.bool), depth[:M]) if with_obs else res


def refine_cameras_tensors(track_offsets, obs, obs_image, kps, cams, R, t, X, n_tracks=None, obs_keep=None, refine=None, max_trials=20, ftol=1e-12,
                           with_err=False, with_table=False, **unknown):
    """Refine camera poses against triangulated tracks, on the device and without a host synchronisation (include/mi_degensac.h
    mi_degensac_camera_refine_tracks_dev): the other block of the reprojection problem after triangulate_tracks_tensors.  The tables,
    kps, cams, R, t and n_tracks go in exactly as that call takes them and X [T, 3] float64 as it returned it (NaN rows are simply not
    used); obs_keep [M] uint8 / bool (None: all) takes its `ok` as it is, and with it every used observation lies in front of its camera
    at the start; refine [n_images] uint8 / bool (None: all): an image with 0 is scored but not moved, which fixes the gauge when the two
    calls alternate.  Per image a Levenberg-Marquardt run over the six degrees of freedom of its pose (R' = C(w) R, t' = t + tau) on the
    reprojection error in pixels with the points held fixed: at most max_trials trial steps, an accepted step that lowers the cost by no
    more than ftol times the cost ends the run, a step that puts an observation behind the camera is rejected.  The call regroups the
    track-major tables by image itself (a stable sort on the device), so nothing is read back.
    Returns (R [n_images, 3, 3], t [n_images, 3], cost [n_images, 2] = (start, end), info [n_images, 4] int32 = (observations used,
    trials, trials accepted, _lib.CAMREF_* status)[, err [M]: the reprojection error in px of the used observations at the final pose, at
    their positions in obs, next to the triangulation's err, NaN elsewhere][, img_offsets [n_images + 1] int64, img_obs [M] int32: the
    positions into obs of every image's used observations, ascending inside an image, -1 behind the last]) on the device, asynchronous
    on the current stream.  An image without a usable start (CAMREF_BAD_CAMERA, BAD_POSE, SHORT, NOT_FINITE, BEHIND) keeps its pose."""
    import torch
    from . import matcher
    if unknown:
        raise ValueError(f"refine_cameras_tensors: unknown keyword {sorted(unknown)[0]!r}")
    ts = [track_offsets, obs, obs_image, kps, cams, R, t, X] + [x for x in (n_tracks, obs_keep, refine) if x is not None]
    names = "track_offsets, obs, obs_image, kps, cams, R, t, X (and n_tracks, obs_keep, refine)"
    _require(names, ts)
    T, M, rows, n, mt, ft = matcher.check_camera_refine_args(tuple(track_offsets.shape), track_offsets.dtype, tuple(obs.shape), obs.dtype,
                                                             tuple(obs_image.shape), obs_image.dtype, tuple(kps.shape), kps.dtype, tuple(cams.shape),
                                                             cams.dtype, tuple(R.shape), R.dtype, tuple(t.shape), t.dtype, tuple(X.shape), X.dtype,
                                                             _sd(n_tracks), _sd(obs_keep), _sd(refine), max_trials, ftol)
    _require(names, ts, "cuda")
    dev = obs.device
    o = track_offsets.contiguous(); ob = obs.contiguous(); oi = obs_image.contiguous(); cm = cams.contiguous(); Xc = X.contiguous()
    xy = kps[:, :2].contiguous()
    poses = torch.cat([R.reshape(n, 9), t], 1).contiguous()
    ok = None if obs_keep is None else obs_keep.contiguous().view(torch.uint8)
    rf = None if refine is None else refine.contiguous().view(torch.uint8)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)          # noqa: E731
    out = f64(max(n, 1), 12); cost = f64(max(n, 1), 2)                # (an address also where n_images == 0)
    info = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
    err = f64(max(M, 1)) if with_err else None
    io = torch.zeros(n + 1, dtype=torch.int64, device=dev) if with_table else None          # (n_images == 0 and M == 0 write nothing)
    iobs = torch.empty(max(M, 1), dtype=torch.int32, device=dev) if with_table else None
    di, stream, sp = _stream(dev)
    p = lambda x: _p(x, empty_none=True)          # noqa: E731
    rc = _lib.lib().mi_degensac_camera_refine_tracks_dev(p(o), p(ob), p(oi), p(n_tracks), p(xy), rows, p(cm), p(poses), n, p(Xc), p(ok), p(rf), T, M, mt,
                                                         ft, di, sp, p(out), p(cost), p(info), p(err), p(io), p(iobs))
    _lib.check_match(rc)
    _keep_alive(stream, o, ob, oi, n_tracks, xy, cm, poses, Xc, ok, rf)
    res = (out[:n, :9].reshape(n, 3, 3), out[:n, 9:], cost[:n], info[:n])
    if with_err:
        res += (err[:M],)
    return res + (io, iobs[:M]) if with_table else res


def average_rotations_tensors(pairs, R_rel, n_images, weight=None, edge_keep=None, R0=None, known=None, root=0, sweeps=200, damping=0.5,
                              robust_deg=5.0, tol=1e-9, with_edges=False, **unknown):
    """Rotation averaging on the device and without a host synchronisation (include/mi_degensac.h mi_degensac_rotation_average_dev): the
    step between the pair-list calls, which end with one (R, t) per pair, and the track calls, which start from one pose per image.
    pairs [K, 2] (int32 or int64, both columns images of ONE store of n_images images) and R_rel [K, 3, 3] float64 exactly as
    relative_pose_tensors / refine_pose_tensors return R for that list: X_j = R_rel X_i with i, j = pairs[k].  weight [K] float64 (None:
    1), e.g. the pose call's info[:, 3].double(); edge_keep [K] bool / uint8 (None: all), e.g. info[:, 4] == _lib.POSE_OK: tensor
    expressions, nothing is read back.  An edge with an end out of range, i == j, a weight that is not > 0 and finite, or an R_rel whose
    squared elements do not add up to 3 within 1e-6 (the zeros of a failed pose entry) is unused.  The gauge: camera `root` is held at
    the identity, or the cameras with known [n] != 0 are held at R0 [n, 3, 3] (this also registers new images against an existing
    reconstruction).  Cameras are first set breadth-first over their heaviest edge, one level per sweep; then every camera that is not
    held moves by `damping` times the weighted mean of its edges' residual Cayley vectors (|w| = tan(angle / 2)); with robust_deg an
    edge's weight is multiplied by (s^2 / (s^2 + |w|^2))^2, s = tan(robust_deg / 2).  `sweeps` Jacobi sweeps are queued, one launch
    each; the first that sets no camera and gives no camera a squared mean above tol^2 is the last that does anything.
    Returns (R [n, 3, 3] world-to-camera, zeros where a camera was never set; info [n, 4] int32 = (half-edges used, the sweep in which
    the camera was set: 0 held, -1 never, opposed edges in the last sweep, _lib.ROTAVG_KNOWN / OK / UNREACHED / ISOLATED); step [n]: the
    squared norm of the camera's last mean vector, NaN where none was formed; summary [4] int64 = (sweeps that changed something, cameras
    set, edges used, _lib.ROTAVG_CONVERGED / MAX_SWEEPS / NO_ROOT)[, edge_cos [K]: the cosine of the angle between R_rel and R_j R_i^T
    at the end, NaN for an edge that is unused or has an end that was never set]) on the device, asynchronous on the current stream.
    Camera positions are not estimated."""
    import torch
    from . import matcher
    if unknown:
        raise ValueError(f"average_rotations_tensors: unknown keyword {sorted(unknown)[0]!r}")
    ts = [pairs, R_rel] + [x for x in (weight, edge_keep, R0, known) if x is not None]
    names = "pairs, R_rel (and weight, edge_keep, R0, known)"
    _require(names, ts)
    K, n, rt, sw, dm, rb, tl = matcher.check_rotavg_args(tuple(pairs.shape), pairs.dtype, tuple(R_rel.shape), R_rel.dtype, n_images, _sd(weight),
                                                         _sd(edge_keep), _sd(R0), _sd(known), root, sweeps, damping, robust_deg, tol)
    _require(names, ts, "cuda")
    dev = R_rel.device
    pr = pairs.contiguous() if pairs.dtype == torch.int32 else pairs.clamp(-1, 0x7fffffff).to(torch.int32).contiguous()
    Rr = R_rel.contiguous()
    w = None if weight is None else weight.contiguous()
    kp = None if edge_keep is None else edge_keep.contiguous().view(torch.uint8)
    r0 = None if R0 is None else R0.contiguous()
    kn = None if known is None else known.contiguous().view(torch.uint8)
    R = torch.empty((n, 3, 3), dtype=torch.float64, device=dev); info = torch.empty((n, 4), dtype=torch.int32, device=dev)
    step = torch.empty(n, dtype=torch.float64, device=dev); summary = torch.empty(4, dtype=torch.int64, device=dev)
    cosv = torch.empty(max(K, 1), dtype=torch.float64, device=dev) if with_edges else None          # (an address also where K == 0)
    di, stream, sp = _stream(dev)
    p = lambda x: _p(x, empty_none=True)          # noqa: E731
    rc = _lib.lib().mi_degensac_rotation_average_dev(p(pr), p(Rr), p(w), p(kp), K, n, _p(r0), _p(kn), rt, sw, dm, rb, tl, di, sp, _p(R), _p(info),
                                                     _p(step), _p(summary), _p(cosv))
    _lib.check_match(rc)
    _keep_alive(stream, pr, Rr, w, kp, r0, kn)
    res = (R, info, step, summary)
    return res + (cosv[:K],) if with_edges else res
