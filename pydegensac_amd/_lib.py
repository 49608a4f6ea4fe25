"""ctypes binding of libmi_degensac.so (include/mi_degensac.h).  No CPU fallback: if the HIP
library is missing or no gfx950 device is usable, every call raises."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI_DEGENSAC_LIB") or os.path.join(_HERE, "libmi_degensac.so")
STATS_LEN = 16
OK, EINVAL, ENODEV, EHIP, ENOMEM = 0, -1, -2, -3, -4          # include/mi_degensac.h MI_DEGENSAC_OK / _EINVAL / _ENODEV / _EHIP / _ENOMEM
STAT_NAMES = ["samples", "lo_runs", "rejected", "I", "models", "degen", "Ih", "best_sample",
              "full_passes", "ex_passes", "h_passes", "aux_passes", "ticks_best", "ticks_total", "threads", "placement"]
FLAG_FINAL_LAF_FILTER = 1
FLAG_LEGACY_F = 2            # exp_ransacF / exp_ransacFcustom sample-budget rule (include/mi_degensac.h)
# per-call scheduling switches (results never depend on them; they win over set_stream_mode / set_hjob_mode)
FLAG_NO_STREAM, FLAG_STREAM_ON, FLAG_NO_HJOB, FLAG_STREAM_AUTO, FLAG_HJOB_ON = 4, 8, 16, 64, 128


def FLAG_STREAM_TEST(b): return (int(b) & 3) << 8        # noqa: E704  with FLAG_STREAM_ON: bit 0 = owner re-scores, bit 1 = ask at once
# params.tuning (include/mi_degensac.h MI_DEGENSAC_TUNE_*): speed knobs only, results never depend on them
TUNE_LATENCY, TUNE_THROUGHPUT, TUNE_THROUGHPUT4 = 1, 2, 3   # kernel variant: 512- / 256- / 128-thread workgroups
TUNE_PLACE_HBM, TUNE_PLACE_LDS, TUNE_PLACE_POOL_LDS = 1 << 2, 2 << 2, 3 << 2
TUNE_SEQ_POOL = 1 << 4
TUNE_H_SERIAL_LO = 1 << 5   # homography only: local-optimisation repetitions one after the other (default: one per wave)
TUNE_COOP_ALL_PASSES = 1 << 6   # fundamental matrix with helper workgroups: distribute every full pass (tests)
TUNE_F_SERIAL_REPS = 1 << 7   # fundamental matrix: the repetitions of innerH and of the local optimisation one after the other (default: one per wave; tests)


def TUNE_HELPERS(h): return (int(h) & 255) << 8          # noqa: E704  helper workgroups per pair (255 = off)
def TUNE_SET_ASIDE(t): return (int(t) & 255) << 16       # noqa: E704  set pairs aside after t * 256 samples (255 = off)
def TUNE_GRID_CAP(g): return (int(g) & 31) << 24         # noqa: E704  cap on resident workgroups (tests)
def TUNE_LONG_SHIFT(l): return (int(l) & 7) << 29        # noqa: E704,E741  "many samples left" = threshold << l
# bits 8-15: cooperative helper workgroups per pair (0 auto, 255 off); bits 16-23: samples after which a running pair is
# set aside while unstarted pairs remain, in units of 256 (0 auto, 255 off); bits 24-31: cap on resident workgroups (tests)
# the correspondence export (csrc/mi_correspond.hip MX_ROWS / MX_SCAN, mi_degensac_correspondences_tile): rows per workgroup of the
# compaction and workgroup counts per step of its scan; MI_DEGENSAC_CORR_STORE_ROWS
CORR_ROWS, CORR_SCAN = 1024, 256
CORR_STORE_ROWS = 1
# the tracks (csrc/mi_tracks.hip TK_ROWS / TK_SCAN, mi_degensac_tracks_tile): sorted positions per workgroup of the boundary passes and
# workgroup counts per step of their scan
TRACK_ROWS, TRACK_SCAN = 1024, 256
# the refit (csrc/mi_refit.hip RF_STEP / RF_GRID, mi_degensac_refit_tile): rows per workgroup and step of a scoring pass, the cap on the
# grid; the status column of its info rows (MI_DEGENSAC_REFIT_*)
REFIT_STEP, REFIT_GRID = 1024, 256
REFIT_FIXED, REFIT_MAX_FITS, REFIT_SHORT, REFIT_BAD_FIT, REFIT_WORSE, REFIT_TRUNCATED = range(6)
# the relative pose (csrc/mi_pose_dev.h MI_POSE_STEP / MI_POSE_GRID, mi_degensac_pose_tile): rows per workgroup and step of a row pass, the cap on the
# grid; the status column of its info rows (MI_DEGENSAC_POSE_*)
POSE_STEP, POSE_GRID = 1024, 256
POSE_OK, POSE_BAD_MODEL, POSE_BAD_CAMERA, POSE_TRUNCATED, POSE_EMPTY = range(5)
# the relative pose from a homography (csrc/mi_pose_dev.h MI_POSE_STEP / MI_POSE_GRID, mi_degensac_pose_h_tile): the same tile constants; its info
# rows reuse the POSE_* statuses and add POSE_ROTATION for a pure rotation (MI_DEGENSAC_POSE_ROTATION)
POSE_H_STEP, POSE_H_GRID = 1024, 256
POSE_ROTATION = 5
# the pose refinement (csrc/mi_pose_refine.hip PR_STEP / PR_GRID, mi_degensac_pose_refine_tile): rows per workgroup and step of a row pass,
# the cap on the grid; the status column of its info rows (MI_DEGENSAC_REFINE_*)
REFINE_STEP, REFINE_GRID = 1024, 256
REFINE_CONVERGED, REFINE_STALLED, REFINE_MAX_TRIALS, REFINE_SHORT, REFINE_NOT_FINITE, REFINE_BAD_POSE, REFINE_BAD_CAMERA, REFINE_TRUNCATED = range(8)
# the triangulation of tracks (csrc/mi_triangulate.hip TR_GRID / TR_CH, mi_degensac_triangulate_tile): the cap on the grid, rays per staging
# area of the pair pass; the lanes per track are a build constant (TR_G) that tri_group() reads from the loaded library; the status column
# of its info rows (MI_DEGENSAC_TRI_*)
TRI_GRID, TRI_CHUNK = 1024, 64
TRI_OK, TRI_NARROW, TRI_DEGENERATE, TRI_SHORT, TRI_TRUNCATED = range(5)
# the refinement of camera poses against tracks (csrc/mi_camera_refine.hip CR_STEP / CR_GRID / CR_G, mi_degensac_camera_refine_tile):
# observations per workgroup and step of a row pass, the cap on the grid, lanes per track of the mark kernel; the status column of its info
# rows (MI_DEGENSAC_CAMREF_*)
CAMREF_STEP, CAMREF_GRID, CAMREF_GROUP = 512, 256, 16
(CAMREF_CONVERGED, CAMREF_STALLED, CAMREF_MAX_TRIALS, CAMREF_FIXED, CAMREF_BEHIND, CAMREF_NOT_FINITE, CAMREF_SHORT, CAMREF_BAD_POSE,
 CAMREF_BAD_CAMERA) = range(9)
# rotation averaging (csrc/mi_rotavg.hip RA_GRID / RA_CPW, mi_degensac_rotation_average_tile): the cap on the grid of a sweep, cameras per
# workgroup; the lanes per camera are a build constant (RA_G) that rotavg_group() reads from the loaded library; the status column of its
# info rows and the global status of its summary (MI_DEGENSAC_ROTAVG_*)
ROTAVG_GRID, ROTAVG_CAMERAS = 1024, 16
ROTAVG_KNOWN, ROTAVG_OK, ROTAVG_UNREACHED, ROTAVG_ISOLATED = range(4)
ROTAVG_CONVERGED, ROTAVG_MAX_SWEEPS, ROTAVG_NO_ROOT = range(3)


class Params(C.Structure):
    _fields_ = [("px_th", C.c_double), ("conf", C.c_double), ("max_iters", C.c_int32), ("error_type", C.c_int32),
                ("symmetric_error_check", C.c_int32), ("enable_degeneracy_check", C.c_int32),
                ("laf_consistensy_coef", C.c_double), ("flags", C.c_uint32), ("tuning", C.c_uint32)]


class Diag(C.Structure):
    """mi_degensac_diag (include/mi_degensac.h): optional device buffers of the *_batch_dev_ex entry points.  struct_size is filled
    in here (the library reads fields added after the first layout only when the stated size covers them)."""
    _fields_ = [("d_resids", C.c_void_p), ("resid_runs", C.c_int32), ("struct_size", C.c_int32), ("d_hist", C.c_void_p), ("d_screen", C.c_void_p)]

    def __init__(self, d_resids=None, resid_runs=0, struct_size=0, d_hist=None, d_screen=None):
        super().__init__(d_resids, int(resid_runs), int(struct_size) or C.sizeof(Diag), d_hist, d_screen)


class H2elParams(C.Structure):
    _fields_ = [("th", C.c_double), ("conf", C.c_double), ("max_iters", C.c_int32), ("do_lo", C.c_int32),
                ("inl_limit", C.c_int32), ("reserved", C.c_int32)]


class MatchParams(C.Structure):
    """mi_degensac_match_params (include/mi_degensac.h) of the batched match-and-verify entry points.  fginn_th: None = the plain
    second neighbour, a number = the FGINN ratio test at that radius (second_nn = 1, spatial_th)"""
    _fields_ = [("norm", C.c_int32), ("dim", C.c_int32), ("ratio", C.c_float), ("mutual", C.c_int32), ("struct_size", C.c_int32),
                ("second_nn", C.c_int32), ("spatial_th", C.c_double)]

    def __init__(self, norm=0, dim=0, ratio=0.9, mutual=False, fginn_th=None):
        super().__init__(int(norm), int(dim), float(ratio), int(bool(mutual)), C.sizeof(MatchParams), int(fginn_th is not None),
                         0.0 if fginn_th is None else float(fginn_th))


DECIDE_NO_RATIO, DECIDE_BACK_RATIO, DECIDE_MAX_DIST = 1, 2, 4        # include/mi_degensac.h MI_DEGENSAC_DECIDE_*


class MatchParamsEx(MatchParams):
    """mi_degensac_match_params with the decision rule behind spatial_th (40 bytes): decide = DECIDE_* bit flags, max_dist read with
    DECIDE_MAX_DIST.  MatchParams keeps the 32-byte layout, which the library reads as decide = 0."""
    _fields_ = [("decide", C.c_int32), ("max_dist", C.c_float)]

    def __init__(self, norm=0, dim=0, ratio=0.9, mutual=False, fginn_th=None, decide=0, max_dist=0.0):
        super().__init__(norm, dim, ratio, mutual, fginn_th)
        self.struct_size = C.sizeof(MatchParamsEx); self.decide = int(decide); self.max_dist = float(max_dist)


def match_params(norm, dim, rule, fginn_th=None):
    """the match params of a checked rule (matcher.check_rule): the 32-byte struct for the plain ratio test, the extended one as soon as
    a new option is given"""
    if rule.decide == 0:
        return MatchParams(norm, dim, rule.ratio, rule.mutual, fginn_th)
    return MatchParamsEx(norm, dim, rule.ratio, rule.mutual, fginn_th, rule.decide, rule.max_dist)


class QuantParams(C.Structure):
    """mi_degensac_quant_params (include/mi_degensac.h): normalize 0 none / 1 L2 / 2 L1-root, scale, offset of mi_degensac_desc_quantize*"""
    _fields_ = [("struct_size", C.c_int), ("normalize", C.c_int), ("scale", C.c_double), ("offset", C.c_int)]

    def __init__(self, normalize=0, scale=1.0, offset=0):
        super().__init__(C.sizeof(QuantParams), int(normalize), float(scale), int(offset))


class GuideParams(C.Structure):
    """mi_degensac_guide_params (include/mi_degensac.h): the gate of the guided-matching entry points"""
    _fields_ = [("homography", C.c_int32), ("error_type", C.c_int32), ("px_th", C.c_double), ("struct_size", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, homography=0, error_type=0, px_th=0.5):
        super().__init__(int(bool(homography)), int(error_type), float(px_th), C.sizeof(GuideParams), 0)

    def __repr__(self):                 # the fields, not the object's address: stable in logs and in parametrised test ids
        return f"GuideParams(homography={self.homography}, error_type={self.error_type}, px_th={self.px_th!r}, struct_size={self.struct_size})"


class MiDegensacError(RuntimeError):
    pass


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1 (same SONAMEs as /opt/rocm's).
    Whichever copy is mapped first serves the whole process; if /opt/rocm's comes first, a later `import torch` finds
    "No HIP GPUs".  So when torch is installed, map ITS runtime before libmi_degensac.so (without importing torch:
    that costs seconds); the library then runs on that runtime, exactly as when the caller imported torch first."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("MI_DEGENSAC_NO_TORCH_RUNTIME"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MiDegensacError(f"{LIB_PATH} is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                                  "there is no CPU fallback")
        _preload_torch_hip_runtime()
        l = C.CDLL(LIB_PATH)
        dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32); up = C.POINTER(C.c_uint32); bp = C.POINTER(C.c_uint8)
        lp = C.POINTER(C.c_int64); pp = C.POINTER(Params)
        for name in ("mi_degensac_find_fundamental", "mi_degensac_find_homography"):
            f = getattr(l, name); f.restype = C.c_int
            f.argtypes = [dp, dp, C.c_int, C.c_int, pp, C.c_uint32, C.c_int, dp, bp, ip]
        for name in ("mi_degensac_find_fundamental_batch", "mi_degensac_find_homography_batch"):
            f = getattr(l, name); f.restype = C.c_int
            f.argtypes = [dp, dp, lp, C.c_int, C.c_int, pp, up, C.c_int, dp, bp, ip]
        for name in ("mi_degensac_find_fundamental_batch_multi", "mi_degensac_find_homography_batch_multi"):
            f = getattr(l, name); f.restype = C.c_int
            f.argtypes = [dp, dp, lp, C.c_int, C.c_int, pp, up, ip, C.c_int, dp, bp, ip]
        l.mi_degensac_set_wait_ticks.restype = C.c_longlong
        l.mi_degensac_set_wait_ticks.argtypes = [C.c_longlong]
        l.mi_degensac_ransac_h2el_batch.restype = C.c_int
        l.mi_degensac_ransac_h2el_batch.argtypes = [dp, lp, C.c_int, C.POINTER(H2elParams), up, C.c_int, dp, bp, ip]
        l.mi_degensac_ransac_h2el_batch_dev.restype = C.c_int
        l.mi_degensac_ransac_h2el_batch_dev.argtypes = [C.c_void_p, C.c_void_p, lp, C.c_int, C.POINTER(H2elParams), C.c_void_p, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("mi_degensac_find_fundamental_batch_dev", "mi_degensac_find_homography_batch_dev"):
            f = getattr(l, name); f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, lp, C.c_int, C.c_int, pp, C.c_void_p, C.c_int, C.c_void_p,
                          C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("mi_degensac_find_fundamental_batch_dev_ex", "mi_degensac_find_homography_batch_dev_ex"):
            f = getattr(l, name); f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, lp, C.c_int, C.c_int, pp, C.c_void_p, C.c_int, C.c_void_p,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Diag)]
        for name in ("mi_degensac_ctx_find_fundamental_batch", "mi_degensac_ctx_find_homography_batch"):
            f = getattr(l, name); f.restype = C.c_int
            f.argtypes = [C.c_void_p, dp, dp, lp, C.c_int, C.c_int, pp, up, dp, bp, ip]
        l.mi_degensac_ctx_create.restype = C.c_int
        l.mi_degensac_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        l.mi_degensac_ctx_destroy.restype = None
        l.mi_degensac_ctx_destroy.argtypes = [C.c_void_p]
        l.mi_degensac_ctx_stream.restype = C.c_void_p
        l.mi_degensac_ctx_stream.argtypes = [C.c_void_p]
        if hasattr(l, "mi_degensac_ctx_set_scheduling"):          # (absent from older builds loaded through MI_DEGENSAC_LIB for A/B runs)
            l.mi_degensac_ctx_set_scheduling.restype = C.c_int
            l.mi_degensac_ctx_set_scheduling.argtypes = [C.c_void_p, C.c_int, C.c_int]
        l.mi_degensac_release_scratch.restype = C.c_int
        l.mi_degensac_release_scratch.argtypes = [C.c_int, C.c_void_p]
        l.mi_degensac_pool_stage_parallel.restype = C.c_int
        l.mi_degensac_pool_stage_parallel.argtypes = [C.c_int]
        l.mi_degensac_sample_stream_ex.restype = C.c_int
        l.mi_degensac_sample_stream_ex.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip]
        l.mi_degensac_score_models.restype = C.c_int
        l.mi_degensac_score_models.argtypes = [dp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_double, C.c_int, up, dp, dp]
        l.mi_degensac_sample_stream.restype = C.c_int
        l.mi_degensac_sample_stream.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, ip]
        l.mi_degensac_solve7.restype = C.c_int
        l.mi_degensac_solve7.argtypes = [dp, dp, C.c_int, C.c_int, ip, C.c_int, C.c_int, ip, ip, dp]
        for name in ("mi_degensac_find_fundamental_resids", "mi_degensac_find_homography_resids"):
            f = getattr(l, name); f.restype = C.c_int
            f.argtypes = [dp, dp, C.c_int, C.c_int, pp, C.c_uint32, C.c_int, dp, bp, ip, dp, C.c_int]
        l.mi_degensac_find_fundamental_hist.restype = C.c_int
        l.mi_degensac_find_fundamental_hist.argtypes = [dp, dp, C.c_int, C.c_int, pp, C.c_uint32, C.c_int, dp, bp, ip, ip]
        l.mi_degensac_match.restype = C.c_int
        l.mi_degensac_match.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, ip,
                                        C.POINTER(C.c_float), bp]
        l.mi_degensac_match_knn2_dev.restype = C.c_int
        l.mi_degensac_match_knn2_dev.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.mi_degensac_match_filter_dev.restype = C.c_int
        l.mi_degensac_match_filter_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        mpp = C.POINTER(MatchParams)
        if hasattr(l, "mi_degensac_match_decide_dev"):                    # (absent from older builds loaded through MI_DEGENSAC_LIB)
            l.mi_degensac_match_decide_dev.restype = C.c_int
            l.mi_degensac_match_decide_dev.argtypes = [mpp, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            l.mi_degensac_match_ex.restype = C.c_int
            l.mi_degensac_match_ex.argtypes = [mpp, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, ip, C.POINTER(C.c_float), bp]
        l.mi_degensac_match_knn2_batch_dev.restype = C.c_int
        l.mi_degensac_match_knn2_batch_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, lp, lp, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
        if hasattr(l, "mi_degensac_match_fginn_knn2_batch_dev"):          # (absent from older builds loaded through MI_DEGENSAC_LIB)
            l.mi_degensac_match_fginn_knn2_batch_dev.restype = C.c_int
            l.mi_degensac_match_fginn_knn2_batch_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, lp, lp, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                                 C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.mi_degensac_match_verify_batch_dev.restype = C.c_int
        l.mi_degensac_match_verify_batch_dev.argtypes = [C.c_int, mpp, C.c_void_p, C.c_void_p, lp, lp, C.c_void_p, C.c_void_p, C.c_int, C.c_int, pp,
                                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ip]
        l.mi_degensac_match_verify_batch.restype = C.c_int
        l.mi_degensac_match_verify_batch.argtypes = [C.c_int, mpp, C.c_void_p, C.c_void_p, lp, lp, dp, dp, C.c_int, C.c_int, pp, up, C.c_int,
                                                     dp, ip, bp, ip, ip]
        if hasattr(l, "mi_degensac_match_knn2_pairs_dev"):                # (absent from older builds loaded through MI_DEGENSAC_LIB)
            l.mi_degensac_match_knn2_pairs_dev.restype = C.c_int
            l.mi_degensac_match_knn2_pairs_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, lp, C.c_int, lp, C.c_int, ip, C.c_int, C.c_int, C.c_int,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]
            l.mi_degensac_match_verify_pairs_dev.restype = C.c_int
            l.mi_degensac_match_verify_pairs_dev.argtypes = [C.c_int, mpp, C.c_void_p, C.c_void_p, lp, C.c_int, lp, C.c_int, C.c_void_p, C.c_void_p,
                                                             C.c_int, ip, C.c_int, pp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_void_p, ip]
            l.mi_degensac_match_verify_pairs.restype = C.c_int
            l.mi_degensac_match_verify_pairs.argtypes = [C.c_int, mpp, C.c_void_p, C.c_void_p, lp, C.c_int, lp, C.c_int, dp, dp, C.c_int, ip, C.c_int,
                                                         pp, up, C.c_int, dp, ip, bp, ip, ip]
        if hasattr(l, "mi_degensac_match_fginn_knn2_pairs_dev"):          # (absent from older builds loaded through MI_DEGENSAC_LIB)
            l.mi_degensac_match_fginn_knn2_pairs_dev.restype = C.c_int
            l.mi_degensac_match_fginn_knn2_pairs_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, lp, C.c_int, lp, C.c_int, ip, C.c_int, C.c_int,
                                                                 C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            l.mi_degensac_match_verify_fginn_pairs_dev.restype = C.c_int
            l.mi_degensac_match_verify_fginn_pairs_dev.argtypes = l.mi_degensac_match_verify_pairs_dev.argtypes
            l.mi_degensac_match_verify_fginn_pairs.restype = C.c_int
            l.mi_degensac_match_verify_fginn_pairs.argtypes = l.mi_degensac_match_verify_pairs.argtypes
        if hasattr(l, "mi_degensac_match_verify_fh_pairs_dev"):           # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # both models on the same tentatives: no homography flag, two parameter blocks, and after the stream (_dev) / the device
            # model_f, model_h, match, inlier_f, inlier_h, stats_f, stats_h, summary, counts
            vp = C.c_void_p
            l.mi_degensac_match_verify_fh_batch_dev.restype = C.c_int
            l.mi_degensac_match_verify_fh_batch_dev.argtypes = [mpp, vp, vp, lp, lp, vp, vp, C.c_int, C.c_int, pp, pp, vp, C.c_int, vp,
                                                                vp, vp, vp, vp, vp, vp, vp, vp, ip]
            l.mi_degensac_match_verify_fh_batch.restype = C.c_int
            l.mi_degensac_match_verify_fh_batch.argtypes = [mpp, vp, vp, lp, lp, dp, dp, C.c_int, C.c_int, pp, pp, up, C.c_int,
                                                            dp, dp, ip, bp, bp, ip, ip, ip, ip]
            l.mi_degensac_match_verify_fh_pairs_dev.restype = C.c_int
            l.mi_degensac_match_verify_fh_pairs_dev.argtypes = [mpp, vp, vp, lp, C.c_int, lp, C.c_int, vp, vp, C.c_int, ip, C.c_int, pp, pp, vp,
                                                                C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, ip]
            l.mi_degensac_match_verify_fh_pairs.restype = C.c_int
            l.mi_degensac_match_verify_fh_pairs.argtypes = [mpp, vp, vp, lp, C.c_int, lp, C.c_int, dp, dp, C.c_int, ip, C.c_int, pp, pp, up,
                                                            C.c_int, dp, dp, ip, bp, bp, ip, ip, ip, ip]
        gpp = C.POINTER(GuideParams)
        l.mi_degensac_match_guided_knn2_batch_dev.restype = C.c_int
        l.mi_degensac_match_guided_knn2_batch_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, lp, lp, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                              C.c_void_p, gpp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.mi_degensac_match_guided_batch_dev.restype = C.c_int
        l.mi_degensac_match_guided_batch_dev.argtypes = [mpp, C.c_void_p, C.c_void_p, lp, lp, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, gpp,
                                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ip]
        l.mi_degensac_match_guided_batch.restype = C.c_int
        l.mi_degensac_match_guided_batch.argtypes = [mpp, C.c_void_p, C.c_void_p, lp, lp, dp, dp, C.c_int, C.c_int, dp, gpp, C.c_int, ip,
                                                     C.POINTER(C.c_float), ip, ip]
        if hasattr(l, "mi_degensac_match_guided_pairs_dev"):              # (absent from older builds loaded through MI_DEGENSAC_LIB)
            l.mi_degensac_match_guided_knn2_pairs_dev.restype = C.c_int
            l.mi_degensac_match_guided_knn2_pairs_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, lp, C.c_int, lp, C.c_int, ip, C.c_int, C.c_int,
                                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, gpp, C.c_int, C.c_void_p, C.c_void_p,
                                                                  C.c_void_p]
            l.mi_degensac_match_guided_pairs_dev.restype = C.c_int
            l.mi_degensac_match_guided_pairs_dev.argtypes = [mpp, C.c_void_p, C.c_void_p, lp, C.c_int, lp, C.c_int, ip, C.c_int, C.c_void_p, C.c_void_p,
                                                             C.c_int, C.c_void_p, gpp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, ip]
            l.mi_degensac_match_guided_pairs.restype = C.c_int
            l.mi_degensac_match_guided_pairs.argtypes = [mpp, C.c_void_p, C.c_void_p, lp, C.c_int, lp, C.c_int, ip, C.c_int, dp, dp, C.c_int, dp, gpp,
                                                         C.c_int, ip, C.POINTER(C.c_float), ip, ip]
        if hasattr(l, "mi_degensac_match_guided_fginn_pairs_dev"):        # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # FGINN inside the gate: the knn2 forms take the radius after the guide params, the others read it from the match params
            for lay in ("batch", "pairs"):
                f = getattr(l, f"mi_degensac_match_guided_fginn_knn2_{lay}_dev"); f.restype = C.c_int
                at = list(getattr(l, f"mi_degensac_match_guided_knn2_{lay}_dev").argtypes)
                f.argtypes = at[:at.index(gpp) + 1] + [C.c_double] + at[at.index(gpp) + 1:]
                for tail in ("_dev", ""):
                    f = getattr(l, f"mi_degensac_match_guided_fginn_{lay}{tail}"); f.restype = C.c_int
                    f.argtypes = getattr(l, f"mi_degensac_match_guided_{lay}{tail}").argtypes
        if hasattr(l, "mi_degensac_desc_quantize_dev"):                   # (absent from older builds loaded through MI_DEGENSAC_LIB)
            qpp = C.POINTER(QuantParams)
            l.mi_degensac_desc_quantize_dev.restype = C.c_int
            l.mi_degensac_desc_quantize_dev.argtypes = [qpp, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            l.mi_degensac_desc_quantize.restype = C.c_int
            l.mi_degensac_desc_quantize.argtypes = [qpp, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            l.mi_degensac_desc_quantize_pass_rows.restype = C.c_int64
            l.mi_degensac_desc_quantize_pass_rows.argtypes = [C.c_int]
        if hasattr(l, "mi_degensac_correspondences_pairs_dev"):           # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # layout | match, keep, flags, kp1, kp2, kp_dim, models, gp, capacity, device[, stream] | corr_offsets, total, rows, entry, pts, resid
            vp = C.c_void_p
            mid = [vp, vp, C.c_uint32, vp, vp, C.c_int, vp, gpp, C.c_int64, C.c_int]
            outs = [vp, vp, vp, vp, vp, vp]
            for name, lay in (("pairs", [lp, C.c_int, lp, C.c_int, ip, C.c_int]), ("batch", [lp, lp, C.c_int])):
                f = getattr(l, f"mi_degensac_correspondences_{name}_dev"); f.restype = C.c_int
                f.argtypes = lay + mid + [vp] + outs
                f = getattr(l, f"mi_degensac_correspondences_{name}"); f.restype = C.c_int
                f.argtypes = lay + mid + outs
            l.mi_degensac_correspondences_tile.restype = C.c_int
            l.mi_degensac_correspondences_tile.argtypes = [C.c_int]
        if hasattr(l, "mi_degensac_tracks_dev"):                          # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # offsets, n_images, rows, n_edges, total, device[, stream] | label, track, n_tracks, n_obs, track_offsets, obs, obs_image, track_images
            vp = C.c_void_p
            l.mi_degensac_tracks_dev.restype = C.c_int
            l.mi_degensac_tracks_dev.argtypes = [lp, C.c_int, vp, C.c_int64, vp, C.c_int, vp] + [vp] * 8
            l.mi_degensac_tracks.restype = C.c_int
            l.mi_degensac_tracks.argtypes = [lp, C.c_int, vp, C.c_int64, C.c_int64, C.c_int] + [vp] * 8
            l.mi_degensac_tracks_tile.restype = C.c_int
            l.mi_degensac_tracks_tile.argtypes = [C.c_int]
        if hasattr(l, "mi_degensac_refit_lists_dev"):                     # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # pts, corr_offsets, models, K, cap, gp, max_fits, device[, stream] | models_out, inlier, models_user, info, resid
            vp = C.c_void_p
            l.mi_degensac_refit_lists_dev.restype = C.c_int
            l.mi_degensac_refit_lists_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int64, gpp, C.c_int, C.c_int, vp] + [vp] * 5
            l.mi_degensac_refit_lists.restype = C.c_int
            l.mi_degensac_refit_lists.argtypes = [vp, vp, vp, C.c_int, C.c_int64, gpp, C.c_int, C.c_int] + [vp] * 5
            l.mi_degensac_refit_tile.restype = C.c_int
            l.mi_degensac_refit_tile.argtypes = [C.c_int]
        # pts, corr_offsets, keep, F | H, cams, n_cams, cam_idx, K, cap, cos_min[, rotation_eps], device[, stream] | pose, front, info[, normal,
        # t_over_d], X, depth, cosang, cand[, cand_normal], cand_front
        for name, scalars, n_out in (("pose", [C.c_double], 8), ("pose_h", [C.c_double, C.c_double], 11)):
            if hasattr(l, "mi_degensac_%s_lists_dev" % name):             # (absent from older builds loaded through MI_DEGENSAC_LIB)
                vp = C.c_void_p
                head = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int64] + scalars + [C.c_int]
                for fn, args in (("lists_dev", head + [vp] + [vp] * n_out), ("lists", head + [vp] * n_out), ("tile", [C.c_int])):
                    f = getattr(l, "mi_degensac_%s_%s" % (name, fn))
                    f.restype = C.c_int; f.argtypes = args
        if hasattr(l, "mi_degensac_pose_refine_lists_dev"):               # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # pts, corr_offsets, keep, pose, cams, n_cams, cam_idx, K, cap, max_trials, ftol, device[, stream] | pose_out, cost, info, resid, F
            vp = C.c_void_p
            head = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_double, C.c_int]
            l.mi_degensac_pose_refine_lists_dev.restype = C.c_int
            l.mi_degensac_pose_refine_lists_dev.argtypes = head + [vp] + [vp] * 5
            l.mi_degensac_pose_refine_lists.restype = C.c_int
            l.mi_degensac_pose_refine_lists.argtypes = head + [vp] * 5
            l.mi_degensac_pose_refine_tile.restype = C.c_int
            l.mi_degensac_pose_refine_tile.argtypes = [C.c_int]
        if hasattr(l, "mi_degensac_triangulate_tracks_dev"):              # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # track_offsets, obs, obs_image, n_tracks, kps, rows, cams, poses, n_images, T, M, min_angle_deg, max_reproj_px, max_iters, ftol,
            # device[, stream] | X, info, cost, cosang, err, ok, depth
            vp = C.c_void_p
            tail = [vp, C.c_int64, vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int]
            l.mi_degensac_triangulate_tracks_dev.restype = C.c_int
            l.mi_degensac_triangulate_tracks_dev.argtypes = [vp, vp, vp, vp] + tail + [vp] + [vp] * 7
            l.mi_degensac_triangulate_tracks.restype = C.c_int
            l.mi_degensac_triangulate_tracks.argtypes = [vp, vp, vp, C.c_int64] + tail + [vp] * 7
            l.mi_degensac_triangulate_tile.restype = C.c_int
            l.mi_degensac_triangulate_tile.argtypes = [C.c_int]
        if hasattr(l, "mi_degensac_camera_refine_tracks_dev"):            # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # track_offsets, obs, obs_image, n_tracks, kps, rows, cams, poses, n_images, X, obs_keep, refine, T, M, max_trials, ftol,
            # device[, stream] | poses_out, cost, info, err, img_offsets, img_obs
            vp = C.c_void_p
            tail = [vp, C.c_int64, vp, vp, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_int]
            l.mi_degensac_camera_refine_tracks_dev.restype = C.c_int
            l.mi_degensac_camera_refine_tracks_dev.argtypes = [vp, vp, vp, vp] + tail + [vp] + [vp] * 6
            l.mi_degensac_camera_refine_tracks.restype = C.c_int
            l.mi_degensac_camera_refine_tracks.argtypes = [vp, vp, vp, C.c_int64] + tail + [vp] * 6
            l.mi_degensac_camera_refine_tile.restype = C.c_int
            l.mi_degensac_camera_refine_tile.argtypes = [C.c_int]
        if hasattr(l, "mi_degensac_rotation_average_dev"):                # (absent from older builds loaded through MI_DEGENSAC_LIB)
            # pairs, R_rel, weight, edge_keep, K, n_images, R0, known, root, sweeps, damping, robust_deg, tol, device[, stream] | R, info, step,
            # summary, edge_cos
            vp = C.c_void_p
            head = [vp, vp, vp, vp, C.c_int64, C.c_int, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]
            l.mi_degensac_rotation_average_dev.restype = C.c_int
            l.mi_degensac_rotation_average_dev.argtypes = head + [vp] + [vp] * 5
            l.mi_degensac_rotation_average.restype = C.c_int
            l.mi_degensac_rotation_average.argtypes = head + [vp] * 5
            l.mi_degensac_rotation_average_tile.restype = C.c_int
            l.mi_degensac_rotation_average_tile.argtypes = [C.c_int]
        l.mi_degensac_kpts_to_xyA.restype = C.c_int
        l.mi_degensac_kpts_to_xyA.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, dp]
        l.mi_degensac_kpts_to_xyA_dev.restype = C.c_int
        l.mi_degensac_kpts_to_xyA_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.mi_degensac_match_last_error.restype = C.c_char_p
        l.mi_degensac_mat3.restype = C.c_int
        l.mi_degensac_mat3.argtypes = [C.c_int, dp, C.c_int, C.c_int, dp, ip]
        l.mi_degensac_screen_counts.restype = C.c_int
        l.mi_degensac_screen_counts.argtypes = [dp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_double, C.c_int, up, up]
        l.mi_degensac_screen_counts_h.restype = C.c_int
        l.mi_degensac_screen_counts_h.argtypes = [dp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int, up, bp]
        l.mi_degensac_rng_wave.restype = C.c_int
        l.mi_degensac_rng_wave.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, ip]
        if hasattr(l, "mi_degensac_set_call_timing"):
            l.mi_degensac_set_call_timing.restype = C.c_int
            l.mi_degensac_set_call_timing.argtypes = [C.c_int]
            l.mi_degensac_last_call_timing.restype = C.c_int
            l.mi_degensac_last_call_timing.argtypes = [dp]
        l.mi_degensac_last_error.restype = C.c_char_p
        l.mi_degensac_version.restype = C.c_char_p
        l.mi_degensac_kernel_name.restype = C.c_char_p
        l.mi_degensac_device_count.restype = C.c_int
        _lib = l
    return _lib


def tri_group():
    """lanes per track of the loaded library's triangulation kernel (mi_degensac_triangulate_tile(0)): the order of its sums depends on it"""
    return int(lib().mi_degensac_triangulate_tile(0))


def rotavg_group():
    """lanes per camera of the loaded library's rotation-averaging sweep (mi_degensac_rotation_average_tile(0)): the order of its sums
    depends on it"""
    return int(lib().mi_degensac_rotation_average_tile(0))


def check(rc, last_error="mi_degensac_last_error", value_error=True):
    if rc != 0:
        msg = getattr(lib(), last_error)().decode()
        if rc == -1 and value_error:
            raise ValueError(msg)          # std::invalid_argument -> ValueError in the reference binding
        raise MiDegensacError(f"mi_degensac error {rc}: {msg}")


def check_match(rc, value_error=True):
    """check() for the matcher-stage entry points, whose message is mi_degensac_match_last_error(); value_error=False: the calls that
    have always raised MiDegensacError for an invalid argument too"""
    check(rc, "mi_degensac_match_last_error", value_error)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# keyed by the dtype itself: its name is slow to form, and this sits under every call
_POINTERS = {np.dtype(name): C.POINTER(ct) for name, ct in (("float64", C.c_double), ("float32", C.c_float), ("int64", C.c_int64),
                                                            ("int32", C.c_int32), ("uint32", C.c_uint32), ("uint8", C.c_uint8))}


def ptr(a):
    """a numpy array as the typed pointer the argtypes table asks for"""
    return a.ctypes.data_as(_POINTERS[a.dtype])


def vptr(a, empty_none=False):
    """a numpy array as void *; None stays None (a nullable argument), and with empty_none so does an array without elements"""
    return None if a is None or (empty_none and a.size == 0) else a.ctypes.data_as(C.c_void_p)


def make_params(px_th, conf, max_iters, error_type, sym_check, laf_coef, degen=True, flags=0, tuning=0):
    return Params(float(px_th), float(conf), int(max_iters), int(error_type), int(bool(sym_check)), int(bool(degen)),
                  float(laf_coef), int(flags), int(tuning))


def set_stream_mode(mode):
    """stream mode of the fundamental-matrix kernel (include/mi_degensac.h): -1 automatic, 0 off, odd > 0 = on with test bits; returns the previous mode"""
    f = lib().mi_degensac_set_stream_mode
    f.restype = C.c_int; f.argtypes = [C.c_int]
    return int(f(int(mode)))


def set_hjob_mode(mode):
    """homography helper workgroups (include/mi_degensac.h): 1 on, 0 off; returns the previous mode"""
    f = lib().mi_degensac_set_hjob_mode
    f.restype = C.c_int; f.argtypes = [C.c_int]
    return int(f(int(mode)))


def set_wait_ticks(ticks):
    """test hook: limit of the stream mode's data waits in 100 MHz device ticks (0: every data wait fails at once; < 0: the default
    4 s); returns the previous limit"""
    return int(lib().mi_degensac_set_wait_ticks(int(ticks)))


TIMING_NAMES = ["call_ms", "pack_ms", "enqueue_ms", "wait_ms", "unpack_ms", "dev_h2d_ms", "dev_kernel_ms", "dev_d2h_ms"]


def set_call_timing(on):
    """per-call timing of the host-pointer entry points (include/mi_degensac.h); returns the previous switch"""
    return int(lib().mi_degensac_set_call_timing(int(bool(on))))


def last_call_timing():
    """the calling thread's last timed host-pointer call: dict of TIMING_NAMES (milliseconds)"""
    out = (C.c_double * len(TIMING_NAMES))()
    check(lib().mi_degensac_last_call_timing(out))
    return {k: float(v) for k, v in zip(TIMING_NAMES, out)}


def stats_dict(st):
    d = {k: int(v) for k, v in zip(STAT_NAMES, st)}
    d["set_aside"] = (d["placement"] >> 8) & 1    # the pair was written back to its workspace once and resumed later
    d["streamed"] = (d["placement"] >> 9) & 1     # the pair took chunks from a producer workgroup (stream mode)
    d["discarded"] = (d["placement"] >> 10) & 1   # a hand-over wait of the launch timed out: results discarded (zero model / mask)
    d["rerun"] = (d["placement"] >> 11) & 1       # ... and the host-pointer entry point ran the pair again without helpers
    d["placement"] &= 255
    return d
