"""GPU: the HIP path against the committed golden fixtures produced by the unmodified reference."""
import os

import numpy as np
import pytest

import pydegensac_amd as pd
from tests import golden_util as gu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", gu.fixtures("F"), ids=lambda p: os.path.basename(p)[:-4])
def test_fundamental_matches_reference_golden(path):
    g = gu.load(path); kw = g["call"]
    F, m = pd.findFundamentalMatrix_(g["p1"], g["p2"], kw.get("px_th", 0.5), kw.get("conf", 0.9999), kw.get("max_iters", 100000),
                                     kw.get("error_type", 0), kw.get("sym_check", True), kw.get("laf_coef", 0.0),
                                     kw.get("degen", True), seed=g["seed"])
    st = pd.last_stats()
    assert st["samples"] == g["samples"] and st["lo_runs"] == g["lo_runs"]
    assert st["full_passes"] == g["full_passes"] and st["ex_passes"] == g["ex_passes"]
    if np.abs(g["model"]).sum() == 0:
        assert np.abs(F).sum() == 0 and not np.asarray(m).any()
    else:
        assert np.array_equal(np.asarray(m), g["mask"])
        assert gu.rel(F, g["model"]) < 1e-6


@pytest.mark.parametrize("path", gu.fixtures("H"), ids=lambda p: os.path.basename(p)[:-4])
def test_homography_matches_reference_golden(path, oracle_port):
    g = gu.load(path); kw = g["call"]
    H, m = pd.findHomography_(g["p1"], g["p2"], kw.get("px_th", 1.0), kw.get("conf", 0.999), kw.get("max_iters", 50000),
                              kw.get("error_type", 0), kw.get("sym_check", True), kw.get("laf_coef", 0.0), seed=g["seed"])
    st = pd.last_stats()
    if g["n"] <= 10:
        # n <= 10 runs through the reference's 4-point u2h path, which reads uninitialised memory (Htools.c:108-114): the fixture's own
        # outputs came from that memory and stay unused.  The fixture's inputs and call go to the restatement instead, which zero-fills
        # there as the device does.
        Ho, mo, so = oracle_port.find_homography(g["p1"], g["p2"], kw.get("px_th", 1.0), kw.get("conf", 0.999), kw.get("max_iters", 50000),
                                                 kw.get("error_type", 0), kw.get("sym_check", True), kw.get("laf_coef", 0.0), seed=g["seed"])
        msg = "against oracle/port.py on the fixture's inputs; the fixture's outputs came from uninitialised memory and are not used"
        assert all(st[k] == so[k] for k in ("samples", "lo_runs", "rejected", "I", "models", "best_sample")), msg
        if np.abs(Ho).sum() == 0:
            assert np.abs(H).sum() == 0 and not np.asarray(m).any(), msg
        else:
            assert np.array_equal(np.asarray(m), mo), msg
            assert gu.rel(H, Ho) < 1e-6, msg
        return
    assert (st["samples"], st["lo_runs"], st["rejected"]) == (g["samples"], g["lo_runs"], g["rejected"])
    assert st["models"] == g["full_passes"]
    if np.abs(g["model"]).sum() == 0:
        assert np.abs(H).sum() == 0
    else:
        assert np.array_equal(np.asarray(m), g["mask"])
        assert gu.rel(H, g["model"]) < 1e-6
