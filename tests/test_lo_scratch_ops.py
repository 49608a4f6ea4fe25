"""CPU only: the one-repetition-per-wave local optimisation of the fundamental-matrix kernel runs without call frames, and its
small solvers reach their LDS scratch through ds_ instructions only.  Compiles the 256-thread translation unit to gfx950
assembly (`hipcc -S`) and counts instructions per function (tools/scratch_ops.py)."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pydegensac_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# the repetition, its passes and its small fit were three non-inlined functions whose callee-saved register saves were
# 88 + 88, 8 + 8 and 25 + 25 scratch instructions per call; the round that runs them inline holds 53 in all
LO_ROUND_SCRATCH_BOUND = 80


def _load_tool():
    spec = importlib.util.spec_from_file_location("scratch_ops", os.path.join(ROOT, "tools", "scratch_ops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def t256_functions(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("asm") / "t256.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-value",
                    "--cuda-device-only", "-S", "mi_degensac_t256.hip", "-o", out], cwd=CSRC, check=True, capture_output=True)
    tool = _load_tool()
    fns = tool.functions(open(out).read())
    names = list(fns)
    return {d: fns[k] for k, d in zip(names, tool.demangle(names))}


def _find(fns, *parts):
    return {k: v for k, v in fns.items() if all(p in k for p in parts)}


def test_lo_repetition_has_no_call_frames(t256_functions):
    for name in ("dg_lo_rep_wave", "dg_f_wpass", "dg_u2f_small_wave"):
        assert not _find(t256_functions, name), f"{name} is a function of its own again (callee-saved saves per call)"
    rounds = _find(t256_functions, "dg_inFrani_waves<", ", false>")
    assert len(rounds) == 3, sorted(rounds)
    for k, c in rounds.items():
        ops = c["scratch_store"] + c["scratch_load"]
        assert ops <= LO_ROUND_SCRATCH_BOUND, (k, c)


def test_small_solvers_of_the_lo_fit_use_lds_by_type(t256_functions):
    for name in ("dg_eig_sym_wave<", "dg_svd_lastcol_9x8_wave<"):
        typed = {k: v for k, v in _find(t256_functions, name).items() if "AS3" in k}
        assert len(typed) == 1, (name, sorted(_find(t256_functions, name)))
        for k, c in typed.items():
            assert c["flat_store"] == 0 and c["flat_load"] == 0, (k, c)
            assert c["scratch_store"] == 0 and c["scratch_load"] == 0, (k, c)
