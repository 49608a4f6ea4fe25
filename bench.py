#!/usr/bin/env python3
"""bench.py — models/sec of findFundamentalMatrix @ 2000 correspondences on MI355X.

A "step" is one pass of the hot path (the persistent LO-RANSAC/DEGENSAC kernel, one workgroup
per image pair) over one batch of synthetic image pairs.  Workload at every N: each GPU owns
PAIRS_PER_GPU independent pairs of BASELINE config C2 (2000 correspondences, 40 % inliers,
sigma 0.1 px, px_th 0.5, conf 0.9999, max_iters 100000, degeneracy check on, symmetric check on);
PAIRS_PER_GPU = 4096 is config C4's batch size, held per GPU: weak scaling.  (One workgroup owns
one pair and ~9 % of C2 pairs run all 100 000 samples, so a batch needs many pairs per CU for the
256 CUs to stay busy; --pairs-per-gpu 512 gives C4's 8-GPU share and is tail-latency bound.)  Inputs
are resident in HBM before the timed region; the per-pair results are gathered over RCCL inside it.

  python bench.py --gpus 1 --steps K --warmup W
  python bench.py --gpus N --steps K --warmup W        (no WORLD_SIZE in the environment: starts itself as a child process under
                                                        torch.distributed.run with N ranks, one per GPU; fails loudly when
                                                        fewer than N devices are visible)
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
  python bench.py --gpus N --single-process             (ONE process, the C-ABI's device-list mode *_batch_multi, no collective)
  ... --full                                            (everything besides the headline, see below)
  ... --gpus N --full --c4-single-process               (N ranks, and rank 0 also measures the literal C4 batch through one process: on request only)
  ... --dump-outputs DIR                                (the last timed step's results as DIR/*.npy, see dump_outputs)

Prints ONE JSON line on rank 0 (contract of the driver).  A plain run sets up, warms up, times the K steps and prints the line
(`value`, `ms_per_step`, `roofline` from the same steps' HIP events and stats).  --full adds what takes runs or checks of its own:
the parity check of the timed batch against the CPU oracle (--parity-pairs, default 16 with --full, 0 without), `cpu_baseline`
(the reference on one host core, the north-star denominator) and `cpu_baseline_all_cores` (one reference process per host core,
SURVEY 8d) with the parity check over every pair that leg ran, `single_call_ms`, the `secondary` configurations and, with
N > 1 ranks, the literal C4 batch.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec (MI355X_MICROARCH.md)
# --config c2 (default, the configuration BASELINE.json's metric is quoted on): findFundamentalMatrix, 2000 correspondences
# --config c3: findHomography, 5000 correspondences with LAFs, LAF + symmetric checks, LO on (BASELINE configs[2])
CONFIGS = {
    "c2": dict(which="F", n_corr=2000, dim=2, pairs=4096,
               prm=dict(px_th=0.5, conf=0.9999, max_iters=100000, error_type=0, sym=True, laf=0.0, degen=True)),
    "c3": dict(which="H", n_corr=5000, dim=6, pairs=1024,
               prm=dict(px_th=2.0, conf=0.999, max_iters=50000, error_type=0, sym=True, laf=3.0, degen=True)),
    # --config c5: the stress case of BASELINE configs[4]: 50000 correspondences, 10 % inliers, max_iters 200000, one pair
    "c5": dict(which="F", n_corr=50000, dim=2, pairs=1, inlier_ratio=0.1,
               prm=dict(px_th=0.5, conf=0.9999, max_iters=200000, error_type=0, sym=True, laf=0.0, degen=True)),
}
CFG = CONFIGS["c2"]
N_CORR = CFG["n_corr"]
PAIRS_PER_GPU = CFG["pairs"]
PRM = CFG["prm"]


def set_config(name):
    global CFG, N_CORR, PAIRS_PER_GPU, PRM
    CFG = CONFIGS[name]; N_CORR = CFG["n_corr"]; PAIRS_PER_GPU = CFG["pairs"]; PRM = CFG["prm"]


def make_pair(pid):
    """synthetic correspondences of global pair id `pid` (SURVEY 8d generators)"""
    from pydegensac_amd import synthetic
    if CFG["which"] == "F":
        return synthetic.two_view_fundamental(N_CORR, CFG.get("inlier_ratio", 0.4), 0.1, seed=pid)[:2]
    return synthetic.homography_pairs(N_CORR, 0.4, 0.5, seed=pid, laf=True)[:2]


def cpu_call(mod, p1, p2, seed, **kw):
    """one pair through oracle/_ref (mod = oracle.ref) or the restatement (oracle.port) with the bench parameters"""
    if CFG["which"] == "F":
        return mod.find_fundamental(p1, p2, PRM["px_th"], PRM["conf"], PRM["max_iters"], PRM["error_type"], PRM["sym"], PRM["laf"],
                                    PRM["degen"], seed=seed, **kw)
    return mod.find_homography(p1, p2, PRM["px_th"], PRM["conf"], PRM["max_iters"], PRM["error_type"], PRM["sym"], PRM["laf"],
                               seed=seed, **kw)


def cpu_baseline(budget_s=20.0, max_pairs=1024, skip_first=True):
    """The reference CPU path timed on this box's host cores (1 thread): oracle/_ref (the unmodified
    reference build, kind 'reference') when it loads, else the restatement (kind 'port')."""
    from pydegensac_amd import synthetic, parallel
    kind = "port"
    try:
        from oracle import ref
        if ref.available():
            ref.lib(); kind = "reference"
    except Exception:
        kind = "port"
    if kind == "port":
        from oracle import port
        port.lib()
    models = 0; samples = 0; t_total = 0.0; n_done = 0; tbest = []; ids = []
    for p in range(max_pairs):
        p1, p2 = make_pair(p)
        seed = parallel.pair_seed(p)
        t = time.perf_counter()
        if kind == "reference":
            _, _, st = cpu_call(ref, p1, p2, seed, count_models=True)
        else:
            _, _, st = cpu_call(port, p1, p2, seed)
        dt = time.perf_counter() - t
        if p == 0 and skip_first:
            continue                                   # first call warms LAPACK / page cache
        models += st["models"]; samples += st["samples"]; t_total += dt; n_done += 1; ids.append(p)
        if st.get("time_to_best_s", -1) >= 0:
            tbest.append(st["time_to_best_s"] * 1e3)
        if t_total > budget_s:
            break
    out = {"value": models / t_total, "unit": "models/s", "cores": 1, "kind": kind,
           "sample": f"{n_done} pairs of the workload (pair ids {1 if skip_first else 0}..{n_done - (0 if skip_first else 1)}, same generator/seeds as the GPU batch), "
                     f"{t_total:.1f} s, {samples / t_total:.0f} samples/s, {t_total / n_done * 1e3:.1f} ms/pair",
           "pair_ids": [ids[0], ids[-1]]}
    if tbest:
        # the reference-side half of the metric's "time-to-best-inlier-set": from the driver's start to the end of the first
        # scoring pass over the model it RETURNS (oracle/ref_shim.c logs every FDS1 / EXFDS1 / HDS1 pass with its model)
        out["time_to_best_ms"] = {"mean": float(np.mean(tbest)), "p50": float(np.median(tbest)), "max": float(np.max(tbest)), "pairs": len(tbest),
                                  "note": "wall clock of one host core, from the driver's start to the end of the first scoring pass over the returned model"}
    return out


def _cpu_worker(args):
    """One host core: the reference CPU path on its share of pair ids for `budget` seconds (spawned process, no torch)."""
    ids, budget, cfg_name = args
    import time as _t
    sys.path.insert(0, ROOT)
    set_config(cfg_name)
    from pydegensac_amd import parallel
    from oracle import ref
    ref.lib()
    models = 0; t_used = 0.0; n = 0; recs = []
    for p in ids:
        p1, p2 = make_pair(p)
        t = _t.perf_counter()
        M, m, st = cpu_call(ref, p1, p2, parallel.pair_seed(p), count_models=True)
        t_used += _t.perf_counter() - t; models += st["models"]; n += 1
        # what the reference returned for this pair: compared with the timed GPU batch afterwards (parity_against_cpu_leg)
        recs.append((p, st["samples"], st["lo_runs"], st["I"], st["models"], np.packbits(m), np.asarray(M, dtype=np.float64).ravel().copy()))
        if t_used > budget:
            break
    return models, t_used, n, recs


def cpu_baseline_all_cores(cfg_name, budget_s=8.0):
    """Embarrassingly parallel reference run, one process per host core, pairs disjoint from each other.
    Returns None when the reference build is not loadable or the pool cannot be started."""
    try:
        import multiprocessing as mp
        from oracle import ref
        if not ref.available():
            return None
        cores = min(os.cpu_count() or 1, 64)
        ctx = mp.get_context("spawn")
        shares = [(list(range(1 + c, 4096, cores)), budget_s, cfg_name) for c in range(cores)]
        t = time.perf_counter()
        with ctx.Pool(cores) as pool:
            res = pool.map_async(_cpu_worker, shares).get(timeout=budget_s * 4 + 60)
        wall = time.perf_counter() - t
        models = sum(r[0] for r in res); busy = max(r[1] for r in res); pairs = sum(r[2] for r in res)
        return {"value": models / busy, "unit": "models/s", "cores": cores, "kind": "reference",
                "sample": f"{pairs} pairs over {cores} processes, {busy:.1f} s of solver time per process ({wall:.1f} s wall incl. start-up)",
                "_records": [x for r in res for x in r[3]]}
    except Exception as e:                                     # never let the side measurement break the bench line
        return {"value": None, "error": str(e)[:200]}


def source_id():
    """hash of the kernel sources: ties a committed PMC pass to the build it was measured on"""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "pydegensac_amd", "csrc", "*.h")) + glob.glob(os.path.join(ROOT, "pydegensac_amd", "csrc", "*.hip")) +
                    glob.glob(os.path.join(ROOT, "pydegensac_amd", "csrc", "*.inc"))):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(cfg_name, pairs_per_gpu):
    """HBM bytes per launch from the committed rocprofv3 PMC passes of this same command (profiles/README.md):
    2 x FETCH_SIZE + WRITE_SIZE KiB (MI355X_MICROARCH.md: FETCH_SIZE under-reports coalesced reads 2x on gfx950).
    Counters cannot be read from inside the process, so the figure comes from profiles/r5_pmc_<config>.json (older rounds' files as a fallback), which
    tools/pmc_summary.py writes next to the rocprofv3 CSVs together with the hash of the kernel sources it was measured
    on and the batch size; any mismatch with this build / this batch gives null instead of a stale number."""
    path = None
    for rnd in ("r6", "r5", "r4", "r3"):
        cand = os.path.join(ROOT, "profiles", f"{rnd}_pmc_{cfg_name}.json")
        if os.path.exists(cand):
            path = cand
            break
    if path is None:
        return None, "none: no committed PMC pass for this configuration"
    rel = os.path.relpath(path, ROOT)
    try:
        m = json.load(open(path))
        if m.get("source_id") != source_id():
            return None, f"none: {rel} was measured on other kernel sources (stamp {m.get('source_id')}, this build {source_id()})"
        if int(m.get("pairs_per_gpu", -1)) != pairs_per_gpu:
            return None, f"none: {rel} was measured on {m.get('pairs_per_gpu')} pairs per GPU"
        return ((2.0 * float(m["FETCH_SIZE_KiB"]) + float(m["WRITE_SIZE_KiB"])) * 1024.0,
                f"committed rocprofv3 PMC passes of this command ({rel}: 2 x FETCH_SIZE + WRITE_SIZE, stamped with the hash of the kernel "
                f"sources = this build's {source_id()}); NOT measured inside this run (counters cannot be read from inside the process)")
    except Exception as e:
        return None, f"none: {rel} unreadable ({str(e)[:80]})"


def model_rel(a, b):
    """relative Frobenius distance of two homogeneous 3x3 models UP TO SIGN: (distance, sign_flipped).  F and H are defined up to
    scale; the sign of the returned vector is the sign LAPACK's dsyev gives the eigenvector, which differs between LAPACK builds on
    about one input in 7000 (profiles/r5_cpu_port_vs_ref.log: reference on MKL vs reference on OpenBLAS) — same model, same mask."""
    a = np.asarray(a, float).ravel(); b = np.asarray(b, float).ravel()
    na, nb = np.linalg.norm(a), np.linalg.norm(b)
    if na == 0 or nb == 0:
        return (0.0 if na == nb else 1.0), False
    d_same, d_flip = np.linalg.norm(a / na - b / nb), np.linalg.norm(a / na + b / nb)
    return (d_flip, True) if d_flip < d_same else (d_same, False)


SIGN_FLIPS = []        # (pair id, against what): models equal up to sign only — listed in the line, never fatal


def parity_check(which, cfg_pairs, n_check, lo, models, masks, stats):
    """After the timed region: `n_check` pairs of the timed batch (spread over it) against the CPU oracle — masks and
    counters bit-exact, model within 1e-6 relative Frobenius.  Raises on any mismatch; returns the number checked."""
    from oracle import port
    from pydegensac_amd import parallel
    port.lib()
    P = models.shape[0]
    pick = set(int(x) for x in np.linspace(0, P - 1, n_check))
    # pairs that were set aside and resumed (stats word 15, bit 8) must be among the checked ones: at least four, spread over the batch
    aside = np.flatnonzero((stats[:, 15] >> 8) & 1)
    n_aside_checked = 0
    if len(aside):
        extra = [int(aside[i]) for i in np.linspace(0, len(aside) - 1, min(4, len(aside))).astype(int)]
        pick.update(extra)
    pick = sorted(pick)
    n_aside_checked = int(sum(int((stats[p, 15] >> 8) & 1) for p in pick))
    for p in pick:
        p1, p2 = make_pair(lo + p)
        Mo, mo, so = cpu_call(port, p1, p2, parallel.pair_seed(lo + p))
        st = stats[p]
        if (int(st[0]), int(st[1])) != (so["samples"], so["lo_runs"]):
            raise SystemExit(f"parity check failed: pair {lo + p} counters {int(st[0])},{int(st[1])} vs oracle {so['samples']},{so['lo_runs']}")
        if not np.array_equal(masks[p].astype(bool), mo):
            raise SystemExit(f"parity check failed: pair {lo + p} mask differs in {(masks[p].astype(bool) != mo).sum()} bits")
        d_, flipped = model_rel(models[p], Mo)
        if d_ > 1e-6:
            raise SystemExit(f"parity check failed: pair {lo + p} model differs (relative Frobenius distance {d_:.3g})")
        if flipped:
            SIGN_FLIPS.append([int(lo + p), "restatement"])
    return len(pick), n_aside_checked


def parity_against_cpu_leg(records, lo, models, masks, stats):
    """Every pair the all-cores CPU leg ran through the UNMODIFIED reference (oracle/_ref) against the same pair of the timed GPU
    batch: sample / LO / scored-model counters and inlier count equal, mask bit for bit, model within 1e-6 relative Frobenius
    (north_star's tolerance).  Any mismatch ends the bench (SystemExit).  Returns (pairs checked, of them set-aside pairs)."""
    P = models.shape[0]; n_ok = 0; n_aside = 0; soft = []
    for pid, samples, lo_runs, I, n_models, mbits, M in records:
        p = pid - lo
        if p < 0 or p >= P:
            continue
        st = stats[p]
        if (int(st[0]), int(st[1]), int(st[3])) != (samples, lo_runs, I):
            raise SystemExit(f"parity check failed (reference leg): pair {pid} counters {[int(x) for x in st[:5]]} vs reference {(samples, lo_runs, I, n_models)}")
        if int(st[4]) != n_models:
            # the reference's OWN count of scoring passes is not stable: four consecutive calls of oracle/_ref on C3 pair 463 in one process
            # gave 138 / 140 / 138 / 138, a fresh process 131, the restatement and the kernel 130 — with identical samples, LO runs,
            # inlier count, mask and model every time.  So this counter is compared and listed, not fatal; mask and model below are.
            soft.append((pid, int(st[4]), n_models))
        na, nb = np.linalg.norm(models[p]), np.linalg.norm(M)
        if nb == 0 or not np.isfinite(M).all():
            if na != 0:
                raise SystemExit(f"parity check failed (reference leg): pair {pid}: the reference found no model")
        else:
            mo = np.unpackbits(mbits)[:masks.shape[1]].astype(bool)
            if not np.array_equal(masks[p].astype(bool), mo):
                raise SystemExit(f"parity check failed (reference leg): pair {pid} mask differs in {(masks[p].astype(bool) != mo).sum()} bits")
            d_, flipped = model_rel(models[p], M)
            if na == 0 or d_ > 1e-6:
                raise SystemExit(f"parity check failed (reference leg): pair {pid} model differs (relative Frobenius distance {d_:.3g})")
            if flipped:
                SIGN_FLIPS.append([int(pid), "reference"])
        n_ok += 1; n_aside += int((st[15] >> 8) & 1)
    return n_ok, n_aside, soft


def models_by_arithmetic(screen, models, ex_passes):
    """What share of this rank's counted models (MI_ST_MODELS, the reference-equivalent count behind `achieved`) ran which arithmetic
    over all N points: from the kernel's own counters (mi_degensac_diag.d_screen) of the main loop's scoring phase."""
    if screen is None:
        return None
    l1, l2, exact, allm = (int(x) for x in screen)
    if allm <= 0:
        return None
    return {"main_loop_models": allm, "entered_level1_fp32_screen": l1, "entered_level2_fp64_screen": l2, "exact_metric_in_main_loop": exact,
            "exact_metric_in_events_at_least": models - (allm if allm < models else models),
            "share_exact_in_main_loop": exact / allm, "share_stopped_at_level1": (l1 - l2) / allm if l1 else 0.0,
            "share_stopped_at_level2": (l2 - exact) / allm if l2 else 0.0,
            "note": "every counted model costs the reference one pass of 32 B x N; here a main-loop model whose inlier bound cannot beat the best "
                    "score stops at a division-free screen over all N points (level 1: fp32, two points per instruction; level 2: fp64) and only "
                    "the survivors run the exact metric in the reference's operation order; main_loop_models includes samples speculated past the "
                    "final budget, which MI_ST_MODELS does not count"}


def single_call_ms(reps=7):
    """wall time of ONE call through the host-pointer API (pageable numpy arrays in, numpy out: staging over PCIe, one
    pair on one CU, sync): the reference's own use case.  Median over `reps` seeds after one warm-up call, with the library's own
    account of where each call's time went (mi_degensac_last_call_timing: host clocks + HIP events on the context's stream)."""
    import pydegensac_amd as pd
    from pydegensac_amd import _lib
    p1, p2 = make_pair(0)
    ts = []; parts = []
    prev = _lib.set_call_timing(1)
    try:
        for r in range(reps + 1):
            t = time.perf_counter()
            if CFG["which"] == "F":
                pd.findFundamentalMatrix_(p1, p2, PRM["px_th"], PRM["conf"], PRM["max_iters"], PRM["error_type"], PRM["sym"], PRM["laf"], PRM["degen"], seed=r + 1)
            else:
                pd.findHomography_(p1, p2, PRM["px_th"], PRM["conf"], PRM["max_iters"], PRM["error_type"], PRM["sym"], PRM["laf"], seed=r + 1)
            ts.append((time.perf_counter() - t) * 1e3)
            tm = _lib.last_call_timing(); tm["python_ms"] = ts[-1] - tm["call_ms"]
            tm["host_overhead_ms"] = ts[-1] - tm["dev_kernel_ms"]
            parts.append(tm)
    finally:
        _lib.set_call_timing(prev)
    med = {k: float(np.median([q[k] for q in parts[1:]])) for k in parts[0]}
    return {"median": float(np.median(ts[1:])), "min": float(min(ts[1:])), "max": float(max(ts[1:])),
            "breakdown": dict(med, note="medians over the same calls (seeds 2.. of one pair): call_ms = the C entry point, of it pack / enqueue (H2D, scratch "
                                        "set-up, launch, D2H) / wait (stream sync) / unpack on the host clock; dev_* = HIP events on the call's stream "
                                        "(dev_kernel_ms = header memsets + the kernel); python_ms = wall - call_ms (ctypes + numpy marshalling); "
                                        "host_overhead_ms = wall - dev_kernel_ms"),
            "note": "host-pointer API, PCIe staging included, 1 pair = 1 workgroup; never used as `value`"}


DUMP_CAP_BYTES = 64 << 20
DUMP_STATS_WORDS = 12            # MI_ST_SAMPLES .. MI_ST_AUX_PASSES; words 12-15 are device-clock ticks and the kernel variant


def dump_outputs(out_dir, models, masks, stats, cap=DUMP_CAP_BYTES):
    """--dump-outputs: what the timed path returned in its last step, as .npy files in float64 / float32, at most `cap` bytes
    in all, so that two builds can be compared output for output (same arguments = same inputs and seeds):
      models.npy   [k, 9] float64  the returned model of each pair (homogeneous, sign as returned)
      masks.npy    [k, n] float32  the inlier mask (0 / 1)
      stats.npy    [k, 12] float64 the per-pair counters MI_ST_SAMPLES .. MI_ST_AUX_PASSES (include/mi_degensac.h); the
                                   device-clock and kernel-variant words vary from run to run and are left out
      pair_ids.npy [k] float64     the global pair id of each row
    k = every pair when they fit, else a fixed sample (seed 0) of pairs in ascending order.  Returns k."""
    models = np.asarray(models, dtype=np.float64).reshape(-1, 9)
    masks = np.asarray(masks)
    P = models.shape[0]
    masks = masks.reshape(P, -1)
    stats = np.asarray(stats).reshape(P, -1)[:, :DUMP_STATS_WORDS]
    per_pair = 8 * 9 + 4 * masks.shape[1] + 8 * DUMP_STATS_WORDS + 8
    fit = max(1, (cap - 4 * 4096) // per_pair)                  # room for the four .npy headers
    ids = np.arange(P) if P <= fit else np.sort(np.random.default_rng(0).choice(P, size=fit, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "models.npy"), models[ids])
    np.save(os.path.join(out_dir, "masks.npy"), masks[ids].astype(np.float32))
    np.save(os.path.join(out_dir, "stats.npy"), stats[ids].astype(np.float64))
    np.save(os.path.join(out_dir, "pair_ids.npy"), ids.astype(np.float64))
    return len(ids)


def measure(pairs_per_gpu, steps, warmup, parity_pairs, world, rank, local_rank, dev, always_collective=False):
    """K timed steps of the hot path for the CURRENT config (set_config) on this rank's shard of `pairs_per_gpu * world`
    pairs.  Returns a dict of raw results (rank-local stats, gathered stats, times); the caller formats the JSON line."""
    import torch
    import torch.distributed as dist
    from pydegensac_amd import parallel, _lib
    P = pairs_per_gpu
    total_pairs = P * world
    lo, hi = parallel.shard_range(total_pairs, rank, world)
    # synthetic inputs of this rank's pairs (data seed = global pair id), staged to HBM once
    DIM = CFG["dim"]; homography = CFG["which"] == "H"
    a = np.empty((P * N_CORR, DIM)); b = np.empty((P * N_CORR, DIM))
    for i, pid in enumerate(range(lo, hi)):
        p1, p2 = make_pair(pid)
        a[i * N_CORR:(i + 1) * N_CORR] = p1; b[i * N_CORR:(i + 1) * N_CORR] = p2
    offs = np.arange(P + 1, dtype=np.int64) * N_CORR
    d_a = torch.from_numpy(a).to(dev); d_b = torch.from_numpy(b).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    d_seeds = torch.from_numpy(parallel.pair_seeds(lo, hi).astype(np.int64)).to(dev).to(torch.int32)  # bit pattern of uint32 < 2^31
    d_F = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    d_mask = torch.zeros(P * N_CORR, dtype=torch.uint8, device=dev)
    d_st = torch.zeros((P, 16), dtype=torch.int32, device=dev)
    prm = _lib.make_params(PRM["px_th"], PRM["conf"], PRM["max_iters"], PRM["error_type"], PRM["sym"], PRM["laf"], PRM["degen"])
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev)
    entry = L.mi_degensac_find_homography_batch_dev_ex if homography else L.mi_degensac_find_fundamental_batch_dev_ex
    # main-loop models by the arithmetic they got (mi_degensac_diag.d_screen; fundamental matrix only): feeds roofline.models_by_arithmetic
    d_scr = torch.zeros((P, 4), dtype=torch.int32, device=dev)
    diag = _lib.Diag(None, 0, 0, None, None if homography else d_scr.data_ptr())

    def step(timed_events=None):
        if timed_events:
            timed_events[0].record(stream)
        rc = entry(d_a.data_ptr(), d_b.data_ptr(), d_off.data_ptr(),
                   offs.ctypes.data_as(C.POINTER(C.c_int64)), P, DIM, C.byref(prm),
                   d_seeds.data_ptr(), local_rank, C.c_void_p(stream.cuda_stream),
                   d_F.data_ptr(), d_mask.data_ptr(), d_st.data_ptr(), C.byref(diag))
        _lib.check(rc)
        if timed_events:
            timed_events[1].record(stream)
        return parallel.gather_results(d_F, d_st, d_mask, N_CORR, total_pairs, always_collective=always_collective)

    def barrier():
        if world > 1 or (always_collective and dist.is_initialized()):
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(warmup):
        step()
    barrier()
    kernel_ms = []
    t0 = time.perf_counter()
    for _ in range(steps):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        g = step(e); kernel_ms.append(e)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t.item())
    gm, gs, gmask = g
    st = gs.cpu().numpy()
    kms = float(np.mean([a_.elapsed_time(b_) for a_, b_ in kernel_ms]))       # this rank's kernel, HIP events on its stream
    local_st = d_st.cpu().numpy()
    local_models = int(local_st[:, 4].sum())
    alg_bytes = local_models * 32.0 * N_CORR                                   # 32*N bytes per model scored
    # spot check of THIS rank's timed batch against the CPU oracle (outside the timed region)
    n_checked = 0; n_aside_checked = 0
    if parity_pairs > 0:
        n_checked, n_aside_checked = parity_check(CFG["which"], P, parity_pairs, lo, d_F.cpu().numpy().reshape(P, 9),
                                                  d_mask.cpu().numpy().reshape(P, N_CORR), local_st)
    return dict(dt=dt, st=st, local_st=local_st, kms=kms, alg_bytes=alg_bytes, gmask=gmask, gm=gm, total_pairs=total_pairs, P=P, lo=lo,
                screen=None if homography else d_scr.cpu().numpy().astype(np.int64).sum(0),
                host_models=d_F.cpu().numpy().reshape(P, 9), host_masks=d_mask.cpu().numpy().reshape(P, N_CORR),
                n_checked=n_checked, n_aside_checked=n_aside_checked, homography=homography,
                kernel=L.mi_degensac_kernel_name(int(homography)).decode())


def secondary_line(name, pairs, steps, warmup, parity_pairs, cpu_budget_s, dev):
    """One of the other BASELINE configs, measured the same way on one GPU and reduced to a few numbers (driver-visible: the
    `secondary` object of the bench line).  An ordinary failure (e.g. out of memory) is reported in place of the numbers; a
    parity mismatch (SystemExit from parity_check) is NOT swallowed: it ends the bench with a non-zero exit code."""
    old = [k for k, v in CONFIGS.items() if v is CFG][0]
    try:
        set_config(name)
        r = measure(pairs, steps, warmup, parity_pairs, 1, 0, dev.index or 0, dev)
        models = int(r["st"][:, 4].sum())
        ach = r["alg_bytes"] / (r["kms"] * 1e-3) / 1e9
        out = {"workload": f"{name.upper()} x {pairs}", "ms_per_step": r["dt"] / steps * 1e3, "kernel_ms": r["kms"], "kernel": r["kernel"],
               "models_per_s": models * steps / r["dt"], "pairs_per_s": pairs * steps / r["dt"], "models_per_pair": models / pairs,
               "samples_per_pair": float(r["st"][:, 0].mean()), "threads": int(r["local_st"][0, 14]), "placement": int(r["local_st"][0, 15]) & 255,
               "roofline_frac": ach / HBM_PEAK_GBS, "achieved_GBs": ach, "parity_checked": r["n_checked"]}
        if name == "c3":
            out["single_call_ms"] = single_call_ms(reps=5)          # one C3 pair through the host-pointer API (the reference: ~10.5 ms on one core)
        if cpu_budget_s > 0:
            cb = cpu_baseline(budget_s=cpu_budget_s, max_pairs=max(2, min(pairs, 256)), skip_first=pairs > 1)
            out["cpu_baseline"] = cb
            out["gpu_over_cpu"] = out["models_per_s"] / cb["value"] if cb.get("value") else None
        return out
    except Exception as e:        # a failed parity check is a SystemExit and ends the bench; so does KeyboardInterrupt
        return {"workload": name, "error": str(e)[:300]}
    finally:
        set_config(old)


def h2el_line(pairs=64, n=5000, reps=3, n_check=8):
    """SURVEY 8f #4's last driver, ransacH2el (ranH2el.c:19), on `pairs` synthetic ellipse-correspondence sets through the
    host-pointer API (PCIe staging included); `n_check` pairs spread over the batch are checked against the CPU oracle
    (a mismatch ends the bench)."""
    try:
        import pydegensac_amd as pd
        from pydegensac_amd import synthetic as syn
        U = [syn.ellipse_pairs(n, 0.4, 1.0, 500 + i, 0.05)[0] for i in range(pairs)]
        seeds = list(range(1, pairs + 1))
        pd.ransacH2el_batch(U, 4.0, 0.99, 10000, True, 0, seeds=seeds)
        best = 1e9
        for _ in range(reps):
            t = time.perf_counter(); H, m = pd.ransacH2el_batch(U, 4.0, 0.99, 10000, True, 0, seeds=seeds); best = min(best, time.perf_counter() - t)
        st = pd.last_stats()
        from oracle import port
        pick = sorted(set(int(x) for x in np.linspace(0, pairs - 1, n_check)))
        for q in pick:
            Ho, mo, so = port.ransacH2el(U[q], 4.0, 0.99, 10000, True, 0, seeds[q])
            if (st[q]["samples"], st[q]["lo_runs"], st[q]["I"]) != (so["samples"], so["lo_runs"], so["I"]) or not np.array_equal(np.asarray(m[q]), mo):
                raise SystemExit(f"parity check failed: ransacH2el pair {q} differs from the oracle")
        return {"workload": f"ransacH2el x {pairs}, {n} ellipse correspondences (40 % inliers), host-pointer API", "ms_per_call": best * 1e3,
                "pairs_per_s": pairs / best, "samples_per_pair": float(np.mean([s_["samples"] for s_ in st])), "parity_checked": len(pick)}
    except Exception as e:
        return {"workload": "ransacH2el", "error": str(e)[:300]}


def relaunch_argv(n_gpus, argv, port=None):
    """The command line `bench.py --gpus N` (N > 1, no launcher in the environment) re-executes itself with: one rank per GPU
    under torch.distributed.run on 127.0.0.1 (the container's hostname may not resolve), the driver's own launch form."""
    if port is None:
        import socket
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={int(n_gpus)}",
            "--master-addr", "127.0.0.1", "--master-port", str(int(port)), os.path.abspath(__file__)] + list(argv)


def visible_gpus():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def resolve_world(gpus, single_process, env, n_visible):
    """What `--gpus N` means in this environment (pure function: tests/test_host_cpu.py).  Returns ("run", world) to measure in this
    process, ("exec", N) to re-execute under torch.distributed.run; raises SystemExit with a message for every inconsistent case — a
    request for N GPUs never silently becomes a one-GPU run labelled n_gpus 1."""
    if gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    launched = "WORLD_SIZE" in env
    world = int(env.get("WORLD_SIZE", "1"))
    if launched:
        if single_process:
            raise SystemExit("bench.py: --single-process drives all GPUs from ONE process; do not start it under torch.distributed.run")
        if world != gpus:
            raise SystemExit(f"bench.py: --gpus {gpus} but the launcher started WORLD_SIZE={world} ranks; the two must agree")
        if int(env.get("LOCAL_RANK", "0")) >= n_visible:
            raise SystemExit(f"bench.py: LOCAL_RANK {env.get('LOCAL_RANK')} but only {n_visible} GPU(s) are visible on this node")
        return "run", world
    if n_visible < gpus:
        raise SystemExit(f"bench.py: --gpus {gpus} requested but only {n_visible} GPU(s) are visible on this node; refusing to print a "
                         f"{n_visible}-GPU measurement under an n_gpus={gpus} request")
    if gpus > 1 and not single_process:
        return "exec", gpus
    return "run", 1


def measure_single_process(n_dev, pairs_per_gpu, steps, warmup, parity_pairs):
    """--single-process: ONE process drives `n_dev` GPUs through the C-ABI's device-list mode (mi_degensac_find_*_batch_multi: one host
    thread per device, contiguous blocks of pairs, NO collective; SURVEY 8e "no collective at all in single-process multi-device
    mode (host gathers D2H)").  The boundary takes HOST buffers here, so PCIe staging of inputs and results is inside the timed
    region — the line says so, and this mode is never the default."""
    from pydegensac_amd import parallel, _lib
    P = pairs_per_gpu * n_dev
    DIM = CFG["dim"]; homography = CFG["which"] == "H"
    a = np.empty((P * N_CORR, DIM)); b = np.empty((P * N_CORR, DIM))
    for pid in range(P):
        p1, p2 = make_pair(pid)
        a[pid * N_CORR:(pid + 1) * N_CORR] = p1; b[pid * N_CORR:(pid + 1) * N_CORR] = p2
    offs = np.arange(P + 1, dtype=np.int64) * N_CORR
    seeds = parallel.pair_seeds(0, P)
    M = np.zeros((P, 9)); mask = np.zeros(P * N_CORR, np.uint8); st = np.zeros((P, 16), np.int32)
    devs = (C.c_int32 * n_dev)(*range(n_dev))
    prm = _lib.make_params(PRM["px_th"], PRM["conf"], PRM["max_iters"], PRM["error_type"], PRM["sym"], PRM["laf"], PRM["degen"])
    L = _lib.lib()
    fn = L.mi_degensac_find_homography_batch_multi if homography else L.mi_degensac_find_fundamental_batch_multi

    def step():
        _lib.check(fn(_lib.dptr(a), _lib.dptr(b), offs.ctypes.data_as(C.POINTER(C.c_int64)), P, DIM, C.byref(prm),
                      seeds.ctypes.data_as(C.POINTER(C.c_uint32)), devs, n_dev, _lib.dptr(M), mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                      st.ctypes.data_as(C.POINTER(C.c_int32))))
    for _ in range(warmup):
        step()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    dt = time.perf_counter() - t0
    n_checked = n_aside = 0
    if parity_pairs > 0:
        n_checked, n_aside = parity_check(CFG["which"], P, parity_pairs, 0, M, mask.reshape(P, N_CORR), st)
    return dict(dt=dt, st=st, P=P, n_checked=n_checked, n_aside_checked=n_aside, masks=mask.reshape(P, N_CORR), models=M)


def single_process_line(args, n_dev):
    r = measure_single_process(n_dev, args.pairs_per_gpu, args.steps, args.warmup, args.parity_pairs)
    st, dt = r["st"], r["dt"]
    models_step = int(st[:, 4].sum())
    dumped = dump_outputs(args.dump_outputs, r["models"], r["masks"], st) if args.dump_outputs else None
    line = {"metric": "models/sec, findFundamentalMatrix @2000 corrs (LO-RANSAC + DEGENSAC, batched pairs)" if args.config == "c2" else f"models/sec, config {args.config}",
            "value": models_step * args.steps / dt, "unit": "models/s", "n_gpus": n_dev, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{args.config.upper()} x {args.pairs_per_gpu} pairs per GPU, {N_CORR} correspondences", "pairs_total": r["P"],
                       "pairs_per_gpu": args.pairs_per_gpu, "n_corr": N_CORR,
                       "parallelism": f"ONE process, device list [0..{n_dev - 1}] through mi_degensac_find_*_batch_multi (one host thread per device), no collective",
                       "collective": "none (the host gathers D2H)", "process_group": None,
                       "inputs": "HOST buffers: PCIe staging of inputs and results is INSIDE the timed region (the default multi-rank mode keeps inputs resident in HBM)"},
            "pairs_per_s": r["P"] * args.steps / dt, "models_per_pair": models_step / r["P"], "mean_inliers": float(r["masks"].sum(1).mean()),
            "roofline": None, "cpu_baseline": None,
            "parity_checked": r["n_checked"], "parity_checked_set_aside": r["n_aside_checked"], "sign_flips": SIGN_FLIPS[:8],
            "devices_used": sorted(set(int(x) for x in range(n_dev)))}
    if dumped is not None:
        line["outputs_dumped"] = {"dir": args.dump_outputs, "pairs": dumped}
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2")
    ap.add_argument("--pairs-per-gpu", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the short C2 x 512 / C3 / C5 measurements of the `secondary` object")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: the parity check of the timed batch (--parity-pairs), the CPU baselines with "
                         "their parity check, single_call_ms, the `secondary` configurations and, with N > 1 ranks, the literal C4 batch")
    ap.add_argument("--parity-pairs", type=int, default=None,
                    help="pairs of the timed batch checked against the oracle afterwards (default: 16 with --full, 0 without)")
    ap.add_argument("--dump-results", default="", help="rank 0 writes the gathered per-pair results of the last timed step to this .npz (tests)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="rank 0 writes what the last timed step returned as DIR/*.npy in float64 / float32, at most 64 MB (see dump_outputs)")
    ap.add_argument("--single-process", action="store_true",
                    help="drive the N GPUs from ONE process through the device-list entry points (*_batch_multi, no collective, host buffers)")
    ap.add_argument("--c4-single-process", action="store_true",
                    help="with N > 1 ranks and --full: rank 0 also measures the literal C4 batch through ONE process over the same N GPUs (secondary.c4_literal_single_process) "
                         "while the other ranks wait at a barrier; off by default: it opens every GPU from rank 0 next to the ranks' own processes, and the N-rank "
                         "line must not depend on it")
    ap.add_argument("--dist-always", action="store_true",
                    help="initialise the RCCL process group and run the result all-gather even with one rank (tests the N > 1 code path on one GPU)")
    args = ap.parse_args()
    if args.parity_pairs is None:
        args.parity_pairs = 16 if args.full else 0
    set_config(args.config)
    if args.pairs_per_gpu <= 0:
        args.pairs_per_gpu = PAIRS_PER_GPU

    import torch
    import torch.distributed as dist

    # --gpus N is a REQUEST for N GPUs: N ranks from a launcher (WORLD_SIZE must agree), or this process starts them itself
    action, world = resolve_world(args.gpus, args.single_process, os.environ, visible_gpus())
    if action == "exec":
        cmd = relaunch_argv(args.gpus, sys.argv[1:])
        print("bench.py: --gpus %d without a launcher: running  %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
        env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # a child process, not an exec: counting the devices above has already initialised the GPU runtime in this one
        sys.exit(subprocess.call(cmd, env=env))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    if args.single_process:
        print(json.dumps(single_process_line(args, args.gpus)))
        return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or (args.dist_always and "MASTER_ADDR" in os.environ)
    if use_dist:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    P = args.pairs_per_gpu
    r = measure(P, args.steps, args.warmup, args.parity_pairs, world, rank, local_rank, dev, always_collective=use_dist)
    dt, st, local_st, kms, alg_bytes, gmask, total_pairs = r["dt"], r["st"], r["local_st"], r["kms"], r["alg_bytes"], r["gmask"], r["total_pairs"]
    homography = r["homography"]
    models_step = int(st[:, 4].sum()); samples_step = int(st[:, 0].sum())
    achieved = alg_bytes / (kms * 1e-3) / 1e9
    # C4 as BASELINE.json words it: ONE batch of 4096 pairs over the N GPUs (strong scaling, 4096 / N pairs per GPU), measured
    # by every rank next to the weak-scaling headline (4096 pairs PER GPU); at N = 1 it IS the headline
    c4 = None
    if args.full and args.config == "c2" and world > 1 and not args.no_secondary and 4096 % world == 0:
        r4 = measure(4096 // world, 3, 1, 4, world, rank, local_rank, dev, always_collective=use_dist)
        m4 = int(r4["st"][:, 4].sum())
        c4 = {"workload": f"C4 literal: 4096 C2 pairs over {world} GPUs = {4096 // world} per GPU (strong scaling)", "n_gpus": world,
              "pairs_per_gpu": 4096 // world, "ms_per_step": r4["dt"] / 3 * 1e3, "kernel_ms_rank0": r4["kms"], "models_per_s": m4 * 3 / r4["dt"],
              "pairs_per_s": 4096 * 3 / r4["dt"], "parity_checked_rank0": r4["n_checked"]}

    # ... and the same literal C4 batch driven from ONE process over the same N GPUs (device-list mode, no collective): rank 0 measures
    # it while the other ranks wait at a barrier with their GPUs idle
    sp = None
    if c4 is not None and args.c4_single_process:
        dist.barrier()
        if rank == 0:
            try:
                r1 = measure_single_process(world, 4096 // world, 3, 1, 4)
                sp = {"workload": f"C4 literal through ONE process: mi_degensac_find_fundamental_batch_multi, devices [0..{world - 1}], host buffers (PCIe staging timed), no collective",
                      "n_gpus": world, "pairs_per_gpu": 4096 // world, "ms_per_step": r1["dt"] / 3 * 1e3, "models_per_s": int(r1["st"][:, 4].sum()) * 3 / r1["dt"],
                      "pairs_per_s": 4096 * 3 / r1["dt"], "parity_checked": r1["n_checked"]}
            except BaseException as e:    # reported, never fatal here: the other ranks wait at the barrier below (the headline's own parity checks above are fatal)
                sp = {"workload": "C4 literal through one process", "error": f"{type(e).__name__}: {str(e)[:300]}"}
        dist.barrier()

    if rank == 0 and args.dump_results:
        np.savez(args.dump_results, models=r["gm"].cpu().numpy(), stats=st, masks=gmask.cpu().numpy())
    dumped = None
    if rank == 0 and args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, r["gm"].cpu().numpy(), gmask.cpu().numpy(), st)
    if rank == 0:
        inl = gmask.sum(dim=1).cpu().numpy()
        ticks = st[:, 13].astype(np.float64) / 100e6                           # 100 MHz device wall clock
        tbest = st[:, 12].astype(np.float64) / 100e6
        wl = {"c2": (f"C2 x {P} pairs per GPU (C4 is a batch of 4096 such pairs): findFundamentalMatrix, "
                     f"{N_CORR} correspondences, 40% inliers, sigma 0.1 px, px_th 0.5, conf 0.9999, max_iters 100000, "
                     "sampson error, symmetric check on, degeneracy check on"),
              "c3": (f"C3 x {P} pairs per GPU: findHomography, {N_CORR} correspondences with LAFs, 40% inliers, sigma 0.5 px, "
                     "px_th 2, conf 0.999, max_iters 50000, sampson error, laf_consistensy_coef 3, symmetric check on, LO on"),
              "c5": (f"C5 x {P} pairs per GPU: findFundamentalMatrix, {N_CORR} correspondences, 10% inliers, sigma 0.1 px, px_th 0.5, "
                     "conf 0.9999, max_iters 200000, sampson error, symmetric check on, degeneracy check on")}[args.config]
        traffic, traffic_src = pmc_traffic(args.config, P)
        out = {
            "metric": ("models/sec, findFundamentalMatrix @2000 corrs (LO-RANSAC + DEGENSAC, batched pairs)" if args.config == "c2" else
                       "models/sec, findHomography @5000 corrs with LAFs (LO-RANSAC, LAF + symmetric checks, batched pairs)" if homography else
                       "models/sec, findFundamentalMatrix @50000 corrs (LO-RANSAC + DEGENSAC)"),
            "value": models_step * args.steps / dt,
            "unit": "models/s",
            "n_gpus": (dist.get_world_size() if use_dist else 1), "steps": args.steps, "warmup": args.warmup,   # the ranks the process group (RCCL) actually has
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": wl,
                       "pairs_total": total_pairs, "pairs_per_gpu": P, "n_corr": N_CORR,
                       "parallelism": f"pair-sharded x{world}, RCCL all-gather of per-pair results",
                       "collective": "nccl (RCCL) all_gather_into_tensor" if use_dist else "none (one rank)",
                       "process_group": ({"backend": dist.get_backend(), "world_size": dist.get_world_size()} if use_dist else None)},
            "samples_per_s": samples_step * args.steps / dt,
            "pairs_per_s": total_pairs * args.steps / dt,
            "models_per_pair": models_step / total_pairs,
            "mean_inliers": float(inl.mean()),
            "time_to_best_ms": {"mean": float(tbest.mean() * 1e3), "p50": float(np.median(tbest) * 1e3), "max": float(tbest.max() * 1e3),
                                "note": "from a pair's start to the commit of its returned model, on the device clock, while the pair is being worked on (the time a pair waits in the set-aside queues of a batch is not counted)"},
            "pair_latency_ms": {"mean": float(ticks.mean() * 1e3), "p50": float(np.median(ticks) * 1e3), "max": float(ticks.max() * 1e3),
                                "note": "device clock, time the pair was being worked on; the time a pair waits in the set-aside queues of a batch is excluded (as in time_to_best_ms)"},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "hbm_frac": (traffic / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                         "hbm_frac_note": "measured HBM bytes per launch (traffic) / kernel time / peak: the share of the HBM bandwidth the kernel "
                                          "really uses; `frac` above is the reference-equivalent (algorithmic) rate, not bandwidth use",
                         "kernel": r["kernel"], "kernel_ms": kms,
                         "models_by_arithmetic": models_by_arithmetic(r.get("screen"), int(local_st[:, 4].sum()), int(local_st[:, 9].sum())),
                         "algorithmic_bytes_per_launch": alg_bytes,
                         "note": "achieved = algorithmic bytes (models scored x 32 B x N, SURVEY 8d) / kernel time; the point set is "
                                 "LDS/L2-resident, so `traffic` (HBM bytes per launch from the committed PMC passes, profiles/) is far "
                                 "below it: inputs once, then model tables, lists and scratch"},
            "parity_checked": r["n_checked"], "parity_checked_set_aside": r["n_aside_checked"],
            "kernel_variant": {"threads": int(local_st[0, 14]), "placement": int(local_st[0, 15]) & 255},
            "pairs_set_aside": int(((local_st[:, 15] >> 8) & 1).sum()),
            "pairs_streamed": int(((local_st[:, 15] >> 9) & 1).sum()),   # pairs whose sample stream / solves / scoring moved to a producer workgroup (stream mode)        # pairs written back after the discovery round and resumed by priority
        }
        if dumped is not None:
            out["outputs_dumped"] = {"dir": args.dump_outputs, "pairs": dumped}
        if args.full and world == 1:
            out["single_call_ms"] = single_call_ms()
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cb = cpu_baseline()
            out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
            if "time_to_best_ms" in cb and cb["pair_ids"][1] < P:
                # the GPU figure on exactly the pairs the CPU leg ran (device clock, inside the timed 4096-pair batch)
                a_, b_ = cb["pair_ids"]; g_ = tbest[a_:b_ + 1] * 1e3
                cb["time_to_best_ms"]["gpu_same_pairs"] = {"mean": float(g_.mean()), "p50": float(np.median(g_)), "max": float(g_.max())}
            allc = cpu_baseline_all_cores(args.config)
            if allc is not None:
                recs = allc.pop("_records", None)
                out["cpu_baseline_all_cores"] = allc
                if recs:
                    # the whole CPU leg doubles as the parity sample: every pair it ran, against the timed GPU batch
                    n_ref, n_ref_aside, soft = parity_against_cpu_leg(recs, r["lo"], r["host_models"], r["host_masks"], local_st)
                    out["parity_checked_vs_restatement"] = out["parity_checked"]
                    out["parity_checked"] = out["parity_checked"] + n_ref
                    out["parity_checked_set_aside"] = out["parity_checked_set_aside"] + n_ref_aside
                    out["parity_checked_vs_reference"] = {"pairs": n_ref, "set_aside": n_ref_aside,
                        "scored_model_count_differs": [list(x) for x in soft[:8]], "scored_model_count_differs_n": len(soft),
                        "what": "every pair of the all-cores CPU leg (the unmodified reference, oracle/_ref) against the same pair of the timed GPU "
                                "batch: samples, LO runs, inlier count equal, mask bit-exact, model <= 1e-6 relative Frobenius (any mismatch ends the "
                                "bench); the scored-model count is compared too and its differences are listed (pair, GPU, reference): the reference's own "
                                "count varies from call to call on some homography pairs (same mask, model and trajectory), see bench.py"}
        if args.full and world == 1 and not args.no_secondary and args.config == "c2":
            # the other BASELINE configurations, short runs inside the same driver-timed process (about a minute together)
            sec = {}
            if P != 512:
                sec["c2_512_pairs"] = secondary_line("c2", 512, 3, 1, 8, 0.0, dev)           # C4's own share of one GPU (8-GPU run of 4096 pairs)
            sec["c3"] = secondary_line("c3", 1024, 3, 1, 16, 0.0 if args.no_cpu_baseline else 4.0, dev)
            sec["c5"] = secondary_line("c5", 1, 2, 1, 1, 0.0 if args.no_cpu_baseline else 1.0, dev)
            sec["h2el"] = h2el_line()
            sec["c4_literal"] = {"workload": "C4 literal at 1 GPU = the headline (4096 pairs on this GPU); with --gpus N every rank also measures 4096 / N pairs per GPU",
                                 "n_gpus": 1, "pairs_per_gpu": P, "ms_per_step": out["ms_per_step"], "models_per_s": out["value"]} if P == 4096 else None
            out["secondary"] = sec
        if c4 is not None:
            out.setdefault("secondary", {})["c4_literal"] = c4
        if sp is not None:
            out.setdefault("secondary", {})["c4_literal_single_process"] = sp
        out["sign_flips"] = {"pairs": SIGN_FLIPS[:16], "n": len(SIGN_FLIPS),
                             "what": "pairs whose model equals the CPU side's only up to SIGN (same mask and counters): F and H are homogeneous, and the sign "
                                     "is the one LAPACK's dsyev gives the eigenvector, which differs between LAPACK builds on about one input in 7000; never fatal"}
        print(json.dumps(out))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
