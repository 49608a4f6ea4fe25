"""The uint8 L2 matcher (norm "l2_u8": int8 matrix cores, mi_matcher_u8.h) against the float32 L2 matcher on the same values.
Workload: K image pairs of 2000 x 2000 descriptors of dim 128 (64 distinct two-view pairs repeated to K); uint8 rows with byte-noisy
true matches, and their float32 casts.
  2-NN    knn_match_batch_tensors, one direction: HIP events around every call, after two warm-up calls
  M&V     match_and_verify_batch_tensors, model F (2-NN both ways is NOT asked for: mutual=False), wall time of the synchronised call
Every side runs in a child process of its own, so that the float32 baseline can come from another build of the library: with
--baseline-lib PATH (a libmi_degensac.so built from the parent commit) the float32 side of the comparison is that build; the float32
path of the build under test is always measured too.  Medians over --reps calls with [min..max]; the speed-up is median over median,
and "separated" says whether the slowest uint8 call was faster than the fastest float32 call.
usage: gpu_matcher_u8.py [K ...] [--reps R] [--baseline-lib PATH] [--log FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, DIM, BASE = 2000, 128, 64


def base_pairs():
    import numpy as np
    from pydegensac_amd import synthetic as syn
    rng = np.random.default_rng(0)
    K1, K2, D1, D2 = [], [], [], []
    for i in range(BASE):
        p1, p2, lab, _ = syn.two_view_fundamental(N, 0.5, 0.1, seed=500 + i)
        d1 = rng.integers(0, 256, (N, DIM), dtype=np.uint8)
        d2 = np.clip(d1.astype(np.int64) + rng.integers(-12, 13, d1.shape), 0, 255).astype(np.uint8)
        d2[~lab] = rng.integers(0, 256, (int((~lab).sum()), DIM), dtype=np.uint8)
        perm = rng.permutation(N)
        K1.append(p1); K2.append(p2[perm]); D1.append(d1); D2.append(d2[perm])
    return [np.stack(x) for x in (K1, K2, D1, D2)]


def child(side, Ks, reps):
    """one side's timings as JSON lines on stdout: {"side", "K", "knn2_ms": [...], "mv_ms": [...], "checksum"}"""
    import numpy as np
    import torch
    from pydegensac_amd import parallel, tensor_api
    dev = torch.device("cuda", 0)
    bk1, bk2, bd1, bd2 = [torch.from_numpy(x).to(dev) for x in base_pairs()]
    norm = "l2_u8" if side == "u8" else None
    if side != "u8":
        bd1 = bd1.float(); bd2 = bd2.float()
    for K in Ks:
        rep = [(p % BASE) for p in range(K)]
        k1 = bk1[rep].reshape(K * N, 2).contiguous(); k2 = bk2[rep].reshape(K * N, 2).contiguous()
        d1 = bd1[rep].reshape(K * N, DIM).contiguous(); d2 = bd2[rep].reshape(K * N, DIM).contiguous()
        c = [N] * K; seeds = parallel.pair_seeds(0, K)
        knn, mv = [], []
        for r in range(reps + 2):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            idx, dist = tensor_api.knn_match_batch_tensors(d1, d2, c, c, norm=norm)
            e1.record(); torch.cuda.synchronize()
            if r >= 2:
                knn.append(e0.elapsed_time(e1))
        checksum = [int(idx.to(torch.int64).sum().item()), float(dist.double().sum().item())]
        for r in range(reps + 1):
            t0 = time.perf_counter()
            tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, c, c, model="F", seeds=seeds, norm=norm)
            torch.cuda.synchronize()
            if r >= 1:
                mv.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"side": side, "K": K, "knn2_ms": knn, "mv_ms": mv, "checksum": checksum}), flush=True)
        del k1, k2, d1, d2, idx, dist
        torch.cuda.empty_cache()


def run_child(side, Ks, reps, lib):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--reps", str(reps)] + [str(k) for k in Ks]
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
    return {r["K"]: r for r in (json.loads(ln) for ln in out.splitlines() if ln.startswith("{"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("K", nargs="*", type=int, default=[64, 512, 2048])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.K, a.reps)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    u8 = run_child("u8", a.K, a.reps, None)
    f32 = run_child("f32", a.K, a.reps, None)
    base = run_child("f32", a.K, a.reps, a.baseline_lib) if a.baseline_lib else None
    say(f"# {N} x {N} x {DIM} descriptors per pair; uint8 rows under norm l2_u8 against the same values as float32 under L2; medians over "
        f"{a.reps} calls [min..max]")
    say("# float32 baseline: " + ("a build of the parent commit (--baseline-lib)" if base else "the build under test (no --baseline-lib given)"))
    ref = base or f32
    for what, key in (("batched 2-NN (HIP events)", "knn2_ms"), ("match_and_verify_batch_tensors F (wall)", "mv_ms")):
        say(f"## {what}")
        for K in a.K:
            u, f = u8[K][key], ref[K][key]
            same = u8[K]["checksum"] == ref[K]["checksum"]
            say(f"K={K:5d}  uint8 l2_u8 {fmt(u)}  float32 baseline {fmt(f)}" + (f"  float32 this build {fmt(f32[K][key])}" if base else "") +
                f"  speed-up {np.median(f) / np.median(u):6.2f}x  separated: {'yes' if max(u) < min(f) else 'NO'}"
                f"  idx / dist checksums equal: {'yes' if same else 'NO'}")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
