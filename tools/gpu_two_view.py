"""Match once, verify F and H (tensor_api.match_and_verify_fh_pairs_tensors) against what a caller had before: the two existing pair-list
calls, model F then model H, on the same stores, list and seeds.  Workload of tools/gpu_match_pairs.py: M = 65 images x 2000 keypoints x
dim 128 (synthetic.image_collection), matcher.exhaustive_pairs(65) = 2080 pairs, ratio 0.9, the estimators' default parameters.  Arms:
  f32          float32 under L2, mutual=False
  f32 mutual   float32 under L2, mutual=True
  l2_u8        the same descriptors as bytes under norm l2_u8
  f32 fginn    float32 with fginn_th=10 on the twinned collection of tools/gpu_fginn_pairs.py at 10 % needy queries
  time      the PARENT build (--baseline-lib: a libmi_degensac.so built from the parent commit, loaded through MI_DEGENSAC_LIB) and this
            build run in child processes of their own.  Per repetition the parent times its F call and its H call one after the other, each
            from the call to a synchronised stream (wall clock), and reports their sum; this build times the new call the same way, and its
            own two calls.  --reps calls after one warm-up of every form; medians with [min..max].
  memory    torch.cuda.max_memory_allocated of one new call and of the two existing calls in a row (this build).
  identity  this build: F / inlier_f of the new call equal the F call's, H / inlier_h the H call's, match either's.
usage: gpu_two_view.py [--images M] [--rows N] [--reps R] [--baseline-lib FILE] [--log FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

DIM = 128
ARMS = [("f32", dict(u8=False, mutual=False, fginn=None)), ("f32 mutual", dict(u8=False, mutual=True, fginn=None)),
        ("l2_u8", dict(u8=True, mutual=False, fginn=None)), ("f32 fginn", dict(u8=False, mutual=False, fginn=10.0))]


def stores(m, n, arm):
    """(keypoints [m n, 2] float64, descriptors [m n, DIM]) of an arm"""
    if arm["fginn"] is not None:
        import gpu_fginn_pairs
        desc, kps = gpu_fginn_pairs.collection(m, n, 0.1, arm["u8"])
        return kps, desc
    import gpu_match_pairs
    kps, descs = gpu_match_pairs.collection(m, n, arm["u8"])
    return np.concatenate(kps), np.concatenate(descs)


def child(a):
    """one process of one build: a JSON line per arm"""
    import torch
    from pydegensac_amd import matcher, parallel, tensor_api
    dev = torch.device("cuda", 0)
    M, N = a.images, a.rows
    pairs = matcher.exhaustive_pairs(M); K = len(pairs); counts = [N] * M
    seeds = parallel.pair_seeds(0, K)
    new = a.child == "this"

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter(); out = fn(); torch.cuda.current_stream(dev).synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def peak(fn):
        torch.cuda.synchronize(dev); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn(); torch.cuda.synchronize(dev)
        return torch.cuda.max_memory_allocated(dev), base
    for name, arm in ARMS:
        kps, desc = stores(M, N, arm)
        k = torch.from_numpy(kps).to(dev); d = torch.from_numpy(desc).to(dev)
        kw = dict(ratio=0.9, mutual=arm["mutual"], seeds=seeds, norm="l2_u8" if arm["u8"] else None)

        def old(model):
            if arm["fginn"] is None:
                return tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model=model, **kw)
            return tensor_api.match_and_verify_fginn_pairs_tensors(k, k, d, d, counts, counts, pairs, arm["fginn"], model=model, **kw)

        def fh():
            return tensor_api.match_and_verify_fh_pairs_tensors(k, k, d, d, counts, counts, pairs, fginn_th=arm["fginn"], **kw)
        out = {"arm": name}
        _, wf = timed(lambda: old("F")); _, wh = timed(lambda: old("H"))          # warm-up
        if new:
            _, g = timed(fh)
            out["same"] = bool(torch.equal(g[0], wf[0]) and torch.equal(g[1], wh[0]) and torch.equal(g[2], wf[1]) and torch.equal(g[2], wh[1])
                               and torch.equal(g[3], wf[2]) and torch.equal(g[4], wh[2]) and np.array_equal(g[8], wf[4]))
            s = g[7].cpu().numpy()
            out["summary_mean"] = [float(x) for x in s.mean(axis=0)]
            out["classes"] = [int(x) for x in np.bincount(matcher.two_view_config(s), minlength=3)]
            del g
        del wf, wh
        t_f, t_h, t_fh = [], [], []
        for _ in range(a.reps):
            t_f.append(timed(lambda: old("F"))[0]); t_h.append(timed(lambda: old("H"))[0])
            if new:
                t_fh.append(timed(fh)[0])
        out["f_ms"], out["h_ms"], out["fh_ms"] = t_f, t_h, t_fh
        if new:
            out["peak_fh"], out["base"] = peak(fh)
            out["peak_two"], _ = peak(lambda: (old("F"), old("H")))
        print(json.dumps(out), flush=True)
        del k, d
        torch.cuda.empty_cache()


def run_child(a, which, lib):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    else:
        env.pop("MI_DEGENSAC_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--images", str(a.images), "--rows", str(a.rows), "--reps", str(a.reps), "--child", which]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(f"child process failed ({out.returncode}): {out.stderr[-2000:]}")
    return {r["arm"]: r for r in (json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{"))}


def fmt(v):
    return f"{np.median(v):8.2f} ms [{min(v):.2f}..{max(v):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=65)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    K = a.images * (a.images - 1) // 2
    say(f"# {a.images} images x {a.rows} x {DIM}, exhaustive_pairs({a.images}) = {K} pairs, ratio 0.9, default estimator parameters; wall clock from the "
        f"call to a synchronised stream, {a.reps} calls after one warm-up of every form; every build in a child process of its own")
    par = run_child(a, "parent", a.baseline_lib) if a.baseline_lib else None
    new = run_child(a, "this", None)
    if par is None:
        say("# no --baseline-lib: the two existing calls are those of THIS build")
    for name, _ in ARMS:
        n = new[name]; p = (par or new)[name]
        two = [f + h for f, h in zip(p["f_ms"], p["h_ms"])]
        two_new = [f + h for f, h in zip(n["f_ms"], n["h_ms"])]
        m = np.median(n["fh_ms"])
        where = "below the lower end of" if m < min(two) else ("inside" if m <= max(two) else "ABOVE")
        say(f"## {name}")
        say(f"   parent build, F call {fmt(p['f_ms'])} + H call {fmt(p['h_ms'])} = {fmt(two)}")
        say(f"   this build,   F call {fmt(n['f_ms'])} + H call {fmt(n['h_ms'])} = {fmt(two_new)}")
        say(f"   this build,   match_and_verify_fh_pairs_tensors {fmt(n['fh_ms'])}: {where} the parent's summed range, saving {np.median(two) - m:.2f} ms "
            f"({100 * (1 - m / np.median(two)):.1f} % of the parent's median)")
        say(f"   torch.cuda.max_memory_allocated: new call {n['peak_fh'] / 1e6:.1f} MB, the two existing calls in a row {n['peak_two'] / 1e6:.1f} MB "
            f"(stores held before either: {n['base'] / 1e6:.1f} MB); outputs identical to the two calls: {n['same']}")
        say(f"   mean summary (tentatives, nF, nH, nFH) = ({', '.join(f'{x:.1f}' for x in n['summary_mean'])}); two_view_config: "
            f"{n['classes'][0]} rejected, {n['classes'][1]} general, {n['classes'][2]} planar")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
