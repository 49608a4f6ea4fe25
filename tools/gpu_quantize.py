"""Descriptor quantisation on the device (mi_degensac_desc_quantize_dev, tensor_api.quantize_descriptors_tensors): what it costs, what it
buys, and what it changes.  One MI355X; medians over --reps calls with [min..max] after two warm-up calls; HIP events around the calls.
  kernel      the 65 x 2000 x 128 store and 4 M x 128 rows, presets "rootsift" and "sift" with the clip counts.  Bytes moved = 5 per element
              (4 read, 1 written) + 4 per row; share of HBM bandwidth = bytes / time over 6.29 TB/s (measured float4 copy) and over the
              8.0 TB/s of the data sheet.  Baseline: the same conversion as a torch expression on the same tensor, in float64 (the same
              arithmetic, apart from torch's own summation order) and in float32 (what a caller is likely to write; other roundings)
  end to end  the 2080 pairs of exhaustive_pairs(65) on that store: knn_match_pairs_tensors on the float32 rows under "l2", against
              quantise + knn_match_pairs_tensors under "l2_u8"
  agreement   synthetic.image_collection(8, 2000, dim 128), every ordered pair: per preset the share of queries whose nearest neighbour
              is the same row under "l2_u8" on the quantised rows as under "l2" on the normalised float32 rows, and the overlap of the
              ratio = 0.9 kept sets (|both| / |either|).  "sift" and "rootsift" take the magnitudes of the rows.  Recorded, not thresholds
  untouched   match_and_verify_pairs_tensors (F) and guided_match_pairs_tensors on the same store, this build against --parent-lib (a
              libmi_degensac.so of the parent commit), each in a child process of its own, wall time of the synchronised call
usage: gpu_quantize.py [--reps R] [--parent-lib PATH] [--log FILE] [--small]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
M, N, DIM = 65, 2000, 128


def events(fn, reps):
    import torch
    out = []
    for r in range(reps + 2):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); res = fn(); e1.record(); torch.cuda.synchronize()
        if r >= 2:
            out.append(e0.elapsed_time(e1))
        del res
    return out


def torch_expr(x, preset, dt):
    import torch
    y = x.to(dt)
    if preset == "rootsift":
        a = y.abs()
        y = torch.copysign(torch.sqrt(a / a.sum(1, keepdim=True)), y)
    else:
        y = y / torch.sqrt((y * y).sum(1, keepdim=True))
    return torch.clamp(torch.round(512.0 * y), 0, 255).to(torch.uint8)


def store(dev, small):
    import numpy as np
    import torch
    from pydegensac_amd import synthetic
    m, n = (5, 300) if small else (M, N)
    kps, descs = synthetic.image_collection(m, n, 0.6, 0.1, DIM, seed=0)
    return (torch.from_numpy(np.concatenate(kps)).to(dev), torch.from_numpy(np.concatenate(descs)).to(dev), [n] * m)


def child_quant(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import matcher, tensor_api
    dev = torch.device("cuda", 0)
    _, d, counts = store(dev, small)
    big = torch.rand(((1 << 14) if small else (1 << 22), DIM), device=dev, dtype=torch.float32)
    res = {"kernel": [], "e2e": {}, "agree": {}}
    for name, x in (("store %d x %d x %d" % (len(counts), counts[0], DIM), d.abs()), ("%d x %d rows" % (big.shape[0], DIM), big)):
        for preset in ("rootsift", "sift"):
            out = torch.empty((x.shape[0], DIM), dtype=torch.uint8, device=dev)
            k = events(lambda: tensor_api.quantize_descriptors_tensors(x, preset, out=out, return_clipped=True), reps)
            t64 = events(lambda: torch_expr(x, preset, torch.float64), reps)
            t32 = events(lambda: torch_expr(x, preset, torch.float32), reps)
            same64 = float((torch_expr(x, preset, torch.float64) == out).double().mean().item())
            same32 = float((torch_expr(x, preset, torch.float32) == out).double().mean().item())
            res["kernel"].append({"input": name, "preset": preset, "bytes": int(x.numel()) * 5 + int(x.shape[0]) * 4, "kernel_ms": k,
                                  "torch64_ms": t64, "torch32_ms": t32, "bytes_equal_torch64": same64, "bytes_equal_torch32": same32})
    pairs = matcher.exhaustive_pairs(len(counts))
    res["e2e"]["pairs"] = len(pairs)
    res["e2e"]["float32_ms"] = events(lambda: tensor_api.knn_match_pairs_tensors(d, d, counts, counts, pairs, norm="l2"), reps)
    res["e2e"]["quant_u8_ms"] = events(lambda: tensor_api.knn_match_pairs_tensors(*(2 * (tensor_api.quantize_descriptors_tensors(d, "unit"),)),
                                                                                   counts, counts, pairs, norm="l2_u8"), reps)
    q = tensor_api.quantize_descriptors_tensors(d, "unit")
    res["e2e"]["u8_only_ms"] = events(lambda: tensor_api.knn_match_pairs_tensors(q, q, counts, counts, pairs, norm="l2_u8"), reps)
    # agreement on a smaller collection, both orders of every pair
    from pydegensac_amd import synthetic
    m, n = (4, 200) if small else (8, 2000)
    _, descs = synthetic.image_collection(m, n, 0.6, 0.1, DIM, seed=1)
    a = torch.from_numpy(np.concatenate(descs)).to(dev); c = [n] * m
    pr = matcher.exhaustive_pairs(m, ordered=True)
    for preset in ("sift", "rootsift", "unit"):
        x = a if preset == "unit" else a.abs()
        x64 = x.double()
        f = (torch.sqrt(x64 / x64.sum(1, keepdim=True)) if preset == "rootsift" else x64 / torch.sqrt((x64 * x64).sum(1, keepdim=True))).float()
        qx, cl = tensor_api.quantize_descriptors_tensors(x, preset, return_clipped=True)
        fi, fd, _ = tensor_api.knn_match_pairs_tensors(f, f, c, c, pr, norm="l2")
        ui, ud, _ = tensor_api.knn_match_pairs_tensors(qx, qx, c, c, pr, norm="l2_u8")
        fk = fd[:, 0] < 0.9 * fd[:, 1]; uk = ud[:, 0] < 0.9 * ud[:, 1]
        res["agree"][preset] = {"queries": int(fi.shape[0]), "nn_same": float((fi[:, 0] == ui[:, 0]).double().mean().item()),
                                "kept_float": int(fk.sum().item()), "kept_u8": int(uk.sum().item()), "kept_both": int((fk & uk).sum().item()),
                                "kept_either": int((fk | uk).sum().item()), "clipped_columns": int(cl.clamp(min=0).sum().item()),
                                "dead_rows": int((cl < 0).sum().item())}
    print(json.dumps(res), flush=True)


def child_untouched(reps, small):
    import torch
    from pydegensac_amd import tensor_api, matcher, parallel
    dev = torch.device("cuda", 0)
    k, d, counts = store(dev, small)
    pairs = matcher.exhaustive_pairs(len(counts)); seeds = parallel.pair_seeds(0, len(pairs))
    mv, gd = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        out = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", seeds=seeds)
        torch.cuda.synchronize()
        if r >= 1:
            mv.append(1e3 * (time.perf_counter() - t0))
    F = out[0]
    for r in range(reps + 1):
        t0 = time.perf_counter()
        g = tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, model="F")
        torch.cuda.synchronize()
        if r >= 1:
            gd.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"mv_ms": mv, "guided_ms": gd, "checksum": [float(F.abs().sum().item()), int((g[0] >= 0).sum().item())]}), flush=True)


def run_child(what, reps, small, lib=None):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(reps)] + (["--small"] if small else [])
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=500).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")][-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return {"quant": child_quant, "untouched": child_untouched}[a.child](a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    r = run_child("quant", a.reps, a.small)
    say(f"# descriptor quantisation; medians over {a.reps} calls [min..max], HIP events" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say("## kernel (with clip counts) against the same conversion as a torch expression")
    for k in r["kernel"]:
        t = np.median(k["kernel_ms"]) * 1e-3
        say(f"{k['input']:>24s} {k['preset']:>8s}  kernel {fmt(k['kernel_ms'])}  {k['bytes'] / t / 1e12:5.2f} TB/s = "
            f"{100 * k['bytes'] / t / HBM_MEASURED:4.1f} % of 6.29 TB/s, {100 * k['bytes'] / t / HBM_SPEC:4.1f} % of 8.0 TB/s"
            f"  torch float64 {fmt(k['torch64_ms'])} ({np.median(k['torch64_ms']) / np.median(k['kernel_ms']):.1f}x, bytes equal "
            f"{100 * k['bytes_equal_torch64']:.4f} %)  torch float32 {fmt(k['torch32_ms'])} "
            f"({np.median(k['torch32_ms']) / np.median(k['kernel_ms']):.1f}x, bytes equal {100 * k['bytes_equal_torch32']:.4f} %)")
    e = r["e2e"]
    say(f"## end to end, {e['pairs']} pairs: 2-NN over the pair list")
    say(f"float32 rows under l2 {fmt(e['float32_ms'])}   quantise (preset unit) + l2_u8 {fmt(e['quant_u8_ms'])}   l2_u8 on rows already quantised "
        f"{fmt(e['u8_only_ms'])}   speed-up {np.median(e['float32_ms']) / np.median(e['quant_u8_ms']):.2f}x")
    say("## agreement of the byte path with the float path (recorded figures)")
    for p, g in r["agree"].items():
        say(f"{p:>8s}: nearest neighbour unchanged for {100 * g['nn_same']:.3f} % of {g['queries']} queries; ratio 0.9 kept sets: float {g['kept_float']}, "
            f"uint8 {g['kept_u8']}, both {g['kept_both']}, overlap {100 * g['kept_both'] / max(g['kept_either'], 1):.2f} %; clipped columns "
            f"{g['clipped_columns']}, dead rows {g['dead_rows']}")
    if a.parent_lib:
        say("## untouched calls: this build against a build of the parent commit, wall time of the synchronised call")
        runs = [("parent", run_child("untouched", a.reps, a.small, a.parent_lib)), ("this", run_child("untouched", a.reps, a.small)),
                ("parent", run_child("untouched", a.reps, a.small, a.parent_lib)), ("this", run_child("untouched", a.reps, a.small))]
        for key, name in (("mv_ms", "match_and_verify_pairs_tensors F"), ("guided_ms", "guided_match_pairs_tensors F")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (model and guided-match checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
    else:
        say("## untouched calls: not measured (no --parent-lib)")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
