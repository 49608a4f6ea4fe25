"""The correspondence export on the device (mi_degensac_correspondences_pairs_dev, tensor_api.correspondences_pairs_tensors): what it costs
against a plain copy and against the torch expression a caller would write, what it allocates, and that the calls next to it are untouched.
One MI355X; medians over --reps calls with [min..max] after two warm-up calls.  The 65 x 2000 x 128 collection of synthetic.image_collection
and the 2080 pairs of exhaustive_pairs(65): 4.16 M output rows; match / inlier / F come from match_and_verify_pairs_tensors (F).
  export      the call with rows only and with rows + points + residuals, HIP events around the call (it pre-fills its outputs, which is part
              of the time).  Bytes counted from the shapes: both passes read match and keep (2 x 5 N), the write pass stores 8 bytes per
              correspondence (+ 32 read, 32 + 8 written with points and residuals) and 8 per entry.  Share of copy bandwidth = the time of a
              torch copy that moves the same number of bytes (half read, half written), measured in the same run, over the call's time
  torch       nonzero (a host synchronisation), searchsorted on pair_offsets, the gathers and a float64 Sampson formula on the same tensors,
              wall time of the synchronised expression; how many of its residuals have the estimator's bits
  memory      torch.cuda.max_memory_allocated over the call with capacity=None and with capacity=int(n_tentatives.sum())
  untouched   match_and_verify_pairs_tensors (F) and guided_match_pairs_tensors on the same store, this build against --parent-lib (a
              libmi_degensac.so of the parent commit), each in a child process of its own, alternating, wall time of the synchronised call
usage: gpu_correspond.py [--reps R] [--parent-lib PATH] [--log FILE] [--small]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def wall(fn, reps):
    import torch
    out = []
    for r in range(reps + 2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = fn(); torch.cuda.synchronize()
        if r >= 2:
            out.append(1e3 * (time.perf_counter() - t0))
        del res
    return out


def store(dev, small):
    import numpy as np
    import torch
    from pydegensac_amd import synthetic
    m, n = (5, 300) if small else (M, N)
    kps, descs = synthetic.image_collection(m, n, 0.6, 0.1, DIM, seed=0)
    return (torch.from_numpy(np.concatenate(kps)).to(dev), torch.from_numpy(np.concatenate(descs)).to(dev), [n] * m)


def torch_expr(match, inlier, po, o1, pr, k, F):
    """what a caller writes today: (rows [n, 2], entry [n], pts [n, 4], Sampson residual [n]) in float64"""
    import torch
    sel = torch.nonzero((match >= 0) & inlier).flatten()              # synchronises with the host
    e = torch.searchsorted(po, sel, right=True) - 1
    q = sel - po[e]
    t = match[sel].long()
    x1 = k[o1[pr[e, 0]] + q, :2]; x2 = k[o1[pr[e, 1]] + t, :2]
    one = torch.ones((len(sel), 1), dtype=torch.float64, device=k.device)
    h1 = torch.cat([x1, one], 1); h2 = torch.cat([x2, one], 1)
    Fe = F[e]
    l2 = torch.bmm(Fe, h1[:, :, None])[:, :, 0]; l1 = torch.bmm(Fe.transpose(1, 2), h2[:, :, None])[:, :, 0]
    r = (h2 * l2).sum(1)
    d = r * r / (l2[:, 0] ** 2 + l2[:, 1] ** 2 + l1[:, 0] ** 2 + l1[:, 1] ** 2)
    return torch.stack([q, t], 1), e, torch.cat([x1, x2], 1), d


def child_corr(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import matcher, parallel, tensor_api
    dev = torch.device("cuda", 0)
    k, d, c = store(dev, small)
    pairs = matcher.exhaustive_pairs(len(c)); K = len(pairs)
    F, match, inlier, _, nten, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, c, c, pairs, model="F", seeds=parallel.pair_seeds(0, K))
    torch.cuda.synchronize()
    n_rows = int(po[-1]); cap = int(nten.sum())
    call = tensor_api.correspondences_pairs_tensors
    lean = lambda capacity=None: call(match, c, c, pairs, keep=inlier, capacity=capacity)                                   # noqa: E731
    full = lambda capacity=None: call(match, c, c, pairs, keep=inlier, kps1=k, kps2=k, models=F, with_entry=True, capacity=capacity)   # noqa: E731
    total = int(lean()[2].item())
    b_lean = 2 * 5 * n_rows + 8 * total + 8 * (K + 1)
    b_full = b_lean + (4 + 32 + 32 + 8) * total + 72 * K
    res = {"rows": n_rows, "pairs": K, "total": total, "tentatives": cap, "bytes": {"rows": b_lean, "full": b_full}, "ms": {}, "copy_ms": {}}
    for name, fn, nbytes in (("rows", lean, b_lean), ("full", full, b_full)):
        for capname, capacity in (("N", None), ("tent", cap)):
            res["ms"][f"{name}/{capname}"] = events(lambda: fn(capacity), reps)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        res["copy_ms"][name] = events(lambda: dst.copy_(src), reps)
        del src, dst
    # the torch expression on the same tensors
    po_d = torch.from_numpy(po).to(dev); o1_d = torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev)
    pr_d = torch.from_numpy(np.ascontiguousarray(pairs, np.int64)).to(dev)
    res["torch_ms"] = wall(lambda: torch_expr(match, inlier, po_d, o1_d, pr_d, k, F), reps)
    res["call_wall_ms"] = wall(lambda: full(cap), reps)
    rows, co, tot, entry, pts, resid = full()
    t_rows, t_e, t_pts, t_d = torch_expr(match, inlier, po_d, o1_d, pr_d, k, F)
    n = total
    res["torch_same"] = {"rows": bool(torch.equal(rows[:n].long(), t_rows)), "entry": bool(torch.equal(entry[:n].long(), t_e)),
                         "pts": bool(torch.equal(pts[:n], t_pts)), "resid_equal_bits": int((resid[:n].view(torch.int64) == t_d.view(torch.int64)).sum().item()),
                         "resid_max_rel": float(((resid[:n] - t_d).abs() / resid[:n].abs().clamp(min=1e-300)).max().item())}
    # peak memory of the call
    res["mem"] = {}
    for capname, capacity in (("N", None), ("tent", cap)):
        torch.cuda.synchronize(); base = torch.cuda.memory_allocated(dev); torch.cuda.reset_peak_memory_stats(dev)
        out = full(capacity); torch.cuda.synchronize()
        res["mem"][capname] = int(torch.cuda.max_memory_allocated(dev) - base)
        del out
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
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=400).stdout
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
        return {"corr": child_corr, "untouched": child_untouched}[a.child](a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    r = run_child("corr", a.reps, a.small)
    say(f"# correspondence export; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"{r['pairs']} list entries, {r['rows']} output rows, {r['tentatives']} tentatives, {r['total']} verified correspondences (keep = inlier)")
    say("## the call (HIP events; outputs pre-filled inside the call) against a torch copy of the same number of bytes")
    for name, label in (("rows", "rows only"), ("full", "rows + entry + points + residuals")):
        for capname, cl in (("N", "capacity=None"), ("tent", "capacity=tentatives")):
            ms = r["ms"][f"{name}/{capname}"]
            say(f"{label:>34s} {cl:>20s}: {fmt(ms)}  {r['bytes'][name]} bytes, {r['bytes'][name] / (np.median(ms) * 1e-3) / 1e12:5.2f} TB/s; copy of as many "
                f"bytes {fmt(r['copy_ms'][name])}: {100 * np.median(r['copy_ms'][name]) / np.median(ms):5.1f} % of copy bandwidth")
    say("## the torch expression a caller writes today (nonzero, searchsorted, gathers, float64 Sampson), wall time with its host synchronisation")
    say(f"torch expression {fmt(r['torch_ms'])}   this call, rows + entry + points + residuals, capacity=tentatives, wall {fmt(r['call_wall_ms'])}   "
        f"{np.median(r['torch_ms']) / np.median(r['call_wall_ms']):.1f}x")
    s = r["torch_same"]
    say(f"same rows {s['rows']}, same entries {s['entry']}, same points {s['pts']}; residuals with the estimator's bits: {s['resid_equal_bits']} of {r['total']} "
        f"(largest relative difference {s['resid_max_rel']:.2e})")
    say("## torch.cuda.max_memory_allocated over the call (rows + entry + points + residuals), above what was allocated before it")
    say(f"capacity=None {r['mem']['N'] / 2**20:.1f} MiB   capacity=int(n_tentatives.sum()) {r['mem']['tent'] / 2**20:.1f} MiB")
    if a.parent_lib:
        say("## untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
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
