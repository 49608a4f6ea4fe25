"""Tracks on the device (mi_degensac_tracks_dev, tensor_api.tracks_tensors): what the call costs on the edge list of the correspondence
export, against what a caller does today and against a sort of as many keys, what the tracks look like, and that the calls next to it are
untouched.  One MI355X; medians over --reps calls with [min..max] after two warm-up calls.  The 65 x 2000 x 128 collection of
synthetic.image_collection and the 2080 pairs of exhaustive_pairs(65); match / inlier come from match_and_verify_pairs_tensors (F), rows and
total from correspondences_pairs_tensors(keep=inlier, store_rows=True).
  tracks      tracks_tensors(rows, counts, total), HIP events around the call (its output allocations are part of the time)
  today       rows[:total].cpu() and the union-find of tests/tracks_ref.py (labels only), wall time with the synchronisation; here the
              restatement is the baseline, not the code under test
  sort        torch.sort of as many 32-bit keys as the store has rows, HIP events: the yardstick for the grouping step
  tracks      their number, the length histogram, the share that is consistent; the device's result against the restatement
  per kernel  --child loop runs the call alone reps + 2 times for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
              tools/gpu_tracks.py --child loop`; --kernel-stats DIR/.../*_kernel_stats.csv then adds the kernels of the call to the log
  untouched   match_and_verify_pairs_tensors (F) and guided_match_pairs_tensors on the same store, this build against --parent-lib (a
              libmi_degensac.so of the parent commit), each in a child process of its own, alternating (tools/gpu_correspond.py's children)
usage: gpu_tracks.py [--reps R] [--parent-lib PATH] [--kernel-stats CSV] [--log FILE] [--small]"""
import argparse
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gpu_correspond as gc          # noqa: E402  events, wall, store and the "untouched" children


def edges(dev, small):
    """(rows, total, counts) of the export call on the verified matches of the collection"""
    import torch
    from pydegensac_amd import matcher, parallel, tensor_api
    k, d, c = gc.store(dev, small)
    pairs = matcher.exhaustive_pairs(len(c)); K = len(pairs)
    F, match, inlier, _, nten, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, c, c, pairs, model="F", seeds=parallel.pair_seeds(0, K))
    rows, co, total = tensor_api.correspondences_pairs_tensors(match, c, c, pairs, keep=inlier, store_rows=True, capacity=int(nten.sum()))[:3]
    torch.cuda.synchronize()
    return rows, total, c, K


def child_tracks(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import tensor_api
    from tests import tracks_ref as tr
    dev = torch.device("cuda", 0)
    rows, total, c, K = edges(dev, small)
    R = int(sum(c)); n = int(total.item())
    off = tr.offsets(c)
    res = {"pairs": K, "nodes": R, "edges": n, "capacity": int(rows.shape[0])}
    res["tracks_ms"] = gc.events(lambda: tensor_api.tracks_tensors(rows, c, total=total), reps)
    res["tracks_wall_ms"] = gc.wall(lambda: tensor_api.tracks_tensors(rows, c, total=total), reps)
    res["today_ms"] = gc.wall(lambda: tr.labels(rows[:int(total.item())].cpu().numpy(), off), reps)
    keys = torch.randint(0, R + 1, (R,), dtype=torch.int32, device=dev)
    res["sort_ms"] = gc.events(lambda: torch.sort(keys), reps)
    track, nt, to, obs, oi, ti, no, label = (x.cpu().numpy() for x in tensor_api.tracks_tensors(rows, c, total=total, with_label=True))
    nt, no = int(nt[0]), int(no[0])
    got = {"label": label, "track": track, "n_tracks": nt, "n_obs": no, "track_offsets": to, "obs": obs, "obs_image": oi, "track_images": ti}
    res["equal"] = bool(tr.equal(got, tr.tracks(rows.cpu().numpy(), off, n)))
    length = np.diff(to[:nt + 1])
    res["n_tracks"] = nt; res["n_obs"] = no
    res["consistent"] = int((ti[:nt] == length).sum())
    edges_ = [2, 3, 4, 5, 9, 17, 33, 65, 1 << 62]
    res["hist"] = [[edges_[i], edges_[i + 1] - 1, int(((length >= edges_[i]) & (length < edges_[i + 1])).sum())] for i in range(len(edges_) - 1)]
    res["longest"] = int(length.max()) if nt else 0
    print(json.dumps(res), flush=True)


def child_loop(reps, small):
    import torch
    from pydegensac_amd import tensor_api
    rows, total, c, _ = edges(torch.device("cuda", 0), small)
    for _ in range(reps + 2):
        out = tensor_api.tracks_tensors(rows, c, total=total)
        torch.cuda.synchronize()
        del out


def run_child(what, reps, small):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(reps)] + (["--small"] if small else [])
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=500).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")][-1]


def kernel_lines(path, calls):
    """the kernels of the call (tk_* and the sort's) from a rocprofv3 kernel_stats csv of --child loop: name, launches per call, time per call"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "tk_" in name or "rocprim" in name or "radix" in name or "onesweep" in name:
                rows.append((name, int(r["Calls"]), float(r["TotalDurationNs"])))
    all_ns = sum(t for _, _, t in rows)
    out = []
    for name, n, t in sorted(rows, key=lambda x: -x[2]):
        short = name if len(name) <= 90 else name[:87] + "..."
        out.append(f"{t / calls / 1e3:9.2f} us per call ({100 * t / all_ns:5.1f} %)  {n / calls:4.1f} launches per call  {short}")
    out.append(f"{all_ns / calls / 1e3:9.2f} us per call in these kernels, {calls} calls")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of `--child loop` run with the same --reps")
    ap.add_argument("--log", default=None)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return {"tracks": child_tracks, "loop": child_loop}[a.child](a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    r = run_child("tracks", a.reps, a.small)
    say(f"# tracks; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"{r['pairs']} list entries, {r['nodes']} store rows (nodes), {r['edges']} verified correspondences (edges) in rows [{r['capacity']}, 2]")
    say(f"tracks_tensors, HIP events        {fmt(r['tracks_ms'])}")
    say(f"tracks_tensors, wall, synchronised {fmt(r['tracks_wall_ms'])}")
    say(f"today: rows[:total].cpu() + the restatement's union-find (labels only), wall {fmt(r['today_ms'])}   "
        f"{np.median(r['today_ms']) / np.median(r['tracks_wall_ms']):.0f}x the call")
    say(f"torch.sort of {r['nodes']} int32 keys, HIP events {fmt(r['sort_ms'])}")
    say(f"every output equal to the restatement on the device's rows: {'yes' if r['equal'] else 'NO'}")
    say(f"{r['n_tracks']} tracks with {r['n_obs']} observations, longest {r['longest']}; consistent (one keypoint per image at most): {r['consistent']} "
        f"= {100 * r['consistent'] / max(r['n_tracks'], 1):.2f} %")
    say("length histogram: " + ", ".join(f"{lo}{'' if hi == lo else ('+' if hi > 1 << 40 else '..' + str(hi))}: {n}" for lo, hi, n in r["hist"]))
    if a.kernel_stats:
        say("## the kernels of the call (rocprofv3 --kernel-trace --stats on --child loop, a run of its own)")
        for ln in kernel_lines(a.kernel_stats, a.reps + 2):
            say(ln)
    else:
        say("## the kernels of the call: not measured (no --kernel-stats)")
    if a.parent_lib:
        say("## untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = [("parent", gc.run_child("untouched", a.reps, a.small, a.parent_lib)), ("this", gc.run_child("untouched", a.reps, a.small)),
                ("parent", gc.run_child("untouched", a.reps, a.small, a.parent_lib)), ("this", gc.run_child("untouched", a.reps, a.small))]
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
