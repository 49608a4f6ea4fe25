"""The refit on exported correspondence lists on the device (mi_degensac_refit_lists_dev, tensor_api.refit_correspondences_tensors): what it
costs, what a caller does today for the same end, how the scoring pass compares with a plain copy, and that the calls next to it are
untouched.  One MI355X; medians over --reps calls with [min..max] after two warm-up calls.  The 65 x 2000 x 128 collection of
synthetic.image_collection and the 2080 pairs of exhaustive_pairs(65), F models: verify -> guided -> export (points + residuals) -> refit.
  refit       the call on the guided export with max_fits = 4, HIP events around it; members before and after, fits run, status counts
  today       read corr_offsets (a host synchronisation), then find_fundamental_batch_tensors on the exported points: a whole RANSAC per
              entry; wall time of the synchronised expression and its inlier counts next to the refit's members
  scoring     the call with max_fits = 0 is two scoring passes (the members of the start model, then inlier under it) and nothing else:
              bytes counted from the shapes (2 x 32 read per row, 1 written, 4 per member for the list, 72 + 72 + 16 + 16 per entry) over
              its time, against a torch copy that moves as many bytes (half read, half written) in the same run
  untouched   match_and_verify_pairs_tensors (F) and guided_match_pairs_tensors on the same store, this build against --parent-lib (a
              libmi_degensac.so of the parent commit), each in a child process of its own, alternating (tools/gpu_correspond.py's child)
usage: gpu_refit.py [--reps R] [--parent-lib PATH] [--log FILE] [--small]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_correspond as gc          # noqa: E402  (events, wall, store and the "untouched" child)


def child_refit(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import matcher, parallel, tensor_api
    dev = torch.device("cuda", 0)
    k, d, c = gc.store(dev, small)
    pairs = matcher.exhaustive_pairs(len(c)); K = len(pairs)
    F, match, inlier, _, nten, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, c, c, pairs, model="F", seeds=parallel.pair_seeds(0, K))
    gm = tensor_api.guided_match_pairs_tensors(k, k, d, d, c, c, pairs, F, model="F")[0]
    rows, co, total, _, pts, resid = tensor_api.correspondences_pairs_tensors(gm, c, c, pairs, kps1=k, kps2=k, models=F,
                                                                              capacity=int((gm >= 0).sum().item()))
    torch.cuda.synchronize()
    n = int(total.item())
    call = tensor_api.refit_correspondences_tensors
    res = {"pairs": K, "rows": n, "verified": int(inlier.sum().item())}
    res["refit_ms"] = gc.events(lambda: call(pts, co, F, "F"), reps)
    res["refit_resid_ms"] = gc.events(lambda: call(pts, co, F, "F", with_resid=True), reps)
    M, inl, info, r2 = call(pts, co, F, "F", with_resid=True)
    info_h = info.cpu().numpy()
    res["n0"] = int(info_h[:, 0].sum()); res["members"] = int(info_h[:, 1].sum()); res["fits"] = int(info_h[:, 2].sum())
    res["status"] = np.bincount(info_h[:, 3], minlength=6).tolist()
    ok = inl & torch.isfinite(r2)
    res["mean_resid"] = {"start": float(resid[:n].mean().item()), "refit_members": float(r2[ok].mean().item())}
    # what a caller does today: the offsets on the host, then the whole estimator on the exported points
    def today():
        cnt = np.diff(co.cpu().numpy())                                # the second host synchronisation of the pipeline
        return tensor_api.find_fundamental_batch_tensors(pts[:n, :2], pts[:n, 2:], cnt, seeds=parallel.pair_seeds(0, K))
    if (np.diff(co.cpu().numpy()) >= 8).all():
        res["today_ms"] = gc.wall(today, reps)
        res["refit_wall_ms"] = gc.wall(lambda: call(pts, co, F, "F"), reps)
        Ft, mask, _, offs = today()
        m = np.add.reduceat(mask.cpu().numpy().astype(np.int64), offs[:-1])
        res["today_members"] = int(m.sum()); res["entries_refit_ge_today"] = int((info_h[:, 1] >= m).sum())
    # the scoring pass
    res["score_ms"] = gc.events(lambda: call(pts, co, F, "F", max_fits=0), reps)
    nbytes = (2 * 32 + 1) * n + 4 * res["n0"] + (72 + 72 + 16 + 16) * K
    res["score_bytes"] = nbytes
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    res["copy_ms"] = gc.events(lambda: dst.copy_(src), reps)
    print(json.dumps(res), flush=True)


def run_child(reps, small):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "refit", "--reps", str(reps)] + (["--small"] if small else [])
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=500).stdout
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
        return child_refit(a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    r = run_child(a.reps, a.small)
    say(f"# refit on exported correspondence lists; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"{r['pairs']} list entries, F; verify kept {r['verified']} inliers, the guided export holds {r['rows']} rows")
    say("## 1. the refit call on the guided export, max_fits = 4 (HIP events)")
    say(f"models + inlier + info {fmt(r['refit_ms'])}   with resid {fmt(r['refit_resid_ms'])}")
    say(f"members of the start models {r['n0']}, at the end {r['members']}, fits run {r['fits']}; status counts "
        f"(fixed, max_fits, short, bad_fit, worse, truncated) {r['status']}")
    say(f"mean residual of the exported rows under the start models {r['mean_resid']['start']:.5f}, of the members under the refit models "
        f"{r['mean_resid']['refit_members']:.5f}")
    say("## 2. today: corr_offsets to the host, then find_fundamental_batch_tensors on the exported points (wall time, synchronised)")
    if "today_ms" in r:
        say(f"today {fmt(r['today_ms'])}   the refit call, wall {fmt(r['refit_wall_ms'])}   {np.median(r['today_ms']) / np.median(r['refit_wall_ms']):.1f}x")
        say(f"inliers of the re-run RANSAC {r['today_members']}, members of the refit {r['members']}; entries where the refit has at least as many: "
            f"{r['entries_refit_ge_today']} of {r['pairs']}")
    else:
        say("not measured: an entry has fewer than 8 rows, which find_fundamental_batch_tensors refuses")
    say("## 3. the scoring pass: the call with max_fits = 0 (two passes) against a torch copy of as many bytes, same run")
    t = np.median(r["score_ms"]) * 1e-3
    say(f"max_fits = 0 {fmt(r['score_ms'])}  {r['score_bytes']} bytes, {r['score_bytes'] / t / 1e12:5.3f} TB/s; copy of as many bytes {fmt(r['copy_ms'])}: "
        f"{100 * np.median(r['copy_ms']) / np.median(r['score_ms']):5.1f} % of copy bandwidth")
    if a.parent_lib:
        say("## 4. untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = [("parent", gc.run_child("untouched", a.reps, a.small, a.parent_lib)), ("this", gc.run_child("untouched", a.reps, a.small)),
                ("parent", gc.run_child("untouched", a.reps, a.small, a.parent_lib)), ("this", gc.run_child("untouched", a.reps, a.small))]
        for key, name in (("mv_ms", "match_and_verify_pairs_tensors F"), ("guided_ms", "guided_match_pairs_tensors F")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (model and guided-match checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
    else:
        say("## 4. untouched calls: not measured (no --parent-lib)")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
