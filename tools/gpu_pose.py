"""Relative pose and triangulation on exported correspondence lists on the device (mi_degensac_pose_lists_dev,
tensor_api.relative_pose_tensors): what it costs, what a caller writes today for the same end, how the row passes compare with a plain
copy, how good the poses are, and that the calls next to it are untouched.  One MI355X; medians over --reps calls with [min..max] after
two warm-up calls.  The 65 x 2000 x 128 collection of synthetic.image_collection and the 2080 pairs of exhaustive_pairs(65), F models:
verify -> guided -> export (points) -> refit -> pose with the refit's inlier as keep.
  pose        the call by HIP events and by wall time; status counts, rows used / front / wide
  today       read corr_offsets (a host synchronisation), batched torch.linalg.svd of E, the four candidates, cheirality and midpoint as
              tensor expressions over all rows, the counts by index_add_; wall time of the synchronised expression
  row passes  bytes counted from the shapes (2 x 32 + 2 x 1 read per row, 1 written per used row) over the call's time, against a torch
              copy that moves as many bytes (half read, half written) in the same run
  accuracy    rotation and baseline-direction error of every entry against synthetic.collection_cameras: median and maximum, in degrees
  untouched   match_and_verify_pairs_tensors (F), guided_match_pairs_tensors and refit_correspondences_tensors on the same store, this
              build against --parent-lib (a libmi_degensac.so of the parent commit), each in a child process of its own, alternating
usage: gpu_pose.py [--reps R] [--parent-lib PATH] [--log FILE] [--small]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_correspond as gc          # noqa: E402  (events, wall, store and the "untouched" child)


def pipeline(dev, small):
    import torch
    from pydegensac_amd import matcher, parallel, tensor_api
    k, d, c = gc.store(dev, small)
    pairs = matcher.exhaustive_pairs(len(c)); K = len(pairs)
    F, match, inlier, _, nten, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, c, c, pairs, model="F", seeds=parallel.pair_seeds(0, K))
    gm = tensor_api.guided_match_pairs_tensors(k, k, d, d, c, c, pairs, F, model="F")[0]
    rows, co, total, _, pts, resid = tensor_api.correspondences_pairs_tensors(gm, c, c, pairs, kps1=k, kps2=k, models=F,
                                                                              capacity=int((gm >= 0).sum().item()))
    torch.cuda.synchronize()
    return pairs, F, co, int(total.item()), pts


def torch_route(pts, co, F, cam, keep, cos_min):
    """what a caller writes today; one camera for all images.  Returns (R [K, 3, 3], t [K, 3], front [n], counts [K, 4])"""
    import torch
    o = co.cpu()                                                       # the second host synchronisation of the pipeline
    K = len(o) - 1; n = int(o[-1])
    ent = torch.repeat_interleave(torch.arange(K, device=pts.device), (o[1:] - o[:-1]).to(pts.device))
    Km = torch.tensor([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]], dtype=torch.float64, device=pts.device)
    E = Km.T @ F @ Km
    U, S, Vh = torch.linalg.svd(E)
    U = U * torch.sign(torch.linalg.det(U))[:, None, None]; Vh = Vh * torch.sign(torch.linalg.det(Vh))[:, None, None]
    W = torch.tensor([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]], dtype=torch.float64, device=pts.device)
    Rs = torch.stack([U @ W @ Vh, U @ W @ Vh, U @ W.T @ Vh, U @ W.T @ Vh], 1)          # [K, 4, 3, 3]
    ts = torch.stack([U[:, :, 2], -U[:, :, 2], U[:, :, 2], -U[:, :, 2]], 1)             # [K, 4, 3]
    P = pts[:n]
    one = torch.ones(n, dtype=torch.float64, device=pts.device)
    d1 = torch.stack([(P[:, 0] - cam[2]) / cam[0], (P[:, 1] - cam[3]) / cam[1], one], 1)
    d2 = torch.stack([(P[:, 2] - cam[2]) / cam[0], (P[:, 3] - cam[3]) / cam[1], one], 1)
    Rr = Rs[ent]; tr = ts[ent]                                         # [n, 4, 3, 3], [n, 4, 3]
    r2 = torch.einsum("nqij,ni->nqj", Rr, d2); c2 = -torch.einsum("nqij,nqi->nqj", Rr, tr)
    a = (d1 * d1).sum(1)[:, None]; b = torch.einsum("ni,nqi->nq", d1, r2); c = (r2 * r2).sum(2)
    dd = torch.einsum("ni,nqi->nq", d1, c2); e = (r2 * c2).sum(2); den = a * c - b * b
    l1 = (c * dd - b * e) / den; l2 = (b * dd - a * e) / den
    fr = (l1 > 0) & (l2 > 0) & keep[:n, None]
    cnt = torch.zeros((K, 4), dtype=torch.int64, device=pts.device).index_add_(0, ent, fr.long())
    q = cnt.argmax(1)
    ar = torch.arange(K, device=pts.device)
    front = fr[torch.arange(n, device=pts.device), q[ent]]
    wide = front & ((b / torch.sqrt(a * c))[torch.arange(n, device=pts.device), q[ent]] <= cos_min)
    return Rs[ar, q], ts[ar, q], front, cnt, wide


def child_pose(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import synthetic, tensor_api
    sys.path.insert(0, ROOT)
    from tests import pose_ref as R
    dev = torch.device("cuda", 0)
    pairs, F, co, n, pts = pipeline(dev, small)
    K = len(pairs); m = int(np.asarray(pairs).max()) + 1
    M, inl, info_r = tensor_api.refit_correspondences_tensors(pts, co, F, "F")
    Kc, poses = synthetic.collection_cameras(m)
    cam = [float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])]
    cams = torch.tensor([cam] * m, dtype=torch.float64, device=dev)
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
    call = lambda **kw: tensor_api.relative_pose_tensors(pts, co, M, cams, pairs=pr, keep=inl, **kw)          # noqa: E731
    res = {"pairs": K, "rows": n}
    res["pose_ms"] = gc.events(call, reps)
    res["pose_points_ms"] = gc.events(lambda: call(with_points=True, with_candidates=True), reps)
    res["pose_wall_ms"] = gc.wall(call, reps)
    Rm, t, front, info = call()
    ih = info.cpu().numpy()
    res["status"] = np.bincount(ih[:, 4], minlength=5).tolist()
    res["used"] = int(ih[:, 0].sum()); res["front"] = int(ih[:, 1].sum()); res["runner_up"] = int(ih[:, 2].sum()); res["wide"] = int(ih[:, 3].sum())
    cm = R.cos_min(1.5)
    res["today_ms"] = gc.wall(lambda: torch_route(pts, co, M, cam, inl, cm), reps)
    Rt, tt, ft, cnt, wt = torch_route(pts, co, M, cam, inl, cm)
    res["today_front"] = int(ft.sum().item()); res["today_same_front"] = int((ft == front[:n]).sum().item())
    nbytes = (2 * 32 + 2 * 1) * n + res["used"] + (72 + 8 + 96 + 20) * K
    res["bytes"] = nbytes
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    res["copy_ms"] = gc.events(lambda: dst.copy_(src), reps)
    Rh = Rm.cpu().numpy(); th = t.cpu().numpy(); re, te = [], []
    for p, (i, j) in enumerate(np.asarray(pairs)):
        if ih[p, 4] == 0:
            Rg, tg = R.relative(poses, int(i), int(j))
            re.append(R.rot_err_deg(Rh[p], Rg)); te.append(R.dir_err_deg(th[p], tg))
    res["rot_err_deg"] = [float(np.median(re)), float(np.max(re))]; res["dir_err_deg"] = [float(np.median(te)), float(np.max(te))]
    print(json.dumps(res), flush=True)


def child_refit_untouched(reps, small):
    import torch
    from pydegensac_amd import tensor_api
    pairs, F, co, n, pts = pipeline(torch.device("cuda", 0), small)
    out = []
    for r in range(reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        M, inl, info = tensor_api.refit_correspondences_tensors(pts, co, F, "F")
        torch.cuda.synchronize()
        if r >= 1:
            out.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"refit_ms": out, "checksum": [float(M.abs().sum().item()), int(inl.sum().item())]}), flush=True)


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
    if a.child == "pose":
        return child_pose(a.reps, a.small)
    if a.child == "refit":
        return child_refit_untouched(a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    r = run_child("pose", a.reps, a.small)
    say(f"# relative pose on exported correspondence lists; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"{r['pairs']} list entries, the guided export holds {r['rows']} rows, keep = the refit's inlier")
    say("## 1. the pose call (cameras by index, keep given)")
    say(f"HIP events: pose + front + info {fmt(r['pose_ms'])}   with X, depth, cosang and the candidates {fmt(r['pose_points_ms'])}")
    say(f"wall time of the synchronised call {fmt(r['pose_wall_ms'])}")
    say(f"status counts (ok, bad_model, bad_camera, truncated, empty) {r['status']}; rows used {r['used']}, front {r['front']}, "
        f"front of the runner-up {r['runner_up']}, wide at 1.5 degrees {r['wide']}")
    say("## 2. today: corr_offsets to the host, batched torch.linalg.svd, cheirality and midpoint as tensor expressions (wall time, synchronised)")
    say(f"today {fmt(r['today_ms'])}   the pose call, wall {fmt(r['pose_wall_ms'])}   {np.median(r['today_ms']) / np.median(r['pose_wall_ms']):.1f}x")
    say(f"front rows of the torch route {r['today_front']}, of the call {r['front']}; rows with the same flag {r['today_same_front']} of {r['rows']}")
    say("## 3. the row passes against a torch copy of as many bytes, same run")
    t = np.median(r["pose_ms"]) * 1e-3
    say(f"the call {fmt(r['pose_ms'])}  {r['bytes']} bytes, {r['bytes'] / t / 1e12:5.3f} TB/s; copy of as many bytes {fmt(r['copy_ms'])}: "
        f"{100 * np.median(r['copy_ms']) / np.median(r['pose_ms']):5.1f} % of copy bandwidth")
    say("## 4. accuracy against synthetic.collection_cameras over the entries with a pose (degrees; recorded, not asserted)")
    say(f"rotation error median {r['rot_err_deg'][0]:.4f} max {r['rot_err_deg'][1]:.4f}; baseline direction error median {r['dir_err_deg'][0]:.4f} "
        f"max {r['dir_err_deg'][1]:.4f}")
    if a.parent_lib:
        say("## 5. untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = []
        for _ in range(2):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                x = gc.run_child("untouched", a.reps, a.small, lib); y = run_child("refit", a.reps, a.small, lib)
                x["refit_ms"] = y["refit_ms"]; x["checksum"] = x["checksum"] + y["checksum"]
                runs.append((who, x))
        for key, name in (("mv_ms", "match_and_verify_pairs_tensors F"), ("guided_ms", "guided_match_pairs_tensors F"),
                          ("refit_ms", "refit_correspondences_tensors F")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (model, guided-match and refit checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
    else:
        say("## 5. untouched calls: not measured (no --parent-lib)")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
