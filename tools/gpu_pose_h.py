"""Relative pose from homographies on exported correspondence lists on the device (mi_degensac_pose_h_lists_dev,
tensor_api.homography_pose_tensors): what it costs, what a caller writes today for the same end, how good the poses are against the F
pose on the pairs it is for, and that the calls next to it are untouched.  One MI355X; medians over --reps calls with [min..max] after two
warm-up calls.  Two 65 x 2000 x 128 collections of synthetic.planar_collection (one plane; one centre) and the 2080 pairs of
exhaustive_pairs(65): F + H verify -> export under H (points) -> both pose calls with the H inliers as the rows.
  pose        the call by HIP events and by wall time; status counts, rows used / front / runner-up / wide
  today       read corr_offsets (a host synchronisation), batched torch.linalg.svd of G, Faugeras' closed form, cheirality, plane side and
              midpoint as tensor expressions over all rows, the counts by index_add_; wall time of the synchronised expression; the front
              flags of both, row for row
  accuracy    rotation and baseline-direction error of every entry against the generator, under the F pose and under the H pose, for the
              planar and for the panoramic collection: median and maximum, in degrees
  untouched   relative_pose_tensors, refine_pose_tensors and match_and_verify_pairs_tensors (F) on the general collection, this build
              against --parent-lib (a libmi_degensac.so of the parent commit), each in a child process of its own, alternating
usage: gpu_pose_h.py [--reps R] [--parent-lib PATH] [--log FILE] [--small]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_correspond as gc          # noqa: E402  (events, wall, store)
import gpu_pose as gp                # noqa: E402  (the F pipeline of the untouched calls)


def pipeline(dev, small, kind):
    import numpy as np
    import torch
    from pydegensac_amd import matcher, parallel, synthetic, tensor_api
    m, n = (5, 300) if small else (gc.M, gc.N)
    kps, descs, truth = synthetic.planar_collection(m, n, 0.6, 0.1, gc.DIM, seed=0, kind=kind)
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev); c = [n] * m
    pairs = matcher.exhaustive_pairs(m); K = len(pairs)
    ver = tensor_api.match_and_verify_fh_pairs_tensors(k, k, d, d, c, c, pairs, seeds=parallel.pair_seeds(0, K))
    F, H, match, inl_h, summary = ver[0], ver[1], ver[2], ver[4], ver[7]
    rows, co, total, _, pts, resid = tensor_api.correspondences_pairs_tensors(match, c, c, pairs, keep=inl_h, kps1=k, kps2=k, models=H, model="H",
                                                                              capacity=int(inl_h.sum().item()))
    torch.cuda.synchronize()
    return pairs, F, H, co, int(total.item()), pts, truth, summary, float(resid[:int(total.item())].abs().max().item())


def torch_route(pts, co, H, cam, cos_min, eps=1e-3):
    """what a caller writes today; one camera for all images.  Returns (R [K, 3, 3], t [K, 3], front [n], counts [K, 4])"""
    import torch
    o = co.cpu()                                                       # a host synchronisation
    K = len(o) - 1; n = int(o[-1]); dev = pts.device
    ent = torch.repeat_interleave(torch.arange(K, device=dev), (o[1:] - o[:-1]).to(dev))
    Km = torch.tensor([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]], dtype=torch.float64, device=dev)
    G = torch.linalg.inv(Km) @ H @ Km
    G = G / torch.linalg.svdvals(G)[:, 1, None, None] * torch.sign(torch.linalg.det(G))[:, None, None]
    U, d, Vh = torch.linalg.svd(G)
    s = (torch.linalg.det(U) * torch.linalg.det(Vh))[:, None, None]
    d1_, d2_, d3_ = d[:, 0], d[:, 1], d[:, 2]
    rot = d1_ - d3_ <= eps
    den = (d1_ ** 2 - d3_ ** 2).clamp_min(1e-300)
    x1 = torch.sqrt(((d1_ ** 2 - d2_ ** 2) / den).clamp_min(0)); x3 = torch.sqrt(((d2_ ** 2 - d3_ ** 2) / den).clamp_min(0))
    sin = torch.sqrt(((d1_ ** 2 - d2_ ** 2) * (d2_ ** 2 - d3_ ** 2)).clamp_min(0)) / ((d1_ + d3_) * d2_)
    cos = (d2_ ** 2 + d1_ * d3_) / ((d1_ + d3_) * d2_)
    Rs, ts, ns = [], [], []
    z = torch.zeros_like(cos); one_ = torch.ones_like(cos)
    for e1 in (1.0, -1.0):
        for e3 in (1.0, -1.0):
            sn = e1 * e3 * sin
            Rp = torch.stack([torch.stack([cos, z, -sn], 1), torch.stack([z, one_, z], 1), torch.stack([sn, z, cos], 1)], 1)
            tp = (d1_ - d3_)[:, None] * torch.stack([e1 * x1, z, -e3 * x3], 1); npr = torch.stack([e1 * x1, z, e3 * x3], 1)
            Rs.append(s * (U @ Rp @ Vh)); t = (U @ tp[:, :, None])[:, :, 0]
            ts.append(t / torch.linalg.norm(t, dim=1, keepdim=True).clamp_min(1e-300)); ns.append((Vh.transpose(1, 2) @ npr[:, :, None])[:, :, 0])
    Rs = torch.stack(Rs, 1); ts = torch.stack(ts, 1); ns = torch.stack(ns, 1)
    P = pts[:n]
    one = torch.ones(n, dtype=torch.float64, device=dev)
    d1 = torch.stack([(P[:, 0] - cam[2]) / cam[0], (P[:, 1] - cam[3]) / cam[1], one], 1)
    d2 = torch.stack([(P[:, 2] - cam[2]) / cam[0], (P[:, 3] - cam[3]) / cam[1], one], 1)
    Rr = Rs[ent]; tr = ts[ent]
    r2 = torch.einsum("nqij,ni->nqj", Rr, d2); c2 = -torch.einsum("nqij,nqi->nqj", Rr, tr)
    a = (d1 * d1).sum(1)[:, None]; b = torch.einsum("ni,nqi->nq", d1, r2); c = (r2 * r2).sum(2)
    dd = torch.einsum("ni,nqi->nq", d1, c2); e = (r2 * c2).sum(2); dn = a * c - b * b
    l1 = (c * dd - b * e) / dn; l2 = (b * dd - a * e) / dn
    fr = (l1 > 0) & (l2 > 0) & (torch.einsum("ni,nqi->nq", d1, ns[ent]) > 0)
    cnt = torch.zeros((K, 4), dtype=torch.int64, device=dev).index_add_(0, ent, fr.long())
    q = cnt.argmax(1); ar = torch.arange(K, device=dev)
    Rrot = U @ Vh
    Rrot = Rrot * torch.sign(torch.linalg.det(Rrot))[:, None, None]
    fr_rot = torch.einsum("nj,nj->n", Rrot[ent][:, 2, :], d1) > 0
    front = torch.where(rot[ent], fr_rot, fr[torch.arange(n, device=dev), q[ent]])
    return torch.where(rot[:, None, None], Rrot, Rs[ar, q]), torch.where(rot[:, None], torch.zeros_like(ts[:, 0]), ts[ar, q]), front, cnt


def errors(R, pairs, poses, Rm, t, ok, with_t):
    import numpy as np
    re, te = [], []
    for p, (i, j) in enumerate(np.asarray(pairs)):
        if ok[p]:
            Rg, tg = R.relative(poses, int(i), int(j)) if with_t else (poses[int(j)][0] @ poses[int(i)][0].T, None)
            re.append(R.rot_err_deg(Rm[p], Rg))
            if with_t and np.abs(t[p]).sum() > 0:
                te.append(R.dir_err_deg(t[p], tg))
    med = lambda v: [float(np.median(v)), float(np.max(v)), len(v)] if len(v) else [float("nan"), float("nan"), 0]          # noqa: E731
    return med(re), med(te)


def child_pose(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import matcher, tensor_api
    from tests import pose_ref as R
    dev = torch.device("cuda", 0)
    res = {}
    for kind in ("planar", "panoramic"):
        pairs, F, H, co, n, pts, truth, summary, resid = pipeline(dev, small, kind)
        K = len(pairs); m = int(np.asarray(pairs).max()) + 1
        Kc = truth["K"]; cam = [float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])]
        cams = torch.tensor([cam] * m, dtype=torch.float64, device=dev)
        pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
        call = lambda **kw: tensor_api.homography_pose_tensors(pts, co, H, cams, pairs=pr, **kw)          # noqa: E731
        r = {"pairs": K, "rows": n, "max_resid": resid, "classes": np.bincount(matcher.two_view_config(summary), minlength=3).tolist()}
        r["pose_ms"] = gc.events(call, reps)
        r["pose_points_ms"] = gc.events(lambda: call(with_points=True, with_candidates=True), reps)
        r["pose_wall_ms"] = gc.wall(call, reps)
        r["pose_f_ms"] = gc.events(lambda: tensor_api.relative_pose_tensors(pts, co, F, cams, pairs=pr), reps)
        Rh, th, front, info, normal, tod = call()
        Rf, tf, front_f, info_f = tensor_api.relative_pose_tensors(pts, co, F, cams, pairs=pr)
        ih = info.cpu().numpy(); iF = info_f.cpu().numpy()
        r["status"] = np.bincount(ih[:, 4], minlength=6).tolist()
        r["used"] = int(ih[:, 0].sum()); r["front"] = int(ih[:, 1].sum()); r["runner_up"] = int(ih[:, 2].sum()); r["wide"] = int(ih[:, 3].sum())
        r["undecided"] = int(((ih[:, 4] == 0) & (ih[:, 1] == ih[:, 2])).sum())
        cm = R.cos_min(1.5)
        r["today_ms"] = gc.wall(lambda: torch_route(pts, co, H, cam, cm), reps)
        Rt, tt, ft, cnt = torch_route(pts, co, H, cam, cm)
        r["today_front"] = int(ft.sum().item()); r["today_same_front"] = int((ft == front[:n]).sum().item())
        with_t = kind == "planar"
        r["err_h"] = errors(R, pairs, truth["poses"], Rh.cpu().numpy(), th.cpu().numpy(), np.isin(ih[:, 4], (0, 5)), with_t)
        r["err_f"] = errors(R, pairs, truth["poses"], Rf.cpu().numpy(), tf.cpu().numpy(), iF[:, 4] == 0, with_t)
        res[kind] = r
    print(json.dumps(res), flush=True)


def child_untouched(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import matcher, parallel, synthetic, tensor_api
    dev = torch.device("cuda", 0)
    pairs, F, co, n, pts = gp.pipeline(dev, small)
    K = len(pairs); m = int(np.asarray(pairs).max()) + 1
    Kc, _ = synthetic.collection_cameras(m)
    cams = torch.tensor([[float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])]] * m, dtype=torch.float64, device=dev)
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
    k, d, c = gc.store(dev, small)
    out = {"pose_ms": [], "refine_ms": [], "mv_ms": []}
    for r in range(reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        Rm, t, front, info = tensor_api.relative_pose_tensors(pts, co, F, cams, pairs=pr)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        Rr, tr, cost, info_r = tensor_api.refine_pose_tensors(pts, co, Rm, t, cams, pairs=pr, keep=front)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        mv = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, c, c, pairs, model="F", seeds=parallel.pair_seeds(0, K))
        torch.cuda.synchronize(); t3 = time.perf_counter()
        if r >= 1:
            out["pose_ms"].append(1e3 * (t1 - t0)); out["refine_ms"].append(1e3 * (t2 - t1)); out["mv_ms"].append(1e3 * (t3 - t2))
    out["checksum"] = [float(Rm.abs().sum().item()), int(front.sum().item()), float(Rr.abs().sum().item()), float(mv[0].abs().sum().item())]
    print(json.dumps(out), flush=True)


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
        return {"pose": child_pose, "untouched": child_untouched}[a.child](a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    res = run_child("pose", a.reps, a.small)
    say(f"# relative pose from homographies on exported correspondence lists; medians over {a.reps} calls [min..max]"
        + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    for kind in ("planar", "panoramic"):
        r = res[kind]
        say(f"## {kind} collection: {r['pairs']} list entries, the export under H holds {r['rows']} rows (largest |resid| under the H that goes in "
            f"{r['max_resid']:.3f}); two_view_config classes (rejected, general, planar / panoramic) {r['classes']}")
        say(f"HIP events: pose + front + info + normal {fmt(r['pose_ms'])}   with X, depth, cosang and the candidates {fmt(r['pose_points_ms'])}   "
            f"relative_pose_tensors on the same lists {fmt(r['pose_f_ms'])}")
        say(f"status counts (ok, bad_model, bad_camera, truncated, empty, rotation) {r['status']}; rows used {r['used']}, front {r['front']}, "
            f"front of the runner-up {r['runner_up']}, wide at 1.5 degrees {r['wide']}; entries whose two solutions are not told apart {r['undecided']}")
        say(f"today (corr_offsets to the host, torch.linalg.svd, closed form and cheirality as tensor expressions; wall, synchronised) {fmt(r['today_ms'])}   "
            f"the call, wall {fmt(r['pose_wall_ms'])}   {np.median(r['today_ms']) / np.median(r['pose_wall_ms']):.1f}x")
        say(f"front rows of the torch route {r['today_front']}, of the call {r['front']}; rows with the same flag {r['today_same_front']} of {r['rows']}")
        for name, key in (("F pose", "err_f"), ("H pose", "err_h")):
            (rm, rx, rn), (tm, tx, tn) = r[key]
            say(f"{name}: rotation error median {rm:.4f} max {rx:.4f} degrees over {rn} entries with a pose"
                + (f"; baseline direction error median {tm:.4f} max {tx:.4f} over {tn}" if tn else "; no baseline"))
    if a.parent_lib:
        say("## untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = []
        for _ in range(2):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                runs.append((who, run_child("untouched", a.reps, a.small, lib)))
        for key, name in (("pose_ms", "relative_pose_tensors"), ("refine_ms", "refine_pose_tensors"), ("mv_ms", "match_and_verify_pairs_tensors F")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (pose, front, refined pose and model checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
    else:
        say("## untouched calls: not measured (no --parent-lib)")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
