"""Refinement of relative poses on exported correspondence lists on the device (mi_degensac_pose_refine_lists_dev,
tensor_api.refine_pose_tensors): what it costs, what a caller writes today for the same rule, how the runs end, how good the poses are
before and after, and that the calls next to it are untouched.  One MI355X; medians over --reps calls with [min..max] after two warm-up
calls.  The 65 x 2000 x 128 collection of synthetic.image_collection and the 2080 pairs of exhaustive_pairs(65), F models:
verify -> guided -> export (points) -> refit -> pose -> refine with the pose call's front as keep.
  refine      the call by HIP events and by wall time; status counts, trials per entry
  today       read corr_offsets (a host synchronisation), pad the entries to the longest, the same Levenberg-Marquardt rule as batched
              float64 tensor expressions (torch.linalg.cholesky_ex / cholesky_solve), one more synchronisation at the end; wall time
  accuracy    rotation and baseline-direction error of every entry with a pose against synthetic.collection_cameras before and after:
              median and maximum, in degrees
  fed back    front and wide rows of relative_pose_tensors on the models of the refit and on the returned F
  untouched   match_and_verify_pairs_tensors (F), guided_match_pairs_tensors, refit_correspondences_tensors and relative_pose_tensors on
              the same store, this build against --parent-lib (a libmi_degensac.so of the parent commit), each in a child process of its
              own, alternating
usage: gpu_pose_refine.py [--reps R] [--parent-lib PATH] [--log FILE] [--small]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_correspond as gc          # noqa: E402  (events, wall, store and the "untouched" child)
import gpu_pose as gp                # noqa: E402  (the pipeline up to the export, the refit and pose children)


def torch_route(pts, co, R, t, cam, keep, max_trials=20, ftol=1e-12):
    """what a caller writes today: the same rule, every entry padded to the longest; one camera for all images.  Returns (R, t, cost [K, 2])"""
    import torch
    dev = pts.device
    o = co.cpu()                                                       # the second host synchronisation of the pipeline
    K = len(o) - 1; lens = (o[1:] - o[:-1]); Lm = int(lens.max())
    ar = torch.arange(Lm, device=dev)[None, :]; ln = lens.to(dev)[:, None]
    idx = (o[:-1].to(dev)[:, None] + ar).clamp(max=int(o[-1]) - 1)
    use = (ar < ln) & keep[idx]
    P = pts[idx]                                                       # [K, L, 4], ragged entries as padded tensors
    fx, fy, cx, cy = cam
    one = torch.ones_like(P[..., 0])
    d1 = torch.stack([(P[..., 0] - cx) / fx, (P[..., 1] - cy) / fy, one], -1); d2 = torch.stack([(P[..., 2] - cx) / fx, (P[..., 3] - cy) / fy, one], -1)
    w8 = use.to(torch.float64)
    eye = torch.eye(3, dtype=torch.float64, device=dev); eye5 = torch.eye(5, dtype=torch.float64, device=dev)

    def skew(x):
        z = torch.zeros_like(x[..., 0])
        return torch.stack([torch.stack([z, -x[..., 2], x[..., 1]], -1), torch.stack([x[..., 2], z, -x[..., 0]], -1),
                            torch.stack([-x[..., 1], x[..., 0], z], -1)], -2)

    def epi(M):                                                        # M [K, m, 3, 3] -> n, (a0, a1, b0, b1) [K, m, L]
        a = torch.einsum("kmij,klj->kmli", M, d1); b = torch.einsum("kmij,kli->kmlj", M, d2)
        n = (a * d2[:, None]).sum(-1)
        return n, torch.stack([a[..., 0] / fx, a[..., 1] / fy, b[..., 0] / fx, b[..., 1] / fy], -1)

    def sums(R, t):
        E = skew(t) @ R
        i = t.abs().argmin(1)
        u = torch.linalg.cross(eye[i], t); u = u / u.norm(dim=1, keepdim=True); v = torch.linalg.cross(t, u)
        G = torch.stack([E] + [E @ skew(eye[k].expand(K, 3)) for k in range(3)] + [skew(u) @ R, skew(v) @ R], 1)
        n, ab = epi(G)
        s = (ab[:, 0] ** 2).sum(-1); q = s.sqrt(); r = n[:, 0] / q
        h = (ab[:, :1] * ab[:, 1:]).sum(-1)
        J = (n[:, 1:] / q[:, None] - n[:, :1] * h / (s * q)[:, None]) * w8[:, None]
        r = torch.where(use, r, torch.zeros_like(r))
        return (r * r).sum(1), torch.einsum("kml,kl->km", J, r), torch.einsum("kml,knl->kmn", J, J), u, v

    cost, g, A, u, v = sums(R, t)
    cost0 = cost.clone()
    lam = torch.full((K,), 1e-3, dtype=torch.float64, device=dev); live = torch.isfinite(cost) & (use.sum(1) >= 5)
    for _ in range(max_trials):
        M = A + lam[:, None, None] * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
        Lc, bad = torch.linalg.cholesky_ex(torch.where(live[:, None, None], M, eye5))
        dl = torch.cholesky_solve(-g[:, :, None], Lc)[:, :, 0]
        a = 0.5 * dl[:, :3]; aa = (a * a).sum(1)[:, None, None]
        C = ((1 - aa) * eye + 2 * a[:, :, None] * a[:, None, :] + 2 * skew(a)) / (1 + aa)
        Rn = R @ C; tn = t + dl[:, 3:4] * u + dl[:, 4:5] * v; tn = tn / tn.norm(dim=1, keepdim=True)
        cn, gn, An, un, vn = sums(Rn, tn)
        acc = live & (bad == 0) & (cn < cost)
        done = acc & ((cost - cn) <= ftol * cost)
        m1 = acc[:, None]; m2 = acc[:, None, None]
        R = torch.where(m2, Rn, R); t = torch.where(m1, tn, t); u = torch.where(m1, un, u); v = torch.where(m1, vn, v)
        g = torch.where(m1, gn, g); A = torch.where(m2, An, A); cost = torch.where(acc, cn, cost)
        lam = torch.where(acc, (lam / 10).clamp(min=1e-12), lam * 10)
        live = live & ~done & ~(lam > 1e12)
    return R, t, torch.stack([cost0, cost], 1)


def child_refine(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import synthetic, tensor_api
    from tests import pose_ref as R
    dev = torch.device("cuda", 0)
    pairs, F, co, n, pts = gp.pipeline(dev, small)
    K = len(pairs); m = int(np.asarray(pairs).max()) + 1
    M, inl, info_r = tensor_api.refit_correspondences_tensors(pts, co, F, "F")
    Kc, poses = synthetic.collection_cameras(m)
    cam = [float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])]
    cams = torch.tensor([cam] * m, dtype=torch.float64, device=dev)
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
    Rm, t, front, info = tensor_api.relative_pose_tensors(pts, co, M, cams, pairs=pr, keep=inl)
    call = lambda **kw: tensor_api.refine_pose_tensors(pts, co, Rm, t, cams, pairs=pr, keep=front, **kw)          # noqa: E731
    res = {"pairs": K, "rows": n}
    res["refine_ms"] = gc.events(call, reps)
    res["refine_all_ms"] = gc.events(lambda: call(with_resid=True, with_F=True), reps)
    res["refine_wall_ms"] = gc.wall(call, reps)
    R2, t2, cost, inf2, F2 = call(with_F=True)
    ih = inf2.cpu().numpy(); ch = cost.cpu().numpy()
    res["status"] = np.bincount(ih[:, 3], minlength=8).tolist()
    run = ih[:, 3] <= 2
    res["used"] = int(ih[:, 0].sum()); res["trials"] = [float(np.median(ih[run, 1])), int(ih[run, 1].max()), int(ih[run, 1].sum())]
    res["accepted"] = [float(np.median(ih[run, 2])), int(ih[run, 2].max())]
    res["cost"] = [float(ch[run, 0].sum()), float(ch[run, 1].sum())]
    res["today_ms"] = gc.wall(lambda: torch_route(pts, co, Rm, t, cam, front), reps)
    Rt, tt, ct = torch_route(pts, co, Rm, t, cam, front)
    res["today_cost"] = float(ct[torch.from_numpy(run).to(dev), 1].sum().item())
    res["today_max_pose_diff"] = float(max((Rt - R2)[torch.from_numpy(run).to(dev)].abs().max().item(), (tt - t2)[torch.from_numpy(run).to(dev)].abs().max().item()))
    p0 = info.cpu().numpy()
    ok = (p0[:, 4] == 0) & run
    for tag, Ra, ta in (("before", Rm, t), ("after", R2, t2)):
        Rh = Ra.cpu().numpy(); th = ta.cpu().numpy(); re, te = [], []
        for p, (i, j) in enumerate(np.asarray(pairs)):
            if ok[p]:
                Rg, tg = R.relative(poses, int(i), int(j))
                re.append(R.rot_err_deg(Rh[p], Rg)); te.append(R.dir_err_deg(th[p], tg))
        res["rot_" + tag] = [float(np.median(re)), float(np.max(re))]; res["dir_" + tag] = [float(np.median(te)), float(np.max(te))]
        res["dir_over_5_" + tag] = int((np.array(te) > 5.0).sum())
    back = tensor_api.relative_pose_tensors(pts, co, F2, cams, pairs=pr, keep=front)[3].cpu().numpy()
    res["front_wide_refit"] = [int(p0[:, 1].sum()), int(p0[:, 3].sum())]; res["front_wide_refined"] = [int(back[:, 1].sum()), int(back[:, 3].sum())]
    res["back_status"] = np.bincount(back[:, 4], minlength=5).tolist()
    print(json.dumps(res), flush=True)


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
    if a.child == "refine":
        return child_refine(a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
        if a.log:                                                      # kept up to date: a run that is cut short leaves what it had
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    def fmt(v):
        return f"{np.median(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    r = run_child("refine", a.reps, a.small)
    say(f"# pose refinement on exported correspondence lists; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"{r['pairs']} list entries, the guided export holds {r['rows']} rows, keep = the pose call's front ({r['used']} used rows)")
    say("## 1. the refine call (cameras by index, keep given, max_trials 20, ftol 1e-12)")
    say(f"HIP events: pose + cost + info {fmt(r['refine_ms'])}   with resid and F {fmt(r['refine_all_ms'])}")
    say(f"wall time of the synchronised call {fmt(r['refine_wall_ms'])}")
    say(f"status counts (converged, stalled, max_trials, short, not_finite, bad_pose, bad_camera, truncated) {r['status']}")
    say(f"trials per entry that ran: median {r['trials'][0]:.0f} max {r['trials'][1]} (sum {r['trials'][2]}); accepted: median {r['accepted'][0]:.0f} "
        f"max {r['accepted'][1]}; cost summed over them {r['cost'][0]:.6g} -> {r['cost'][1]:.6g} px^2")
    say("## 2. today: corr_offsets to the host, entries padded to the longest, the same rule as batched float64 torch expressions (wall, synchronised)")
    say(f"today {fmt(r['today_ms'])}   the refine call, wall {fmt(r['refine_wall_ms'])}   {np.median(r['today_ms']) / np.median(r['refine_wall_ms']):.1f}x")
    say(f"end cost of the torch route {r['today_cost']:.6g} px^2; largest difference of a pose entry between the two {r['today_max_pose_diff']:.3g}")
    say("## 3. accuracy against synthetic.collection_cameras over the entries that ran (degrees; recorded, not asserted)")
    for tag in ("before", "after"):
        say(f"{tag:>6s}: rotation error median {r['rot_' + tag][0]:.4f} max {r['rot_' + tag][1]:.4f}; baseline direction error median "
            f"{r['dir_' + tag][0]:.4f} max {r['dir_' + tag][1]:.4f}; entries with more than 5 degrees {r['dir_over_5_' + tag]}")
    say("## 4. the pose call on the returned F (keep = the same front rows)")
    say(f"front / wide rows under the refit's models {r['front_wide_refit']}, under the returned F {r['front_wide_refined']}; status counts of the "
        f"second pose call (ok, bad_model, bad_camera, truncated, empty) {r['back_status']}")
    if a.parent_lib:
        say("## 5. untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = []
        for _ in range(2):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                x = gc.run_child("untouched", a.reps, a.small, lib); y = gp.run_child("refit", a.reps, a.small, lib); z = gp.run_child("pose", a.reps, a.small, lib)
                x["refit_ms"] = y["refit_ms"]; x["pose_ms"] = z["pose_wall_ms"]; x["checksum"] = x["checksum"] + y["checksum"] + [z["front"], z["wide"]]
                runs.append((who, x))
        for key, name in (("mv_ms", "match_and_verify_pairs_tensors F"), ("guided_ms", "guided_match_pairs_tensors F"),
                          ("refit_ms", "refit_correspondences_tensors F"), ("pose_ms", "relative_pose_tensors")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (model, guided-match, refit and pose checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
    else:
        say("## 5. untouched calls: not measured (no --parent-lib)")


if __name__ == "__main__":
    main()
