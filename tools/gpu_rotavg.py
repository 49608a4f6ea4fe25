"""Rotation averaging on the device (mi_degensac_rotation_average_dev, tensor_api.average_rotations_tensors): what it costs, what a caller
writes today for the same rule, what it does to the rotations, and that the calls next to it are untouched.  One MI355X; medians over
--reps calls with [min..max] after two warm-up calls.  The 65 x 2000 x 128 collection of synthetic.image_collection and the 2080 pairs
of exhaustive_pairs(65): verify -> guided matches -> export -> pose -> refine, then the averaging of the refined rotations with the pose
call's wide rows as weights and its status as edge_keep.
  call        the tensor call by HIP events and by wall time, with the default 200 sweeps and with as many as changed something
  sweeps      the time per queued sweep from two sweep counts; the sweeps that changed something
  today       the same rule as batched float64 tensor expressions: index_add_ over the half-edges, one synchronisation per sweep to
              learn whether anything changed; wall time; agreement with the call
  accuracy    rotation error against synthetic.collection_cameras, gauge aligned at the root: after the first level and at the end
  untouched   relative_pose_tensors, refine_pose_tensors and match_and_verify_pairs_tensors on the same store and bench.py, this build
              against --parent-lib (a libmi_degensac.so of the parent commit), each in a child process of its own, alternating passes
usage: gpu_rotavg.py [--reps R] [--parent-lib PATH] [--log FILE] [--small]"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_correspond as gc          # noqa: E402  (events, wall, store and the "untouched" child)
import gpu_pose as gp                # noqa: E402  (the pipeline up to the exported lists)
import gpu_triangulate as gtri       # noqa: E402  (bench.py)


def poses(dev, small):
    """the pipeline up to the refined pairwise poses -> dict of what the averaging and the untouched calls take"""
    import numpy as np
    import torch
    from pydegensac_amd import _lib, synthetic, tensor_api
    pairs, F, co, total, pts = gp.pipeline(dev, small)
    m = int(np.asarray(pairs).max()) + 1
    Kc, gen = synthetic.collection_cameras(m)
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * m, dtype=torch.float64, device=dev)
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
    R, t, front, info = tensor_api.relative_pose_tensors(pts, co, F, cams, pairs=pr)
    R2, t2, cost, info2 = tensor_api.refine_pose_tensors(pts, co, R, t, cams, pairs=pr, keep=front)
    torch.cuda.synchronize()
    return dict(pairs=pairs, pr=pr, F=F, co=co, pts=pts, cams=cams, R=R, t=t, front=front, R2=R2.contiguous(), weight=info[:, 3].double(),
                keep=info[:, 4] == _lib.POSE_OK, m=m, truth=torch.from_numpy(np.stack([Rm for Rm, _ in gen])).to(dev))


def errors(R, truth, root=0):
    """the angle in degrees between R[c] and the generator's rotation, the gauge aligned at the root"""
    import torch
    G = truth[root].T @ R[root]
    c = ((R * (truth @ G)).sum((1, 2)) - 1.0) / 2.0
    return torch.rad2deg(torch.acos(c.clamp(-1, 1)))


def torch_route(pr, Rr, n, weight, keep, root=0, sweeps=200, damping=0.5, robust_deg=5.0, tol=1e-9):
    """what a caller writes today: the same rule over all half-edges at once, index_add_ for the sums (their order is the runtime's), one
    .item() per sweep.  Returns (R [n, 3, 3], sweeps that changed something)"""
    import torch
    dev = Rr.device
    i, j = pr[:, 0].long(), pr[:, 1].long()
    w = weight.clone()
    s = (Rr * Rr).sum((1, 2))
    used = keep & (i != j) & (w > 0) & torch.isfinite(w) & ((s - 3.0).abs() <= 1e-6)
    i, j, w, A = i[used], j[used], w[used], Rr[used]
    cam = torch.cat([i, j]); oth = torch.cat([j, i]); hw = torch.cat([w, w]); M = torch.cat([A.transpose(1, 2), A])          # P = M R_other
    R = torch.zeros((n, 3, 3), dtype=torch.float64, device=dev); R[root] = torch.eye(3, dtype=torch.float64, device=dev)
    isset = torch.zeros(n, dtype=torch.bool, device=dev); isset[root] = True
    held = isset.clone()
    s2 = math.tan(math.radians(robust_deg) / 2) ** 2
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    changed = 0
    for _ in range(sweeps):
        P = M @ R[oth]
        el = isset[oth]
        # the start of the cameras that are not set: the heaviest eligible half-edge (ties: any)
        score = torch.where(el & ~isset[cam], hw, torch.zeros_like(hw))
        best = torch.zeros(n, dtype=torch.float64, device=dev).scatter_reduce(0, cam, score, "amax")
        pick = (score > 0) & (score == best[cam])
        Rn = R.clone(); newset = isset.clone()
        idx = torch.nonzero(pick).squeeze(1)
        Rn[cam[idx]] = P[idx]; newset[cam[idx]] = True
        # the move of the others
        Q = P @ R[cam].transpose(1, 2)
        q = 1.0 + Q.diagonal(dim1=1, dim2=2).sum(1)
        good = el & isset[cam] & ~held[cam] & (q > 2.0 ** -10)
        om = torch.stack([Q[:, 2, 1] - Q[:, 1, 2], Q[:, 0, 2] - Q[:, 2, 0], Q[:, 1, 0] - Q[:, 0, 1]], 1) / q[:, None]
        f = hw * (s2 / (s2 + (om * om).sum(1))) ** 2
        f = torch.where(good, f, torch.zeros_like(f)); om = torch.where(good[:, None], om, torch.zeros_like(om))
        S = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, cam, f)
        W = torch.zeros((n, 3), dtype=torch.float64, device=dev).index_add_(0, cam, f[:, None] * om)
        upd = S > 0
        u = torch.where(upd[:, None], W / S.clamp(min=1e-300)[:, None], torch.zeros_like(W))
        a = damping * u
        aa = (a * a).sum(1)[:, None, None]
        ax = torch.zeros((n, 3, 3), dtype=torch.float64, device=dev)
        ax[:, 0, 1] = -a[:, 2]; ax[:, 0, 2] = a[:, 1]; ax[:, 1, 0] = a[:, 2]; ax[:, 1, 2] = -a[:, 0]; ax[:, 2, 0] = -a[:, 1]; ax[:, 2, 1] = a[:, 0]
        Cm = ((1 - aa) * eye + 2 * a[:, :, None] * a[:, None, :] + 2 * ax) / (1 + aa)
        Rn = torch.where(upd[:, None, None], Cm @ R, Rn)
        moved = bool(((newset != isset).any() | ((u * u).sum(1) > tol * tol).any()).item())          # the synchronisation of every sweep
        R, isset = Rn, newset
        if not moved:
            break
        changed += 1
    return R, changed


def child_rotavg(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import _lib, tensor_api
    dev = torch.device("cuda", 0)
    s = poses(dev, small)
    n = s["m"]
    L = _lib.lib()
    call = lambda sw=200, **kw: tensor_api.average_rotations_tensors(s["pr"], s["R2"], n, weight=s["weight"], edge_keep=s["keep"], sweeps=sw, **kw)   # noqa: E731
    R, info, step, summary, ecos = call(with_edges=True)
    torch.cuda.synchronize()
    sm = [int(x) for x in summary.cpu().numpy()]
    r = {"tile": [L.mi_degensac_rotation_average_tile(i) for i in range(3)], "images": n, "pairs": len(s["pairs"]), "summary": sm,
         "call_ms": gc.events(call, reps), "call_wall_ms": gc.wall(call, reps)}
    need = sm[0] + 1
    r["need"] = need
    r["call_need_ms"] = gc.events(lambda: call(need), reps); r["call_need_wall_ms"] = gc.wall(lambda: call(need), reps)
    r["call_1000_ms"] = gc.events(lambda: call(1000), reps)
    r["call_1000_tol0_ms"] = gc.events(lambda: call(1000, tol=0.0), reps)
    r["tol0_summary"] = [int(x) for x in call(1000, tol=0.0)[3].cpu().numpy()]
    today = lambda: torch_route(s["pr"], s["R2"], n, s["weight"], s["keep"])          # noqa: E731
    r["today_ms"] = gc.wall(today, reps)
    Rt, ch = today()
    r["today_changed"] = ch
    r["today_diff"] = float((Rt - R).abs().max().item())
    Rl = call(1)[0]
    e1 = errors(Rl, s["truth"]); e2 = errors(R, s["truth"])
    rel = s["truth"][s["pr"][:, 1].long()] @ s["truth"][s["pr"][:, 0].long()].transpose(1, 2)
    pc = ((s["R2"] * rel).sum((1, 2)) - 1.0) / 2.0
    pe = torch.rad2deg(torch.acos(pc.clamp(-1, 1)))[s["keep"]]
    st = lambda e: [float(e[1:].mean().item()), float(e[1:].median().item()), float(e.max().item())]          # noqa: E731
    r["err_level"] = st(e1); r["err_end"] = st(e2); r["err_pairs"] = [float(pe.mean().item()), float(pe.median().item()), float(pe.max().item())]
    r["below5"] = int((ecos < math.cos(math.radians(5.0))).sum().item()); r["nan_edges"] = int(torch.isnan(ecos).sum().item())
    r["status"] = np.bincount(info[:, 3].cpu().numpy(), minlength=4).tolist()
    print(json.dumps(r), flush=True)


def child_untouched(reps, small):
    import torch
    from pydegensac_amd import tensor_api
    dev = torch.device("cuda", 0)
    s = poses(dev, small)
    pose = lambda: tensor_api.relative_pose_tensors(s["pts"], s["co"], s["F"], s["cams"], pairs=s["pr"])          # noqa: E731
    ref = lambda: tensor_api.refine_pose_tensors(s["pts"], s["co"], s["R"], s["t"], s["cams"], pairs=s["pr"], keep=s["front"])          # noqa: E731
    r = {"pose_ms": gc.wall(pose, reps), "refine_ms": gc.wall(ref, reps)}
    r["checksum"] = [float(torch.nan_to_num(pose()[0]).abs().sum().item()), float(torch.nan_to_num(ref()[0]).abs().sum().item())]
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return {"rotavg": child_rotavg, "untouched": child_untouched}[a.child](a.reps, a.small)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
        if a.log:                                                      # kept up to date: a run that is cut short leaves what it had
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    def fmt(v):
        return f"{np.median(v):8.3f} ms [{min(v):.3f}..{max(v):.3f}]"

    def run_child(what, lib=None):
        env = dict(os.environ)
        if lib:
            env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(a.reps)] + (["--small"] if a.small else [])
        out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=500).stdout
        return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")][-1]
    r = run_child("rotavg")
    sm = r["summary"]
    say(f"# rotation averaging; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"{r['tile'][0]} lanes per camera, {r['tile'][2]} cameras per workgroup, grid cap {r['tile'][1]}; {r['images']} images, {r['pairs']} pairs, "
        f"{sm[2]} used; weights = the pose call's wide rows, edge_keep = its status")
    say(f"summary: {sm[0]} sweeps changed something, {sm[1]} cameras set, global status {sm[3]}; camera statuses KNOWN/OK/UNREACHED/ISOLATED {r['status']}")
    say(f"tensor call, 200 sweeps queued, HIP events: {fmt(r['call_ms'])}   wall, synchronised: {fmt(r['call_wall_ms'])}")
    say(f"tensor call, {r['need']} sweeps queued (as many as did something), HIP events: {fmt(r['call_need_ms'])}   wall: {fmt(r['call_need_wall_ms'])}")
    say(f"tensor call, 1000 sweeps queued, HIP events: {fmt(r['call_1000_ms'])}")
    idle = (np.median(r["call_1000_ms"]) - np.median(r["call_ms"])) / 800 * 1e3
    busy = (np.median(r["call_1000_tol0_ms"]) - np.median(r["call_need_ms"])) / max(r["tol0_summary"][0] + 1 - r["need"], 1) * 1e3
    say(f"a queued sweep that finds nothing to do: {idle:.2f} us (from 1000 against 200 sweeps)")
    say(f"tensor call, 1000 sweeps, tol = 0 ({r['tol0_summary'][0]} sweeps changed something), HIP events: {fmt(r['call_1000_tol0_ms'])}")
    say(f"a sweep that runs the rule: about {busy:.2f} us (tol = 0 against the {r['need']}-sweep call; the idle ones of that call counted in)")
    say("## today: the same rule as batched float64 tensor expressions, index_add_ over the half-edges, one .item() per sweep (wall, synchronised)")
    say(f"today {fmt(r['today_ms'])}   the tensor call, wall {fmt(r['call_wall_ms'])}   {np.median(r['today_ms']) / np.median(r['call_wall_ms']):.1f}x"
        f"   against the {r['need']}-sweep call {np.median(r['today_ms']) / np.median(r['call_need_wall_ms']):.1f}x")
    say(f"today's route: {r['today_changed']} sweeps changed something; rotations agree to {r['today_diff']:.3g} (largest element difference)")
    say("## rotation error against synthetic.collection_cameras in degrees, gauge aligned at the root (mean and median over the other cameras, max)")
    say(f"pairwise rotations that go in (kept pairs): mean {r['err_pairs'][0]:.4f} median {r['err_pairs'][1]:.4f} max {r['err_pairs'][2]:.4f}")
    say(f"after the first level (sweeps = 1): mean {r['err_level'][0]:.4f} median {r['err_level'][1]:.4f} max {r['err_level'][2]:.4f}")
    say(f"at the end                        : mean {r['err_end'][0]:.4f} median {r['err_end'][1]:.4f} max {r['err_end'][2]:.4f}")
    say(f"pairs whose edge_cos lies below cos 5 degrees: {r['below5']}; NaN (unused): {r['nan_edges']}")
    if a.parent_lib:
        say("## untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = []
        for _ in range(2):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                x = gc.run_child("untouched", a.reps, a.small, lib); y = run_child("untouched", lib)
                x["pose_ms"] = y["pose_ms"]; x["refine_ms"] = y["refine_ms"]; x["checksum"] = x["checksum"] + y["checksum"]
                runs.append((who, x))
        for key, name in (("mv_ms", "match_and_verify_pairs_tensors F"), ("pose_ms", "relative_pose_tensors"), ("refine_ms", "refine_pose_tensors")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (model and pose checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
        if not a.small:
            say("## bench.py --gpus 1 --steps 5 --warmup 2, ms per step, alternating")
            b = [(who, gtri.run_bench(lib)) for _ in range(2) for who, lib in (("parent", a.parent_lib), ("this", None))]
            par = [v[0] for w, v in b if w == "parent"]; new = [v[0] for w, v in b if w == "this"]
            say(f"parent {par[0]:.2f}, {par[1]:.2f}   this build {new[0]:.2f}, {new[1]:.2f}   mean inliers equal: "
                + ("yes" if len({v[1] for _, v in b}) == 1 else "NO"))
    else:
        say("## untouched calls and bench.py: not measured (no --parent-lib)")


if __name__ == "__main__":
    main()
