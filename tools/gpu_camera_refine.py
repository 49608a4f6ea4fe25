"""Refinement of camera poses against triangulated tracks on the device (mi_degensac_camera_refine_tracks_dev,
tensor_api.refine_cameras_tensors): what it costs, what a caller writes today for the same rule, what it does to the poses, and that the
calls next to it are untouched.  One MI355X; medians over --reps calls with [min..max] after two warm-up calls.  The 65 x 2000 x 128
collection of synthetic.image_collection and the 2080 pairs of exhaustive_pairs(65): verify -> export (store rows) -> tracks ->
triangulate under the generator's poses perturbed by --rot radians and --trans, cameras 0 and 1 held.
  call        the tensor call by HIP events and by wall time; the C entry point alone on buffers allocated before
  kernels     mark / sort / bounds / refine from a rocprofv3 --kernel-trace --stats run of a child of its own (--kernel-stats CSV: the
              kernel_stats file of `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/gpu_camera_refine.py --child loop`)
  today       read n_obs and n_tracks (a host synchronisation), regroup by image with a stable sort, pad to the longest image, the same
              LM as batched float64 tensor expressions with torch.linalg.cholesky_ex, one more synchronisation at the end; wall time
  accuracy    summed cost and pose error against synthetic.collection_cameras before and after, and after a second round
  untouched   triangulate_tracks_tensors, tracks_tensors and match_and_verify_pairs_tensors on the same store and bench.py, this build
              against --parent-lib (a libmi_degensac.so of the parent commit), each in a child process of its own, two alternating passes
usage: gpu_camera_refine.py [--reps R] [--parent-lib PATH] [--kernel-stats CSV] [--log FILE] [--small]"""
import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_correspond as gc          # noqa: E402  (events, wall, store and the "untouched" child)
import gpu_triangulate as gtri       # noqa: E402  (the scene and bench.py)

ROT, TRANS = 0.01, 0.02              # the perturbation of the generator's poses: radians about a random axis, length of the offset of t
TRI_PX = 20.0                        # max_reproj_px of the triangulation that feeds obs_keep: 0.01 rad at f = 800 is 8 px, and the default of 4 px
                                     # would drop most observations of a perturbed camera before its pose can be refined


def perturbed(s, rot, trans):
    """(R, t) of the scene perturbed on the left, cameras 0 and 1 exact; the refine mask that holds them"""
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    R = s["R"].cpu().numpy().copy(); t = s["t"].cpu().numpy().copy()
    for i in range(2, len(R)):
        a = rng.normal(size=3); a *= rot / np.linalg.norm(a); th = np.linalg.norm(a); k = a / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R[i] = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K) @ R[i]
        d = rng.normal(size=3); t[i] = t[i] + d * trans / np.linalg.norm(d)
    dev = s["obs"].device
    fix = torch.ones(len(R), dtype=torch.uint8, device=dev); fix[:2] = 0
    return torch.from_numpy(R).to(dev), torch.from_numpy(t).to(dev), fix


def pose_error(R, t, s):
    """(largest rotation angle in radians, largest |t - t_true|) against the generator's poses"""
    import torch
    dR = R @ s["R"].transpose(1, 2)
    ang = torch.acos(((dR.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1))
    return float(ang.max().item()), float((t - s["t"]).norm(dim=1).max().item())


def torch_route(to, obs, oi, nt, no, k, cams, R, t, X, keep, fix, max_trials=20, ftol=1e-12):
    """what a caller writes today: the same LM, every image padded to the longest.  Returns (R, t, cost [n, 2])"""
    import torch
    dev = obs.device; n = len(cams)
    n_t = int(nt.item()); n_o = int(no.item())                          # the second host synchronisation of the pipeline
    lens = to[1:n_t + 1] - to[:n_t]
    trk = torch.repeat_interleave(torch.arange(n_t, device=dev), lens)
    pos = torch.arange(n_o, device=dev) + to[0]
    im = oi[pos].long(); row = obs[pos].long()
    used = (im >= 0) & (im < n) & (row >= 0) & keep[pos].bool() & torch.isfinite(X[trk]).all(1)
    pos, im, row, trk = pos[used], im[used], row[used], trk[used]
    order = torch.sort(im, stable=True).indices
    im, row, trk = im[order], row[order], trk[order]
    cnt = torch.bincount(im, minlength=n); Lm = int(cnt.max().item()); start = torch.cumsum(cnt, 0) - cnt
    ar = torch.arange(Lm, device=dev)[None, :]
    use = ar < cnt[:, None]; idx = (start[:, None] + ar).clamp(max=len(im) - 1)
    xy = k[row[idx]][..., :2]; Xp = X[trk[idx]]; w8 = use.to(torch.float64)
    fx, fy, cx, cy = (cams[:, i:i + 1] for i in range(4))

    def sums(R, t):
        P = torch.einsum("nij,nlj->nli", R, Xp); Xc = P + t[:, None, :]; z = Xc[..., 2]
        u, v = Xc[..., 0] / z, Xc[..., 1] / z
        r = torch.stack([fx * u + cx - xy[..., 0], fy * v + cy - xy[..., 1]], -1) * w8[..., None]
        ax, ex, ay, ey = fx / z, fx * u / z, fy / z, fy * v / z; zero = torch.zeros_like(ax)
        Jx = torch.stack([-ex * P[..., 1], ax * P[..., 2] + ex * P[..., 0], -ax * P[..., 1], ax, zero, -ex], -1)
        Jy = torch.stack([-(ay * P[..., 2] + ey * P[..., 1]), ey * P[..., 0], ay * P[..., 0], zero, ay, -ey], -1)
        J = torch.stack([Jx, Jy], -2) * w8[..., None, None]
        return (r * r).sum((1, 2)), torch.einsum("nlki,nlkj->nij", J, J), torch.einsum("nlki,nlk->ni", J, r), (use & ~(z > 0)).sum(1)

    cost, A, g, behind = sums(R, t)
    cost0 = cost.clone()
    run = (cnt >= 3) & torch.isfinite(cost) & (behind == 0) & fix.bool()
    lam = torch.full((n,), 1e-3, dtype=torch.float64, device=dev)
    eye = torch.eye(6, dtype=torch.float64, device=dev); I3 = torch.eye(3, dtype=torch.float64, device=dev)
    for _ in range(max_trials):
        Mx = A + torch.diag_embed(lam[:, None] * A.diagonal(dim1=1, dim2=2))
        L, bad = torch.linalg.cholesky_ex(torch.where(run[:, None, None], Mx, eye))
        dl = torch.cholesky_solve(-g[..., None], L)[..., 0]
        a = 0.5 * dl[:, :3]
        S = torch.zeros((n, 3, 3), dtype=torch.float64, device=dev)
        S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
        Cm = torch.linalg.solve(I3 - S, I3 + S)                        # the Cayley rotation of w = 2 a
        R2 = Cm @ R; t2 = t + dl[:, 3:]
        cn, An, gn, bn = sums(R2, t2)
        acc = run & (bad == 0) & (cn < cost) & (bn == 0)
        done = acc & ((cost - cn) <= ftol * cost)
        R = torch.where(acc[:, None, None], R2, R); t = torch.where(acc[:, None], t2, t)
        A = torch.where(acc[:, None, None], An, A); g = torch.where(acc[:, None], gn, g); cost = torch.where(acc, cn, cost)
        lam = torch.where(acc, (lam / 10).clamp(min=1e-12), lam * 10)
        run = run & ~done & (lam <= 1e12)
    torch.cuda.synchronize()
    return R, t, torch.stack([cost0, cost], 1)


def setup(dev, small, rot=ROT, trans=TRANS):
    from pydegensac_amd import tensor_api
    s = gtri.scene(dev, small)
    R0, t0, fix = perturbed(s, rot, trans)
    tri = lambda R, t: tensor_api.triangulate_tracks_tensors(s["to"], s["obs"], s["oi"], s["k"], s["cams"], R, t, n_tracks=s["nt"], with_obs=True,   # noqa: E731
                                                                max_reproj_px=TRI_PX)
    X, _, _, _, _, ok, _ = tri(R0, t0)
    return s, R0, t0, fix, X, ok, tri


def c_entry(s, R0, t0, fix, X, ok):
    """the C entry point on buffers allocated before: a callable"""
    import torch
    from pydegensac_amd import _lib
    dev = s["obs"].device
    T = len(s["to"]) - 1; M = len(s["obs"]); m = len(s["cams"])
    xy = s["k"][:, :2].contiguous(); poses = torch.cat([R0.reshape(m, 9), t0], 1).contiguous(); okb = ok.view(torch.uint8)
    out = torch.empty((m, 12), dtype=torch.float64, device=dev); cost = torch.empty((m, 2), dtype=torch.float64, device=dev)
    info = torch.empty((m, 4), dtype=torch.int32, device=dev)
    L = _lib.lib(); st = torch.cuda.current_stream(dev)

    def fn():
        _lib.check_match(L.mi_degensac_camera_refine_tracks_dev(s["to"].data_ptr(), s["obs"].data_ptr(), s["oi"].data_ptr(), s["nt"].data_ptr(), xy.data_ptr(),
                                                                len(xy), s["cams"].data_ptr(), poses.data_ptr(), m, X.data_ptr(), okb.data_ptr(),
                                                                fix.data_ptr(), T, M, 20, 1e-12, 0, C.c_void_p(st.cuda_stream), out.data_ptr(),
                                                                cost.data_ptr(), info.data_ptr(), None, None, None))
    return fn


def child_refine(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import _lib, tensor_api
    dev = torch.device("cuda", 0)
    s, R0, t0, fix, X, ok, tri = setup(dev, small)
    call = lambda **kw: tensor_api.refine_cameras_tensors(s["to"], s["obs"], s["oi"], s["k"], s["cams"], R0, t0, X, n_tracks=s["nt"], obs_keep=ok,   # noqa: E731
                                                          refine=fix, **kw)
    L = _lib.lib()
    r = {"tile": [L.mi_degensac_camera_refine_tile(i) for i in range(3)], "pairs": s["pairs"], "tracks": int(s["nt"].item()), "obs": int(s["no"].item()),
         "T": len(s["to"]) - 1, "M": len(s["obs"]), "images": len(s["cams"])}
    r["entry_ms"] = gc.events(c_entry(s, R0, t0, fix, X, ok), reps)
    r["call_ms"] = gc.events(call, reps); r["call_all_ms"] = gc.events(lambda: call(with_err=True, with_table=True), reps)
    r["call_wall_ms"] = gc.wall(call, reps)
    R1, t1, cost, info = call()
    ih = info.cpu().numpy()
    r["used"] = [int(ih[:, 0].min()), float(np.median(ih[:, 0])), int(ih[:, 0].max())]
    r["status"] = np.bincount(ih[:, 3], minlength=9).tolist(); r["trials"] = int(ih[:, 1].sum()); r["accepted"] = int(ih[:, 2].sum())
    r["cost"] = [float(cost[:, 0].nansum().item()), float(cost[:, 1].nansum().item())]
    r["err0"] = pose_error(R0, t0, s); r["err1"] = pose_error(R1, t1, s)
    X2, _, _, _, _, ok2, _ = tri(R1, t1)
    R2, t2, cost2, _ = tensor_api.refine_cameras_tensors(s["to"], s["obs"], s["oi"], s["k"], s["cams"], R1, t1, X2, n_tracks=s["nt"], obs_keep=ok2, refine=fix)
    r["cost2"] = [float(cost2[:, 0].nansum().item()), float(cost2[:, 1].nansum().item())]; r["err2"] = pose_error(R2, t2, s)
    today = lambda: torch_route(s["to"], s["obs"], s["oi"], s["nt"], s["no"], s["k"], s["cams"], R0, t0, X, ok, fix)          # noqa: E731
    r["today_ms"] = gc.wall(today, reps)
    Rt, tt, ct = today()
    r["today_pose_diff"] = [float((Rt - R1).abs().max().item()), float((tt - t1).abs().max().item())]
    ran = torch.isfinite(cost[:, 1])
    r["today_cost_rel"] = float(((ct[:, 1] - cost[:, 1]).abs() / cost[:, 1].abs().clamp(min=1e-300))[ran].max().item())
    print(json.dumps(r), flush=True)


def child_loop(reps, small):
    """the C entry point reps times, for a rocprofv3 run"""
    import torch
    s, R0, t0, fix, X, ok, _ = setup(torch.device("cuda", 0), small)
    fn = c_entry(s, R0, t0, fix, X, ok)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    print(json.dumps({"calls": reps}), flush=True)


def child_untouched(reps, small):
    import torch
    from pydegensac_amd import tensor_api
    dev = torch.device("cuda", 0)
    s = gtri.scene(dev, small)
    rows, total, c, _ = gtri.gt.edges(dev, small)
    tri = lambda: tensor_api.triangulate_tracks_tensors(s["to"], s["obs"], s["oi"], s["k"], s["cams"], s["R"], s["t"], n_tracks=s["nt"], with_obs=True)   # noqa: E731
    r = {"tri_ms": gc.wall(tri, reps), "tracks_ms": gc.wall(lambda: tensor_api.tracks_tensors(rows, c, total=total), reps)}
    X = tri()[0]
    r["checksum"] = [float(torch.nan_to_num(X).abs().sum().item()), int(s["nt"].item()), int(s["no"].item())]
    print(json.dumps(r), flush=True)


def kernel_lines(path, calls):
    """the kernels of the call (cr_* and the sort's) from a rocprofv3 kernel_stats csv of --child loop: name, launches per call, us per call"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "cr_" in name or "rocprim" in name or "radix" in name or "onesweep" in name:
                rows.append((name[:70], int(r["Calls"]) / calls, float(r["TotalDurationNs"]) / calls / 1e3))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--stats-calls", type=int, default=7)
    ap.add_argument("--log", default=None)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return {"refine": child_refine, "loop": child_loop, "untouched": child_untouched}[a.child](a.reps, a.small)
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
    r = run_child("refine")
    names = ["CONVERGED", "STALLED", "MAX_TRIALS", "FIXED", "BEHIND", "NOT_FINITE", "SHORT", "BAD_POSE", "BAD_CAMERA"]
    say(f"# refinement of camera poses against triangulated tracks; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"row-pass step {r['tile'][0]}, grid cap {r['tile'][1]}, {r['tile'][2]} lanes per track in mark; {r['pairs']} pairs, {r['images']} images, "
        f"{r['tracks']} tracks, {r['obs']} observations; tables T = {r['T']}, M = {r['M']}")
    say(f"poses: the generator's, perturbed by {ROT} rad about a random axis and {TRANS} in t (depth 4 .. 8); cameras 0 and 1 held; obs_keep = the triangulation's ok at max_reproj_px = {TRI_PX}")
    say(f"used observations per image: min {r['used'][0]} median {r['used'][1]:.0f} max {r['used'][2]}; statuses "
        + ", ".join(f"{n} {c}" for n, c in zip(names, r["status"]) if c) + f"; trials in all {r['trials']}, accepted {r['accepted']}")
    say(f"C entry alone (buffers allocated before; fill, mark, sort, bounds, refine and the stream-ordered block), HIP events: {fmt(r['entry_ms'])}")
    say(f"tensor call, HIP events (with the wrapper's slice, cat, allocations): {fmt(r['call_ms'])}   with err and the table {fmt(r['call_all_ms'])}")
    say(f"tensor call, wall, synchronised: {fmt(r['call_wall_ms'])}")
    passes = r["images"] + r["trials"]
    say(f"bound: {passes} dependent passes of at most {r['used'][2]} observations on {min(r['images'], r['tile'][1])} workgroups, each pass two levels of "
        f"gathers and a barrier pair: latency, not bandwidth ({r['obs'] * 60 / 1e6:.1f} MB of tables and points stay in the caches)")
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        say(f"## kernels of one call (rocprofv3 --kernel-trace --stats over {a.stats_calls} calls of the C entry)")
        for name, calls, us in kernel_lines(a.kernel_stats, a.stats_calls):
            say(f"{us:10.1f} us  x{calls:4.1f}  {name}")
    else:
        say("## kernels of one call: not measured (no --kernel-stats)")
    say("## today: n_obs and n_tracks to the host, a stable sort by image, images padded to the longest, the same LM as batched float64 torch expressions (wall, synchronised)")
    say(f"today {fmt(r['today_ms'])}   the tensor call, wall {fmt(r['call_wall_ms'])}   {np.median(r['today_ms']) / np.median(r['call_wall_ms']):.0f}x")
    say(f"poses agree to {r['today_pose_diff'][0]:.3g} (R) and {r['today_pose_diff'][1]:.3g} (t), end costs to {r['today_cost_rel']:.3g} relative")
    say("## cost (px^2, summed over the images) and pose error against synthetic.collection_cameras (largest angle in rad, largest |t - t_true|)")
    say(f"start            : cost {r['cost'][0]:.1f}   angle {r['err0'][0]:.6f}  t {r['err0'][1]:.6f}")
    say(f"after one call   : cost {r['cost'][1]:.1f}   angle {r['err1'][0]:.6f}  t {r['err1'][1]:.6f}")
    say(f"after re-triangulation and a second call: cost {r['cost2'][0]:.1f} -> {r['cost2'][1]:.1f}   angle {r['err2'][0]:.6f}  t {r['err2'][1]:.6f}")
    if a.parent_lib:
        say("## untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = []
        for _ in range(2):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                x = gc.run_child("untouched", a.reps, a.small, lib); y = run_child("untouched", lib)
                x["tri_ms"] = y["tri_ms"]; x["tracks_ms"] = y["tracks_ms"]; x["checksum"] = x["checksum"] + y["checksum"]
                runs.append((who, x))
        for key, name in (("mv_ms", "match_and_verify_pairs_tensors F"), ("tracks_ms", "tracks_tensors"), ("tri_ms", "triangulate_tracks_tensors")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (model, tracks and point checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
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
