"""Triangulation of tracks under known camera poses on the device (mi_degensac_triangulate_tracks_dev,
tensor_api.triangulate_tracks_tensors): what it costs, what a caller writes today for the same rule, 16 against 64 lanes per track, how
good the points are, and that the calls next to it are untouched.  One MI355X; medians over --reps calls with [min..max] after two
warm-up calls.  The 65 x 2000 x 128 collection of synthetic.image_collection and the 2080 pairs of exhaustive_pairs(65): verify ->
export (store rows) -> tracks, then the generator's cameras.
  call        the tensor call by HIP events and by wall time, with and without the per-observation outputs.  The events cover what the
              wrapper enqueues besides the kernel (the slice of kps, the cat of R and t, the output allocations, three fills); the
              kernel with its fills alone is measured through the C entry point on buffers allocated before
  bound       bytes counted from the shapes over the kernel's time against the HBM bandwidth
  today       read n_obs and n_tracks (a host synchronisation), pad the tracks to the longest, the same rule as batched float64 tensor
              expressions, one more synchronisation at the end; wall time; how far its points lie from the call's
  G           the product build (16 lanes per track) against --g64-lib (the same code with 64), each in a child process of its own, on
              the collection and on a second scene of the same observations cut into tracks of 2 .. 5 on the host
  accuracy    statuses, median and maximum error against synthetic.collection_truth at the linear point and after the refinement
  untouched   match_and_verify_pairs_tensors (F), guided_match_pairs_tensors, tracks_tensors and relative_pose_tensors on the same store
              and bench.py, this build against --parent-lib (a libmi_degensac.so of the parent commit), each in a child process of its
              own, two alternating passes
usage: gpu_triangulate.py [--reps R] [--parent-lib PATH] [--g64-lib PATH] [--log FILE] [--small]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_correspond as gc          # noqa: E402  (events, wall, store and the "untouched" child)
import gpu_pose as gp                # noqa: E402  (the "pose" child)
import gpu_tracks as gt              # noqa: E402  (the edge list of the export)

HBM_GBS = 8000.0                     # MI355X, the figure bench.py uses for its roofline


def scene(dev, small):
    """(tables of tracks_tensors, kps, cams, R, t, truth [n_tracks, 3] with NaN where a track is not one cloud point seen once per image)"""
    import numpy as np
    import torch
    from pydegensac_amd import synthetic, tensor_api
    rows, total, c, K = gt.edges(dev, small)
    m, n = len(c), c[0]
    k = gc.store(dev, small)[0]
    track, nt, to, obs, oi, ti, no = tensor_api.tracks_tensors(rows, c, total=total)
    Kc, poses = synthetic.collection_cameras(m)
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * m, dtype=torch.float64, device=dev)
    R = torch.from_numpy(np.stack([p[0] for p in poses])).to(dev); t = torch.from_numpy(np.stack([p[1] for p in poses])).to(dev)
    cloud, point, _ = synthetic.collection_truth(m, n, 0.6, 0.1, gc.DIM, seed=0)
    pt = np.concatenate(point); n_t = int(nt.item())
    o_h = obs.cpu().numpy(); off = to.cpu().numpy(); ti_h = ti.cpu().numpy()
    truth = np.full((n_t, 3), np.nan)
    for j in range(n_t):
        ids = pt[o_h[off[j]:off[j + 1]]]
        if ti_h[j] == len(ids) and ids[0] >= 0 and (ids == ids[0]).all():
            truth[j] = cloud[ids[0]]
    return dict(to=to, obs=obs, oi=oi, nt=nt, no=no, k=k, cams=cams, R=R, t=t, truth=truth, pairs=K)


def split_tracks(to, nt):
    """the same observations cut into tracks of 2 .. 5 on the host: every track in pieces of 2, 3, 4, 5, 2, .. observations, a last single
    one joined to the piece before it.  Returns (track_offsets of the same length as `to`, n_tracks [1]) on the device of `to`."""
    import numpy as np
    import torch
    off = to.cpu().numpy(); n_t = int(nt.item())
    cuts = [int(off[0])]; turn = 0
    for j in range(n_t):
        b, e = int(off[j]), int(off[j + 1])
        while b < e:
            step = 2 + turn % 4; turn += 1
            nb = e if e - (b + step) < 2 else b + step
            cuts.append(nb); b = nb
    assert len(cuts) <= len(off), "tracks of at least two observations cannot outnumber half the rows"
    out = np.full(len(off), cuts[-1], np.int64); out[:len(cuts)] = cuts
    return torch.from_numpy(out).to(to.device), torch.tensor([len(cuts) - 1], dtype=torch.int64, device=to.device)


def torch_route(to, obs, oi, nt, no, k, cams, R, t, min_angle_deg=1.5, max_reproj_px=4.0, max_iters=10, ftol=1e-12):
    """what a caller writes today: the same rule, every track padded to the longest.  Returns (X [n_tracks, 3], cost [n_tracks, 2], ok counts,
    cosang)"""
    import math
    import torch
    dev = obs.device
    n_t = int(nt.item()); n_o = int(no.item())                          # the second host synchronisation of the pipeline
    off = to[:n_t + 1]; lens = off[1:] - off[:-1]; Lm = int(lens.max().item())
    ar = torch.arange(Lm, device=dev)[None, :]
    idx = (off[:-1, None] + ar).clamp(max=max(n_o - 1, 0))
    use = ar < lens[:, None]
    im = oi[idx].long().clamp(min=0); row = obs[idx].long().clamp(min=0)
    xy = k[row][..., :2]; cm = cams[im]; Rm = R[im]; tm = t[im]         # [T, L, ..], ragged tracks as padded tensors
    w8 = use.to(torch.float64)
    d = torch.stack([(xy[..., 0] - cm[..., 2]) / cm[..., 0], (xy[..., 1] - cm[..., 3]) / cm[..., 1], torch.ones_like(xy[..., 0])], -1)
    w = torch.einsum("tlij,tli->tlj", Rm, d); w = w / w.norm(dim=-1, keepdim=True)
    c = -torch.einsum("tlij,tli->tlj", Rm, tm)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    P = (eye - w[..., :, None] * w[..., None, :]) * w8[..., None, None]
    A = P.sum(1); b = (P @ c[..., None])[..., 0].sum(1)
    L, bad = torch.linalg.cholesky_ex(A)
    X = torch.cholesky_solve(b[..., None], L)[..., 0]
    live = (bad == 0) & torch.isfinite(X).all(1) & (use.sum(1) >= 2)

    def sums(X):
        Xc = torch.einsum("tlij,tj->tli", Rm, X) + tm
        z = Xc[..., 2]
        r = torch.stack([cm[..., 0] * Xc[..., 0] / z + cm[..., 2] - xy[..., 0], cm[..., 1] * Xc[..., 1] / z + cm[..., 3] - xy[..., 1]], -1)
        Jx = (cm[..., 0] / z)[..., None] * Rm[..., 0, :] - (cm[..., 0] * Xc[..., 0] / (z * z))[..., None] * Rm[..., 2, :]
        Jy = (cm[..., 1] / z)[..., None] * Rm[..., 1, :] - (cm[..., 1] * Xc[..., 1] / (z * z))[..., None] * Rm[..., 2, :]
        J = torch.stack([Jx, Jy], -2) * w8[..., None, None]            # [T, L, 2, 3]
        r = torch.where(use[..., None], r, torch.zeros_like(r))
        return (r * r).sum((1, 2)), torch.einsum("tlki,tlkj->tij", J, J), torch.einsum("tlki,tlk->ti", J, r), r, z

    cost, H, g, r, z = sums(X)
    cost0 = cost.clone()
    run = live.clone()
    for _ in range(max_iters):
        Lc, bad = torch.linalg.cholesky_ex(torch.where(run[:, None, None], H, eye))
        Z = X - torch.cholesky_solve(g[..., None], Lc)[..., 0]
        cn, Hn, gn, _, _ = sums(Z)
        acc = run & (bad == 0) & torch.isfinite(cn) & (cn < cost)
        done = acc & ((cost - cn) <= ftol * cost)
        X = torch.where(acc[:, None], Z, X); H = torch.where(acc[:, None, None], Hn, H); g = torch.where(acc[:, None], gn, g)
        cost = torch.where(acc, cn, cost)
        run = acc & ~done
    _, _, _, r, z = sums(X)
    ok = use & (z > 0) & (r.norm(dim=-1) <= max_reproj_px)
    dots = torch.einsum("tli,tmi->tlm", w, w)
    pair = use[:, :, None] & use[:, None, :] & ~torch.eye(Lm, dtype=torch.bool, device=dev)[None]
    cosang = torch.where(pair, dots, torch.full_like(dots, float("inf"))).flatten(1).min(1).values
    narrow = cosang > math.cos(math.radians(min_angle_deg))
    nan = torch.full_like(X, float("nan"))
    out = (torch.where(live[:, None], X, nan), torch.stack([cost0, cost], 1), ok.sum(1), cosang, narrow)
    torch.cuda.synchronize()
    return out


def kernel_alone(s, to, nt, reps, with_obs):
    """the C entry point on buffers allocated before: the kernel and the three fills of the per-observation outputs, HIP events"""
    import torch
    from pydegensac_amd import _lib
    dev = s["obs"].device
    T = len(to) - 1; M = len(s["obs"]); m = len(s["cams"])
    xy = s["k"][:, :2].contiguous(); poses = torch.cat([s["R"].reshape(m, 9), s["t"]], 1).contiguous()
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)          # noqa: E731
    X, cost, ca = f64(T, 3), f64(T, 2), f64(T); info = torch.empty((T, 5), dtype=torch.int32, device=dev)
    err, depth = f64(M), f64(M); ok = torch.empty(M, dtype=torch.uint8, device=dev)
    p = lambda x: x.data_ptr() if with_obs else None                   # noqa: E731
    L = _lib.lib(); st = torch.cuda.current_stream(dev)

    def fn():
        _lib.check_match(L.mi_degensac_triangulate_tracks_dev(to.data_ptr(), s["obs"].data_ptr(), s["oi"].data_ptr(), nt.data_ptr(), xy.data_ptr(),
                                                              len(xy), s["cams"].data_ptr(), poses.data_ptr(), m, T, M, 1.5, 4.0, 10, 1e-12, 0,
                                                              C.c_void_p(st.cuda_stream), X.data_ptr(), info.data_ptr(), cost.data_ptr(), ca.data_ptr(),
                                                              p(err), p(ok), p(depth)))
    return gc.events(fn, reps)


def child_tri(reps, small):
    import numpy as np
    import torch
    from pydegensac_amd import _lib, tensor_api
    dev = torch.device("cuda", 0)
    s = scene(dev, small)
    L = _lib.lib()
    res = {"G": L.mi_degensac_triangulate_tile(0), "grid": L.mi_degensac_triangulate_tile(1), "gpw": L.mi_degensac_triangulate_tile(2), "pairs": s["pairs"]}
    to2, nt2 = split_tracks(s["to"], s["nt"])
    names = ["OK", "NARROW", "DEGENERATE", "SHORT", "TRUNCATED"]
    for tag, to, nt in (("collection", s["to"], s["nt"]), ("split", to2, nt2)):
        call = lambda **kw: tensor_api.triangulate_tracks_tensors(to, s["obs"], s["oi"], s["k"], s["cams"], s["R"], s["t"], n_tracks=nt, **kw)   # noqa: E731
        n_t = int(nt.item()); n_o = int(s["no"].item())
        lens = np.diff(to.cpu().numpy()[:n_t + 1])
        r = {"tracks": n_t, "obs": n_o, "len": [int(lens.min()), float(np.median(lens)), int(lens.max())], "T": len(to) - 1, "M": len(s["obs"])}
        r["kernel_ms"] = kernel_alone(s, to, nt, reps, False); r["kernel_obs_ms"] = kernel_alone(s, to, nt, reps, True)
        r["call_ms"] = gc.events(call, reps); r["call_obs_ms"] = gc.events(lambda: call(with_obs=True), reps)
        r["call_wall_ms"] = gc.wall(call, reps); r["call_obs_wall_ms"] = gc.wall(lambda: call(with_obs=True), reps)
        X, info, cost, ca = call()
        ih = info.cpu().numpy()[:n_t]
        r["status"] = dict(zip(names, np.bincount(ih[:, 4], minlength=5).tolist()))
        r["trials"] = int(ih[:, 3].sum())
        # bytes from the shapes: per pass and observation two int32 and the keypoint from HBM once (later passes find them in the caches, as
        # the 128 bytes of camera and pose per observation always are: the table has 128 bytes per image); the offsets; the outputs
        passes = 3 * n_t + int(ih[:, 3].sum()) + n_t                   # linear, first GN pass and flags; one per trial; the staging of the pair pass
        r["passes_per_track"] = passes / max(n_t, 1)
        r["bytes_once"] = n_o * 24 + (len(to) + 1) * 8 + (len(to) - 1) * 68
        r["bytes_all_passes"] = int(n_o / max(n_t, 1) * passes) * 24 + (len(to) + 1) * 8 + (len(to) - 1) * 68
        r["X_sum"] = float(torch.nan_to_num(X[:n_t]).abs().sum().item())
        if tag == "collection":
            point = ih[:, 4] <= 1
            for name, iters in (("linear", 0), ("refined", 10)):
                Xi, ii = (x.cpu().numpy()[:n_t] for x in call(max_iters=iters)[:2])
                sel = ~np.isnan(s["truth"][:, 0]) & (ii[:, 4] == 0)
                e = np.linalg.norm(Xi[sel] - s["truth"][sel], axis=1)
                r["err_" + name] = [int(sel.sum()), float(np.median(e)), float(e.max())]
            r["today_ms"] = gc.wall(lambda: torch_route(to, s["obs"], s["oi"], nt, s["no"], s["k"], s["cams"], s["R"], s["t"]), reps)
            Xt, ct, okt, cat, nar = torch_route(to, s["obs"], s["oi"], nt, s["no"], s["k"], s["cams"], s["R"], s["t"])
            pd = torch.from_numpy(point).to(dev)
            r["today_max_point_diff"] = float((Xt - X[:n_t])[pd].abs().max().item())
            r["today_max_cost_rel"] = float(((ct - cost[:n_t]).abs() / cost[:n_t].abs().clamp(min=1e-300))[pd].max().item())
            r["today_same_ok_counts"] = bool(torch.equal(okt[pd].to(torch.int32), info[:n_t, 1][pd]))
            r["today_max_cosang_diff"] = float((cat - ca[:n_t])[pd].abs().max().item())
            r["X_head"] = X[:4].cpu().numpy().tolist()
        res[tag] = r
    print(json.dumps(res), flush=True)


def child_tracks(reps, small):
    import torch
    from pydegensac_amd import tensor_api
    rows, total, c, _ = gt.edges(torch.device("cuda", 0), small)
    ms = gc.wall(lambda: tensor_api.tracks_tensors(rows, c, total=total), reps)
    out = tensor_api.tracks_tensors(rows, c, total=total)
    print(json.dumps({"tracks_ms": ms, "checksum": [int(out[1].item()), int(out[6].item()), int(out[3].long().clamp(min=0).sum().item())]}), flush=True)


def run_child(what, reps, small, lib=None):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(reps)] + (["--small"] if small else [])
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=500).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")][-1]


def run_bench(lib=None):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=500, cwd=ROOT).stdout
    j = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")][-1]
    return j["ms_per_step"], j["mean_inliers"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--g64-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return {"tri": child_tri, "tracks": child_tracks}[a.child](a.reps, a.small)
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
    r = run_child("tri", a.reps, a.small)
    say(f"# triangulation of tracks under known poses; medians over {a.reps} calls [min..max]" + ("  (TOY SIZES: a rehearsal)" if a.small else ""))
    say(f"product build: G = {r['G']} lanes per track, {r['gpw']} tracks per workgroup, grid cap {r['grid']}; {r['pairs']} pairs")
    for tag in ("collection", "split"):
        s = r[tag]
        say(f"## scene `{tag}`: {s['tracks']} tracks, {s['obs']} observations, length min {s['len'][0]} median {s['len'][1]:.0f} max {s['len'][2]}; "
            f"tables T = {s['T']}, M = {s['M']}")
        say(f"kernel alone (C entry, buffers allocated before), HIP events: {fmt(s['kernel_ms'])}   with err / ok / depth and their fills {fmt(s['kernel_obs_ms'])}")
        say(f"tensor call, HIP events (with the wrapper's slice, cat, allocations): {fmt(s['call_ms'])}   with_obs {fmt(s['call_obs_ms'])}")
        say(f"tensor call, wall, synchronised: {fmt(s['call_wall_ms'])}   with_obs {fmt(s['call_obs_wall_ms'])}")
        say(f"statuses {s['status']}; trials in all {s['trials']}; passes over a track's observations {s['passes_per_track']:.2f} per track")
        km = float(np.median(s["kernel_ms"]))
        for name, key in (("every table read once", "bytes_once"), ("every pass read from HBM again (an upper bound: later passes hit the caches)", "bytes_all_passes")):
            gbs = s[key] / (km * 1e-3) / 1e9
            say(f"bound: {s[key] / 1e6:.2f} MB with {name}: {gbs:.1f} GB/s = {100 * gbs / HBM_GBS:.2f} % of {HBM_GBS:.0f} GB/s")
        say("bound: " + ("latency (dependent passes of a few observations per lane; far below the bandwidth either way)"
                         if s["bytes_all_passes"] / (km * 1e-3) / 1e9 < 0.5 * HBM_GBS else "bandwidth"))
    s = r["collection"]
    say("## today: n_obs and n_tracks to the host, tracks padded to the longest, the same rule as batched float64 torch expressions (wall, synchronised)")
    say(f"today {fmt(s['today_ms'])}   the tensor call, wall {fmt(s['call_wall_ms'])}   {np.median(s['today_ms']) / np.median(s['call_wall_ms']):.0f}x")
    say(f"points agree to {s['today_max_point_diff']:.3g} (largest difference of a coordinate), end costs to {s['today_max_cost_rel']:.3g} relative, "
        f"cosang to {s['today_max_cosang_diff']:.3g}; ok counts equal: {'yes' if s['today_same_ok_counts'] else 'NO'}")
    say("## accuracy against synthetic.collection_truth: consistent tracks of one cloud point with status OK (recorded, not asserted)")
    for name in ("linear", "refined"):
        e = s["err_" + name]
        say(f"{name:>8s}: {e[0]} tracks, error median {e[1]:.5f} max {e[2]:.5f}")
    if a.g64_lib:
        say("## G = 16 against 64: the kernel alone (HIP events), alternating child processes")
        runs = []
        for _ in range(2):
            for who, lib in (("G64", a.g64_lib), ("G16", None)):
                runs.append((who, run_child("tri", a.reps, a.small, lib)))
        for tag in ("collection", "split"):
            for key, name in (("kernel_ms", "X, info, cost, cosang"), ("kernel_obs_ms", "with err / ok / depth")):
                row = []
                for who in ("G16", "G64"):
                    v = [x for w, q in runs if w == who for x in q[tag][key]]
                    row.append((who, v))
                say(f"{tag:>10s}, {name:>22s}: " + "   ".join(f"G = {who[1:]} {fmt(v)}" for who, v in row)
                    + f"   64 / 16 = {np.median(row[1][1]) / np.median(row[0][1]):.2f}")
        g = {w: q for w, q in runs}
        say(f"lanes per track reported by the builds: {g['G16']['G']} and {g['G64']['G']}; statuses equal: "
            + ("yes" if all(g['G16'][t]['status'] == g['G64'][t]['status'] for t in ('collection', 'split')) else "NO")
            + f"; sum |X| {g['G16']['collection']['X_sum']:.9f} against {g['G64']['collection']['X_sum']:.9f} (another order of the sums)")
    else:
        say("## G = 16 against 64: not measured (no --g64-lib)")
    if a.parent_lib:
        say("## untouched calls: this build against a build of the parent commit, alternating, wall time of the synchronised call")
        runs = []
        for _ in range(2):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                x = gc.run_child("untouched", a.reps, a.small, lib); y = run_child("tracks", a.reps, a.small, lib); z = gp.run_child("pose", a.reps, a.small, lib)
                x["tracks_ms"] = y["tracks_ms"]; x["pose_ms"] = z["pose_wall_ms"]; x["checksum"] = x["checksum"] + y["checksum"] + [z["front"], z["wide"]]
                runs.append((who, x))
        for key, name in (("mv_ms", "match_and_verify_pairs_tensors F"), ("guided_ms", "guided_match_pairs_tensors F"), ("tracks_ms", "tracks_tensors"),
                          ("pose_ms", "relative_pose_tensors")):
            par = [v for w, x in runs if w == "parent" for v in x[key]]; new = [v for w, x in runs if w == "this" for v in x[key]]
            inside = min(par) <= np.median(new) <= max(par)
            say(f"{name:>34s}: parent {fmt(par)}  this build {fmt(new)}  median inside the parent's range: "
                f"{'yes' if inside else ('NO, below it' if np.median(new) < min(par) else 'NO, above it')}")
        say("results equal (model, guided-match, tracks and pose checksums): " + ("yes" if len({json.dumps(x["checksum"]) for _, x in runs}) == 1 else "NO"))
        if not a.small:
            say("## bench.py --gpus 1 --steps 5 --warmup 2, ms per step, alternating")
            b = [(who, run_bench(lib)) for _ in range(2) for who, lib in (("parent", a.parent_lib), ("this", None))]
            par = [v[0] for w, v in b if w == "parent"]; new = [v[0] for w, v in b if w == "this"]
            say(f"parent {par[0]:.2f}, {par[1]:.2f}   this build {new[0]:.2f}, {new[1]:.2f}   mean inliers equal: "
                + ("yes" if len({v[1] for _, v in b}) == 1 else "NO"))
    else:
        say("## untouched calls and bench.py: not measured (no --parent-lib)")


if __name__ == "__main__":
    main()
