"""FGINN inside the gate of guided matching (tensor_api.guided_match_pairs_tensors(fginn_th=)) against the plain guided call of the same
commit, and the plain call against the parent commit's.  Workload: M = 65 images x 2000 keypoints x dim 128 (synthetic.image_collection),
matcher.exhaustive_pairs(65) = 2080 pairs, F models from match_and_verify_pairs_tensors, guided with the estimator's defaults (px_th 0.5,
Sampson, ratio 0.9); float32 under L2 and uint8 under norm l2_u8.  A share of every image's keypoints is TWINNED: the last share of its
rows become twins of its first rows (1.5 px beside them, a near-equal descriptor), as a detector emits for a second orientation.
  new call  fginn_th = 10 with 0 %, 10 % and 50 % twinned, alternating with the plain call on the same input: medians with [min..max], the
            needy queries (plain slot 1 exists and lies inside the radius of slot 0, counted from the plain call's output) and their
            needy x n_t gate tests, guided matches per pair of both calls
  memory    torch.cuda.max_memory_allocated of both calls
  parent    with --parent-lib (a libmi_degensac.so built from the parent commit, loaded through MI_DEGENSAC_LIB in a child process of its
            own) guided_match_pairs_tensors(fginn_th=None) of the parent and of this commit on the same untwinned input, alternating child
            processes; this commit's median is placed against the parent's [min..max]
usage: gpu_guided_fginn.py [--images M] [--rows N] [--reps R] [--parent-lib FILE] [--log FILE]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pydegensac_amd import matcher, parallel, synthetic as syn, tensor_api

DIM = 128
R = 10.0


def collection(m, n, u8, share):
    kps, descs = syn.image_collection(m, n, 0.5, 0.1, DIM, seed=0)
    rng = np.random.default_rng(1)
    t = int(round(n * share / 2))                           # t rows get a twin: 2 t of n keypoints are twinned
    for k, d in zip(kps, descs):
        if t:
            k[n - t:] = k[:t] + np.array([1.5, 0.0])
            d[n - t:] = d[:t] + 0.002 * rng.normal(size=(t, DIM)).astype(np.float32)
    if u8:                                                  # quantised as SIFT-like bytes: 0 .. 255 around 128
        descs = [np.clip(np.rint(128 + 40 * d), 0, 255).astype(np.uint8) for d in descs]
    return kps, descs


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def peak(fn, dev):
    torch.cuda.synchronize(dev); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn(); torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev), base


def fmt(v):
    return f"{np.median(v):8.2f} ms [{min(v):.2f}..{max(v):.2f}]"


def side(v, ref):
    m = np.median(v)
    return "inside" if min(ref) <= m <= max(ref) else ("BELOW it (faster)" if m < min(ref) else "ABOVE it (slower)")


def child(a):
    """the plain guided pair-list call of whatever library MI_DEGENSAC_LIB names: one JSON line of per-call times"""
    dev = torch.device("cuda", 0)
    M, N = a.images, a.rows
    pairs = matcher.exhaustive_pairs(M)
    kps, descs = collection(M, N, a.u8, 0.0)
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F = torch.from_numpy(np.load(a.child)).to(dev)
    kw = dict(model="F", norm="l2_u8" if a.u8 else None, driver_form=True, fginn_th=None)

    def call():
        return tensor_api.guided_match_pairs_tensors(k, k, d, d, [N] * M, [N] * M, pairs, F, **kw)
    call(); call(); torch.cuda.synchronize()
    t = [timed(call)[0] for _ in range(a.reps)]
    m = call()[0]
    print(json.dumps({"ms": t, "matches": int((m >= 0).sum().item()), "sum": int(m.to(torch.int64).sum().item())}), flush=True)


def run_child(a, u8, model_file, lib):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    else:
        env.pop("MI_DEGENSAC_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--images", str(a.images), "--rows", str(a.rows), "--reps", str(a.reps), "--child", model_file]
    cmd += ["--u8"] if u8 else []
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"child process failed ({out.returncode}): {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=65)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--u8", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    dev = torch.device("cuda", 0)
    M, N = a.images, a.rows
    pairs = matcher.exhaustive_pairs(M); K = len(pairs)
    seeds = parallel.pair_seeds(0, K)
    counts = [N] * M
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    say(f"# {torch.cuda.get_device_name(0)}; {M} images x {N} x {DIM}, exhaustive_pairs({M}) = {K} pairs, F models from "
        f"match_and_verify_pairs_tensors, guided px_th 0.5 Sampson ratio 0.9, fginn_th {R}; HIP events around each call, {a.reps} alternating "
        f"calls after two warm-ups of each")
    for u8 in (False, True):
        norm = "l2_u8" if u8 else None
        say(f"## {'uint8 under l2_u8' if u8 else 'float32 under L2'}")
        for share in (0.0, 0.1, 0.5):
            kps, descs = collection(M, N, u8, share)
            k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
            F = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.9, seeds=seeds, norm=norm)[0].contiguous()
            kw = dict(model="F", norm=norm, driver_form=True)

            def plain():
                return tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, **kw)

            def new():
                return tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, fginn_th=R, **kw)
            p_pl, base = peak(plain, dev)
            p_nw, _ = peak(new, dev)
            for _ in range(2):
                A = plain(); B = new()
            torch.cuda.synchronize()
            # the needy queries, from the plain call's output: slot 1 exists and its keypoint lies inside the radius of slot 0's
            j = torch.from_numpy(np.repeat(pairs[:, 1], N)).to(dev) * N
            i0, i1 = A[1][:, 0].long(), A[1][:, 1].long()
            both = (i0 >= 0) & (i1 >= 0)
            dxy = k[(j + i1.clamp(min=0))] - k[(j + i0.clamp(min=0))]
            needy = int((both & ~((dxy * dxy).sum(1) >= R * R)).sum().item())
            same0 = torch.equal(A[1][:, 0], B[1][:, 0])
            t_pl, t_nw = [], []
            for _ in range(a.reps):
                t_pl.append(timed(plain)[0]); t_nw.append(timed(new)[0])
            extra = np.median(t_nw) - np.median(t_pl)
            say(f"   {100 * share:3.0f} % twinned: plain {fmt(t_pl)}   fginn_th={R:g} {fmt(t_nw)}   extra {extra:+.2f} ms "
                f"({100 * extra / np.median(t_pl):+.1f} %); needy queries {needy} of {K * N} ({100 * needy / (K * N):.2f} %) = {needy * N / 1e6:.1f} M "
                f"gate tests, {1e3 * extra / max(needy * N / 1e6, 1e-9):.2f} us per M tests; guided matches/pair plain {int((A[0] >= 0).sum()) / K:.0f}, "
                f"new {int((B[0] >= 0).sum()) / K:.0f}; slot 0 identical: {same0}")
            say(f"                 torch.cuda.max_memory_allocated: plain {p_pl / 1e6:.1f} MB, new {p_nw / 1e6:.1f} MB (stores and models "
                f"allocated before either call: {base / 1e6:.1f} MB)")
            if a.parent_lib and share == 0.0:
                n_match = int((A[0] >= 0).sum().item()); m_sum = int(A[0].to(torch.int64).sum().item())
                with tempfile.TemporaryDirectory() as tmp:
                    mf = os.path.join(tmp, "models.npy")
                    np.save(mf, F.cpu().numpy())
                    runs = [run_child(a, u8, mf, lib) for lib in (a.parent_lib, None, a.parent_lib, None)]
                t_par = runs[0]["ms"] + runs[2]["ms"]; t_new = runs[1]["ms"] + runs[3]["ms"]
                ok = all(r["matches"] == n_match and r["sum"] == m_sum for r in runs)
                say(f"   the untouched call, guided_match_pairs_tensors(fginn_th=None) on the untwinned input (child processes parent / this / "
                    f"parent / this, {a.reps} calls each):")
                say(f"                 parent {fmt(t_par)}   this commit {fmt(t_new)}  ({100 * (np.median(t_new) / np.median(t_par) - 1):+.1f} % of the "
                    f"parent's median; against the parent's [min..max]: {side(t_new, t_par)}); match counts and sums equal in every process: {ok}")
            del k, d, F, A, B
            torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
