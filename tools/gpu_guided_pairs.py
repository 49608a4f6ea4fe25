"""Guided matching over a pair list (tensor_api.guided_match_pairs_tensors: descriptors and keypoints stored once per image, one model per
list entry) against guided_match_batch_tensors on the duplicated tensors (every entry's rows copied out of the stores: the path a caller
had before).  Workload: a collection of M = 65 images x 2000 keypoints x dim 128 (synthetic.image_collection), matcher.exhaustive_pairs(65)
= 2080 pairs, F models from match_and_verify_pairs_tensors, guided with the estimator's defaults (px_th 0.5, Sampson, ratio 0.9); as
float32 under L2 and as uint8 under norm l2_u8.
  memory    torch.cuda.max_memory_allocated of the pair-list call against the batched call on duplicated tensors (the device gather that
            builds them included), next to the descriptor bytes the shapes give (M n row against 2 K n row)
  time      the two calls alternate, HIP events around each call after a warm-up of both; medians with [min..max]; the duplicated form is
            timed with its tensors already on the device.  Outputs are checked for identity.
  parent    with --parent-lib (a libmi_degensac.so built from the parent commit, loaded through MI_DEGENSAC_LIB in a child process of its
            own) the ragged guided_match_batch_tensors of the parent on the same duplicated input and models, alternating child
            processes parent / this commit; both medians of this commit are then placed against the PARENT's [min..max].  The two forms do
            the same kernel work on different addresses: the stores of the pair list are M n rows that the caches can hold, the
            duplicated tensors 2 K n rows that they cannot
usage: gpu_guided_pairs.py [--images M] [--rows N] [--reps R] [--mutual] [--parent-lib FILE] [--log FILE]"""
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


def collection(m, n, u8):
    kps, descs = syn.image_collection(m, n, 0.5, 0.1, DIM, seed=0)
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
    """where the median of v lies against the [min..max] of ref"""
    m = np.median(v)
    return "inside" if min(ref) <= m <= max(ref) else ("BELOW it (faster)" if m < min(ref) else "ABOVE it (slower)")


def rows_of(pairs, N, dev):
    i_rows = torch.from_numpy((pairs[:, 0, None] * N + np.arange(N)[None]).ravel()).to(dev)
    j_rows = torch.from_numpy((pairs[:, 1, None] * N + np.arange(N)[None]).ravel()).to(dev)
    return i_rows, j_rows


def child(a):
    """the ragged call of whatever library MI_DEGENSAC_LIB names, on the duplicated input: one JSON line of per-call times"""
    dev = torch.device("cuda", 0)
    M, N = a.images, a.rows
    pairs = matcher.exhaustive_pairs(M); K = len(pairs)
    kps, descs = collection(M, N, a.u8)
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    i_rows, j_rows = rows_of(pairs, N, dev)
    k1, k2, d1, d2 = k[i_rows], k[j_rows], d[i_rows], d[j_rows]
    F = torch.from_numpy(np.load(a.child)).to(dev)
    kw = dict(model="F", mutual=a.mutual, norm="l2_u8" if a.u8 else None, driver_form=True)

    def call():
        return tensor_api.guided_match_batch_tensors(k1, k2, d1, d2, [N] * K, [N] * K, F, **kw)
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
    cmd += (["--u8"] if u8 else []) + (["--mutual"] if a.mutual else [])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"child process failed ({out.returncode}): {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=65)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--mutual", action="store_true")
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
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    say(f"# {torch.cuda.get_device_name(0)}; {M} images x {N} x {DIM}, exhaustive_pairs({M}) = {K} pairs, F models from "
        f"match_and_verify_pairs_tensors, guided px_th 0.5 Sampson ratio 0.9 mutual={a.mutual}; HIP events around each call, {a.reps} alternating "
        f"calls after two warm-ups of each form")
    for u8 in (False, True):
        norm = "l2_u8" if u8 else None
        row = DIM * (1 if u8 else 4)
        kps, descs = collection(M, N, u8)
        counts = [N] * M
        k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
        F = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.9, seeds=seeds, norm=norm)[0].contiguous()
        i_rows, j_rows = rows_of(pairs, N, dev)
        kw = dict(model="F", mutual=a.mutual, norm=norm, driver_form=True)

        def pair_list():
            return tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, **kw)

        def gather():
            return k[i_rows], k[j_rows], d[i_rows], d[j_rows]

        def duplicated(t=None):
            k1, k2, d1, d2 = t or gather()
            return tensor_api.guided_match_batch_tensors(k1, k2, d1, d2, [N] * K, [N] * K, F, **kw)
        say(f"## {'uint8 under l2_u8' if u8 else 'float32 under L2'}: descriptor bytes from the shapes: stores M n row = {M * N * row / 1e6:.1f} MB, "
            f"duplicated 2 K n row = {2 * K * N * row / 1e6:.1f} MB; models found for {int((F.abs().sum(dim=(1, 2)) != 0).sum().item())} of {K} pairs")
        p_pl, b_pl = peak(pair_list, dev)
        p_du, b_du = peak(duplicated, dev)
        say(f"   torch.cuda.max_memory_allocated: pair list {p_pl / 1e6:9.1f} MB, duplicated (gather + call) {p_du / 1e6:9.1f} MB "
            f"(allocated before either call, stores, models and row indices: {b_pl / 1e6:.1f} MB)")
        dup = gather()
        for _ in range(2):
            A = pair_list(); B = duplicated(dup)
        torch.cuda.synchronize()
        same = torch.equal(A[0], B[0]) and torch.equal(A[1], B[1]) and torch.equal(A[2].view(torch.int32), B[2].view(torch.int32))
        n_match = int((A[0] >= 0).sum().item()); m_sum = int(A[0].to(torch.int64).sum().item())
        t_pl, t_du = [], []
        for _ in range(a.reps):
            t_pl.append(timed(pair_list)[0]); t_du.append(timed(lambda: duplicated(dup))[0])
        say(f"   this commit:  pair list {fmt(t_pl)}   ragged batch on duplicated tensors {fmt(t_du)}   pair list vs ragged median "
            f"{100 * (np.median(t_pl) / np.median(t_du) - 1):+.1f} %; outputs identical (match, idx, dist bits): {same}; guided matches/pair {n_match / K:.0f}")
        del dup, A, B
        torch.cuda.empty_cache()
        if a.parent_lib:
            with tempfile.TemporaryDirectory() as tmp:
                mf = os.path.join(tmp, "models.npy")
                np.save(mf, F.cpu().numpy())
                runs = [run_child(a, u8, mf, lib) for lib in (a.parent_lib, None, a.parent_lib, None)]
            t_par = runs[0]["ms"] + runs[2]["ms"]; t_new = runs[1]["ms"] + runs[3]["ms"]
            ok = all(r["matches"] == n_match and r["sum"] == m_sum for r in runs)
            say(f"   parent commit, ragged batch on the same duplicated input (child processes parent / this / parent / this, {a.reps} calls each):")
            say(f"                 parent {fmt(t_par)}   this commit's ragged batch {fmt(t_new)}  ({100 * (np.median(t_new) / np.median(t_par) - 1):+.1f} % "
                f"of the parent's median; against the parent's [min..max]: {side(t_new, t_par)})")
            say(f"                 pair-list median against the parent's [min..max]: {side(t_pl, t_par)} "
                f"({100 * (np.median(t_pl) / np.median(t_par) - 1):+.1f} % of its median); match counts and sums equal in every process: {ok}")
        del k, d, i_rows, j_rows, F
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
