"""The pair-list match-and-verify (tensor_api.match_and_verify_pairs_tensors: descriptors and keypoints stored once per image) against
match_and_verify_batch_tensors on the duplicated tensors (every pair's rows copied out of the stores: the path a caller had before).
Workload: a collection of M = 65 images x 2000 keypoints x dim 128 (synthetic.image_collection), matched exhaustively:
matcher.exhaustive_pairs(65) = 2080 pairs, model F, ratio 0.9; as float32 under L2 and as uint8 under norm l2_u8.
  device tensors: the two calls alternate, each timed from the call to a synchronised stream (wall clock); the duplicated form is
                  timed with its tensors already built on the device, and once more with the device-side row gather that builds them
  numpy lists:    matcher.match_and_verify_pairs (each image uploaded once) against matcher.match_and_verify_batch on per-pair lists
                  (the copies and their upload are part of the call)
Medians with [min..max]; torch.cuda.max_memory_allocated of each form next to the descriptor bytes the shapes give (M n row against
2 K n row); the outputs of the two forms are checked for identity (the stats columns that count passes or record the placement
follow the scheduling of a 2080-pair launch and are only counted).
usage: gpu_match_pairs.py [--images M] [--rows N] [--reps R] [--host-reps R] [--log FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pydegensac_amd import matcher, parallel, synthetic as syn, tensor_api

DIM = 128
CNT = [0, 1, 3]                                            # samples, LO runs, I: what tools/gpu_match_verify.py compares
DET = [c for c in range(16) if c not in (12, 13)]          # every stats column but the device clock readings


def collection(m, n, u8):
    kps, descs = syn.image_collection(m, n, 0.5, 0.1, DIM, seed=0)
    if u8:                                                  # quantised as SIFT-like bytes: 0 .. 255 around 128
        descs = [np.clip(np.rint(128 + 40 * d), 0, 255).astype(np.uint8) for d in descs]
    return kps, descs


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter(); out = fn(); torch.cuda.current_stream(dev).synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak(fn, dev):
    torch.cuda.synchronize(dev); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn(); torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev), base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=65)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    M, N = a.images, a.rows
    pairs = matcher.exhaustive_pairs(M); K = len(pairs)
    seeds = parallel.pair_seeds(0, K)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):9.2f} ms [{min(v):.2f}..{max(v):.2f}]"
    say(f"# {torch.cuda.get_device_name(0)}; {M} images x {N} x {DIM}, exhaustive_pairs({M}) = {K} pairs, model F, ratio 0.9; wall clock from the call "
        f"to a synchronised stream, {a.reps} alternating runs after one warm-up of each form (numpy entry points: {a.host_reps})")
    for u8 in (False, True):
        norm = "l2_u8" if u8 else None
        row = DIM * (1 if u8 else 4)
        kps, descs = collection(M, N, u8)
        counts = [N] * M
        k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
        i_rows = torch.from_numpy((pairs[:, 0, None] * N + np.arange(N)[None]).ravel()).to(dev)
        j_rows = torch.from_numpy((pairs[:, 1, None] * N + np.arange(N)[None]).ravel()).to(dev)
        kw = dict(model="F", ratio=0.9, seeds=seeds, norm=norm)

        def pair_list():
            return tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, **kw)

        def gather():
            return k[i_rows], k[j_rows], d[i_rows], d[j_rows]

        def duplicated(t=None):
            k1, k2, d1, d2 = t or gather()
            return tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, [N] * K, [N] * K, **kw)
        say(f"## {'uint8 under l2_u8' if u8 else 'float32 under L2'}: descriptor bytes from the shapes: stores M n row = {M * N * row / 1e6:.1f} MB, "
            f"duplicated 2 K n row = {2 * K * N * row / 1e6:.1f} MB")
        p_pl, b_pl = peak(pair_list, dev)
        p_du, b_du = peak(duplicated, dev)
        say(f"   torch.cuda.max_memory_allocated: pair list {p_pl / 1e6:9.1f} MB, duplicated (gather + call) {p_du / 1e6:9.1f} MB "
            f"(allocated before either call, stores and row indices: {b_pl / 1e6:.1f} MB)")
        dup = gather()
        _, A = timed(pair_list, dev); _, B = timed(lambda: duplicated(dup), dev)
        same = (torch.equal(A[0], B[0]) and torch.equal(A[1], B[1]) and torch.equal(A[2], B[2]) and torch.equal(A[3][:, CNT], B[3][:, CNT])
                and np.array_equal(A[4], B[4]))
        sched = int((A[3][:, DET] != B[3][:, DET]).any(dim=1).sum().item())
        t_pl, t_du, t_dg = [], [], []
        for _ in range(a.reps):
            t_pl.append(timed(pair_list, dev)[0]); t_du.append(timed(lambda: duplicated(dup), dev)[0]); t_dg.append(timed(duplicated, dev)[0])
        inside = min(t_du) <= np.median(t_pl) <= max(t_du)
        say(f"   device tensors: pair list {fmt(t_pl)}  duplicated, tensors ready {fmt(t_du)}  duplicated, with the device gather {fmt(t_dg)}")
        say(f"                   pair-list median inside the duplicated form's [min..max]: {'yes' if inside else 'NO'} "
            f"({100 * (np.median(t_pl) / np.median(t_du) - 1):+.1f} % of its median); outputs identical (models, match, inlier, counts, samples / LO runs / I): {same}; pairs whose pass counters or placement differ between the two runs: {sched}; tentatives/pair {np.mean(A[4]):.0f}, "
            f"short pairs {int((A[4] < 8).sum())}")
        del dup, A, B
        torch.cuda.empty_cache()
        # the numpy entry points, copies included (the per-pair lists are views: the copy happens inside the duplicated call)
        h_pl, h_du = [], []
        for r in range(a.host_reps + 1):
            t0 = time.perf_counter(); Hp = matcher.match_and_verify_pairs(kps, descs, pairs, **kw); tp = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            Hd = matcher.match_and_verify_batch([kps[i] for i in pairs[:, 0]], [kps[j] for j in pairs[:, 1]], [descs[i] for i in pairs[:, 0]],
                                                [descs[j] for j in pairs[:, 1]], **kw)
            td = (time.perf_counter() - t0) * 1e3
            if r:
                h_pl.append(tp); h_du.append(td)
        same_h = np.array_equal(Hp[0], Hd[0]) and all(np.array_equal(x, y) for x, y in zip(Hp[1], Hd[1])) and all(np.array_equal(x, y) for x, y in zip(Hp[2], Hd[2]))
        say(f"   numpy lists:    pair list {fmt(h_pl)}  duplicated (copies and upload included) {fmt(h_du)}  speed-up {np.median(h_du) / np.median(h_pl):.2f}x; "
            f"outputs identical: {same_h}")
        del k, d, i_rows, j_rows, Hp, Hd
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
