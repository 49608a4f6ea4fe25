"""Batched match-and-verify against the per-pair loop on the device (tensor_api.match_and_verify_batch_tensors).
Workload: K image pairs of 2000 x 2000 float32 descriptors of dim 128 (two-view geometry + descriptors as
examples/simple_example_amd.py builds them; 64 distinct pairs repeated to K, every pair with its own seed), model F.
  loop:    per pair match_snn_tensors + row gather (one host synchronisation per pair), then ONE find_fundamental_batch_tensors
           over the pairs with >= 8 tentatives (what a caller had to write before the batched call)
  batched: one match_and_verify_batch_tensors call (one host synchronisation)
Both paths are warmed up, then alternated; the median and the spread (min..max) of the wall time to a synchronised result are
reported, and the outputs of the two paths are checked for identity.  The matcher stage alone (knn_match_batch_tensors, one
direction) is timed with HIP events, with its share of the fp32 vector peak (157.3 TFLOP/s, MI355X_MICROARCH.md) at 3 n1 n2 dim
flop per pair: the kernel's direct no-FMA form (sub, mul, add as separate roundings) cannot issue at the packed-FMA rate that
peak assumes, so the share stays well below it by construction.
usage: gpu_match_verify.py [K ...] [--reps R] [--log FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pydegensac_amd import parallel, synthetic as syn, tensor_api

N, DIM, BASE = 2000, 128, 64
PEAK_FP32_VECTOR = 157.3e12


def base_pairs(dev):
    rng = np.random.default_rng(0)
    K1, K2, D1, D2 = [], [], [], []
    for i in range(BASE):
        p1, p2, lab, _ = syn.two_view_fundamental(N, 0.5, 0.1, seed=500 + i)
        d1 = rng.normal(size=(N, DIM)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32)
        d2[~lab] = rng.normal(size=((~lab).sum(), DIM)).astype(np.float32)
        perm = rng.permutation(N)
        K1.append(p1); K2.append(p2[perm]); D1.append(d1); D2.append(d2[perm])
    return [torch.from_numpy(np.stack(x)).to(dev) for x in (K1, K2, D1, D2)]


def loop_path(k1, k2, d1, d2, seeds):
    K = d1.shape[0]
    A, B, cnt = [], [], []
    for p in range(K):
        q, t, _ = tensor_api.match_snn_tensors(d1[p], d2[p], 0.9)
        A.append(k1[p][q]); B.append(k2[p][t]); cnt.append(int(q.numel()))
    elig = [p for p in range(K) if cnt[p] >= 8]
    F, mask, st, offs = tensor_api.find_fundamental_batch_tensors(torch.cat([A[p] for p in elig]), torch.cat([B[p] for p in elig]),
                                                                  [cnt[p] for p in elig], seeds=[int(seeds[p]) for p in elig])
    torch.cuda.synchronize()
    return F, mask, st, offs, elig, np.array(cnt)


def batched_path(k1, k2, d1, d2, seeds):
    K = d1.shape[0]
    out = tensor_api.match_and_verify_batch_tensors(k1.reshape(K * N, 2), k2.reshape(K * N, 2), d1.reshape(K * N, DIM), d2.reshape(K * N, DIM),
                                                    [N] * K, [N] * K, model="F", seeds=seeds)
    torch.cuda.synchronize()
    return out


def same(lo, ba):
    F, mask, st, offs, elig, cnt = lo
    M, match, inl, bst, bcnt = ba
    if not np.array_equal(cnt, bcnt):
        return False
    M = M.cpu().numpy(); inl = inl.cpu().numpy().reshape(len(cnt), N); match = match.cpu().numpy().reshape(len(cnt), N)
    F = F.cpu().numpy(); mask = mask.cpu().numpy(); st = st.cpu().numpy(); bst = bst.cpu().numpy()
    for e, p in enumerate(elig):
        if not np.array_equal(M[p], F[e]) or not np.array_equal(inl[p][match[p] >= 0], mask[offs[e]:offs[e + 1]]):
            return False
        if not np.array_equal(bst[p, [0, 1, 3]], st[e, [0, 1, 3]]):
            return False
    short = [p for p in range(len(cnt)) if p not in set(elig)]
    return not M[short].any() and not inl[short].any()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("K", nargs="*", type=int, default=[64, 512, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    say(f"# {torch.cuda.get_device_name(0)}; {N} x {N} x {DIM} float32 descriptors per pair, model F, ratio 0.9, "
        f"reps {a.reps} (alternating, after one warm-up of each path)")
    say("# matcher share of peak: 3 n1 n2 dim flop per pair over kernel time against 157.3 TFLOP/s; the kernel's direct form rounds sub, mul and "
        "add separately (no FMA, for bit-reproducible ranks), so it cannot issue at the packed-FMA (v_pk_fma_f32) rate that peak assumes")
    bk1, bk2, bd1, bd2 = base_pairs(dev)
    for K in a.K:
        rep = [(p % BASE) for p in range(K)]
        k1, k2, d1, d2 = bk1[rep].contiguous(), bk2[rep].contiguous(), bd1[rep].contiguous(), bd2[rep].contiguous()
        seeds = parallel.pair_seeds(0, K)
        lo = loop_path(k1, k2, d1, d2, seeds); ba = batched_path(k1, k2, d1, d2, seeds)          # warm-up
        ident = same(lo, ba)
        tl, tb = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); loop_path(k1, k2, d1, d2, seeds); tl.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); batched_path(k1, k2, d1, d2, seeds); tb.append(time.perf_counter() - t0)
        # the matcher stage alone: one direction, HIP events around `reps` back-to-back calls
        q = d1.reshape(K * N, DIM); t = d2.reshape(K * N, DIM)
        tensor_api.knn_match_batch_tensors(q, t, [N] * K, [N] * K); torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            tensor_api.knn_match_batch_tensors(q, t, [N] * K, [N] * K)
        e1.record(); torch.cuda.synchronize()
        kms = e0.elapsed_time(e1) / a.reps
        flop = 3.0 * N * N * DIM * K
        ml, mb = np.median(tl) * 1e3, np.median(tb) * 1e3
        say(f"K={K:5d}  loop {ml:9.2f} ms [{min(tl) * 1e3:.2f}..{max(tl) * 1e3:.2f}]  batched {mb:9.2f} ms [{min(tb) * 1e3:.2f}..{max(tb) * 1e3:.2f}]"
            f"  speed-up {ml / mb:5.2f}x  outputs identical: {ident}  tentatives/pair {np.mean(lo[5]):.0f} (short pairs {K - len(lo[4])})")
        say(f"         matcher alone (batched 2-NN, one direction): {kms:.3f} ms, {flop / kms / 1e9:.1f} TFLOP/s = "
            f"{100 * flop / kms / 1e-3 / PEAK_FP32_VECTOR:.1f} % of the fp32 vector peak")
        del k1, k2, d1, d2
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
