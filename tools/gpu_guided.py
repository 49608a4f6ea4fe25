"""Guided matching against the unguided batched 2-NN on the device (tensor_api.guided_match_batch_tensors vs knn_match_batch_tensors).
Workload: K image pairs of 2000 x 2000 float32 descriptors of dim 128 (64 distinct pairs repeated to K), keypoints of synthetic
geometry with the true model per pair: F (two-view scene, px_th 0.5, Sampson) and H (plane, px_th 1.0, Sampson).
  unguided   knn_match_batch_tensors, one direction (the dense tile kernel)
  guided     guided_match_batch_tensors with the driver-form true models, ratio 0.9 (gate + compaction + distances + decision)
  gate only  the same with px_th = 1e-6: every (q, t) goes through the screen, almost nothing passes, so no distances are formed
Kernel-side times come from HIP events around `reps` back-to-back calls after a warm-up.  The mean gate pass rate is counted on the
host for four pairs, with the division-free Sampson forms (F: r^2 / den; H: q / det of dg_HDs_maybe_below).  Last, the added wall
time of guided=True inside match_and_verify_batch_tensors (F, the estimator's own models), alternating the two forms.
usage: gpu_guided.py [K ...] [--reps R] [--log FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pydegensac_amd import parallel, synthetic as syn, tensor_api

N, DIM, BASE = 2000, 128, 64


def base_pairs(model, dev):
    rng = np.random.default_rng(0)
    K1, K2, D1, D2, M = [], [], [], [], []
    for i in range(BASE):
        if model == "F":
            p1, p2, lab, Mt = syn.two_view_fundamental(N, 0.5, 0.1, seed=500 + i); Md = Mt
        else:
            p1, p2, lab, Mt = syn.homography_pairs(N, 0.5, 0.3, seed=500 + i); Md = np.linalg.inv(Mt).T
        d1 = rng.normal(size=(N, DIM)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32)
        d2[~lab] = rng.normal(size=((~lab).sum(), DIM)).astype(np.float32)
        perm = rng.permutation(N)
        K1.append(p1); K2.append(p2[perm]); D1.append(d1); D2.append(d2[perm]); M.append(Md)
    return [torch.from_numpy(np.stack(x)).to(dev) for x in (K1, K2, D1, D2)], np.stack(M)


def pass_rate(model, k1, k2, Md, th):
    x1, y1 = k1[:, 0, None], k1[:, 1, None]; x2, y2 = k2[None, :, 0], k2[None, :, 1]
    H = Md.ravel()
    if model == "F":
        rxc = H[0] * x2 + H[3] * y2 + H[6]; ryc = H[1] * x2 + H[4] * y2 + H[7]; rwc = H[2] * x2 + H[5] * y2 + H[8]
        r = x1 * rxc + y1 * ryc + rwc; rx = H[0] * x1 + H[1] * y1 + H[2]; ry = H[3] * x1 + H[4] * y1 + H[5]
        return float(np.mean(r * r <= th * (rxc * rxc + ryc * ryc + rx * rx + ry * ry)))
    w = H[2] * x2 + H[5] * y2 + H[8]
    r1 = (H[0] * x2 + H[3] * y2 + H[6]) - x1 * w; r2 = (H[1] * x2 + H[4] * y2 + H[7]) - y1 * w
    a = H[0] - H[2] * x1; b = H[3] - H[5] * x1; d = H[1] - H[2] * y1; e = H[4] - H[5] * y1
    m11 = a * a + b * b + w * w; m22 = d * d + e * e + w * w; m12 = a * d + b * e
    return float(np.mean(m22 * r1 * r1 - 2 * m12 * r1 * r2 + m11 * r2 * r2 <= th * (m11 * m22 - m12 * m12)))


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


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
    say(f"# {torch.cuda.get_device_name(0)}; {N} x {N} x {DIM} float32 descriptors per pair, ratio 0.9, HIP events over {a.reps} calls after a warm-up")
    for model, px in (("F", 0.5), ("H", 1.0)):
        (bk1, bk2, bd1, bd2), bM = base_pairs(model, dev)
        th = px * px
        rate = np.mean([pass_rate(model, bk1[i].cpu().numpy(), bk2[i].cpu().numpy(), bM[i], th) for i in range(4)])
        say(f"## model {model}, px_th {px} (Sampson, th {th}): mean gate pass rate {100 * rate:.3f} % of the n1 n2 (query, train) pairs")
        for K in a.K:
            rep = [(p % BASE) for p in range(K)]
            k1 = bk1[rep].reshape(K * N, 2).contiguous(); k2 = bk2[rep].reshape(K * N, 2).contiguous()
            d1 = bd1[rep].reshape(K * N, DIM).contiguous(); d2 = bd2[rep].reshape(K * N, DIM).contiguous()
            Md = torch.from_numpy(bM[rep]).to(dev)
            c = [N] * K
            t_u = timed(lambda: tensor_api.knn_match_batch_tensors(d1, d2, c, c), a.reps)
            t_g = timed(lambda: tensor_api.guided_match_batch_tensors(k1, k2, d1, d2, c, c, Md, model=model, px_th=px, driver_form=True), a.reps)
            t_0 = timed(lambda: tensor_api.guided_match_batch_tensors(k1, k2, d1, d2, c, c, Md, model=model, px_th=1e-6, driver_form=True), a.reps)
            m = tensor_api.guided_match_batch_tensors(k1, k2, d1, d2, c, c, Md, model=model, px_th=px, driver_form=True)[0]
            nm = int((m >= 0).sum().item())
            say(f"K={K:5d}  unguided 2-NN {t_u:9.2f} ms  guided {t_g:8.2f} ms ({100 * t_g / t_u:5.1f} % of unguided)  gate only {t_0:8.2f} ms"
                f"  -> compaction + distances + decision {t_g - t_0:7.2f} ms  guided matches/pair {nm / K:.0f}")
            del k1, k2, d1, d2, Md
            torch.cuda.empty_cache()
        del bk1, bk2, bd1, bd2
    # the added cost of guided=True inside match-and-verify (F, the estimator's models)
    (bk1, bk2, bd1, bd2), _ = base_pairs("F", dev)
    for K in a.K:
        rep = [(p % BASE) for p in range(K)]
        args = (bk1[rep].reshape(K * N, 2).contiguous(), bk2[rep].reshape(K * N, 2).contiguous(), bd1[rep].reshape(K * N, DIM).contiguous(),
                bd2[rep].reshape(K * N, DIM).contiguous(), [N] * K, [N] * K)
        seeds = parallel.pair_seeds(0, K)
        tp, tg = [], []
        for guided, acc in ((False, None), (True, None)) + ((False, tp), (True, tg)) * a.reps:       # warm-up, then alternating
            t0 = time.perf_counter()
            tensor_api.match_and_verify_batch_tensors(*args, model="F", seeds=seeds, guided=guided)
            torch.cuda.synchronize()
            if acc is not None:
                acc.append(time.perf_counter() - t0)
        say(f"K={K:5d}  match_and_verify_batch_tensors F: guided=False {np.median(tp) * 1e3:8.2f} ms [{min(tp) * 1e3:.2f}..{max(tp) * 1e3:.2f}]"
            f"  guided=True {np.median(tg) * 1e3:8.2f} ms [{min(tg) * 1e3:.2f}..{max(tg) * 1e3:.2f}]  added {1e3 * (np.median(tg) - np.median(tp)):7.2f} ms")
        del args
        torch.cuda.empty_cache()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
