#!/usr/bin/env python
"""simple_example_amd.py's pipeline over a few hundred image pairs at once: keypoints + descriptors of every pair go to the
GPU, one call matches them (2-NN ratio test) and estimates a fundamental matrix per pair, with one host synchronisation in
all.  Pairs that match too poorly (fewer than 8 tentatives) come back with a zero model instead of failing the batch."""
import os
import sys
from time import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import synthetic, tensor_api

if __name__ == '__main__':
    K, dim = 300, 64
    rng = np.random.default_rng(0)
    kps1, kps2, descs1, descs2 = [], [], [], []
    for p in range(K):
        # "detector": two views of a 3-D scene, keypoints with descriptors (inliers share a noisy descriptor)
        n = int(rng.integers(500, 3000)) if p % 50 else 5                  # every 50th pair is nearly empty
        p1, p2, lab, _ = synthetic.two_view_fundamental(max(n, 50), 0.4, 0.1, seed=p)
        p1, p2, lab = p1[:n], p2[:n], lab[:n]
        d1 = rng.normal(size=(n, dim)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32)
        d2[~lab] = rng.normal(size=((~lab).sum(), dim)).astype(np.float32)
        kps1.append(p1); kps2.append(p2); descs1.append(d1); descs2.append(d2)
    dev = torch.device("cuda", 0)
    c1 = [len(d) for d in descs1]; c2 = [len(d) for d in descs2]
    k1, k2 = (torch.from_numpy(np.concatenate(x)).to(dev) for x in (kps1, kps2))
    d1, d2 = (torch.from_numpy(np.concatenate(x)).to(dev) for x in (descs1, descs2))
    t0 = time()
    F, match, inlier, stats, n_tent = tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, c1, c2, model="F", ratio=0.9,
                                                                               px_th=0.5, conf=0.999, max_iters=50000)
    torch.cuda.synchronize()
    print("{} pairs matched and verified in {:.3f} s".format(K, time() - t0))
    I = stats[:, 3].cpu().numpy()
    print("tentatives per pair: median {:.0f}; pairs too short to estimate: {}".format(np.median(n_tent), int((n_tent < 8).sum())))
    print("inliers per pair: median {:.0f}, total {}".format(np.median(I), int(inlier.sum().item())))
    print("F of pair 1 =", F[1].cpu().numpy())
