#!/usr/bin/env python
"""Guided matching after RANSAC on a scene with repeated texture: every true correspondence has a look-alike (a near-duplicate
descriptor) elsewhere in image 2, so the plain ratio test drops most true matches.  Estimating F from the surviving matches and
then searching again inside each query's epipolar band (guided matching) brings them back: the look-alikes lie outside the band."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import synthetic, tensor_api

if __name__ == '__main__':
    K, n, dim = 64, 1500, 64
    rng = np.random.default_rng(0)
    kps1, kps2, descs1, descs2, truth = [], [], [], [], []
    for p in range(K):
        p1, p2, lab, F = synthetic.two_view_fundamental(n, 0.8, 0.1, seed=p)
        lines = np.c_[p1, np.ones(n)] @ F.T                               # epipolar lines of the queries in image 2
        away = lines[:, :2] / np.linalg.norm(lines[:, :2], axis=1, keepdims=True)
        decoys = p2 + 40.0 * away * rng.choice([-1.0, 1.0], (n, 1))      # 40 px off the line, either side
        d1 = rng.normal(size=(n, dim)).astype(np.float32)
        d_true = d1 + 0.05 * rng.normal(size=d1.shape).astype(np.float32)
        d_true[~lab] = rng.normal(size=((~lab).sum(), dim)).astype(np.float32)
        d_decoy = d1 + 0.05 * rng.normal(size=d1.shape).astype(np.float32)
        kps1.append(p1); kps2.append(np.concatenate([p2, decoys])); descs1.append(d1); descs2.append(np.concatenate([d_true, d_decoy]))
        truth.append(np.where(lab, np.arange(n), -2))
    dev = torch.device("cuda", 0)
    c1 = [len(d) for d in descs1]; c2 = [len(d) for d in descs2]
    k1, k2 = (torch.from_numpy(np.concatenate(x)).to(dev) for x in (kps1, kps2))
    d1, d2 = (torch.from_numpy(np.concatenate(x)).to(dev) for x in (descs1, descs2))
    F, match, inlier, stats, n_tent, guided = tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, c1, c2, model="F", ratio=0.9,
                                                                                       px_th=1.0, max_iters=20000, guided=True)
    truth = np.concatenate(truth); match = match.cpu().numpy(); guided = guided.cpu().numpy()
    n_true = int((truth >= 0).sum())
    print("true correspondences: {}".format(n_true))
    print("ratio test keeps {} of them ({} tentatives in all)".format(int((match == truth).sum()), int((match >= 0).sum())))
    print("guided matching with the estimated F keeps {} ({} matches in all)".format(int((guided == truth).sum()), int((guided >= 0).sum())))
