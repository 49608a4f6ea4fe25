#!/usr/bin/env python
"""Two-view geometry of a pair list in one call: a small collection in which some pairs see one plane and some a general scene.  The
matching runs once per pair, then a fundamental matrix AND a homography are estimated on the same tentatives; the per-pair summary
(tentatives, F inliers, H inliers, inliers of both) goes to matcher.two_view_config, COLMAP's H/F inlier-ratio test, which says per pair:
rejected, general (keep F), or planar / panoramic (H explains what F explains).  Either model then goes into guided_match_pairs_tensors
as it is."""
import os
import sys
from time import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import matcher, synthetic, tensor_api

CLASS = {0: "rejected", 1: "general", 2: "planar / panoramic"}


def image_pair(kind, n, dim, seed):
    """two images of n keypoints: the correspondences of a synthetic plane ("plane") or of a general scene ("general"); a keypoint's
    descriptor in the second image is a noisy copy of its descriptor in the first, the rows of the second image shuffled"""
    rng = np.random.default_rng(seed)
    if kind == "plane":
        p1, p2, _, _ = synthetic.homography_pairs(n, 0.7, 0.5, seed=seed)
    else:
        p1, p2, _, _ = synthetic.two_view_fundamental(n, 0.7, 0.3, seed=seed)
    d1 = rng.normal(size=(n, dim)).astype(np.float32)
    d2 = d1 + 0.1 * rng.normal(size=d1.shape).astype(np.float32)
    perm = rng.permutation(n)
    return (np.ascontiguousarray(p1[:, :2]), d1), (np.ascontiguousarray(p2[perm, :2]), d2[perm])


if __name__ == '__main__':
    n, dim = 800, 64
    kinds = ["plane", "general", "plane", "general", "general"]
    kps, descs, pairs = [], [], []
    for i, kind in enumerate(kinds):
        a, b = image_pair(kind, n, dim, seed=10 + i)
        pairs.append((len(kps), len(kps) + 1))
        kps += [a[0], b[0]]; descs += [a[1], b[1]]
    pairs.append((0, 3))                                                            # two unrelated images: nothing to verify
    kinds.append("unrelated")
    dev = torch.device("cuda", 0)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    t0 = time()
    F, H, match, inl_f, inl_h, st_f, st_h, summary, n_tent, po = tensor_api.match_and_verify_fh_pairs_tensors(
        k, k, d, d, counts, counts, pairs, ratio=0.9, mutual=True, f_params=dict(px_th=0.5, max_iters=20000), h_params=dict(px_th=2.0, max_iters=20000))
    torch.cuda.synchronize()
    print("{} pairs matched once and verified twice in {:.3f} s".format(len(pairs), time() - t0))
    config = matcher.two_view_config(summary, min_inliers=15, max_h_ratio=0.8)
    print("pair        scene      tentatives    nF    nH   nFH   two_view_config")
    for p, (i, j) in enumerate(pairs):
        t, nf, nh, nfh = summary[p].tolist()
        print("({:2d}, {:2d})    {:9s}  {:10d} {:5d} {:5d} {:5d}   {}".format(i, j, kinds[p], t, nf, nh, nfh, CLASS[int(config[p])]))
    # guided matching takes either model as returned: H for the planar pairs, F for the others
    gH = tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, H, model="H", px_th=2.0)[0]
    gF = tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, model="F", px_th=0.5)[0]
    for p in range(len(pairs)):
        g = gH if config[p] == 2 else gF
        print("pair {}: {} guided matches under its {}".format(pairs[p], int((g[po[p]:po[p + 1]] >= 0).sum()), "H" if config[p] == 2 else "F"))
