#!/usr/bin/env python
"""An image collection matched exhaustively, structure-from-motion style: keypoints and descriptors of every image go to the GPU ONCE,
a list of (i, j) image indices says which pairs to run, and one call gives a fundamental matrix, the matches and the inlier flags of
every pair, with one host synchronisation in all.  batch_match_verify_amd.py's call would need every image's rows copied once per pair
it takes part in: 2 K n rows instead of M n."""
import os
import sys
from time import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import matcher, synthetic, tensor_api

if __name__ == '__main__':
    M, n, dim = 12, 1500, 64
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)        # "detector + descriptor" on M views of one scene
    pairs = matcher.exhaustive_pairs(M)                                          # every (i, j) with i < j: M (M - 1) / 2 pairs
    dev = torch.device("cuda", 0)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    t0 = time()
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.9,
                                                                                    mutual=True, px_th=0.5, conf=0.999, max_iters=50000)
    torch.cuda.synchronize()
    print("{} images, {} pairs matched and verified in {:.3f} s".format(M, len(pairs), time() - t0))
    print("descriptor rows on the device: {} (one copy per pair and side would be {})".format(d.shape[0], 2 * len(pairs) * n))
    inl = inlier.cpu().numpy()
    per_pair = np.array([inl[po[p]:po[p + 1]].sum() for p in range(len(pairs))])
    print("tentatives per pair: median {:.0f}; inliers per pair: median {:.0f}".format(np.median(n_tent), np.median(per_pair)))
    best = int(per_pair.argmax())
    print("best pair {}: {} inliers, F =\n{}".format(tuple(pairs[best]), per_pair[best], F[best].cpu().numpy()))
    # the same through numpy lists (each image uploaded once): identical results
    Fh, mh, ih = matcher.match_and_verify_pairs(kps, descs, pairs, model="F", ratio=0.9, mutual=True, px_th=0.5, conf=0.999, max_iters=50000)
    print("numpy entry point identical:", np.array_equal(Fh, F.cpu().numpy()) and all(np.array_equal(ih[p], inl[po[p]:po[p + 1]]) for p in range(len(pairs))))
