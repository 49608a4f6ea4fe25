#!/usr/bin/env python
"""An image collection from pair list to models to guided matches, with every image stored once: keypoints and descriptors go to the GPU
ONCE, match_and_verify_pairs_tensors gives a fundamental matrix per (i, j) of the list, and guided_match_pairs_tensors searches every
pair again inside its model's inlier band.  The collection carries decoys: in every image a share of the keypoints repeat the descriptor
of another keypoint of the same image, so the plain ratio test drops the true match (two equally good neighbours); inside the band the
decoy is usually gone and the match comes back.  guided_match_amd.py's call would need every image's rows copied once per pair."""
import os
import sys
from time import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import matcher, synthetic, tensor_api

if __name__ == '__main__':
    M, n, dim = 10, 1200, 64
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)        # "detector + descriptor" on M views of one scene
    rng = np.random.default_rng(1)
    for d in descs:                                                              # decoys: 300 rows per image repeat another row's descriptor
        src, dst = rng.permutation(n)[:600].reshape(2, 300)
        d[dst] = d[src] + 0.02 * rng.normal(size=(300, dim)).astype(np.float32)
    pairs = matcher.exhaustive_pairs(M)                                          # every (i, j) with i < j: M (M - 1) / 2 pairs
    K = len(pairs)
    dev = torch.device("cuda", 0)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    t0 = time()
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", ratio=0.8,
                                                                                    mutual=True, px_th=0.5, conf=0.999, max_iters=50000)
    # the models go in as they came out; one model per list entry
    gmatch, gidx, gdist, gpo = tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, model="F", ratio=0.8, mutual=True,
                                                                     px_th=0.5)
    torch.cuda.synchronize()
    print("{} images, {} pairs: matched, verified and matched again under their models in {:.3f} s".format(M, K, time() - t0))
    print("descriptor rows on the device: {} (one copy per pair and side would be {})".format(d.shape[0], 2 * K * n))
    assert np.array_equal(po, gpo)
    inl = inlier.cpu().numpy(); gm = gmatch.cpu().numpy()
    per_pair = np.array([inl[po[p]:po[p + 1]].sum() for p in range(K)])
    guided = np.array([(gm[po[p]:po[p + 1]] >= 0).sum() for p in range(K)])
    print("tentatives per pair: median {:.0f}; inliers: median {:.0f}; guided matches: median {:.0f}".format(np.median(n_tent), np.median(per_pair),
                                                                                                          np.median(guided)))
    best = int(guided.argmax())
    print("pair {}: {} tentatives, {} inliers, {} guided matches".format(tuple(int(x) for x in pairs[best]), n_tent[best], per_pair[best], guided[best]))
    # the same through numpy lists (each image uploaded once): identical results
    Fh, mh, ih = matcher.match_and_verify_pairs(kps, descs, pairs, model="F", ratio=0.8, mutual=True, px_th=0.5, conf=0.999, max_iters=50000)
    gh = matcher.guided_match_pairs(kps, descs, pairs, Fh, model="F", ratio=0.8, mutual=True, px_th=0.5)
    same = all(np.array_equal(gh[p][0], np.flatnonzero(gm[po[p]:po[p + 1]] >= 0)) and np.array_equal(gh[p][1], gm[po[p]:po[p + 1]][gh[p][0]])
               for p in range(K))
    print("numpy entry point identical:", np.array_equal(Fh, F.cpu().numpy()) and same)
