#!/usr/bin/env python
"""From a pair list to what a two-view database or a track builder takes: per pair the list of (row in image i, row in image j) that
survived, their four coordinates and their residual under the pair's model.  match_and_verify_pairs_tensors matches and verifies a small
collection; correspondences_pairs_tensors turns its per-query `match` / `inlier` into compact per-pair lists on the device, without a
host synchronisation; guided_match_pairs_tensors searches every pair again inside its model's band and the same call exports that too.
The residual is the estimator's own function, so every inlier lies at or below the threshold it was judged with."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import matcher, synthetic, tensor_api

if __name__ == '__main__':
    M, n, dim, px = 6, 800, 64, 0.5
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)
    pairs = matcher.exhaustive_pairs(M)
    K = len(pairs)
    dev = torch.device("cuda", 0)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    th = px * px                                                                 # Sampson error: the estimator compares with px_th^2
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", px_th=px)
    # inliers are tentatives: the tentative counts (already on the host) bound the length of the lists
    rows, co, total, entry, pts, resid = tensor_api.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inlier, kps1=k, kps2=k, models=F,
                                                                                  model="F", with_entry=True, capacity=int(n_tent.sum()))
    gmatch = tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, model="F", px_th=px)[0]
    grows, gco, gtotal, _, gpts, gresid = tensor_api.correspondences_pairs_tensors(gmatch, counts, counts, pairs, kps1=k, kps2=k, models=F, model="F")
    co = co.cpu().numpy(); gco = gco.cpu().numpy(); resid = resid.cpu().numpy(); gresid = gresid.cpu().numpy()      # the first read of the results
    print("{} images, {} pairs, {} query rows: {} verified and {} guided correspondences".format(M, K, int(po[-1]), int(total), int(gtotal)))
    print("pair      verified  max resid   guided  max resid   (th = {:g})".format(th))
    for p in range(K):
        v = resid[co[p]:co[p + 1]]; g = gresid[gco[p]:gco[p + 1]]
        print("({}, {})   {:8d}  {:9.3g}  {:7d}  {:9.3g}".format(int(pairs[p][0]), int(pairs[p][1]), len(v), v.max() if len(v) else 0.0, len(g),
                                                                g.max() if len(g) else 0.0))
    assert (resid[:int(total)] <= th).all() and (gresid[:int(gtotal)] <= th).all()
    p = int(np.diff(co).argmax())
    r = rows[co[p]:co[p + 1]].cpu().numpy()
    print("pair {}: first correspondences (row in image i, row in image j):".format(tuple(int(x) for x in pairs[p])), r[:4].tolist())
    # the same through numpy lists
    out = matcher.correspondences_pairs(match.cpu().numpy(), counts, counts, pairs, keep=inlier.cpu().numpy(), kps_list=kps, models=F.cpu().numpy())
    print("numpy entry point identical:", all(np.array_equal(out[q]["rows"], rows[co[q]:co[q + 1]].cpu().numpy())
                                              and np.array_equal(out[q]["resid"], resid[co[q]:co[q + 1]]) for q in range(K)))
