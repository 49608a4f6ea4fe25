#!/usr/bin/env python
"""Refit the models on what the guided stage brought back.  match_and_verify_pairs_tensors finds an F per pair from the ratio-test
tentatives; guided_match_pairs_tensors uses it to bring back matches the ratio test dropped; correspondences_pairs_tensors exports them
with points and residuals under the model that never saw them.  refit_correspondences_tensors judges each exported list against its model,
refits the model on the members with the reference's non-minimal solver and repeats while the member set grows, on the device and without
a host synchronisation; a second export with keep = the refit's inlier and the refit models gives the final lists.  A share of decoys
(keypoints with a twin descriptor elsewhere in the image) makes the guided stage matter."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import _lib, matcher, synthetic, tensor_api

if __name__ == '__main__':
    M, n, dim, px = 6, 800, 64, 0.5
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)
    rng = np.random.default_rng(1)
    for kp, ds in zip(kps, descs):                                               # decoys: 15 % of the rows get a twin descriptor far away
        src = rng.permutation(n)[:int(0.15 * n)]; dst = rng.permutation(n)[:len(src)]
        ds[dst] = ds[src] + 0.05 * rng.normal(size=(len(src), dim)).astype(np.float32)
    pairs = matcher.exhaustive_pairs(M); K = len(pairs)
    dev = torch.device("cuda", 0)
    counts = [len(x) for x in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", px_th=px)
    gmatch = tensor_api.guided_match_pairs_tensors(k, k, d, d, counts, counts, pairs, F, model="F", px_th=px)[0]
    rows, co, total, entry, pts, resid = tensor_api.correspondences_pairs_tensors(gmatch, counts, counts, pairs, kps1=k, kps2=k, models=F,
                                                                                  with_entry=True)
    F2, member, info, resid2 = tensor_api.refit_correspondences_tensors(pts, co, F, "F", px_th=px, with_resid=True)
    # the refit's inlier lives on the exported list; back to output rows (query row + the entry's first output row) for the second export
    valid = entry >= 0
    out_row = torch.from_numpy(po).to(dev)[entry.clamp(min=0).long()] + rows[:, 0].long()
    keep = torch.zeros(int(po[-1]), dtype=torch.bool, device=dev)
    keep[out_row[valid]] = member[valid]
    rows3, co3, total3, _, pts3, resid3 = tensor_api.correspondences_pairs_tensors(gmatch, counts, counts, pairs, keep=keep, kps1=k, kps2=k, models=F2)
    # the first read of the results
    co = co.cpu().numpy(); co3 = co3.cpu().numpy(); info = info.cpu().numpy(); resid = resid.cpu().numpy(); resid3 = resid3.cpu().numpy()
    ver = np.add.reduceat(inlier.cpu().numpy().astype(np.int64), po[:-1])
    names = {getattr(_lib, "REFIT_" + s): s.lower() for s in ("FIXED", "MAX_FITS", "SHORT", "BAD_FIT", "WORSE", "TRUNCATED")}
    print("{} images, {} pairs, th = {:g}".format(M, K, px * px))
    print("pair     verified   guided  mean resid   refit  mean resid  fits  status")
    for p in range(K):
        g = resid[co[p]:co[p + 1]]; r = resid3[co3[p]:co3[p + 1]]
        print("({}, {})  {:8d} {:8d}  {:10.4f} {:7d}  {:10.4f}  {:4d}  {}".format(int(pairs[p][0]), int(pairs[p][1]), int(ver[p]), len(g),
                                                                              g.mean() if len(g) else 0.0, len(r), r.mean() if len(r) else 0.0,
                                                                              int(info[p, 2]), names[int(info[p, 3])]))
    assert (np.diff(co3) == info[:, 1]).all() and (info[:, 1] >= info[:, 0]).all()
    assert (resid3[:int(total3)] <= px * px).all()
