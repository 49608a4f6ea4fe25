#!/usr/bin/env python
"""Guided matching with the FGINN second neighbour inside the model's inlier band, on a scene that has BOTH problems of the ratio test:
  decoys  a look-alike descriptor elsewhere in image 2, 40 px off the query's epipolar line: the ratio test drops the match, guided
          matching brings it back (the decoy lies outside the band);
  twins   a second keypoint 1.5 px beside the correct one with a near-equal descriptor (a second orientation, a neighbouring scale):
          the twin lies INSIDE the band, so guided matching alone still drops the match; with fginn_th the second distance comes
          from the nearest gated keypoint at least that many pixels away from the nearest one, and a query whose only gated companion
          is its twin is kept (nothing competes with it).
Prints the correct matches per stage: ratio test, guided, guided + FGINN.  A match to the twin counts as correct."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import synthetic, tensor_api

if __name__ == '__main__':
    K, n, dim = 32, 1500, 64
    n_tw, d_lo, d_hi = int(0.4 * n), int(0.3 * n), int(0.7 * n)          # rows 0 .. n_tw have a twin, rows d_lo .. d_hi a decoy
    rng = np.random.default_rng(0)
    kps1, kps2, descs1, descs2, truth = [], [], [], [], []
    for p in range(K):
        p1, p2, lab, F = synthetic.two_view_fundamental(n, 0.8, 0.1, seed=p)
        lines = np.c_[p1, np.ones(n)] @ F.T                               # epipolar lines of the queries in image 2
        away = lines[:, :2] / np.linalg.norm(lines[:, :2], axis=1, keepdims=True)
        along = np.c_[-away[:, 1], away[:, 0]]
        d1 = rng.normal(size=(n, dim)).astype(np.float32)
        d_true = d1 + 0.05 * rng.normal(size=d1.shape).astype(np.float32)
        d_true[~lab] = rng.normal(size=((~lab).sum(), dim)).astype(np.float32)
        decoys = (p2 + 40.0 * away * rng.choice([-1.0, 1.0], (n, 1)))[d_lo:d_hi]
        d_decoy = (d1 + 0.05 * rng.normal(size=d1.shape).astype(np.float32))[d_lo:d_hi]
        twins = (p2 + 1.5 * along)[:n_tw]
        d_twin = (d_true + 0.002 * rng.normal(size=d1.shape).astype(np.float32))[:n_tw]
        kps1.append(p1); kps2.append(np.concatenate([p2, decoys, twins])); descs1.append(d1)
        descs2.append(np.concatenate([d_true, d_decoy, d_twin]))
        truth.append(np.where(lab, np.arange(n), -2))
    dev = torch.device("cuda", 0)
    c1 = [len(d) for d in descs1]; c2 = [len(d) for d in descs2]
    k1, k2 = (torch.from_numpy(np.concatenate(x)).to(dev) for x in (kps1, kps2))
    d1, d2 = (torch.from_numpy(np.concatenate(x)).to(dev) for x in (descs1, descs2))
    kw = dict(model="F", ratio=0.9, px_th=1.0, max_iters=20000, guided=True)
    F, match, inlier, stats, n_tent, guided = tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, c1, c2, **kw)
    both = tensor_api.match_and_verify_batch_tensors(k1, k2, d1, d2, c1, c2, guided_fginn_th=10.0, **kw)[5]
    truth = np.concatenate(truth)
    row = np.tile(np.arange(n), K)
    twin_of = np.where(row < n_tw, n + (d_hi - d_lo) + row, -3)           # the train row of a query's twin, where it has one

    def correct(m):
        m = m.cpu().numpy()
        ok = (truth >= 0) & ((m == truth) | (m == twin_of))
        return int(ok.sum()), int(ok[row < n_tw].sum()), int((m >= 0).sum())
    print("true correspondences: {} ({} of them twinned)".format(int((truth >= 0).sum()), int(((truth >= 0) & (row < n_tw)).sum())))
    for name, m in (("ratio test", match), ("guided", guided), ("guided + FGINN (fginn_th 10)", both)):
        print("{:30s} keeps {:6d} correct matches, {:6d} of the twinned ones ({} matches in all)".format(name, *correct(m)))
