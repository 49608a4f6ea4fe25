#!/usr/bin/env python
"""From descriptors to 3-D points on the device under known camera poses: match_and_verify_pairs_tensors matches and verifies every
pair of a small collection, correspondences_pairs_tensors(store_rows=True) exports the inliers, tracks_tensors groups them into tracks
and triangulate_tracks_tensors turns every track into a point with its reprojection errors, under the generator's cameras.  Nothing is
read back between the last three calls.  Prints the points per status, their error against the generator's cloud, and the share of ok
observations in consistent and in inconsistent tracks."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import _lib, matcher, synthetic, tensor_api

if __name__ == '__main__':
    M, n, dim = 8, 600, 64
    args = dict(m=M, n=n, inlier_ratio=0.6, sigma=0.3, dim=dim, seed=0)
    kps, descs = synthetic.image_collection(**args)
    cloud, point, _ = synthetic.collection_truth(**args)
    Kc, poses = synthetic.collection_cameras(M)
    pairs = matcher.exhaustive_pairs(M)
    dev = torch.device("cuda", 0)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", px_th=0.5)
    rows, co, total = tensor_api.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inlier, store_rows=True,
                                                               capacity=int(n_tent.sum()))[:3]
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * M, dtype=torch.float64, device=dev)
    R = torch.from_numpy(np.stack([p[0] for p in poses])).to(dev); t = torch.from_numpy(np.stack([p[1] for p in poses])).to(dev)
    track, n_tracks, track_offsets, obs, obs_image, track_images, n_obs = tensor_api.tracks_tensors(rows, counts, total=total)
    X, info, cost, cosang, err, ok, depth = tensor_api.triangulate_tracks_tensors(track_offsets, obs, obs_image, k, cams, R, t, n_tracks=n_tracks,
                                                                                  with_obs=True)
    nt = int(n_tracks)                                                           # the first read of the results
    X, info, cost = X[:nt].cpu().numpy(), info[:nt].cpu().numpy(), cost[:nt].cpu().numpy()
    off = track_offsets[:nt + 1].cpu().numpy(); o = obs.cpu().numpy(); okh = ok.cpu().numpy()
    names = {_lib.TRI_OK: "OK", _lib.TRI_NARROW: "NARROW", _lib.TRI_DEGENERATE: "DEGENERATE", _lib.TRI_SHORT: "SHORT", _lib.TRI_TRUNCATED: "TRUNCATED"}
    print("{} images x {} keypoints, {} pairs: {} tracks".format(M, n, len(pairs), nt))
    print("points per status: " + ", ".join("{} {}".format(names[s], int((info[:, 4] == s).sum())) for s in names))
    consistent = track_images[:nt].cpu().numpy() == np.diff(off)
    pt = np.concatenate(point)
    errs = []
    for j in np.flatnonzero(consistent & (info[:, 4] == _lib.TRI_OK)):
        ids = pt[o[off[j]:off[j + 1]]]
        if ids[0] >= 0 and (ids == ids[0]).all():
            errs.append(np.linalg.norm(X[j] - cloud[ids[0]]))
    print("error against the cloud over {} consistent tracks of one cloud point: median {:.4f}, max {:.4f} (depth 4 .. 8)".format(
        len(errs), float(np.median(errs)), float(np.max(errs))))
    print("reprojection cost, linear point -> refined, median: {:.3f} -> {:.3f} px^2".format(float(np.nanmedian(cost[:, 0])), float(np.nanmedian(cost[:, 1]))))
    for name, sel in (("consistent", consistent), ("inconsistent", ~consistent)):
        members = np.concatenate([np.arange(off[j], off[j + 1]) for j in np.flatnonzero(sel)] or [np.zeros(0, int)])
        share = 100.0 * okh[members].mean() if len(members) else float("nan")
        print("{} tracks: {}, ok observations {:.1f} %".format(name, int(sel.sum()), share))
