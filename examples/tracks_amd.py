#!/usr/bin/env python
"""From descriptors to tracks on the device: match_and_verify_pairs_tensors matches and verifies every pair of a small collection,
correspondences_pairs_tensors(store_rows=True) exports the inliers as (row of the store, row of the store), and tracks_tensors groups
the keypoints that are transitively matched.  Nothing is read back between the three calls.  A track is consistent when it holds at
most one keypoint per image, which track_images tells without a second pass."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import matcher, synthetic, tensor_api

if __name__ == '__main__':
    M, n, dim = 8, 600, 64
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)
    pairs = matcher.exhaustive_pairs(M)
    dev = torch.device("cuda", 0)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", px_th=0.5)
    rows, co, total = tensor_api.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inlier, store_rows=True,
                                                               capacity=int(n_tent.sum()))[:3]
    track, n_tracks, track_offsets, obs, obs_image, track_images, n_obs = tensor_api.tracks_tensors(rows, counts, total=total)
    nt, no = int(n_tracks), int(n_obs)                                           # the first read of the results
    length = np.diff(track_offsets[:nt + 1].cpu().numpy())
    images = track_images[:nt].cpu().numpy()
    print("{} images x {} keypoints, {} pairs: {} verified correspondences -> {} tracks over {} keypoints".format(M, n, len(pairs), int(total), nt, no))
    print("track length: " + ", ".join("{}: {}".format(ln, int((length == ln).sum())) for ln in range(2, int(length.max()) + 1)
                                      if (length == ln).any()))
    print("consistent tracks (one keypoint per image at most): {} of {} = {:.1f} %".format(int((images == length).sum()), nt,
                                                                                        100.0 * (images == length).mean()))
    t = int(length.argmax())
    a, b = int(track_offsets[t]), int(track_offsets[t + 1])
    print("track {}: store rows {} in images {}".format(t, obs[a:b].tolist(), obs_image[a:b].tolist()))
    # the same through numpy
    out = matcher.tracks(rows[:int(total)].cpu().numpy(), counts)
    print("numpy entry point identical:", out["n_tracks"] == nt and np.array_equal(out["obs"], obs[:no].cpu().numpy())
          and np.array_equal(out["track"], track.cpu().numpy()))
