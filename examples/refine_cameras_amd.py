#!/usr/bin/env python
"""A block-coordinate bundle adjustment on the device: match_and_verify_pairs_tensors matches and verifies every pair of a small
collection, correspondences_pairs_tensors(store_rows=True) exports the inliers, tracks_tensors groups them into tracks; then, from the
generator's poses perturbed by ROT radians about a random axis and TRANS in the translation (cameras 0 and 1 exact, and held by
refine=), triangulate_tracks_tensors (structure only) and refine_cameras_tensors (motion only) alternate for a few rounds.  Nothing is
read back between the calls of a round; the sums printed per round are read after it.  Prints per round the summed cost at the start
and at the end of the refinement and the pose error against synthetic.collection_cameras."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import _lib, matcher, synthetic, tensor_api

ROT, TRANS, ROUNDS = 0.01, 0.02, 4          # radians, scene units (the cloud lies at depth 4 .. 8)
TRI_PX = 20.0                               # max_reproj_px of the triangulation: 0.01 rad at f = 800 is 8 px, so the default of 4 px would
                                            # drop most observations of a perturbed camera before its pose can be refined


def rotation(a):
    th = np.linalg.norm(a); k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose_error(R, t, R_true, t_true):
    dR = R @ R_true.transpose(1, 2)
    ang = torch.acos(((dR.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1))
    return float(ang.max()), float((t - t_true).norm(dim=1).max())


if __name__ == '__main__':
    M, n, dim = 8, 600, 64
    args = dict(m=M, n=n, inlier_ratio=0.6, sigma=0.3, dim=dim, seed=0)
    kps, descs = synthetic.image_collection(**args)
    Kc, poses = synthetic.collection_cameras(M)
    pairs = matcher.exhaustive_pairs(M)
    dev = torch.device("cuda", 0)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", px_th=0.5)
    rows, co, total = tensor_api.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inlier, store_rows=True,
                                                               capacity=int(n_tent.sum()))[:3]
    track, n_tracks, track_offsets, obs, obs_image, track_images, n_obs = tensor_api.tracks_tensors(rows, counts, total=total)
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * M, dtype=torch.float64, device=dev)
    R_true = torch.from_numpy(np.stack([p[0] for p in poses])).to(dev); t_true = torch.from_numpy(np.stack([p[1] for p in poses])).to(dev)
    rng = np.random.default_rng(1)
    Rn = np.stack([p[0] for p in poses]); tn = np.stack([p[1] for p in poses])
    for i in range(2, M):
        a = rng.normal(size=3); b = rng.normal(size=3)
        Rn[i] = rotation(a * ROT / np.linalg.norm(a)) @ Rn[i]; tn[i] = tn[i] + b * TRANS / np.linalg.norm(b)
    R = torch.from_numpy(Rn).to(dev); t = torch.from_numpy(tn).to(dev)
    held = torch.ones(M, dtype=torch.uint8, device=dev); held[:2] = 0          # cameras 0 and 1 fix the gauge
    names = ["CONVERGED", "STALLED", "MAX_TRIALS", "FIXED", "BEHIND", "NOT_FINITE", "SHORT", "BAD_POSE", "BAD_CAMERA"]
    assert names[_lib.CAMREF_FIXED] == "FIXED"
    print("{} images x {} keypoints, {} pairs; poses off by {} rad and {}".format(M, n, len(pairs), ROT, TRANS))
    print("start: pose error angle {:.5f} rad, |t - t_true| {:.5f}".format(*pose_error(R, t, R_true, t_true)))
    for rnd in range(ROUNDS):
        X, tinfo, tcost, cosang, err, ok, depth = tensor_api.triangulate_tracks_tensors(track_offsets, obs, obs_image, k, cams, R, t, n_tracks=n_tracks,
                                                                                        with_obs=True, max_reproj_px=TRI_PX)
        R, t, cost, info = tensor_api.refine_cameras_tensors(track_offsets, obs, obs_image, k, cams, R, t, X, n_tracks=n_tracks, obs_keep=ok, refine=held)
        c = cost.nansum(0).cpu().numpy(); ih = info.cpu().numpy()              # the round's first read
        st = ", ".join("{} {}".format(names[s], int((ih[:, 3] == s).sum())) for s in range(9) if (ih[:, 3] == s).any())
        print("round {}: {} observations, summed cost {:.1f} -> {:.1f} px^2, pose error angle {:.5f} rad, |t - t_true| {:.5f}  ({})".format(
            rnd + 1, int(ih[:, 0].sum()), c[0], c[1], *pose_error(R, t, R_true, t_true), st))
