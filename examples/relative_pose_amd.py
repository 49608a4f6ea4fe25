#!/usr/bin/env python
"""From descriptors to relative poses with one host synchronisation.  match_and_verify_pairs_tensors finds an F per pair;
correspondences_pairs_tensors exports the verified matches as compact lists; refit_correspondences_tensors refits every F on its list;
relative_pose_tensors decomposes each refitted F under the cameras' intrinsics, picks the (R, t) under which most of the refit's members
triangulate in front of both cameras and counts the rows with parallax.  Nothing is read back between the calls.  The generator's own
cameras (synthetic.collection_cameras) give the rotation error and the error of the baseline direction per pair."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import _lib, matcher, synthetic, tensor_api


def _angle(c):
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


if __name__ == '__main__':
    M, n, dim, px = 6, 800, 64, 0.5
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)
    Kc, poses = synthetic.collection_cameras(M)
    pairs = matcher.exhaustive_pairs(M); K = len(pairs)
    dev = torch.device("cuda", 0)
    counts = [len(x) for x in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F, match, inlier, stats, n_tent, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, model="F", px_th=px)
    rows, co, total, _, pts, resid = tensor_api.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inlier, kps1=k, kps2=k, models=F)
    F2, member, info_r = tensor_api.refit_correspondences_tensors(pts, co, F, "F", px_th=px)
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * M, dtype=torch.float64, device=dev)      # fx, fy, cx, cy per image
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
    R, t, front, info = tensor_api.relative_pose_tensors(pts, co, F2, cams, pairs=pr, keep=member, min_parallax_deg=1.5)
    # the first read of the results
    R = R.cpu().numpy(); t = t.cpu().numpy(); info = info.cpu().numpy()
    names = {getattr(_lib, "POSE_" + s): s.lower() for s in ("OK", "BAD_MODEL", "BAD_CAMERA", "TRUNCATED", "EMPTY")}
    cls = matcher.pose_config(info)
    print("{} images, {} pairs".format(M, K))
    print("pair      used   front  runner-up   wide  status  class  rotation err  baseline err (degrees)")
    for p, (i, j) in enumerate(np.asarray(pairs)):
        (Ri, ti), (Rj, tj) = poses[i], poses[j]
        Rg = Rj @ Ri.T; tg = tj - Rg @ ti
        re = _angle((np.trace(R[p] @ Rg.T) - 1.0) / 2.0); te = _angle(t[p] @ tg / np.linalg.norm(tg))
        print("({}, {})  {:6d}  {:6d}  {:9d} {:6d}  {:>6s}  {:5d}  {:12.4f}  {:12.4f}".format(int(i), int(j), *(int(x) for x in info[p, :4]),
                                                                                        names[int(info[p, 4])], int(cls[p]), re, te))
    assert (info[:, 4] == _lib.POSE_OK).all() and (info[:, 1] > info[:, 2]).all() and int(front.sum()) == int(info[:, 1].sum())
