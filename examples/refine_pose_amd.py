#!/usr/bin/env python
"""From descriptors to refined relative poses with one host synchronisation.  match_and_verify_pairs_tensors finds an F per pair;
correspondences_pairs_tensors exports the verified matches as compact lists; refit_correspondences_tensors refits every F on its list;
relative_pose_tensors decomposes each refitted F under the cameras' intrinsics; refine_pose_tensors runs a Levenberg-Marquardt refinement
of every (R, t) on the Sampson distance of the rows the pose call found in front of both cameras.  Nothing is read back between the
calls.  The generator's own cameras (synthetic.collection_cameras) give the rotation error and the error of the baseline direction per
pair, before and after the refinement."""
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
    R2, t2, cost, info2, F3 = tensor_api.refine_pose_tensors(pts, co, R, t, cams, pairs=pr, keep=front, with_F=True)
    # the first read of the results
    R, t, R2, t2, cost, info2 = (x.cpu().numpy() for x in (R, t, R2, t2, cost, info2))
    names = {getattr(_lib, "REFINE_" + s): s.lower() for s in ("CONVERGED", "STALLED", "MAX_TRIALS", "SHORT", "NOT_FINITE", "BAD_POSE", "BAD_CAMERA",
                                                               "TRUNCATED")}
    print("{} images, {} pairs".format(M, K))
    print("pair      used  trials  accepted      status   cost before -> after (px^2)   rotation err before -> after   baseline err before -> after (degrees)")
    for p, (i, j) in enumerate(np.asarray(pairs)):
        (Ri, ti), (Rj, tj) = poses[i], poses[j]
        Rg = Rj @ Ri.T; tg = tj - Rg @ ti
        err = lambda Rm, tv: (_angle((np.trace(Rm @ Rg.T) - 1.0) / 2.0), _angle(tv @ tg / np.linalg.norm(tg)))          # noqa: E731
        (r0, b0), (r1, b1) = err(R[p], t[p]), err(R2[p], t2[p])
        print("({}, {})  {:6d}  {:6d}  {:8d}  {:>10s}   {:11.3f} -> {:9.3f}   {:15.4f} -> {:7.4f}   {:15.4f} -> {:7.4f}".format(
            int(i), int(j), *(int(x) for x in info2[p, :3]), names[int(info2[p, 3])], cost[p, 0], cost[p, 1], r0, r1, b0, b1))
    assert (info2[:, 3] <= _lib.REFINE_MAX_TRIALS).all() and (cost[:, 1] <= cost[:, 0]).all() and bool(torch.isfinite(F3).all())
