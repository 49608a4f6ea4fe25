#!/usr/bin/env python
"""From descriptors to one rotation per image with one host synchronisation.  match_and_verify_pairs_tensors finds an F per pair;
correspondences_pairs_tensors exports the verified matches; refit_correspondences_tensors refits every F; relative_pose_tensors and
refine_pose_tensors give one (R, t) per PAIR; average_rotations_tensors turns the pairwise rotations into one world-to-camera rotation
per IMAGE, which is what triangulate_tracks_tensors / refine_cameras_tensors start from (camera positions are not estimated here).
Nothing is read back between the calls.  The generator's own cameras (synthetic.collection_cameras) give, after the gauge is aligned at
the root, the rotation error per image after the first full level (every camera set over one edge) and at the end, and the number of
pairs whose relative rotation disagrees with the result by more than 5 degrees."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import _lib, matcher, synthetic, tensor_api


def _errors(R, truth, root):
    """the angle in degrees between R[c] and the generator's rotation, the gauge aligned at the root"""
    G = truth[root].T @ R[root]
    c = (np.einsum("nij,nij->n", R, truth @ G) - 1.0) / 2.0
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


if __name__ == '__main__':
    M, n, dim, px, root = 8, 800, 64, 0.5, 0
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)
    Kc, poses = synthetic.collection_cameras(M)
    truth = np.stack([R for R, _ in poses])
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
    R2, t2, cost, info2 = tensor_api.refine_pose_tensors(pts, co, R, t, cams, pairs=pr, keep=front)
    weight = info[:, 3].double(); keep = info[:, 4] == _lib.POSE_OK              # tensor expressions: nothing is read back
    # the complete graph has one level: after one sweep every camera is set over its edge to the root
    Rl, infol, _, suml = tensor_api.average_rotations_tensors(pr, R2, M, weight=weight, edge_keep=keep, root=root, sweeps=1)
    Rg, ginfo, step, summary, ecos = tensor_api.average_rotations_tensors(pr, R2, M, weight=weight, edge_keep=keep, root=root, with_edges=True)
    # the first read of the results
    Rl, Rg, ginfo, step, summary, ecos = (x.cpu().numpy() for x in (Rl, Rg, ginfo, step, summary, ecos))
    e1, e2 = _errors(Rl, truth, root), _errors(Rg, truth, root)
    names = {_lib.ROTAVG_KNOWN: "known", _lib.ROTAVG_OK: "ok", _lib.ROTAVG_UNREACHED: "unreached", _lib.ROTAVG_ISOLATED: "isolated"}
    glob = {_lib.ROTAVG_CONVERGED: "converged", _lib.ROTAVG_MAX_SWEEPS: "max_sweeps", _lib.ROTAVG_NO_ROOT: "no_root"}
    print("{} images, {} pairs, {} used; {} sweeps changed something, {} cameras set: {}".format(M, K, int(summary[2]), int(summary[0]), int(summary[1]),
                                                                                             glob[int(summary[3])]))
    print("image  half-edges  set in sweep  opposed     status   rotation error after the first level -> at the end (degrees)")
    for c in range(M):
        print("{:5d}  {:10d}  {:12d}  {:7d}  {:>9s}   {:.4f} -> {:.4f}".format(c, *(int(x) for x in ginfo[c, :3]), names[int(ginfo[c, 3])], e1[c], e2[c]))
    print("mean error {:.4f} -> {:.4f} degrees".format(e1[1:].mean(), e2[1:].mean()))
    print("pairs whose edge_cos lies below cos 5 degrees: {} of {}".format(int((ecos < math.cos(math.radians(5.0))).sum()), K))
    assert summary[1] == M and summary[3] == _lib.ROTAVG_CONVERGED and np.isfinite(Rg).all()
