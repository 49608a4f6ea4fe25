#!/usr/bin/env python
"""The pose of the pairs on which a fundamental matrix is degenerate.  One store holds three groups of images: a 3-D cloud (general
pairs), one plane (planar pairs) and one camera centre (panoramic pairs).  match_and_verify_fh_pairs_tensors verifies F and H per pair
and two_view_config sorts the pairs; correspondences_pairs_tensors exports the matches that either model verified; relative_pose_tensors
decomposes F, homography_pose_tensors decomposes H, select_pose_tensors keeps the H pose where the class says planar / panoramic;
refine_pose_tensors (on the pairs that kept their F pose) and average_rotations_tensors (per group) follow.  Printed per class: the rotation error against the generator under
the F pose and under the selected pose, and the rotation error per image after averaging either."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

import torch

from pydegensac_amd import _lib, matcher, synthetic, tensor_api


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0))))


if __name__ == '__main__':
    m, n, dim = 5, 800, 64
    groups = [("general", synthetic.image_collection(m, n, 0.6, 0.1, dim, seed=0) + (dict(poses=synthetic.collection_cameras(m)[1]),)),
              ("planar", synthetic.planar_collection(m, n, 0.6, 0.1, dim, seed=0, kind="planar")),
              ("panoramic", synthetic.planar_collection(m, n, 0.6, 0.1, dim, seed=0, kind="panoramic"))]
    Kc = synthetic.collection_cameras(m)[0]
    kps = [x for _, g in groups for x in g[0]]; descs = [x for _, g in groups for x in g[1]]
    truth = [R for _, g in groups for R, _ in g[2]["poses"]]
    pairs = np.concatenate([np.asarray(matcher.exhaustive_pairs(m)) + m * gi for gi in range(len(groups))]); K = len(pairs)
    dev = torch.device("cuda", 0)
    counts = [len(x) for x in descs]; M = len(counts)
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    F, H, match, inl_f, inl_h, st_f, st_h, summary, n_tent, po = tensor_api.match_and_verify_fh_pairs_tensors(k, k, d, d, counts, counts, pairs)
    cls = matcher.two_view_config(summary)                              # (the call above synchronised once; this reads its summary)
    rows, co, total, _, pts, resid = tensor_api.correspondences_pairs_tensors(match, counts, counts, pairs, keep=inl_f | inl_h, kps1=k, kps2=k)
    cams = torch.tensor([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]] * M, dtype=torch.float64, device=dev)
    pr = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
    # from here on nothing is read back until the results are printed
    pose_f = tensor_api.relative_pose_tensors(pts, co, F, cams, pairs=pr)
    pose_h = tensor_api.homography_pose_tensors(pts, co, H, cams, pairs=pr)
    R, t, front, info, use_h, edge = tensor_api.select_pose_tensors(torch.from_numpy(cls).to(dev), pose_f, pose_h, co)
    R2, t2, cost, info2 = tensor_api.refine_pose_tensors(pts, co, R, t, cams, pairs=pr, keep=front)
    # the refinement minimises the epipolar error, which is as degenerate on a plane or a rotation as F itself: H poses stay as they are
    refined = ((info2[:, 3] <= _lib.REFINE_MAX_TRIALS) & ~use_h)[:, None, None]
    R2 = torch.where(refined, R2, R)
    avg = {}
    for name, Rp, ek in (("F pose", pose_f[0], pose_f[3][:, 4] == _lib.POSE_OK), ("selected", R2, edge)):
        avg[name] = [tensor_api.average_rotations_tensors(pr, Rp, M, edge_keep=ek, root=m * gi)[0].cpu().numpy() for gi in range(len(groups))]
    Rf, Rs, cls_h, ih = pose_f[0].cpu().numpy(), R2.cpu().numpy(), use_h.cpu().numpy(), pose_h[3].cpu().numpy()
    print("group       pairs  class 2  H pose used  rotations   rotation error of the pairs, median / max degrees: F pose | selected pose")
    for gi, (name, _) in enumerate(groups):
        sel = np.flatnonzero((pairs[:, 0] >= m * gi) & (pairs[:, 0] < m * (gi + 1)))
        ef = [_angle(Rf[p], truth[pairs[p, 1]] @ truth[pairs[p, 0]].T) for p in sel]
        es = [_angle(Rs[p], truth[pairs[p, 1]] @ truth[pairs[p, 0]].T) for p in sel]
        print("{:10s}  {:5d}  {:7d}  {:11d}  {:9d}   {:8.4f} / {:8.4f} | {:8.4f} / {:8.4f}".format(
            name, len(sel), int((cls[sel] == 2).sum()), int(cls_h[sel].sum()), int((ih[sel, 4] == _lib.POSE_ROTATION).sum()),
            np.median(ef), np.max(ef), np.median(es), np.max(es)))
    print("rotation error per image after averaging (gauge at the group's first image), mean degrees: F pose | selected pose")
    for gi, (name, _) in enumerate(groups):
        out = []
        for key in ("F pose", "selected"):
            Ra = avg[key][gi]; root = m * gi
            out.append(np.mean([_angle(Ra[c] @ Ra[root].T, truth[c] @ truth[root].T) for c in range(root + 1, root + m)]))
        print("{:10s}  {:8.4f} | {:8.4f}".format(name, *out))
