"""The FGINN ratio test on a scene with twinned keypoints.  A detector such as SIFT emits several keypoints for one image structure
(a second orientation, a neighbouring scale); their descriptors are nearly equal, so the second neighbour of a correct match is its
own twin and the plain ratio test `d0 < 0.9 d1` rejects it.  FGINN takes d1 from the nearest train row whose keypoint lies at least
spatial_th pixels from the nearest neighbour's.  Compares tentatives and inliers of the two rules on K synthetic two-view pairs.
usage: fginn_match_amd.py [K] [n]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pydegensac_amd import synthetic as syn, tensor_api


def scene(K, n, dim=128, twin_share=0.6, seed=0):
    rng = np.random.default_rng(seed)
    K1, K2, D1, D2, lab2 = [], [], [], [], []
    for i in range(K):
        p1, p2, lab, _ = syn.two_view_fundamental(n, 0.6, 0.1, seed=100 + i)
        d1 = rng.normal(size=(n, dim)).astype(np.float32)
        d2 = d1 + 0.15 * rng.normal(size=d1.shape).astype(np.float32)
        d2[~lab] = rng.normal(size=(int((~lab).sum()), dim)).astype(np.float32)
        tw = rng.permutation(n)[:int(twin_share * n)]                   # twins: 1.5 px away, near-equal descriptor
        p2 = np.r_[p2, p2[tw] + [1.5, 0.0]]; d2 = np.r_[d2, d2[tw] + 0.002 * rng.normal(size=(len(tw), dim)).astype(np.float32)]
        perm = rng.permutation(len(p2))
        K1.append(p1); K2.append(p2[perm]); D1.append(d1); D2.append(d2[perm]); lab2.append(lab)
    return K1, K2, D1, D2, lab2


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1500
    dev = torch.device("cuda", 0)
    K1, K2, D1, D2, lab = scene(K, n)
    c1 = [len(x) for x in D1]; c2 = [len(x) for x in D2]
    args = [torch.from_numpy(np.concatenate(x)).to(dev) for x in (K1, K2, D1, D2)] + [c1, c2]
    true = sum(int(x.sum()) for x in lab)
    for name, th in (("plain ratio test", None), ("FGINN, spatial_th 10", 10.0)):
        F, match, inl, st, cnt = tensor_api.match_and_verify_batch_tensors(*args, model="F", ratio=0.9, fginn_th=th)
        print(f"{name:22s} tentatives {int(cnt.sum()):6d}  inliers {int(inl.sum().item()):6d}  (true correspondences in the scene: {true})")


if __name__ == "__main__":
    main()
