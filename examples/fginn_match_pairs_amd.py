"""The FGINN ratio test over a pair list: a small image collection with twinned keypoints, every image stored once.  A detector such as
SIFT emits several keypoints for one image structure (a second orientation, a neighbouring scale) with nearly equal descriptors; the
second neighbour of a correct match is then its own twin and the plain ratio test `d0 < 0.9 d1` rejects it.  FGINN takes d1 from the
nearest row of the train image whose keypoint lies at least spatial_th pixels from the nearest neighbour's.  Prints tentatives and
inliers per pair with and without the rule; both calls read the same image stores, no row is copied per pair.
usage: fginn_match_pairs_amd.py [M] [n]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pydegensac_amd import matcher, synthetic as syn, tensor_api


def twinned_collection(M, n, dim=64, twin_share=0.5, seed=0):
    """synthetic.image_collection with a twin for a share of every image's keypoints: one more row 1.5 px away, near-equal descriptor"""
    rng = np.random.default_rng(seed)
    kps, descs = syn.image_collection(M, n, 0.6, 0.1, dim, seed=seed)
    for i in range(M):
        tw = rng.permutation(n)[:int(twin_share * n)]
        k = np.r_[kps[i], kps[i][tw] + [1.5, 0.0]]
        d = np.r_[descs[i], descs[i][tw] + 0.002 * rng.normal(size=(len(tw), dim)).astype(np.float32)]
        perm = rng.permutation(len(k))
        kps[i] = np.ascontiguousarray(k[perm]); descs[i] = np.ascontiguousarray(d[perm])
    return kps, descs


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    dev = torch.device("cuda", 0)
    kps, descs = twinned_collection(M, n)
    pairs = matcher.exhaustive_pairs(M)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    kw = dict(model="F", ratio=0.9, max_iters=20000)
    plain = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, **kw)
    fginn = tensor_api.match_and_verify_fginn_pairs_tensors(k, k, d, d, counts, counts, pairs, 10.0, **kw)
    po = plain[5]
    print(f"{M} images x {counts[0]} keypoints (half of them twinned), {len(pairs)} pairs, descriptor rows on the device: {d.shape[0]}")
    print("pair      plain: tentatives inliers    FGINN (spatial_th 10): tentatives inliers")
    for p, (i, j) in enumerate(pairs):
        a = int(plain[2][po[p]:po[p + 1]].sum().item()); b = int(fginn[2][po[p]:po[p + 1]].sum().item())
        print(f"({i}, {j})  {int(plain[4][p]):18d} {a:7d} {int(fginn[4][p]):33d} {b:7d}")
    # the same through numpy lists (each image uploaded once): identical results
    Fh, mh, ih = matcher.match_and_verify_fginn_pairs(kps, descs, pairs, 10.0, **kw)
    inl = fginn[2].cpu().numpy()
    print("numpy entry point identical:", np.array_equal(Fh, fginn[0].cpu().numpy()) and all(np.array_equal(ih[p], inl[po[p]:po[p + 1]]) for p in range(len(pairs))))


if __name__ == "__main__":
    main()
