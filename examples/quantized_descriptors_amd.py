#!/usr/bin/env python
"""Float descriptors, as every extractor emits them, through the fast matcher path: quantise once to uint8 rows on the GPU
(matcher.quantize_descriptors), then match and verify a whole collection under norm="l2_u8", whose distances are exact integers on
the int8 matrix cores and whose stores are a quarter of the float32 size."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))    # run from a checkout

from pydegensac_amd import matcher, synthetic

if __name__ == '__main__':
    M, n, dim = 8, 1500, 128
    kps, descs = synthetic.image_collection(M, n, 0.6, 0.1, dim, seed=0)        # signed float32 descriptors, like a learned extractor's
    pairs = matcher.exhaustive_pairs(M)
    # preset "unit": L2-normalise, scale by 256, centre on 128 (a common offset cancels in every difference).  "sift" and
    # "rootsift" are the x 512 conventions for non-negative histograms; normalize= / scale= / offset= override a preset
    q, clipped = zip(*(matcher.quantize_descriptors(d, "unit", return_clipped=True) for d in descs))
    print("{} images x {} x {} float32 -> uint8: {} clipped columns, {} dead rows".format(
        M, n, dim, sum(int(c[c > 0].sum()) for c in clipped), sum(int((c < 0).sum()) for c in clipped)))
    Fq, mq, iq = matcher.match_and_verify_pairs(kps, list(q), pairs, model="F", ratio=0.9, mutual=True, px_th=0.5, conf=0.999, max_iters=50000,
                                                norm="l2_u8")
    Ff, mf, jf = matcher.match_and_verify_pairs(kps, descs, pairs, model="F", ratio=0.9, mutual=True, px_th=0.5, conf=0.999, max_iters=50000)
    print("{} pairs matched and verified on both stores: {:.2f} MB as uint8, {:.2f} MB as float32".format(
        len(pairs), sum(x.nbytes for x in q) / 1e6, sum(x.nbytes for x in descs) / 1e6))
    print("inliers per pair, uint8 / float32: median {:.0f} / {:.0f}".format(np.median([i.sum() for i in iq]), np.median([i.sum() for i in jf])))
    same = np.mean([np.mean(a[(a >= 0) & (b >= 0)] == b[(a >= 0) & (b >= 0)]) for a, b in zip(mq, mf)])
    print("queries matched on both paths that got the same train row: {:.2f} %".format(100 * same))
    # a distance between quantised rows is about scale x the float distance of the normalised rows: a max_dist of 0.8 in float units
    # is 0.8 * 256 here
    qi, ti, di = matcher.match_mnn(q[0], q[1], max_dist=0.8 * 256, norm="l2_u8")
    print("mutual nearest neighbours of images 0 and 1 within 0.8 (float units): {}, largest distance {:.1f} / 256".format(len(qi), di.max()))
