"""Matching rules for learned descriptors (SuperPoint / DISK / ALIKED / HardNet style) on a synthetic collection.

Dense learned detections have many near neighbours: a keypoint's descriptor lies close to those of the detections around it, so the
second-nearest-neighbour ratio test of SIFT pipelines throws correct matches away.  Their pipelines match by mutual nearest neighbour
under an absolute distance threshold (MNN + max_dist), or with the ratio test checked in both directions (SMNN).  All three rules run
through the same one-synchronisation call; only the decision differs:

    python examples/learned_descriptors_amd.py [--images 6] [--rows 1500]

prints tentatives and F inliers per pair under ratio=0.9, under MNN + max_dist, and under SMNN at two ratios."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # run from a checkout without installing
from pydegensac_amd import matcher, synthetic as syn, tensor_api

DIM = 128


def collection(m, n, twins=3, spread=(0.1, 1.0), seed=0):
    """image_collection with `twins` extra detections around every keypoint of every image: nearly the same place (within 2 px) and a
    descriptor (unit rows) near the keypoint's own, as a dense detector emits them.  How near differs from keypoint to keypoint, between
    spread[0] (indistinguishable twins) and spread[1] (a distinctive structure), drawn once per keypoint and image"""
    kps, descs = syn.image_collection(m, n // (twins + 1), 0.5, 0.1, DIM, seed=seed)
    rng = np.random.default_rng(seed + 1)
    K, D = [], []
    for k, d in zip(kps, descs):
        k = np.repeat(k, twins + 1, 0); d = np.repeat(np.asarray(d, np.float32), twins + 1, 0)
        k[:, :2] += rng.uniform(-2.0, 2.0, (len(k), 2))
        sp = np.repeat(rng.uniform(spread[0], spread[1], len(k) // (twins + 1)), twins + 1)[:, None]
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        d = d + (sp * rng.normal(0.0, 1.0 / np.sqrt(DIM), d.shape)).astype(np.float32)
        K.append(k); D.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    return K, D


def run(images=6, rows=1500, max_dist=0.7, out=print):
    dev = torch.device("cuda", 0)
    kps, descs = collection(images, rows)
    counts = [len(d) for d in descs]
    k = torch.from_numpy(np.concatenate(kps)).to(dev); d = torch.from_numpy(np.concatenate(descs)).to(dev)
    pairs = matcher.exhaustive_pairs(images)
    rules = {"ratio=0.9": dict(ratio=0.9), f"MNN + max_dist={max_dist}": dict(ratio=None, mutual=True, max_dist=max_dist),
             "SMNN ratio=0.9": dict(ratio=0.9, mutual="ratio"), "SMNN ratio=0.98": dict(ratio=0.98, mutual="ratio")}
    table = {}
    for name, kw in rules.items():
        F, match, inl, stats, cnt, po = tensor_api.match_and_verify_pairs_tensors(k, k, d, d, counts, counts, pairs, max_iters=2000, **kw)
        n_in = np.add.reduceat(inl.cpu().numpy().astype(np.int64), po[:-1]) if len(inl) else np.zeros(len(pairs), np.int64)
        table[name] = (cnt, n_in)
    out(f"{images} images x {counts[0]} rows, {len(pairs)} pairs: tentatives / inliers per pair")
    out("pair      " + "".join(f"{name:>28s}" for name in table))
    for p, (i, j) in enumerate(pairs):
        out(f"({i:2d},{j:2d})   " + "".join(f"{int(c[p]):>20d} /{int(n[p]):>6d}" for c, n in table.values()))
    out("mean      " + "".join(f"{c.mean():>20.1f} /{n.mean():>6.1f}" for c, n in table.values()))
    return table


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=6)
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--max-dist", type=float, default=0.7)
    a = ap.parse_args()
    run(a.images, a.rows, a.max_dist)
