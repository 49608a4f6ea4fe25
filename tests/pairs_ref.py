"""TEST INFRASTRUCTURE ONLY: what a pair list over image stores means, in terms of the ragged batch the existing calls take.

Given the stores (row arrays with rows-per-image counts) and a pair list, `expand` copies pair p's rows out of the stores, pair after
pair in list order: the duplicated arrays and counts of knn_match_batch_tensors / match_and_verify_batch[_tensors], and the
pair_offsets the pair-list calls must return.  It has no other logic; the pair-list calls are tested for equality with the existing
calls on this expansion."""
import numpy as np


def offsets(counts):
    o = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=o[1:])
    return o


def expand(store1, counts1, store2, counts2, pairs):
    """store1 / store2: tuples of row arrays of the two stores (descriptors, keypoints, ...), every array with one row per store row.
    Returns (copies1, copies2, c1, c2, pair_offsets): per array of store1 the rows of image pairs[p][0] for p = 0 .. K - 1 concatenated,
    per array of store2 those of image pairs[p][1], the rows per pair of both sides and the int64 offsets [K + 1] of side 1."""
    o1, o2 = offsets(counts1), offsets(counts2)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    r1 = [np.arange(o1[i], o1[i + 1]) for i in pairs[:, 0]]
    r2 = [np.arange(o2[j], o2[j + 1]) for j in pairs[:, 1]]
    rows1 = np.concatenate(r1) if r1 else np.zeros(0, np.int64)
    rows2 = np.concatenate(r2) if r2 else np.zeros(0, np.int64)
    c1 = np.array([len(r) for r in r1], np.int64); c2 = np.array([len(r) for r in r2], np.int64)
    return tuple(np.ascontiguousarray(a[rows1]) for a in store1), tuple(np.ascontiguousarray(a[rows2]) for a in store2), c1, c2, offsets(c1)
