"""numpy / pure-Python restatement of the tracks contract (include/mi_degensac.h mi_degensac_tracks_*): a plain union-find whose root is
the smaller node, then the grouping by a stable argsort.  Written from the header's text, it shares nothing with csrc/mi_tracks.hip."""
import numpy as np


def offsets(counts, first=0):
    return np.concatenate([[first], first + np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def labels(rows, off, total=None):
    """label [R] int32: the smallest node of every node's component.  off: the store's offsets [n_images + 1]; node k = row off[0] + k"""
    lo, hi = int(off[0]), int(off[-1])
    R = hi - lo
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    n = len(rows) if total is None else max(0, min(int(total), len(rows)))
    parent = list(range(R))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for a, b in rows[:n].tolist():
        if not (lo <= a < hi and lo <= b < hi):
            continue
        ra, rb = find(a - lo), find(b - lo)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(k) for k in range(R)], np.int32).reshape(R)


def image_of(off, rows):
    """the last i with off[i] <= row (i < n_images), which skips empty images"""
    off = np.asarray(off, np.int64)
    return (np.searchsorted(off[:-1], np.asarray(rows, np.int64), side="right") - 1).astype(np.int32)


def group(label, off):
    """every output of the call from the labels, at full length with the tail fills"""
    label = np.asarray(label, np.int32)
    R = len(label); half = R // 2; lo = int(off[0])
    size = np.bincount(label, minlength=R)
    in_track = size[label] >= 2
    key = np.where(in_track, label, R)
    order = np.argsort(key, kind="stable")
    n_obs = int(in_track.sum())
    members = order[:n_obs]
    roots = np.flatnonzero(size >= 2)                                  # ascending: the tracks in their numbering
    n_tracks = len(roots)
    number = np.full(R + 1, -1, np.int64); number[roots] = np.arange(n_tracks)
    track = np.where(in_track, number[label], -1).astype(np.int32)
    track_offsets = np.full(half + 1, n_obs, np.int64)
    track_offsets[:n_tracks] = np.concatenate([[0], np.cumsum(size[roots])])[:n_tracks]
    obs = np.full(R, -1, np.int32); obs[:n_obs] = members + lo
    obs_image = np.full(R, -1, np.int32); obs_image[:n_obs] = image_of(off, obs[:n_obs])
    track_images = np.full(half, -1, np.int32)
    n_images = len(off) - 1                                            # the distinct (track, image) couples, counted per track
    couples = np.unique(track[members].astype(np.int64) * max(n_images, 1) + obs_image[:n_obs])
    track_images[:n_tracks] = np.bincount(couples // max(n_images, 1), minlength=n_tracks)
    return {"label": label, "track": track, "n_tracks": n_tracks, "n_obs": n_obs, "track_offsets": track_offsets, "obs": obs,
            "obs_image": obs_image, "track_images": track_images}


def tracks(rows, off, total=None):
    return group(labels(rows, off, total), off)


NAMES = ("label", "track", "track_offsets", "obs", "obs_image", "track_images")


def equal(got, want, names=NAMES):
    """every array at full length and both counts"""
    return (int(got["n_tracks"]) == int(want["n_tracks"]) and int(got["n_obs"]) == int(want["n_obs"])
            and all(np.asarray(got[k]).shape == np.asarray(want[k]).shape and np.array_equal(got[k], want[k]) for k in names))
