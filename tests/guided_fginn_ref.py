"""TEST INFRASTRUCTURE ONLY: FGINN inside the gate of guided matching (include/mi_degensac.h mi_degensac_match_guided_fginn_*), restated
on tests/guided_ref.py (the gate, from the CPU oracle's own residuals) and tests/fginn_ref.py (the exclusion rule), and the scenes the CPU
and GPU tests share.

    G      = guided_ref.gate_matrix;  slot 0 = top2(D, G)[:, 0]  (the plain guided nearest row, the ANCHOR)
    ok     = G & fginn_ref.ok_mask(i0, kp2, r)                    (gated, not the anchor, keypoint at least r from the anchor's)
    slot 1 = top2(D, ok)[:, 0];  needy = the plain guided slot 1 exists and is not ok  (what the device rescans)
    match  = i0 when i0 >= 0 and dist0 < ratio * dist1: the GUIDED decision, so a query whose only gated companions lie inside the radius
             (dist1 = inf) is kept; mutual: the plain reverse guided nearest neighbour must return the query."""
import numpy as np

from oracle import matcher_np as mo
from tests import fginn_ref as fr, guided_ref as gr


def dmat(d1, d2, norm):
    n1, n2 = len(d1), len(d2)
    return fr.dmat(d1, d2, norm) if n1 and n2 else np.zeros((n1, n2), np.float32)


def second_mask(G, i0, k2, r):
    return G & fr.ok_mask(i0, k2, r) if G.shape[1] else G.copy()


def oracle(P, model, et, px, Md, k1, k2, d1, d2, norm, r, ratio, mutual, second=second_mask):
    """(idx [n1, 2], dist [n1, 2], match [n1], needy [n1]) of one entry; `second` = the competition rule (the CPU tests swap in broken ones)"""
    n1 = len(d1)
    G = gr.gate_matrix(P, model, et, px, Md, np.asarray(k1, np.float64)[:, :2], np.asarray(k2, np.float64)[:, :2])
    D = dmat(d1, d2, norm)
    pi, pd = mo.top2(D, G)
    ok = second(G, pi[:, 0], k2, r)
    si, sd = mo.top2(D, ok)
    idx = pi.copy(); dist = pd.copy()
    idx[:, 1] = si[:, 0]; dist[:, 1] = sd[:, 0]
    needy = (pi[:, 1] >= 0) & ~ok[np.arange(n1), np.clip(pi[:, 1], 0, None)] if G.shape[1] else np.zeros(n1, bool)
    keep = (idx[:, 0] >= 0) & (dist[:, 0] < np.float32(ratio) * dist[:, 1])
    if mutual and G.shape[1]:
        back, _ = mo.top2(D.T, G.T)
        keep &= back[np.clip(idx[:, 0], 0, None), 0] == np.arange(n1)
    return idx, dist, np.where(keep, idx[:, 0], -1).astype(np.int32), needy


# ---- scenes ----------------------------------------------------------------------------------------------------------------
F_ROW = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])      # x2^T F x1 = y1 - y2: the band of a query is its own image row


def shift_model(model, a, b):
    """the exact driver-form model of x2 = x1 + (a, b): H_c = inv(H)^T of the translation; F whose band is the image row y2 = y1 + b"""
    return np.array([[1.0, 0, 0], [0, 1, 0], [-a, -b, 1]]) if model == "H" else np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, b]])


def twin_scene(seed, n1, n2, width, norm, n_needy, model, shift=(3.0, -2.0)):
    """fginn_ref.twin_scene under an exact model: query i < m sees train row i through x2 = x1 + shift, so the gate passes the correct row
    AND its twin 1.5 px beside it (same image row: on the F band exactly, 1.5 px inside the H band).  Under H nothing else is gated (the
    grid is 100 px wide): a twinned query's only companion is its twin.  Under F the 37 rows of its grid row are gated too.  The other
    queries lie far off every band.  Exactly n_needy queries are needy at any radius in (1.5, 100].  Returns (k1, k2, a, b, M)."""
    a, b, k2 = fr.twin_scene(seed, n1, n2, width, norm, n_needy)
    m = min(n1, n2 - n_needy)
    k1 = np.c_[-5000.0 - 7.0 * np.arange(n1), -9000.0 - 11.0 * np.arange(n1)]
    k1[:m] = k2[:m] - np.asarray(shift)
    return k1, k2, a, b, shift_model(model, *shift)


def band_scene(levels, gated, xs, n_q=1, width=1):
    """One train image on (gated) or off the image row y = 70 of n_q identical queries at (0, 70) under F_ROW; train row t has x = xs[t] and
    descriptor distance |levels[t]| to every query (float32 rows of `width` words, the level in word 0).  Returns (k1, k2, a, b, M)."""
    n2 = len(levels)
    k2 = np.c_[np.asarray(xs, np.float64), np.where(np.asarray(gated, bool), 70.0, 500.0)]
    k1 = np.tile([[0.0, 70.0]], (n_q, 1))
    a = np.zeros((n_q, width), np.float32); b = np.zeros((n2, width), np.float32); b[:, 0] = levels
    return k1, k2, a, b, F_ROW.copy()


def flush_scene(kind, n_q=3):
    """The rescan's candidate lists at their edges, r = 10.  Every scene: the anchor (level 1), its twin 1 px beside it (level 2: the plain
    second neighbour, so the query is needy) and far competitors 50 px apart with levels from 10 up.
      "exact64"   rows 0 .. 63 compete, anchor 64, twin 65: the list is exactly 64 at the end of step 0, nothing is carried
      "carry63"   rows 0 .. 62 and 64 .. 127 compete, the anchor is row 63, the twin row 128: 63 pending + 64 = 127, a flush leaves 63
      "excluded"  rows 0 .. 63 are twins of the anchor (row 64), rows 65 .. 70 compete: the excluded rows alone would have filled the list
      "chunks"    anchor in the first 1024-row chunk (row 5), twin in the second (row 1050), competitors in both
      "tie_lo" / "tie_hi"  "exact64" with two competitors at the lowest level on both sides of the flush boundary (list positions 63 | 64 /
                  62 | 65): the lower row wins
    Returns (k1, k2, a, b, M, anchor row, expected slot 1)."""
    if kind == "chunks":
        n2, anchor, twins, want = 1100, 5, [1050], 1060
    elif kind == "carry63":
        n2, anchor, twins, want = 130, 63, [128], 100
    elif kind == "excluded":
        n2, anchor, twins, want = 71, 64, list(range(64)), 67
    else:
        n2, anchor, twins, want = 70, 64, [65], 63
    levels = 10.0 + np.arange(n2) % 23 + np.arange(n2) / 4096.0
    xs = 1000.0 + 50.0 * np.arange(n2)
    levels[anchor] = 1.0
    for k, t in enumerate(twins):
        levels[t] = 2.0 + k / 64.0; xs[t] = xs[anchor] + 1.0 + k / 128.0
    if kind == "tie_lo":
        levels[63] = levels[66] = 5.0                        # competitors are rows 0 .. 63, 66 .. 69: list positions 63 and 64
    elif kind == "tie_hi":
        levels[62] = levels[67] = 5.0; want = 62             # positions 62 and 65
    else:
        levels[want] = 5.0
    return band_scene(levels, np.ones(n2, bool), xs, n_q) + (anchor, want)


def offband_scene(n_q=2):
    """the overall nearest train row (row 0) lies OFF the band: the anchor is the nearest GATED row (row 1), its twin row 2; row 3 competes
    and lies within r = 10 of row 0.  A rule anchored at the ungated nearest row excludes row 3 and lets the twin compete.  Returns
    (k1, k2, a, b, M, anchor, expected slot 1)."""
    return band_scene([0.5, 1.0, 2.0, 5.0, 7.0], [False, True, True, True, True], [2000.0, 1000.0, 1001.0, 2003.0, 3000.0], n_q) + (1, 3)


def radius_scene(below=False):
    """integer keypoints under an all-pass gate (identity H, a huge px_th): anchor (0, 0), twin (1, 0), row 2 at (6, 8) — dx dx + dy dy = 100
    = r r exactly at r = 10 — and row 3 far away; below: row 2's y one ulp nearer, so the sum lies below 100.  Three identical queries.
    Returns (k1, k2, a, b, M)."""
    k2 = np.array([[0.0, 0], [1, 0], [6, 8], [60, 80]])
    if below:
        k2[2, 1] = np.nextafter(8.0, 0.0)
    b = np.array([[1.0], [2], [3], [4]], np.float32)
    return np.zeros((3, 2)), k2, np.zeros((3, 1), np.float32), b, np.eye(3)
