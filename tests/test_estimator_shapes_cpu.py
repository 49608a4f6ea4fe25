"""CPU: the families of tests/estimator_shapes.py have teeth before a GPU is involved.  With the restatement alone: the tiling-edge
scenes run several local optimisations, reach DEGENSAC's plane branch and get candidates rejected by the LAF check; every coordinate
frame still yields a model (a frame in which the restatement finds nothing would make the device comparison vacuous); the frame maps
round-trip; and the two predicates that the GPU file applies to the screens' counts reject two broken counters."""
import numpy as np
import pytest

from pydegensac_amd import synthetic as syn
from tests import estimator_shapes as es


def test_edge_family_runs_local_optimisations_the_plane_branch_and_the_laf_check(oracle_port):
    f = [es.oracle_e(oracle_port, "F", n)[2] for n in es.E]
    h = [es.oracle_e(oracle_port, "H", n)[2] for n in es.E]
    print("F (n, samples, lo_runs, Ih, I):", [(n, s["samples"], s["lo_runs"], s["Ih"], s["I"]) for n, s in zip(es.E, f)])
    print("H (n, samples, lo_runs, I):", [(n, s["samples"], s["lo_runs"], s["I"]) for n, s in zip(es.E, h)])
    assert sum(s["lo_runs"] >= 2 for s in f) >= len(es.E) // 2
    assert sum(s["Ih"] > 0 for s in f) >= 4
    assert all(s["lo_runs"] >= 1 for n, s in zip(es.E, h) if n >= 63)
    assert all(s["I"] >= 7 for s in f) and all(s["I"] >= 4 for s in h)      # every scene yields a model
    for n in es.LAF_NS:
        for kind in ("F", "H"):
            s = es.oracle_e(oracle_port, kind, n, laf=True)[2]
            assert s["rejected"] > 0 and s["I"] > 0, (kind, n, s)


def test_cooperative_scenes_find_models(oracle_port):
    for _, n in es.COOP_CASES:
        A, B, seeds = es.coop_scenes(n)
        assert len(set(seeds)) == len(seeds) and all(a.shape == (n, 2) for a in A)
    A, B, seeds = es.coop_scenes(513)
    st = [oracle_port.find_fundamental(A[p], B[p], 0.5, 0.9999, 20000, seed=seeds[p])[2] for p in range(4)]
    assert all(s["I"] > 100 for s in st) and any(s["degen"] > 0 for s in st), st


@pytest.mark.parametrize("kind", ["F", "H"])
def test_every_frame_keeps_the_model(oracle_port, kind):
    """in every frame, every scene and metric: at least 80 % of the identity frame's inliers"""
    n_scenes = len(es.FRAME_F_SCENES if kind == "F" else es.FRAME_H_SCENES)
    for j in range(n_scenes):
        for et in (es.F_METRICS if kind == "F" else es.H_METRICS):
            base = es.oracle_frame(oracle_port, kind, j, "identity", et)
            assert base[2]["I"] >= 16 and np.abs(base[0]).sum() > 0, (kind, j, et, base[2])
            for frame in es.FRAME_NAMES:
                M, mask, st = es.oracle_frame(oracle_port, kind, j, frame, et)
                assert np.abs(M).sum() > 0 and st["I"] >= 0.8 * base[2]["I"] and mask.sum() >= 0.8 * base[1].sum(), (kind, j, et, frame, st, base[2])
            if kind == "F" and es.FRAME_F_SCENES[j][2] > 0:
                assert base[2]["Ih"] > 0, "the plane-dominated scene must reach DEGENSAC's plane branch"
            if es.frame_scene(kind, j)[3] > 0:
                assert base[2]["rejected"] > 0, "the LAF scene must get candidates rejected"


def test_frames_round_trip_and_scale_the_threshold():
    assert set(es.FRAME_NAMES) == {"identity", "centred", "normalised", "x40", "offset", "anisotropic"}
    p1, p2, _, lc = es.frame_scene("F", 2); assert p1.shape[1] == 6 and lc > 0
    for name, kind in [(f, k) for f in es.FRAME_NAMES for k in "FH"]:
        q1, q2, th = es.to_frame(name, p1, p2, 0.5, kind)
        b1, b2, th0 = es.from_frame(name, q1, q2, th, kind)
        # offsets of 1e6 cost log2(1e6 / 1e3) = 10 bits of the pixel value: 2^-52 * 1e6 = 2.2e-10 absolute
        assert np.abs(b1 - p1).max() < 1e-9 and np.abs(b2 - p2).max() < 1e-9 and abs(th0 - 0.5) < 1e-15, name
        f = es.frame(name, kind)
        assert th == 0.5 * f["th"] and f["th"] == max(f["s1"] + f["s2"]), name      # the threshold takes the (largest) scale of the map
        # the LAF columns move with their points: the extra points (x + a11, y + a21), (x + a12, y + a22) are the images of the pixel frame's
        T1, T2 = es.frame_matrices(name, kind)
        for p, q, T in ((p1, q1, T1), (p2, q2, T2)):
            for cx, cy in ((2, 4), (3, 5)):
                e = np.c_[p[:, 0] + p[:, cx], p[:, 1] + p[:, cy], np.ones(len(p))] @ T.T
                scale = max(1.0, np.abs(e).max())
                assert np.abs(e[:, 0] - (q[:, 0] + q[:, cx])).max() < 1e-12 * scale and np.abs(e[:, 1] - (q[:, 1] + q[:, cy])).max() < 1e-12 * scale, name
    c1, c2, _ = es.to_frame("centred", p1, p2, 0.5)
    assert (c1[:, :2] < 0).any() and (c1[:, :2] > 0).any()
    n1, n2, th = es.to_frame("normalised", p1, p2, 0.5)
    assert np.abs(n1[:, :2]).max() < 2 and th == 0.5 / es.FOCAL
    o1, _, _ = es.to_frame("offset", p1, p2, 0.5); assert o1[:, :2].min() > 9e5
    a1, a2, _ = es.to_frame("anisotropic", p1, p2, 0.5); assert a2[:, :2].max() < 0 and a1[:, :2].min() > -50
    assert es.frame("offset", "H")["t1"] == (1e6, 1e6) and es.frame("offset", "H")["t2"] == (1e3, 1e3) and es.frame("offset")["t2"] == (1e6, 1e6)


def test_models_move_into_a_frame_with_their_points():
    p1, p2, lab, F = syn.two_view_fundamental(400, 0.5, 0.0, seed=2)
    h1, h2, hl, H = syn.homography_pairs(400, 0.5, 0.0, seed=2)
    for name in es.FRAME_NAMES:
        q1, q2, th = es.to_frame(name, p1, p2, 1.0)
        d = es.sampson_f(es.f_in_frame(name, F), q1, q2)
        assert d[lab].max() < 1e-6 * th * th and np.median(d[~lab]) > 10 * th * th, (name, d[lab].max())
        g1, g2, _ = es.to_frame(name, h1, h2, 1.0, "H")
        G = es.h_raw_in_frame(name, H).reshape(3, 3).T              # raw is column-wise: image 2 -> image 1
        x = np.c_[g2, np.ones(len(g2))] @ G.T; x = x[:, :2] / x[:, 2:3]
        assert np.abs(x - g1)[hl].max() < 1e-5 * th, (name, np.abs(x - g1)[hl].max())


def _tiled_counts(inside, broken=None):
    """numpy restatement of a tile count (dg_l1_tile_counts): 256 rows per step, lanes past the end load the clamped row n - 1 and are
    masked out.  broken = "drop_last": the mask cuts one row too many; "clamp_twice": the first masked lane is counted."""
    inside = np.asarray(inside, bool); nm, n = inside.shape; cnt = np.zeros(nm, np.int64)
    for base in range(0, n, 256):
        rows = np.minimum(np.arange(base, base + 256), n - 1)
        on = np.arange(base, base + 256) < (n - 1 if broken == "drop_last" else n)
        if broken == "clamp_twice" and not on.all():
            on[np.argmin(on)] = True
        cnt += (inside[:, rows] & on).sum(axis=1)
    return cnt


@pytest.mark.parametrize("n", [64, 255, 256, 257, 513])
def test_superset_predicates_reject_a_dropped_and_a_doubled_row(n):
    p1, p2, lab, F = es.far_outlier_scene(n, seed=900 + n)
    rng = np.random.default_rng(n)
    models = np.stack([F.ravel()] + [rng.normal(size=9) for _ in range(4)])
    R = np.stack([es.sampson_f(m, p1, p2) for m in models])
    huge = 4 * R.max(); tiny = 1e-6
    good = _tiled_counts(R < huge * 9 / 4)
    assert es.superset_ok(good, R, huge) and es.all_in_band_ok(good, R, huge)
    drop = _tiled_counts(R < huge * 9 / 4, "drop_last")
    assert not es.superset_ok(drop, R, huge) and not es.all_in_band_ok(drop, R, huge)
    if n % 256:                                                    # a full last tile has no clamped lane
        twice = _tiled_counts(R < huge * 9 / 4, "clamp_twice")
        assert es.superset_ok(twice, R, huge), "the inequality alone cannot see a row counted twice"
        assert not es.all_in_band_ok(twice, R, huge)
    # noise-free inliers, outliers far from every epipolar line, tiny threshold: the band of the fitted model is the inlier set
    exact = (R[:1] < tiny * 9 / 4).sum(axis=1)
    assert exact[0] == lab.sum() and (R[0][~lab] > 1.0).all(), (exact, lab.sum())
    last_in = np.zeros((1, n), bool); last_in[0] = R[0] < tiny * 9 / 4
    last_in[0, -1] = True                                          # the property "count == exact" sees the doubled row when it is in the band
    if n % 256:
        assert _tiled_counts(last_in, "clamp_twice")[0] == last_in.sum() + 1
    assert _tiled_counts(last_in, "drop_last")[0] == last_in.sum() - 1
