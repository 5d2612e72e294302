"""Descriptor scenes in which the projection matchers' sequential rules decide
the result (numpy and the package's host-side types; no oracle, no device).

synth.synth_scene and build_local_map draw uniformly random descriptors: a
true match sits at distance <= 40 and every distractor near 128, so neither
the claim order, the distance ties, the ratio test nor the <= TH_HIGH boundary
ever changes an assignment there (docs/ORACLE_ASSUMPTIONS.md A29). The scenes
here keep that geometry and replace the descriptors with rows drawn from a
ladder of prototypes, so distances cover 0..130 densely and many keypoints
compete for the same map points; and hand-built clusters in which every
distance is 0, so the candidate order alone decides."""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd import synth
from gf_orb_slam_amd.matcher import MP_VIEW_DTYPE, Frame, FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

GRID_COLS, GRID_ROWS = 64, 48  # Frame.h:35-36

# (rungs, step, flips) of the ladders the tests use
LADDERS = [(5, 24, 6), (6, 20, 4), (4, 33, 8), (5, 25, 3)]


def ladder_descriptors(rng, n: int, rungs: int, step: int, flips: int) -> np.ndarray:
    """n descriptors [n, 32] near a ladder of `rungs` prototypes: prototype 0
    is random, prototype j is prototype j - 1 with `step` further bits flipped
    on positions no other rung uses, so prototypes i and j are exactly
    |i - j| * step apart; each row is a random prototype with 0..flips random
    bits flipped. Map points and keypoints of one scene come from one call."""
    assert (rungs - 1) * step <= 256
    bits = rng.integers(0, 2, 256, dtype=np.uint8)
    order = rng.permutation(256)
    protos = np.empty((rungs, 256), np.uint8)
    protos[0] = bits
    for j in range(1, rungs):
        protos[j] = protos[j - 1]
        protos[j, order[(j - 1) * step:j * step]] ^= 1
    rows = protos[rng.integers(0, rungs, n)]
    for i in range(n):
        k = int(rng.integers(0, flips + 1))
        if k:
            rows[i, rng.choice(256, k, replace=False)] ^= 1
    return np.ascontiguousarray(np.packbits(rows, axis=1, bitorder="little"))


def hamming(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8), axis=-1).sum(-1)


def ladder_scene(camera: str, n_mp: int, n_kp: int, seed: int, ladder) -> dict:
    """synth.synth_scene's geometry with map-point and keypoint descriptors
    from one ladder."""
    sc = synth.synth_scene(camera, n_mp, n_kp, seed)
    rng = np.random.default_rng(seed + 7000)
    d = ladder_descriptors(rng, n_mp + n_kp, *ladder)
    sc["mp_desc"] = np.ascontiguousarray(d[:n_mp])
    sc["descriptors"] = np.ascontiguousarray(d[n_mp:])
    return sc


def quantise_angles(rng, angles: np.ndarray, offsets=(0.0, 3.0, -3.0, 6.0)) -> np.ndarray:
    """Angles snapped to multiples of 12 degrees plus one of a few offsets:
    rotation differences then take few values, some on a histogram bin's
    boundary (15 + 30 k), where the float rounding of `rot * factor` picks
    the bin. The wrong matches of a ladder scene spread over all 13 bins, so
    the orientation check undoes many of them; exact ties between bins and the
    0.1 rule are pinned by cluster_rotation below."""
    q = np.round(np.asarray(angles, np.float64) / 12.0) * 12.0 + rng.choice(np.asarray(offsets), len(angles))
    return (q % 360.0).astype(np.float32)


def lastframe_pair(seed: int, nmp: int = 800, nkp: int = 600, rot_deg: float = 0.3):
    """Two frames for SearchByProjection(Cur, Last) (the geometry of
    test_match_gpu's pairs): the last frame observes a synth_scene with 1/15 of
    its keypoints outliers, the current frame sees the same map from a slightly
    moved camera -> (last, cur, info)."""
    sc = synth.synth_scene("euroc", nmp, nkp, seed)
    info = FrameInfo.make(*sc["camera"])
    rng = np.random.default_rng(seed + 100)
    last = Frame(sc["keypoints"], sc["descriptors"], info, sc["Tcw"])
    last.mvpMapPoints[:] = sc["kp_mp"]
    ok = sc["kp_mp"] >= 0
    last.mp_pos[ok] = sc["map"]["pos"][sc["kp_mp"][ok]]
    last.mvbOutlier[rng.choice(nkp, nkp // 15, replace=False)] = 1
    d = synth.look_pose(rng, 0.01, rot_deg).astype(np.float64)
    Tc = (d @ sc["Tcw"].astype(np.float64)).astype(np.float32)
    u, v, _ = synth.project(Tc, sc["map"]["pos"].astype(np.float64), sc["camera"])
    kps = sc["keypoints"].copy()
    m = sc["kp_mp"]
    kps["x"][ok] = np.clip(u[m[ok]] + rng.uniform(-1, 1, ok.sum()), 0, 751)
    kps["y"][ok] = np.clip(v[m[ok]] + rng.uniform(-1, 1, ok.sum()), 0, 479)
    kps["angle"] = (kps["angle"] + 4.0 + rng.normal(0, 3, nkp)) % 360
    cur = Frame(kps, synth.flip_bits(rng, sc["descriptors"], 10), info, Tc)
    return last, cur, info


RELOC_CAMERA = (752, 480, 458.654, 457.296, 367.215, 248.375)


def _pose(rx, ry, tx, ty, tz):
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (tx, ty, tz)
    return T.astype(np.float32)


def reloc_pair(seed: int, n: int = 540) -> dict:
    """Two frames for the track-loss matchers (the geometry of
    test_track_loss_gpu's pairs): n points seen from two nearby poses, F1
    (last frame, map point ids, 15% NULL) and F2 (the visible points with
    jittered positions and angles plus 10% clutter, in an unrelated order).
    Descriptors are placeholders: relabel_two_frames sets them."""
    w, h, fx, fy, cx, cy = RELOC_CAMERA
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(2.5, 9, n)], 1).astype(np.float32)
    T1, T2 = _pose(0, 0, 0, 0, 0), _pose(0.01, -0.02, 0.05, -0.02, 0.03)

    def proj(T):
        Pc = X.astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]
        return fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy

    (u1, v1), (u2, v2) = proj(T1), proj(T2)
    vis = (u1 > 1) & (u1 < 750) & (v1 > 1) & (v1 < 478) & (u2 > 1) & (u2 < 750) & (v2 > 1) & (v2 < 478)
    X, u1, v1, u2, v2 = X[vis], u1[vis], v1[vis], u2[vis], v2[vis]
    m = len(X)
    oct_ = rng.integers(0, 8, m)
    K1 = np.zeros(m, KEYPOINT_DTYPE)
    K1["x"], K1["y"], K1["octave"], K1["angle"] = u1, v1, oct_, rng.uniform(0, 360, m)
    mp1 = rng.permutation(4000)[:m].astype(np.int32)
    mp1[rng.uniform(size=m) < 0.15] = -1
    nc = m // 10
    K2 = np.zeros(m + nc, KEYPOINT_DTYPE)
    K2["x"][:m] = u2 + rng.normal(0, 0.7, m)
    K2["y"][:m] = v2 + rng.normal(0, 0.7, m)
    K2["octave"][:m] = oct_
    K2["angle"][:m] = (K1["angle"] + rng.normal(0, 4, m)) % 360
    K2["x"][m:], K2["y"][m:] = rng.uniform(0, 751, nc), rng.uniform(0, 479, nc)
    K2["octave"][m:], K2["angle"][m:] = rng.integers(0, 8, nc), rng.uniform(0, 360, nc)
    perm = rng.permutation(len(K2))  # keypoint order unrelated to F1's
    zero = np.zeros((0, 32), np.uint8)
    return dict(X=X, T1=T1, T2=T2, K1=K1, D1=zero, mp1=mp1, K2=K2[perm], D2=zero)


def relabel_two_frames(F: dict, seed: int, ladder, quantise: bool = True) -> dict:
    """A reloc_pair problem with both frames' descriptors from one ladder and
    (optionally) quantised angles."""
    rng = np.random.default_rng(seed + 7100)
    n1, n2 = len(F["K1"]), len(F["K2"])
    d = ladder_descriptors(rng, n1 + n2, *ladder)
    F = dict(F)
    F["D1"], F["D2"] = np.ascontiguousarray(d[:n1]), np.ascontiguousarray(d[n1:])
    if quantise:
        F["K1"], F["K2"] = F["K1"].copy(), F["K2"].copy()
        F["K1"]["angle"] = quantise_angles(rng, F["K1"]["angle"])
        F["K2"]["angle"] = quantise_angles(rng, F["K2"]["angle"])
    return F


# ------------------------------------------------------------------ clusters
CLUSTER_CAMERA = (752, 480, 457.3, 457.3, 367.215, 248.375)
CLUSTER_SIZES = [1, 3, 4, 5, 6, 9, 64, 65, 70, 130]
_DESC = np.arange(32, dtype=np.uint8) * 7 + 3  # the one descriptor of a cluster scene


def _cell(x, y):
    """Frame::PosInGrid (Frame.cc:367-377) in float, as the matchers compute it."""
    w, h = CLUSTER_CAMERA[:2]
    invW, invH = np.float32(GRID_COLS) / np.float32(w), np.float32(GRID_ROWS) / np.float32(h)
    fx, fy = np.asarray(x, np.float32) * invW, np.asarray(y, np.float32) * invH
    assert np.all(np.abs(fx - np.floor(fx) - 0.5) > 1e-3) and np.all(np.abs(fy - np.floor(fy) - 0.5) > 1e-3)
    return np.floor(fx + np.float32(0.5)).astype(int), np.floor(fy + np.float32(0.5)).astype(int)


def _cluster_keypoints(n: int, variant: str):
    """n octave-0 keypoints 0.05 px apart around the image centre, all within
    every query's window. "one": a single grid cell, so the candidate order is
    the keypoint order. "columns": keypoint i sits in grid column 31 - (i % 2)
    and row 20 + (i // 2) % 2, so the candidate order (column, then row, then
    index: Frame.cc:329-360) differs from the keypoint order."""
    kps = np.zeros(n, KEYPOINT_DTYPE)
    i = np.arange(n)
    kps["octave"], kps["size"], kps["class_id"] = 0, 31.0, -1
    if variant == "one":
        kps["x"], kps["y"] = 359.0 + 0.05 * i, 236.0
    else:
        # columns 30 | 31 meet at x = 30.5 * 11.75 = 358.375, rows 20 | 21 at y = 205
        kps["x"] = np.where(i % 2 == 0, 359.0, 357.5 - 0.05 * (n // 2)) + 0.05 * (i // 2)
        kps["y"] = np.where((i // 2) % 2 == 0, 203.0, 207.0)
    cx, cy = _cell(kps["x"], kps["y"])
    order = np.lexsort((i, cy, cx))  # candidate order of a window that holds them all
    return kps, order


def _cluster_expected(n: int, order: np.ndarray, c: int, pre: np.ndarray, ids: np.ndarray):
    """The sequential loop on all-zero distances: `dist < bestDist` keeps the
    first unclaimed candidate, so query k takes the k-th unclaimed keypoint in
    candidate order; the rest stay as they were."""
    kp2mp = np.full(n, -1, np.int32)
    score = np.full(n, 999, np.int32)
    kp2mp[pre] = 500000 + pre
    score[pre] = 7
    free = [j for j in order if kp2mp[j] < 0]
    assert len(free) >= c
    for k in range(c):
        kp2mp[free[k]] = ids[k]
        score[free[k]] = 0
    return kp2mp, score


def _cluster_frame(c: int, extra: int, variant: str, preclaimed: int):
    n = c + extra + preclaimed
    kps, order = _cluster_keypoints(n, variant)
    pre = (1 + np.arange(preclaimed)) * n // (preclaimed + 1)  # spread over the keypoints, distinct
    kp2mp = np.full(n, -1, np.int32)
    score = np.full(n, 999, np.int32)
    kp2mp[pre] = 500000 + pre
    score[pre] = 7
    desc = np.ascontiguousarray(np.tile(_DESC, (n, 1)))
    return n, kps, desc, order, pre, kp2mp, score


def cluster_lastframe(c: int, extra: int = 2, variant: str = "one", preclaimed: int = 0, bins=None,
                      keep=None) -> dict:
    """SearchByProjection(Cur, Last, th = 15) on c last-frame keypoints whose
    map points (depth 4, 0.0005 apart, identity pose) project within a grid
    cell of each other, against c + extra (+ preclaimed) identical-descriptor
    keypoints inside every window. expect_*: the hand-derived result.

    bins (one per query) / keep: the rotation bin query k's match falls in and
    the bins that survive the orientation check. The match of query k is known
    (the k-th free keypoint), so its angles are set to a rotation of
    30 x bins[k] + {-14, 0, 14} degrees (inside the bin), every other pair through the
    `rot < 0` wrap; matches outside `keep` are expected to be undone. Without
    bins all angles are 0 (one bin, nothing undone)."""
    w, h, fx, fy, cx, cy = CLUSTER_CAMERA
    n, kps, desc, order, pre, kp2mp, score = _cluster_frame(c, extra, variant, preclaimed)
    last_kps = np.zeros(c, KEYPOINT_DTYPE)
    last_kps["octave"], last_kps["size"], last_kps["class_id"] = 0, 31.0, -1
    pos = np.zeros((c, 3), np.float32)
    x0, y0 = (359.0 - cx) / fx * 4.0, (np.float32(kps["y"].mean()) - cy) / fy * 4.0
    pos[:, 0], pos[:, 1], pos[:, 2] = x0 + 0.0005 * np.arange(c), y0, 4.0
    # where the points project (0.057 px apart): WindowSearch searches around these
    last_kps["x"], last_kps["y"] = 359.0 + 0.057 * np.arange(c), np.float32(kps["y"].mean())
    ids = (1000 + np.arange(c)).astype(np.int32)
    ekm, esc = _cluster_expected(n, order, c, pre, ids)
    nkeep = c
    if bins is not None:
        assert len(bins) == c and max(bins) <= 12
        free = [j for j in order if kp2mp[j] < 0][:c]
        for k, j in enumerate(free):
            cur = 350.0 if k % 2 else 0.0
            kps["angle"][j] = cur
            jit = (-14.0, 0.0, 14.0)[k % 3]
            if bins[k] == 0 and jit < 0 or bins[k] == 12 and jit >= 0:
                jit = -jit if jit else -7.0  # bin 0 is [0, 15), bin 12 is [345, 360)
            last_kps["angle"][k] = (30.0 * bins[k] + jit + cur) % 360.0
            if bins[k] not in keep:
                ekm[j], esc[j] = -1, 999  # ORBmatcher.cc:2183-2186
                nkeep -= 1
    return dict(camera=CLUSTER_CAMERA, th=15.0, kps=kps, desc=desc, Tcw=np.eye(4, dtype=np.float32),
                last_kps=last_kps, last_desc=np.ascontiguousarray(np.tile(_DESC, (c, 1))), last_kp2mp=ids,
                last_outlier=np.zeros(c, np.uint8), last_pos=pos, kp2mp=kp2mp, score=score, expect_kp2mp=ekm,
                expect_score=esc, expect_n=nkeep)


def cluster_project(c: int, extra: int = 2, variant: str = "one", preclaimed: int = 0) -> dict:
    """SearchByProjection(F, map points, th = 5) on c map points in view at
    level 0 (window 4 x 5 px) 0.057 px apart, against c + extra (+ preclaimed)
    identical-descriptor keypoints inside every window. Every distance is 0,
    so the ratio test (0 > nnratio x 0) never rejects."""
    n, kps, desc, order, pre, kp2mp, score = _cluster_frame(c, extra, variant, preclaimed)
    views = np.zeros(c, MP_VIEW_DTYPE)
    views["u"] = 359.0 + 0.057 * np.arange(c)
    views["v"] = np.float32(kps["y"].mean())
    views["view_cos"], views["level"], views["in_view"] = 0.9, 0, 1
    ids = np.arange(c, dtype=np.int32)
    ekm, esc = _cluster_expected(n, order, c, pre, ids)
    return dict(camera=CLUSTER_CAMERA, th=5.0, kps=kps, desc=desc, views=views,
                mp_desc=np.ascontiguousarray(np.tile(_DESC, (c, 1))), kp2mp=kp2mp, score=score, expect_kp2mp=ekm,
                expect_score=esc, expect_n=c)


CLUSTER_VARIANTS = [("one", 0), ("columns", 0), ("one", 3), ("columns", 5)]


# Rotation histograms for cluster_lastframe, derived by hand from
# ComputeThreeMaxima (ORBmatcher.cc:2338-2379): (matches per bin, surviving bins).
ROTATION_PLANS = {
    # bins 5 and 9 tie for third place: `s > max3` keeps the first, bin 5, and
    # 3 < 0.1f x 30 is false (the float product is exactly 3), so it survives
    "tie_for_third": ({1: 2, 3: 30, 5: 3, 7: 30, 9: 3, 12: 2}, {3, 7, 5}),
    # 4 < 0.1f x 41: the second maximum falls below a tenth, only the first survives
    "second_below_tenth": ({2: 41, 6: 4, 10: 4, 11: 1}, {2}),
    # 3 < 0.1f x 40: the third maximum is dropped, the second stays
    "third_below_tenth": ({0: 3, 4: 40, 8: 20, 12: 2}, {4, 8}),
    # three bins tie for first place: the strict comparisons keep index order
    "three_way_tie": ({2: 10, 5: 10, 6: 10, 11: 10}, {2, 5, 6}),
}


def cluster_rotation(plan: str, variant: str = "one", preclaimed: int = 0) -> dict:
    """cluster_lastframe with the plan's bins dealt over the queries in a fixed
    shuffled order."""
    hist, keep = ROTATION_PLANS[plan]
    bins = np.repeat(list(hist.keys()), list(hist.values()))
    bins = bins[np.random.default_rng(5).permutation(len(bins))]
    return cluster_lastframe(len(bins), 2, variant, preclaimed, bins=[int(b) for b in bins], keep=keep)
