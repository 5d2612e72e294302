"""Two-frame problems for ORBmatcher::SearchForInitialization and frame lists
for Tracking::Initialize. Every scene is a dict with ``kps1``, ``desc1``,
``kps2``, ``desc2`` and ``prev`` (vbPrevMatched before the call, float32
[n1, 2]); all are generated from a seed.

``two_view``   synth_two_view geometry with descriptors that match;
``sequence``   one initial frame and any number of later views of the same
               points (a pure rotation has no parallax);
``contended``  a few hundred keypoints in descriptor clusters, built so that
               queries steal from each other, the vMatchedDistance filter
               hides candidates, distances tie inside one cell and across
               cells, bestDist is exactly 50 and 51, the ratio test sits on
               both sides of 0.9f, robbed queries leave stale histogram
               entries, and vbPrevMatched points lie near and beyond the grid;
``crowded``    at least 600 level-0 keypoints of F2 inside one 200 x 200
               window: more than any per-query list holds;
``edge``       the degenerate shapes by name."""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd.matcher import FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
from gf_orb_slam_amd.synth import synth_two_view

W, H, F = 752, 480, 458.0
INFO = FrameInfo.make(W, H, F, F, W / 2, H / 2)
K = np.array([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1]], np.float32)


def kparr(xy, octave, angle):
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["class_id"], k["response"] = 31.0, -1, 50.0
    k["octave"], k["angle"] = octave, angle
    return k


def prev_of(kps):
    """Tracking::FirstInitialization: mvbPrevMatched = the keypoint positions."""
    return np.ascontiguousarray(np.stack([kps["x"], kps["y"]], 1), np.float32)


def flip(rng, d, nbits, positions=None):
    """A copy of descriptor d with exactly nbits bits flipped (among ``positions``)."""
    bits = np.unpackbits(np.asarray(d, np.uint8))
    pos = rng.choice(np.arange(256) if positions is None else positions, int(nbits), replace=False)
    bits[pos] ^= 1
    return np.packbits(bits)


def _dress(rng, kps1, kps2, m12, level0_frac=0.7, rot=10.0):
    """Octaves, angles and descriptors for a geometric match list: a matched
    pair is level 0 in both frames with probability level0_frac (else both
    above 0), its angles differ by about ``rot`` degrees, and its F2
    descriptor is the F1 descriptor with 0..12 flipped bits."""
    k1, k2 = kps1.copy(), kps2.copy()
    n1, n2 = len(k1), len(k2)
    d1 = rng.integers(0, 256, size=(n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(n2, 32), dtype=np.uint8)
    k1["octave"], k2["octave"] = rng.integers(0, 4, n1), rng.integers(0, 4, n2)
    k1["angle"], k2["angle"] = rng.uniform(0, 360, n1), rng.uniform(0, 360, n2)
    for i in np.nonzero(m12 >= 0)[0]:
        j = m12[i]
        lvl = 0 if rng.random() < level0_frac else int(rng.integers(1, 4))
        k1["octave"][i] = k2["octave"][j] = lvl
        k2["angle"][j] = (k1["angle"][i] - rot + rng.normal(0, 2.0)) % 360.0
        d2[j] = flip(rng, d1[i], rng.integers(0, 13))
    return k1, d1, k2, d2


def two_view(seed, n_match=400, n_extra=200, **kw) -> dict:
    d = synth_two_view(seed, n_match=n_match, n_extra=n_extra, **kw)
    rng = np.random.default_rng(2000 + seed)
    m = d["matches12"]
    k1, d1, k2, d2 = _dress(rng, d["kps1"], d["kps2"], m)
    pairs = np.nonzero(m >= 0)[0]
    both0 = (k1["octave"][pairs] == 0) & (k2["octave"][m[pairs]] == 0)
    assert both0.mean() >= 0.6
    return dict(info=INFO, K=d["K"], kps1=k1, desc1=d1, kps2=k2, desc2=d2, prev=prev_of(k1), gt=m)


def _rot(axis, deg):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    a = np.deg2rad(deg)
    S = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * S + (1 - np.cos(a)) * S @ S


def sequence(seed, motions, n_pts=400, n_extra=150, noise_px=0.5) -> list:
    """One set of points seen from the initial camera and from each (rot_deg,
    baseline) of ``motions`` -> [(kps, desc), ...], frame 0 first. Point i is
    keypoint perm_f[i] of frame f; about 70% of the points are level 0 in every
    frame. baseline 0 is a pure rotation."""
    rng = np.random.default_rng(3000 + seed)
    axis, tdir = rng.normal(size=3), rng.normal(size=3) * [1.0, 0.3, 0.2]
    tdir /= np.linalg.norm(tdir)
    uv = rng.uniform([80, 80], [W - 80, H - 80], size=(n_pts, 2))
    z = rng.uniform(2.0, 8.0, n_pts)
    X = np.c_[(uv - [W / 2, H / 2]) / F * z[:, None], z]
    lvl = np.where(rng.random(n_pts) < 0.7, 0, rng.integers(1, 4, n_pts))
    ang = rng.uniform(0, 360, n_pts)
    base = rng.integers(0, 256, size=(n_pts, 32), dtype=np.uint8)
    out = []
    for f, (rot_deg, baseline) in enumerate([(0.0, 0.0)] + list(motions)):
        P = X @ _rot(axis, rot_deg).T + baseline * tdir
        u = P[:, :2] / P[:, 2:3] * F + [W / 2, H / 2] + rng.normal(0, noise_px if f else 0.0, (n_pts, 2))
        e = rng.uniform([5, 5], [W - 5, H - 5], size=(n_extra, 2))
        k = kparr(np.r_[u, e], np.r_[lvl, rng.integers(0, 4, n_extra)],
                  np.r_[(ang - 3.0 * f) % 360.0, rng.uniform(0, 360, n_extra)])
        d = np.r_[np.stack([flip(rng, b, rng.integers(0, 9)) for b in base]) if f else base,
                  rng.integers(0, 256, size=(n_extra, 32), dtype=np.uint8)]
        perm = rng.permutation(len(k))
        out.append((np.ascontiguousarray(k[perm]), np.ascontiguousarray(d[perm])))
    return out


CLUSTER_BITS = np.arange(16)  # the bit positions in which the members of a cluster differ


def contended(seed, n_clusters=40) -> dict:
    rng = np.random.default_rng(4000 + seed)
    k1, d1, k2, d2, prev = [], [], [], [], []

    def add(dst_k, dst_d, xy, octave, angle, desc):
        dst_k.append((xy[0], xy[1], octave, angle))
        dst_d.append(desc)

    # descriptor clusters: members differ from the centre in 0..6 of 16 bits, so distances inside a
    # cluster are small integers full of ties, and ~128 to everything else. All F1 members of a
    # cluster are rotated by the same angle against its F2 members: a cluster votes for one bin.
    # bin 0 gets most clusters; bins 2, 4, 6 and 8 get a few each, close in size, so the three maxima
    # are decided by a handful of entries, stale ones among them.
    rots = [0.0] * (n_clusters - 22) + [60.0] * 7 + [120.0] * 6 + [180.0] * 6 + [240.0] * 3
    for c, rot in enumerate(rots):
        centre = rng.integers(0, 256, 32, dtype=np.uint8)
        cx, cy = rng.uniform(60, W - 60), rng.uniform(60, H - 60)
        theta = rng.uniform(0, 360)
        n2c, n1c = int(rng.integers(3, 7)), int(rng.integers(3, 8))
        cell = (np.floor(cx / 11.75) * 11.75 + 2.0, np.floor(cy / 10.0) * 10.0 + 2.0)
        twins = c % 4 == 0  # two equal members: an exact tie for every query of the cluster
        for j in range(n2c):
            # two members share a grid cell (the index order decides a tie there), the others spread over cells
            xy = (cell[0] + rng.uniform(0, 3), cell[1] + rng.uniform(0, 3)) if j < 2 else \
                (cx + rng.uniform(-40, 40), cy + rng.uniform(-40, 40))
            nb = 1 if twins and j < 2 else int(rng.integers(0, 7))
            dj = flip(rng, centre, nb, CLUSTER_BITS)
            add(k2, d2, xy, 0, theta, d2[-1] if twins and j == 1 else dj)
        for i in range(n1c):
            xy = (cx + rng.uniform(-30, 30), cy + rng.uniform(-30, 30))
            add(k1, d1, xy, 0, (theta + rot) % 360.0, flip(rng, centre, int(rng.integers(0, 7)), CLUSTER_BITS))
            prev.append(xy)
    # one query, one designed pair of candidates: (best, second) around the thresholds
    for best, second, in [(50, None), (51, None), (9, 10), (8, 10), (17, 19), (18, 20), (5, 5), (0, 1), (50, 56), (45, 50)]:
        q = rng.integers(0, 256, 32, dtype=np.uint8)
        x, y = rng.uniform(60, W - 60), rng.uniform(60, H - 60)
        a = rng.uniform(0, 360)
        add(k1, d1, (x, y), 0, a, q)
        prev.append((x, y))
        add(k2, d2, (x + rng.uniform(-20, 20), y + rng.uniform(-20, 20)), 0, a, flip(rng, q, best))
        if second is not None:
            add(k2, d2, (x + rng.uniform(-20, 20), y + rng.uniform(-20, 20)), 0, a, flip(rng, q, second))
    # vbPrevMatched near and beyond the grid's borders, each with a matching candidate at the border
    for px, py, bx, by in [(-50.0, 200.0, 3.0, 200.0), (-150.0, 200.0, 2.0, 210.0), (W + 40.0, 100.0, W - 2.0, 100.0),
                           (W + 150.0, 100.0, W - 3.0, 110.0), (300.0, -60.0, 300.0, 4.0), (300.0, -101.0, 310.0, 0.5),
                           (300.0, H + 99.0, 300.0, H - 0.5), (300.0, H + 200.0, 320.0, H - 1.0),
                           (-99.0, -99.0, 0.5, 0.5), (W + 99.5, H + 99.5, W - 0.2, H - 0.2),
                           (30.0, 30.0, -10.0, 30.0)]:  # the last candidate lies outside the grid (PosInGrid false)
        q = rng.integers(0, 256, 32, dtype=np.uint8)
        a = rng.uniform(0, 360)
        add(k1, d1, (rng.uniform(100, 600), rng.uniform(100, 400)), 0, a, q)
        prev.append((px, py))
        add(k2, d2, (bx, by), 0, a, flip(rng, q, 3))
    # keypoints above level 0 with the descriptors of level-0 ones: they must neither search nor be found
    for _ in range(30):
        i, j = int(rng.integers(0, len(k1))), int(rng.integers(0, len(k2)))
        add(k1, d1, k1[i][:2], int(rng.integers(1, 4)), k1[i][3], d1[i])
        prev.append(k1[i][:2])
        add(k2, d2, k2[j][:2], int(rng.integers(1, 4)), k2[j][3], d2[j])
    p1, p2 = rng.permutation(len(k1)), rng.permutation(len(k2))

    def pack(ks, ds, perm):
        a = np.asarray(ks, np.float64)
        return (np.ascontiguousarray(kparr(a[:, :2], a[:, 2].astype(np.int32), a[:, 3])[perm]),
                np.ascontiguousarray(np.stack(ds)[perm]))

    kk1, dd1 = pack(k1, d1, p1)
    kk2, dd2 = pack(k2, d2, p2)
    return dict(info=INFO, kps1=kk1, desc1=dd1, kps2=kk2, desc2=dd2,
                prev=np.ascontiguousarray(np.asarray(prev, np.float32)[p1]))


CROWD = 700


def crowded(seed) -> dict:
    """CROWD level-0 keypoints of F2 inside the 200 x 200 window around the
    image centre; F1's queries sit at the centre (the whole crowd in their
    window), at its rim (a part of it) and far away (none)."""
    rng = np.random.default_rng(5000 + seed)
    c = np.array([W / 2, H / 2])
    xy2 = np.r_[c + rng.uniform(-99, 99, (CROWD, 2)), rng.uniform([5, 5], [W - 5, H - 5], (100, 2))]
    d2 = rng.integers(0, 256, size=(len(xy2), 32), dtype=np.uint8)
    a2 = rng.uniform(0, 360, len(xy2))
    k2 = kparr(xy2, np.r_[np.zeros(CROWD, np.int32), rng.integers(0, 4, 100)], a2)
    xy1 = np.r_[c + rng.uniform(-0.5, 0.5, (60, 2)), c + rng.uniform(-150, 150, (60, 2)),
                rng.uniform([5, 5], [W - 5, H - 5], (40, 2))]
    n1 = len(xy1)
    src = rng.choice(CROWD, n1, replace=False)
    d1 = np.stack([flip(rng, d2[j], rng.integers(0, 20)) for j in src])
    k1 = kparr(xy1, np.where(rng.random(n1) < 0.9, 0, 1), (a2[src] + 5.0) % 360.0)
    return dict(info=INFO, kps1=k1, desc1=d1, kps2=k2, desc2=d2, prev=prev_of(k1))


def big(seed, n=4096) -> dict:
    """4096 keypoints a frame, a tenth of them level 0: windows of a few tens
    of candidates, some above any list's length."""
    rng = np.random.default_rng(6000 + seed)
    xy1 = rng.uniform([5, 5], [W - 5, H - 5], (n, 2))
    perm = rng.permutation(n)
    xy2 = xy1[perm] + rng.normal(0, 8.0, (n, 2))
    lvl1 = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 8, n))
    a1 = rng.uniform(0, 360, n)
    d1 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    d2 = np.stack([flip(rng, d1[i], rng.integers(0, 30)) for i in perm])
    k1, k2 = kparr(xy1, lvl1, a1), kparr(xy2, lvl1[perm], (a1[perm] - 20.0) % 360.0)
    return dict(info=INFO, kps1=k1, desc1=d1, kps2=k2, desc2=d2, prev=prev_of(k1))


def edge(name) -> dict:
    rng = np.random.default_rng(7)
    s = two_view(1, n_match=60, n_extra=40)
    e = lambda: (np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8))  # noqa: E731
    if name == "n1=0":
        s["kps1"], s["desc1"] = e()
        s["prev"] = np.zeros((0, 2), np.float32)
    elif name == "n2=0":
        s["kps2"], s["desc2"] = e()
    elif name == "no level 0 in F1":
        s["kps1"]["octave"] = np.maximum(s["kps1"]["octave"], 1)
    elif name == "no level 0 in F2":
        s["kps2"]["octave"] = np.maximum(s["kps2"]["octave"], 1)
    elif name == "one query, one candidate":
        q = rng.integers(0, 256, (1, 32), dtype=np.uint8)
        s = dict(info=INFO, kps1=kparr([(100.0, 100.0)], 0, 10.0), desc1=q, kps2=kparr([(130.0, 90.0)], 0, 5.0),
                 desc2=flip(rng, q[0], 4).reshape(1, 32), prev=np.array([[100.0, 100.0]], np.float32))
    else:
        raise KeyError(name)
    return s


EDGES = ("n1=0", "n2=0", "no level 0 in F1", "no level 0 in F2", "one query, one candidate")
