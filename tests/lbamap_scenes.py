"""Scenes for LocalBundleAdjustment on a LoopMap (tests/test_lbamap_cpu.py,
tests/test_lbamap_gpu.py).

Both scenes are geometrically consistent: poses look at a cloud of points, a
keypoint that holds a point is the point's projection through the true pose
plus sub-pixel noise, octaves are spread over the levels, the covisibility
graph comes from ``update_connections``. The map then holds slightly moved
poses and points, so that the solver has work to do.

``parity()``: ten keyframes on an arc, the last one current. A point is seen
by a run of consecutive keyframes, so the keyframes near the current one are
local and the far ones fixed cameras; keyframe 0 (mnId 0) is among the fixed.
Planted: gross outliers (``OUT_PX`` pixels, level 0..2) on points with six
observations or more, one per point, and ``turn_bad``: points with exactly three
observations and one gross outlier, which turn bad in the first erasure loop
and clear their two other slots. Noise is uniform in +-``NOISE_PX`` at every
level, so an inlier's chi2 stays far below 5.991 and an outlier's far above.

``parity(stale=True)`` adds ``stale``: a point with three observations two of
which are gross outliers, up in one view and down in the next, across the
baseline (no point explains both, their pulls cancel and the third stays an
inlier). It turns bad at the first, the second
is the stale outlier of docs/ORACLE_ASSUMPTIONS.md A31.

``structural()``: ``NKF`` small keyframes in front of a wall of points, built
for the assembly. ``names`` maps roles to keyframe indices, ``pts`` to points:

- the current keyframe ``CUR`` has the highest index, so a point it shares
  with a local keyframe has its first occurrence outside the lowest-indexed one;
- local keyframes ``E0`` .. ``E4096`` of 0 / 1 / 255 / 256 / 257 / 4096 slots
  holding points of the map that do not list them (``E0`` sees nothing);
- ``BADCOV``: a bad keyframe in the ordered list of ``CUR``; ``BADOBS``: a bad
  keyframe that observes local points and is in no list;
- ``twice``: a point in two slots of ``L1``; ``dead``: a local point whose only
  observer is ``BADOBS``; ``badpt``: a bad point in a slot of ``L1``;
  ``past``: an id past the map in a slot of ``L2`` (written by
  ``structural_map`` after the covisibility graph is built); ``long``: a point with a
  row of 70 observers;
- keyframe 0 (mnId 0) observes local points: a fixed camera, until
  ``structural_map(..., first_local=True)`` puts it into the ordered list, which then
  has 32 entries; 31 neighbours otherwise;
- ``EMPTY``: a keyframe without points whose ordered list is ``L1``, ``L2``.
"""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

CAMERA = (640, 480, 500.0, 500.0, 320.0, 240.0)
NOISE_PX, OUT_PX = 0.4, 45.0
EDGE_SIZES = (0, 1, 255, 256, 257, 4096)
NKF = 84
_CACHE = {}


def info():
    return FrameInfo.make(*CAMERA)


def look_at(eye, target):
    """Tcw (float64) of a camera at ``eye`` looking at ``target``, y down."""
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ eye
    return T


def project(T, X):
    c = T[:3, :3] @ X + T[:3, 3]
    return np.array([CAMERA[2] * c[0] / c[2] + CAMERA[4], CAMERA[3] * c[1] / c[2] + CAMERA[5]]), c[2]


class _Builder:
    def __init__(self, poses, rng):
        self.T, self.rng = poses, rng
        n = len(poses)
        self.octave = [[] for _ in range(n)]
        self.slots = [[] for _ in range(n)]
        self.xy = [[] for _ in range(n)]
        self.obs, self.bad, self.pos = [], [], []

    def kp(self, kf, p=-1, octave=None, shift=None):
        """A keypoint of ``kf``: the projection of point ``p`` plus noise (plus
        ``shift``), a random position without one."""
        rng = self.rng
        if 0 <= p < len(self.pos):
            xy, depth = project(self.T[kf], self.pos[p])
            assert depth > 0.5
            xy = xy + rng.uniform(-NOISE_PX, NOISE_PX, 2) + (0 if shift is None else shift)
        else:
            xy = rng.random(2) * (CAMERA[0], CAMERA[1])
        self.octave[kf].append(int(rng.integers(0, 8)) if octave is None else octave)
        self.slots[kf].append(p)
        self.xy[kf].append(xy)
        return len(self.slots[kf]) - 1

    def point(self, X, observers, bad=False, outliers=()):
        """A point at ``X`` observed by ``observers``; those in ``outliers``
        get a gross outlier at level 0..2 (a dict gives its direction)."""
        p = len(self.obs)
        self.pos.append(np.asarray(X, float))
        self.obs.append({})
        self.bad.append(bad)
        for kf in observers:
            if kf in outliers:
                a = outliers[kf] if isinstance(outliers, dict) else self.rng.uniform(0, 2 * np.pi)
                self.obs[p][kf] = self.kp(kf, p, int(self.rng.integers(0, 3)), OUT_PX * np.array([np.cos(a), np.sin(a)]))
            else:
                self.obs[p][kf] = self.kp(kf, p)
        return p

    def arrays(self, move_pose, move_point, fixed_first=True):
        """-> the LoopMap constructor's arguments; the map's poses and points
        are the true ones moved by uniform noise of the given sizes."""
        rng = self.rng
        kf_kps, kf_desc = [], []
        for k in range(len(self.T)):
            kp = np.zeros(len(self.slots[k]), KEYPOINT_DTYPE)
            if len(kp):
                xy = np.asarray(self.xy[k], np.float32).reshape(-1, 2)
                kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
                kp["octave"] = np.asarray(self.octave[k], np.int32)
            kf_kps.append(kp)
            kf_desc.append(rng.integers(0, 256, (len(kp), 32), dtype=np.uint8))
        Tcw = np.asarray(self.T).copy()
        Tcw[:, :3, 3] += rng.uniform(-move_pose, move_pose, (len(Tcw), 3))
        if fixed_first:
            Tcw[0] = self.T[0]
        mps = np.zeros(len(self.obs), MAP_POINT_DTYPE)
        mps["pos"] = np.asarray(self.pos).reshape(-1, 3) + rng.uniform(-move_point, move_point, (len(mps), 3))
        return dict(kf_kps=kf_kps, kf_desc=kf_desc, kf_mp=[np.asarray(s, np.int32) for s in self.slots], mps=mps,
                    mp_desc=rng.integers(0, 256, (len(mps), 32), dtype=np.uint8), mp_bad=np.asarray(self.bad, bool),
                    observations=[dict(o) for o in self.obs], kf_Tcw=Tcw.astype(np.float32))


def _loop_map(sc, **kw):
    from gf_orb_slam_amd.loopmap import LoopMap

    a = sc["arrays"]
    m = LoopMap(info(), a["kf_kps"], a["kf_desc"], a["kf_mp"], a["mps"], a["mp_desc"], mp_bad=a["mp_bad"],
                observations=a["observations"], kf_Tcw=a["kf_Tcw"], kf_bad=sc.get("kf_bad"), **kw)
    m.update_normal_and_depth(range(len(m.mps)))
    for k in range(m.nkf):
        if not m.kf_bad[k]:
            m.update_connections(k)
    return m


def parity(stale=False, seed=5, per_start=28):
    key = ("parity", stale, seed, per_start)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    nkf = 10
    ang = np.linspace(-0.5, 0.5, nkf)
    poses = [look_at(np.array([6 * np.sin(a), 0.2 * np.cos(3 * a), -6 * np.cos(a)]), np.zeros(3)) for a in ang]
    b = _Builder(poses, rng)
    pts = dict(outlier=[], turn_bad=[], stale=[])
    cloud = lambda: rng.uniform(-1.5, 1.5, 3)  # noqa: E731
    for start in range(nkf):
        for _ in range(per_start):
            n = int(rng.integers(3, 8))
            obs = list(range(start, min(start + n, nkf)))
            if len(obs) >= 3:
                b.point(cloud(), obs)
    for _ in range(10):  # one gross outlier in a long track
        obs = list(range(3, 10))
        pts["outlier"].append(b.point(cloud(), obs, outliers=[int(rng.choice(obs))]))
    for _ in range(3):  # three observations, one gross outlier: turns bad
        pts["turn_bad"].append(b.point(cloud(), [7, 8, 9], outliers=[8]))
    if stale:
        # up in one view and down in the next, across the baseline: no point explains both, the pulls cancel and the third observation stays an inlier
        pts["stale"].append(b.point(cloud(), [7, 8, 9], outliers={7: np.pi / 2, 8: -np.pi / 2}))
    for k in range(nkf):  # keypoints without a point
        for _ in range(int(rng.integers(10, 30))):
            b.kp(k)
    sc = dict(arrays=b.arrays(0.02, 0.03), pts=pts, cur=nkf - 1)
    _CACHE[key] = sc
    return sc


def parity_map(sc, **kw):
    """A fresh LoopMap of a parity scene."""
    return _loop_map(sc, **kw)


def structural(seed=3):
    key = ("structural", seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    roles = ["K0", "L1", "L2", "BADCOV", "BADOBS", "EMPTY"] + [f"E{s}" for s in EDGE_SIZES]
    names = {r: i for i, r in enumerate(roles)}
    names["CUR"] = NKF - 1
    n = names
    # cameras on a small grid in front of a wall of points at z in [5, 8]
    poses = []
    for k in range(NKF):
        T = np.eye(4)
        T[:3, 3] = -np.array([0.08 * (k % 10) - 0.4, 0.08 * (k // 10) - 0.3, 0.0])
        poses.append(T)
    b = _Builder(poses, rng)
    wall = lambda: np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(5.0, 8.0)])  # noqa: E731
    plain = [k for k in range(len(roles), NKF - 1)]  # keyframes without a role
    neigh = plain[:20]                                # local through their shared points or planted weights
    far = plain[20:]                                  # observers that stay fixed cameras
    pts = {}
    for k in neigh + [n["L1"], n["L2"]]:  # shared with CUR: 16 each, above the covisibility threshold
        for _ in range(16):
            b.point(wall(), [k, n["CUR"]] + [int(rng.choice(far))])
    for _ in range(120):  # the pool: seen by local and far keyframes, and by keyframe 0
        obs = sorted(set(int(x) for x in rng.choice(neigh + far, int(rng.integers(2, 6)))))
        if rng.random() < 0.3:
            obs = [n["K0"]] + obs
        b.point(wall(), obs)
    pts["long"] = b.point(wall(), plain[:70])
    pts["twice"] = b.point(wall(), [n["L1"], neigh[0], far[0]])
    twice_second = b.kp(n["L1"], pts["twice"])
    pts["dead"] = b.point(wall(), [n["BADOBS"]])
    dead_slot = b.kp(n["L2"], pts["dead"])
    pts["badobs"] = b.point(wall(), [n["L1"], n["BADOBS"], far[1]])
    pts["badpt"] = b.point(wall(), [], bad=True)
    b.kp(n["L1"], pts["badpt"])
    pts["badcov"] = [b.point(wall(), [n["BADCOV"], n["CUR"], far[2]]) for _ in range(16)]
    nmp = len(b.obs)
    past_slot = b.kp(n["L2"])  # structural_map writes the id past the map: UpdateConnections would follow it
    for size in EDGE_SIZES:  # random points of the map, which do not list the keyframe
        k = n[f"E{size}"]
        for p in rng.integers(-1, nmp, size):
            b.kp(k, -1 if rng.random() < 0.25 else int(p))
    for _ in range(30):
        b.kp(n["EMPTY"])
    for k in range(NKF):
        if k not in [n[f"E{s}"] for s in EDGE_SIZES]:
            for _ in range(int(rng.integers(3, 12))):
                b.kp(k)
    kf_bad = np.zeros(NKF, bool)
    kf_bad[[n["BADCOV"], n["BADOBS"]]] = True
    sc = dict(arrays=b.arrays(0.01, 0.03), names=names, pts=pts, cur=n["CUR"], kf_bad=kf_bad, neigh=neigh, far=far,
              slots_of=dict(twice=twice_second, dead=dead_slot, past=past_slot))
    _CACHE[key] = sc
    return sc


def structural_map(sc, first_local=False, **kw):
    """A fresh LoopMap of the structural scene with the planted ordered list of
    ``CUR``: the edge keyframes, ``L1``, ``L2``, the bad covisible, then the
    twenty plain neighbours and three far ones: 31 that are not bad.
    first_local: keyframe 0 joins them as the 32nd."""
    m = _loop_map(sc, **kw)
    n, cur = sc["names"], sc["cur"]
    order = [n[f"E{s}"] for s in EDGE_SIZES] + [n["L1"], n["L2"], n["BADCOV"]] + sc["neigh"] + sc["far"][3:6]
    if first_local:
        order.insert(4, n["K0"])
    m.weights[cur], m.ordered[cur], m.ordered_w[cur] = {}, [], []  # the planted list alone
    m.slots[n["L2"]][sc["slots_of"]["past"]] = len(m.mps) + 5
    for j, k in enumerate(order):
        m.add_connection(cur, k, 1000 - j)
    m.add_connection(n["EMPTY"], n["L1"], 100)
    m.add_connection(n["EMPTY"], n["L2"], 90)
    assert m.ordered[cur][:len(order)] == order
    return m
