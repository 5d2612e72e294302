"""Scenes for KeyFrameCulling (tests/test_kfcull_cpu.py, tests/test_kfcull_gpu.py).

Culling reads no geometry, so a scene is index arrays: keypoints with random
x / y and descriptors, identity poses, octaves 0..7, slot tables, observation
maps. ``scene()`` hand-places the cases below around the current keyframe
``CUR``; ``names`` maps each role to its keyframe index. The support keyframes
S1..S4 (and keyframe 0, mnId 0) come first, so the lowest remaining observer of
a point is a support.

A *redundant* point of keyframe K is ``(K @ level 2, S1 @ 0, S2 @ 0, S3 @ 0)``:
four observations, three of them other keyframes at a level <= 2 + 1. For a
support it is not redundant (K's level 2 > 0 + 1 leaves two). A *single* is a
point K alone observes.

Planted cases (each asserted by name in test_kfcull_cpu.py):

- Row gates, keyframe ``M``: points with 3, 4 and 5 live observations
  (``gate3`` flag 1, ``gate4`` / ``gate5`` flag 2); a bad point with an empty
  row in a slot of ``D0``; the row of 70 entries is appended to the flat
  tables by :func:`raw_tables` (a LoopMap row has at most one entry per
  keyframe).
- Octave boundary, ``M``: ``oct_pass`` has three observers at level + 1
  (redundant by exactly 3), ``oct_fail`` two at level + 1 and one at level + 2
  (fails by exactly 2), ``oct_fail5`` the same with a fifth observer at
  level + 2.
- A26 disagreements, ``M``: ``twice`` sits in two slots (flags 2 and 1: the
  second slot's level 0 is below the observers' level 2); ``unlisted`` is a
  point of S1..S4 in a slot of ``M`` whose observation map does not name
  ``M`` (every observer counts); ``phantom`` lists ``M`` as observer at a
  slot whose table entry is NULL, and is redundant for ``Q`` only through that
  observation. :func:`raw_tables` adds a point id >= nmp.
- Decision boundary: ``D9`` 10 / 9 kept (0.9 * 10 == 9.0 in double), ``D10``
  10 / 10 culled, ``D11`` 11 / 10 culled, ``D0`` 0 / 0 kept.
- Order dependence: ``A`` before ``B`` (B's ten redundant points have A as
  their third other observer: 10 / 10 before, 10 / 0 after A is culled, B
  survives) and ``A`` before ``C`` (C is 12 / 10; its two non-redundant points
  are seen by C, A and S1 only, turn bad when A goes, and C is culled at 10 / 10).
- Protected: keyframe 0 (mnId 0) is listed and above 90 %; ``N`` is
  ``not_erase`` and above 90 % (deferred, culled by a later ``set_erase``);
  ``L`` has a loop edge (``set_erase`` does not clear its flag).
- Spanning tree: ``T`` is culled; its parent is S1 and it has five children:
  ``c1`` covisible with the parent (weight 20, adopted first), ``c2``
  covisible with ``c1`` only (adopted in the second round), ``c3`` and ``c4``
  tying at weight 18 with the parent (``c3``, first in index order, wins;
  ``c4`` then lists ``c3`` and the parent at 18 each and takes the first of
  its list, ``c3``), ``c5`` without a link (goes to the original parent).
- Reference keyframe: ``ref_moves`` has ``D10`` as mpRefKF and moves to S1;
  ``ref_stays`` is ``D11``'s single, left without observations.

``scene(cull=False)`` gives every keyframe above 90 % (keyframe 0 apart) enough
singles to stay below; ``scene(edges=True)`` adds keyframes of 0, 1, 255, 256, 257 and 4096
slots holding random points of the map, which do not list them.
"""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

ROLES = ("K0", "S1", "S2", "S3", "S4", "M", "Q", "D9", "D10", "D11", "D0", "A", "N", "B", "L", "C", "T", "c1", "c2",
         "c3", "c4", "c5", "CUR")
ORDER = ("K0", "M", "Q", "D9", "D10", "D11", "D0", "A", "N", "B", "L", "C", "T")  # the candidates' planted order
EDGE_SIZES = (0, 1, 255, 256, 257, 4096)
ABOVE_90 = ("D10", "D11", "A", "B", "C", "T", "N", "L")  # at their turn or before it
_CACHE = {}


class _Builder:
    def __init__(self, nkf):
        self.octave = [[] for _ in range(nkf)]
        self.slots = [[] for _ in range(nkf)]
        self.obs, self.bad = [], []

    def kp(self, kf, octave, p=-1):
        self.octave[kf].append(octave)
        self.slots[kf].append(p)
        return len(self.slots[kf]) - 1

    def point(self, observers, bad=False):
        p = len(self.obs)
        self.obs.append({kf: self.kp(kf, o, p) for kf, o in observers})
        self.bad.append(bad)
        return p


def scene(cull=True, edges=False, seed=11):
    key = (cull, edges, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    names = {r: i for i, r in enumerate(ROLES)}
    nkf = len(ROLES) + (len(EDGE_SIZES) if edges else 0)
    b = _Builder(nkf)
    n = names
    S = [n["S1"], n["S2"], n["S3"], n["S4"]]
    red = lambda k, cnt, lv=2: [b.point([(k, lv)] + [(s, 0) for s in S[:3]]) for _ in range(cnt)]  # noqa: E731
    single = lambda k, cnt: [b.point([(k, 2)]) for _ in range(cnt)]  # noqa: E731
    pts = {}
    for s in S:  # the supports never reach 90 %
        single(s, 30)
    red(n["K0"], 10)
    # M: row gates, octave boundary, A26
    M = n["M"]
    pts["gate3"] = b.point([(M, 2), (S[0], 0), (S[1], 0)])
    pts["gate4"] = b.point([(M, 2), (S[0], 0), (S[1], 0), (S[2], 0)])
    pts["gate5"] = b.point([(M, 2), (S[0], 0), (S[1], 0), (S[2], 0), (S[3], 0)])
    pts["oct_pass"] = b.point([(M, 2), (S[0], 3), (S[1], 3), (S[2], 3)])
    pts["oct_fail"] = b.point([(M, 2), (S[0], 3), (S[1], 3), (S[2], 4)])
    pts["oct_fail5"] = b.point([(M, 2), (S[0], 3), (S[1], 3), (S[2], 4), (S[3], 4)])
    pts["twice"] = b.point([(M, 2), (S[0], 2), (S[1], 2), (S[2], 2)])
    twice_second = b.kp(M, 0, pts["twice"])
    pts["unlisted"] = b.point([(s, 0) for s in S])
    unlisted_slot = b.kp(M, 2, pts["unlisted"])
    Q = n["Q"]
    pts["phantom"] = b.point([(Q, 2), (S[0], 0), (S[1], 0), (M, 0)])
    phantom_slot = b.obs[pts["phantom"]][M]
    b.slots[M][phantom_slot] = -1  # the observation stays, the table entry is NULL
    single(M, 12)
    red(Q, 4)
    single(Q, 8)
    # decision boundary
    red(n["D9"], 9), single(n["D9"], 1)
    d10 = red(n["D10"], 10)
    pts["ref_moves"] = d10[3]
    red(n["D11"], 10)
    pts["ref_stays"] = single(n["D11"], 1)[0]
    pts["empty_row"] = b.point([], bad=True)
    b.kp(n["D0"], 2, pts["empty_row"])
    # order dependence
    A, B, C = n["A"], n["B"], n["C"]
    red(A, 10)
    pts["ab"] = [b.point([(B, 2), (A, 2), (S[0], 0), (S[1], 0)]) for _ in range(10)]
    red(C, 10)
    pts["ac"] = [b.point([(C, 2), (A, 5), (S[0], 5)]) for _ in range(2)]
    # protected, spanning tree
    for r in ("N", "L", "T"):
        red(n[r], 10)
    if not cull:
        for r in ABOVE_90:
            single(n[r], 6)
    cur_pts = [b.point([(n["CUR"], 0), (S[0], 7)]) for _ in range(20)]
    # every role keyframe is padded with point-less keypoints to 40..300
    for k in range(len(ROLES)):
        want = max(len(b.slots[k]) + int(rng.integers(3, 20)), 40)
        assert want <= 300, (ROLES[k], want)
        while len(b.slots[k]) < want:
            b.kp(k, int(rng.integers(0, 8)))
    if edges:
        nmp = len(b.obs)
        for j, size in enumerate(EDGE_SIZES):
            k = len(ROLES) + j
            names[f"E{size}"] = k
            ids = rng.integers(-1, nmp, size)
            ids[rng.random(size) < 0.25] = -1
            b.octave[k] = [int(o) for o in rng.integers(0, 8, size)]
            b.slots[k] = [int(p) for p in ids]
    kf_kps, kf_desc = [], []
    for k in range(nkf):
        kp = np.zeros(len(b.slots[k]), KEYPOINT_DTYPE)
        kp["x"], kp["y"] = rng.random(len(kp)) * 640, rng.random(len(kp)) * 480
        kp["octave"] = np.asarray(b.octave[k], np.int32)
        kf_kps.append(kp)
        kf_desc.append(rng.integers(0, 256, (len(kp), 32), dtype=np.uint8))
    nmp = len(b.obs)
    ref_kf = np.asarray([min(o) if o else -1 for o in b.obs], np.int32)
    ref_kf[pts["ref_moves"]] = n["D10"]
    sc = dict(names=names, pts=pts, kf_kps=kf_kps, kf_desc=kf_desc,
              kf_mp=[np.asarray(s, np.int32) for s in b.slots], mps=np.zeros(nmp, MAP_POINT_DTYPE),
              mp_desc=rng.integers(0, 256, (nmp, 32), dtype=np.uint8), mp_bad=np.asarray(b.bad, bool),
              observations=[dict(o) for o in b.obs], ref_kf=ref_kf, cur=n["CUR"], cull=cull, edges=edges,
              slots_of=dict(twice=(b.obs[pts["twice"]][M], twice_second), unlisted=unlisted_slot,
                            phantom=phantom_slot), cur_pts=cur_pts)
    _CACHE[key] = sc
    return sc


def loop_map(sc, **kw):
    """A fresh LoopMap of the scene: UpdateConnections of every keyframe in
    index order, then the planted graph: the candidates' order through
    AddConnection weights, the parents, the children's links, the erase flags
    and the loop edge."""
    from gf_orb_slam_amd.loopmap import LoopMap

    n = sc["names"]
    m = LoopMap(None, sc["kf_kps"], sc["kf_desc"], sc["kf_mp"], sc["mps"], sc["mp_desc"], mp_bad=sc["mp_bad"],
                observations=sc["observations"], ref_kf=sc["ref_kf"], distinctive=kw.pop("distinctive", None), **kw)
    for k in range(m.nkf):
        m.update_connections(k)
    cur = sc["cur"]
    assert n["S1"] in m.ordered[cur]  # the natural candidate; the planted ones go in front of it
    order = list(ORDER) + ([f"E{s}" for s in EDGE_SIZES] if sc["edges"] else [])
    for j, r in enumerate(order):
        m.add_connection(cur, n[r], 1000 - j)
        m.add_connection(n[r], cur, 1000 - j)
    T, P = n["T"], n["S1"]
    m.parent[T] = P
    for c in ("c1", "c2", "c3", "c4", "c5"):
        m.parent[n[c]] = T
        m.first_connection[n[c]] = False
    link = lambda a, b_, w: (m.add_connection(n[a], n[b_], w), m.add_connection(n[b_], n[a], w))  # noqa: E731
    link("c1", "S1", 20), link("c1", "T", 50)
    link("c2", "c1", 30)
    link("c3", "S1", 18)
    link("c4", "S1", 18), link("c4", "c3", 18)
    m.set_not_erase(n["N"])
    m.add_loop_edge(n["L"], n["S2"])
    return m


def raw_tables(m, sc):
    """The flat tables of the LoopMap plus what no LoopMap holds: a new point
    with a row of 70 entries (observers picked from the supports' keypoints,
    level 0, so it is redundant wherever it sits) in the last slot of ``M``,
    and a point id >= nmp in the last slot of ``Q``. -> (kf_off, octave,
    slots, mp_bad, obs_off, obs_gkp, dict of the planted global slots)."""
    from gf_orb_slam_amd.localmapping import culling_tables

    n = sc["names"]
    kf_off, octave, slots, mp_bad, obs_off, obs_gkp, _ = culling_tables(m)
    octave, slots = octave.copy(), slots.copy()
    rng = np.random.default_rng(3)
    pool = np.concatenate([np.arange(kf_off[n[s]], kf_off[n[s] + 1]) for s in ("S1", "S2", "S3", "S4")])
    pool = pool[octave[pool] == 0]
    row = rng.choice(pool, 70).astype(np.int32)
    long_p = len(mp_bad)
    obs_gkp = np.concatenate([obs_gkp, row])
    obs_off = np.concatenate([obs_off, [obs_off[-1] + 70]]).astype(np.int32)
    mp_bad = np.concatenate([mp_bad, [0]]).astype(np.uint8)
    g_long, g_out = kf_off[n["M"] + 1] - 1, kf_off[n["Q"] + 1] - 1
    assert slots[g_long] == -1 and slots[g_out] == -1  # padding
    slots[g_long], slots[g_out] = long_p, long_p + 5
    return kf_off, octave, slots, mp_bad, obs_off, obs_gkp, dict(long=int(g_long), out=int(g_out))
