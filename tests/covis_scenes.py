"""Scenes for UpdateConnections / ProcessNewKeyFrame (tests/test_covis_cpu.py,
tests/test_covis_gpu.py).

The counting reads no geometry, so a scene is index arrays as in
kfcull_scenes.py: keypoints with zero coordinates, identity poses, slot tables,
observation maps. ``scene()`` hand-places the cases below; ``names`` maps each
role to its keyframe index (mnId = index, so ``K0`` is the first keyframe) and
``expect`` holds, per query role, the weight map and the ordered lists worked
out by hand. A point "shared by Q and N" is observed by exactly those two.

Planted cases (each asserted by name in test_covis_cpu.py):

- Threshold, ``TH``: ``T14`` / ``T15`` / ``T16`` share exactly 14, 15 and 16
  points with it: the list is T16, T15; T14 is in the weight map only. ``T14``
  itself lists ``TH`` through the fallback.
- Fallback, ``FB``: ``F1`` and ``F2`` tie at 9, ``F3`` has 5, nothing reaches
  15: the lower index ``F1`` wins. ``ONE``: its only neighbour ``ONE_N`` shares
  one point.
- Order, ``ORD``: in index order its neighbours weigh 25, 20, 17, 20, 30, 20:
  the three at 20 come highest index first, between 25 and 17.
- Empty: ``EMPTY0`` has no slots, ``LONE`` points only it observes, ``BADONLY``
  only bad points (whose rows still list ``S`` and ``K0``: the bad test is what
  empties the counter).
- A26, ``AQ``: ``twice`` sits in two slots (2 for ``A1``, which also shares an
  ordinary point: 3); ``unlisted`` is a point of ``A2`` and ``A3`` in a slot of
  ``AQ`` whose row does not list ``AQ``; ``phantom`` is shared with ``A4`` and
  lists ``AQ`` at a slot whose table entry is NULL: nothing for ``AQ``, 1 for
  ``A4``. :func:`raw_tables` adds, in padding slots of ``AQ``, a point whose row
  holds -1 entries and an entry >= nkp around keypoints of ``A2`` and ``A3``,
  and a point id >= nmp; and in ``RAWQ`` points with rows of 0, 1, 63, 64, 65
  and 300 entries.
- Own observation: every query lists itself in its own points' rows.
- First connection: ``K0`` (mnId 0) shares 3 points with ``S``.
- ``scene(edges=True)`` adds keyframes of 0, 1, 255, 256, 257 and 4096 slots
  holding random points of the map, which do not list them.

:func:`thin_tables` builds raw tables for the kernel's tiles: ``nkf`` keyframes
of which the first are queries with 22 points each and the rest single-slot
fillers, query ``i`` with a chosen number of keyframes at 15 or more.
"""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

ROLES = ("K0", "S", "TH", "T14", "T15", "T16", "FB", "F1", "F2", "F3", "ONE", "ONE_N", "ORD", "O25", "Oa", "O17", "Ob",
         "O30", "Oc", "EMPTY0", "LONE", "BADONLY", "AQ", "A1", "A2", "A3", "A4", "RAWQ")
EDGE_SIZES = (0, 1, 255, 256, 257, 4096)
ROW_SIZES = (0, 1, 63, 64, 65, 300)
LIST_SIZES = (0, 1, 63, 64, 65, 300)
PAD = 8  # NULL slots at the end of every keyframe but EMPTY0
_CACHE = {}


class _Builder:
    def __init__(self, nkf):
        self.slots = [[] for _ in range(nkf)]
        self.obs, self.bad = [], []

    def kp(self, kf, p=-1):
        self.slots[kf].append(p)
        return len(self.slots[kf]) - 1

    def point(self, observers, bad=False):
        p = len(self.obs)
        self.obs.append({kf: self.kp(kf, p) for kf in observers})
        self.bad.append(bad)
        return p


def scene(edges=False, seed=4):
    key = (edges, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    n = {r: i for i, r in enumerate(ROLES)}
    nkf = len(ROLES) + (len(EDGE_SIZES) if edges else 0)
    b = _Builder(nkf)
    share = lambda q, o, cnt: [b.point([n[q], n[o]]) for _ in range(cnt)]  # noqa: E731
    pts, expect = {}, {}
    share("K0", "S", 3)
    expect["K0"] = ({n["S"]: 3}, [n["S"]], [3])
    for r, c in (("T14", 14), ("T15", 15), ("T16", 16)):
        share("TH", r, c)
    expect["TH"] = ({n["T14"]: 14, n["T15"]: 15, n["T16"]: 16}, [n["T16"], n["T15"]], [16, 15])
    expect["T14"] = ({n["TH"]: 14}, [n["TH"]], [14])
    expect["T15"] = ({n["TH"]: 15}, [n["TH"]], [15])
    for r, c in (("F2", 9), ("F1", 9), ("F3", 5)):
        share("FB", r, c)
    expect["FB"] = ({n["F1"]: 9, n["F2"]: 9, n["F3"]: 5}, [n["F1"]], [9])
    share("ONE", "ONE_N", 1)
    expect["ONE"] = ({n["ONE_N"]: 1}, [n["ONE_N"]], [1])
    order_w = dict(O25=25, Oa=20, O17=17, Ob=20, O30=30, Oc=20)
    for r, c in order_w.items():
        share("ORD", r, c)
    expect["ORD"] = ({n[r]: c for r, c in order_w.items()},
                     [n[r] for r in ("O30", "O25", "Oc", "Ob", "Oa", "O17")], [30, 25, 20, 20, 20, 17])
    expect["EMPTY0"] = ({}, [], [])
    pts["lone"] = [b.point([n["LONE"]]) for _ in range(20)]
    expect["LONE"] = ({}, [], [])
    pts["badonly"] = [b.point([n["BADONLY"], n["S"], n["K0"]], bad=True) for _ in range(20)]
    expect["BADONLY"] = ({}, [], [])
    expect["S"] = ({n["K0"]: 3}, [n["K0"]], [3])  # the bad points it holds count nothing
    AQ = n["AQ"]
    share("AQ", "A1", 1)
    pts["twice"] = b.point([AQ, n["A1"]])
    twice_second = b.kp(AQ, pts["twice"])
    pts["unlisted"] = b.point([n["A2"], n["A3"]])
    unlisted_slot = b.kp(AQ, pts["unlisted"])
    pts["phantom"] = b.point([AQ, n["A4"]])
    phantom_slot = b.obs[pts["phantom"]][AQ]
    b.slots[AQ][phantom_slot] = -1  # the observation stays, the table entry is NULL
    expect["AQ"] = ({n["A1"]: 3, n["A2"]: 1, n["A3"]: 1}, [n["A1"]], [3])
    expect["A4"] = ({AQ: 1}, [AQ], [1])
    expect["A2"] = ({n["A3"]: 1}, [n["A3"]], [1])  # AQ holds the point but is not in its row
    expect["RAWQ"] = ({}, [], [])
    for k in range(len(ROLES)):
        if k != n["EMPTY0"]:
            for _ in range(PAD):
                b.kp(k)
    names = dict(n)
    if edges:
        nmp = len(b.obs)
        for j, size in enumerate(EDGE_SIZES):
            k = len(ROLES) + j
            names[f"E{size}"] = k
            ids = rng.integers(-1, nmp, size)
            ids[rng.random(size) < 0.25] = -1
            b.slots[k] = [int(p) for p in ids]
    kf_kps = [np.zeros(len(s), KEYPOINT_DTYPE) for s in b.slots]
    kf_desc = [rng.integers(0, 256, (len(s), 32), dtype=np.uint8) for s in b.slots]
    nmp = len(b.obs)
    sc = dict(names=names, pts=pts, expect=expect, kf_kps=kf_kps, kf_desc=kf_desc,
              kf_mp=[np.asarray(s, np.int32) for s in b.slots], mps=np.zeros(nmp, MAP_POINT_DTYPE),
              mp_desc=rng.integers(0, 256, (nmp, 32), dtype=np.uint8), mp_bad=np.asarray(b.bad, bool),
              observations=[dict(o) for o in b.obs], edges=edges,
              slots_of=dict(twice=(b.obs[pts["twice"]][AQ], twice_second), unlisted=unlisted_slot,
                            phantom=phantom_slot))
    _CACHE[key] = sc
    return sc


def loop_map(sc, **kw):
    """A fresh LoopMap of the scene, without a graph."""
    from gf_orb_slam_amd.loopmap import LoopMap

    return LoopMap(None, sc["kf_kps"], sc["kf_desc"], sc["kf_mp"], sc["mps"], sc["mp_desc"], mp_bad=sc["mp_bad"],
                   observations=sc["observations"], **kw)


def raw_tables(m, sc):
    """The flat tables of the LoopMap plus what no LoopMap holds. In padding
    slots of ``AQ``: a point whose row is (-1, a keypoint of A2, nkp + 7, -1, a
    keypoint of A3, -5), and a point id >= nmp. In padding slots of ``RAWQ``:
    points with rows of ROW_SIZES entries drawn from all keypoints but RAWQ's
    (repeats allowed, every tenth entry -1). -> (kf_off, slots, mp_bad,
    obs_off, obs_gkp, info) with ``info["aq"]`` the weight map AQ must get and
    ``info["rawq"]`` that of RAWQ, counted here from the rows."""
    from gf_orb_slam_amd.localmapping import culling_tables

    n = sc["names"]
    kf_off, _, slots, mp_bad, obs_off, obs_gkp, _ = culling_tables(m)
    slots, nkp, nmp = slots.copy(), int(kf_off[-1]), len(mp_bad)
    rng = np.random.default_rng(8)
    rows = [np.asarray([-1, kf_off[n["A2"]], nkp + 7, -1, kf_off[n["A3"]] + 1, -5], np.int32)]
    pool = np.concatenate([np.arange(kf_off[k], kf_off[k + 1]) for k in range(m.nkf) if k != n["RAWQ"]])
    for size in ROW_SIZES:
        row = rng.choice(pool, size).astype(np.int32)
        row[9::10] = -1
        rows.append(row)
    first = nmp
    obs_gkp = np.concatenate([obs_gkp] + rows).astype(np.int32)
    obs_off = np.concatenate([obs_off, obs_off[-1] + np.cumsum([len(r) for r in rows])]).astype(np.int32)
    mp_bad = np.concatenate([mp_bad, np.zeros(len(rows), np.uint8)]).astype(np.uint8)
    aq_pad = int(kf_off[n["AQ"] + 1]) - PAD
    rq_pad = int(kf_off[n["RAWQ"] + 1]) - PAD
    assert np.all(slots[aq_pad:aq_pad + 2] == -1) and np.all(slots[rq_pad:rq_pad + len(ROW_SIZES)] == -1)
    slots[aq_pad], slots[aq_pad + 1] = first, first + len(rows) + 5
    slots[rq_pad:rq_pad + len(ROW_SIZES)] = first + 1 + np.arange(len(ROW_SIZES))
    rawq = {}
    for row in rows[1:]:
        for g in row[row >= 0]:
            k = int(np.searchsorted(kf_off, g, side="right") - 1)
            rawq[k] = rawq.get(k, 0) + 1
    aq = dict(sc["expect"]["AQ"][0])
    aq[n["A2"]] += 1
    aq[n["A3"]] += 1
    return kf_off, slots, mp_bad, obs_off, obs_gkp, dict(aq=aq, rawq=rawq)


def small_without_cur(plant=True, **kw):
    """``neighbors_scenes.small()`` as tracking leaves it: a LoopMap of its
    keyframes without the new one (the last), whose observations are taken out
    of the maps (a point only it observed keeps no reference keyframe), the
    graph built by UpdateConnections in index order, and the new keyframe's
    ``(kps, desc, slots, Tcw, kf_id)`` for ``add_keyframe``. plant: a NULL
    slot after the new keyframe's first good point gets a second copy of that
    point (a duplicated slot); the scene's ``bkeep`` role already puts bad
    points in its slots. -> (map, keyframe tuple, dict naming the duplicated
    slots, a slot with a bad point and a NULL slot)."""
    import neighbors_scenes as NS
    from gf_orb_slam_amd.loopmap import LoopMap

    sc = NS.small()
    cur = sc["cur"]
    assert cur == len(sc["kf_kps"]) - 1
    obs = [{k: i for k, i in o.items() if k != cur} for o in sc["observations"]]
    ref = np.asarray([r if r != cur else (min(o) if o else -1) for r, o in zip(sc["ref_kf"], obs)], np.int32)
    m = LoopMap(sc["info"], sc["kf_kps"][:cur], sc["kf_desc"][:cur], sc["kf_mp"][:cur], sc["mps"], sc["mp_desc"],
                mp_bad=sc["mp_bad"], observations=obs, kf_Tcw=sc["kf_Tcw"][:cur], ref_kf=ref, kf_id=sc["kf_id"][:cur],
                **kw)
    for k in range(m.nkf):
        m.update_connections(k)
    m.kf_bad[:] = sc["kf_bad"][:cur]
    slots = sc["kf_mp"][cur].copy()
    planted = {}
    if plant:
        null = np.nonzero(slots < 0)[0]
        good = [int(i) for i in np.nonzero(slots >= 0)[0] if not sc["mp_bad"][slots[i]] and obs[slots[i]]]
        bad = [int(i) for i in np.nonzero(slots >= 0)[0] if sc["mp_bad"][slots[i]]]
        first = good[0]
        later = null[null > first]  # the copy comes later in slot order: the point ends with it
        assert len(later) >= 2 and bad
        slots[later[0]] = slots[first]
        planted = dict(first=first, second=int(later[0]), point=int(slots[first]), bad=bad[0], null=int(later[1]))
    return m, (sc["kf_kps"][cur], sc["kf_desc"][cur], slots, sc["kf_Tcw"][cur], int(sc["kf_id"][cur])), planted


def thin_tables(nkf, listed=LIST_SIZES, seed=2):
    """Raw tables of a thin map for the kernel's tiles: the first keyframes are
    queries (as many of ``listed`` as leave the wanted number of other
    keyframes), 22 points each plus 3 NULL slots, the others single-slot
    fillers. Query i has ``listed[i]`` other keyframes at a weight drawn from
    15..21 (so with many ties) and up to 10 more below 15: point j of the
    query lists its own keypoint and a keypoint of every keyframe whose weight
    exceeds j, in shuffled order. -> (kf_off, slots, mp_bad, obs_off, obs_gkp,
    queries, the wanted list lengths)."""
    rng = np.random.default_rng(seed + nkf)
    listed = [c for c in listed if c <= nkf - 1]
    nq = min(len(listed), nkf)
    listed = listed[:nq]
    sizes = [25] * nq + [1] * (nkf - nq)
    kf_off = np.zeros(nkf + 1, np.int32)
    kf_off[1:] = np.cumsum(sizes)
    slots = np.full(kf_off[-1], -1, np.int32)
    rows = []
    for q, cnt in enumerate(listed):
        others = np.asarray([k for k in range(nkf) if k != q], np.int64)
        pick = rng.permutation(others)[:min(len(others), cnt + 10)]
        wt = np.concatenate([rng.integers(15, 22, cnt), rng.integers(1, 15, len(pick) - cnt)])
        for j in range(22):
            slots[kf_off[q] + j] = len(rows)
            row = np.concatenate([[kf_off[q] + j], kf_off[pick[wt > j]]]).astype(np.int32)
            rows.append(rng.permutation(row))
    obs_off = np.zeros(len(rows) + 1, np.int32)
    obs_off[1:] = np.cumsum([len(r) for r in rows])
    obs_gkp = np.concatenate([np.zeros(0, np.int32)] + rows).astype(np.int32)
    return kf_off, slots, np.zeros(len(rows), np.uint8), obs_off, obs_gkp, np.arange(nq, dtype=np.int32), listed
