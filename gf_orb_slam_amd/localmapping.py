"""``LocalMapping::CreateNewMapPoints`` (src/LocalMapping.cc:243-409) and
``MapPointCulling`` (:213-241) on a :class:`~gf_orb_slam_amd.loopmap.LoopMap`.

The triangulation chain runs on the device (``gf_create_new_map_points``:
set-up, then SearchForTriangulation and the triangulation kernel per
neighbour, the new keyframe's slot table carried from one neighbour to the
next); the map bookkeeping of :393-406 is done here on the host.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import GFError, check, lib, ptr
from .bow import BowSide
from .orb import default_context

MAX_NEIGHBOURS = 20
STATUS = ("ok", "baseline", "nodepth")
EXITS = ("parallax", "w0", "z1", "z2", "reproj1", "reproj2", "dist0", "scale", "accepted")
NEWPOINT_DTYPE = np.dtype([("neighbour", np.int32), ("idx1", np.int32), ("idx2", np.int32), ("pos", np.float32, 3)])
NEIGH_DTYPE = np.dtype([("status", np.int32), ("F12", np.float32, 9), ("median_depth", np.float32),
                        ("nmatches", np.int32), ("naccepted", np.int32)])


class NewPointsKf(ctypes.Structure):
    """gf_newpoints_kf: a keyframe of gf_create_new_map_points."""

    _fields_ = [("Tcw", ctypes.c_float * 16), ("side", BowSide), ("mp", ctypes.c_void_p)]

    @classmethod
    def make(cls, Tcw, bufs, nfv, n):
        """bufs = (fv_nodes, fv_start, fv_feats, desc, kps, mp): host arrays
        or device tensors."""
        q = cls()
        q.Tcw[:] = [float(x) for x in np.asarray(Tcw, np.float32).reshape(16)]
        p = [ptr(b) for b in bufs]
        q.side = BowSide(p[0], p[1], p[2], int(nfv), p[3], p[4], None, int(n))
        q.mp = p[5]
        return q


def host_keyframe(Tcw, fv, desc, kps, slots):
    """A NewPointsKf over host arrays -> (struct, the arrays it points into).
    ``slots`` (int32, contiguous) is the table the call updates in place."""
    c = np.ascontiguousarray
    keep = [c(fv.nodes, np.int32), c(fv.start, np.int32), c(fv.feats, np.int32), c(desc, np.uint8), c(kps), slots]
    assert slots.dtype == np.int32 and slots.flags.c_contiguous
    return NewPointsKf.make(Tcw, keep, len(keep[0]), len(keep[3])), keep


def create_new_map_points_arrays(info, cur_kf, neigh_kfs, mp_pos, check_ori=False, cap=None, ctx=None):
    """``gf_create_new_map_points`` on host arrays: cur_kf / neigh_kfs are
    (Tcw, FeatureVector, desc, kps, slots) tuples whose slot tables are
    updated in place. -> (report [nneigh] NEIGH_DTYPE, points NEWPOINT_DTYPE in
    creation order, exits [nneigh, n1]). The new points' ids are
    len(mp_pos) + their rank."""
    ctx = ctx or default_context()
    cur, keep = host_keyframe(*cur_kf)
    nn = len(neigh_kfs)
    arr = (NewPointsKf * max(nn, 1))()
    for i, k in enumerate(neigh_kfs):
        arr[i], kk = host_keyframe(*k)
        keep.append(kk)
    n1 = cur.side.n
    cap = n1 if cap is None else int(cap)
    pos = np.ascontiguousarray(mp_pos, np.float32).reshape(-1, 3)
    report = np.zeros(max(nn, 1), NEIGH_DTYPE)
    points = np.zeros(max(cap, 1), NEWPOINT_DTYPE)
    exits = np.full((max(nn, 1), max(n1, 1)), -1, np.int32)
    total = ctypes.c_int()
    check(lib().gf_create_new_map_points(ctx.handle, ctypes.byref(info), ctypes.byref(cur), nn, arr, ptr(pos), len(pos),
                                         int(bool(check_ori)), cap, ptr(report), ptr(points), ptr(exits),
                                         ctypes.byref(total)))
    return report[:nn], points[:total.value].copy(), exits[:nn, :n1]


def create_new_map_points(map, cur: int, kf_fv, neighbours=None, check_ori: bool = False, ctx=None):
    """The whole of CreateNewMapPoints on a LoopMap for the new keyframe
    ``cur``. kf_fv[k]: the FeatureVector of keyframe k. neighbours: default
    ``map.ordered[cur][:20]`` (GetBestCovisibilityKeyFrames(20)). check_ori:
    the reference builds ``ORBmatcher(0.6, false)`` here, so False.

    After the device call, for every new point in creation order (:393-406):
    the point is appended (reference keyframe ``cur``, normal 0, min / max
    distance 0), observed by the neighbour then by ``cur``, and entered in both
    slot tables. ComputeDistinctiveDescriptors and UpdateNormalAndDepth are
    run once over all new points after that loop instead of point by point:
    both read only a point's own observations and the poses, which no later
    point of this call changes, so the result is the same.

    -> (ids of the new points, which are also mlpRecentAddedMapPoints'
    additions in order; report dict: status / F12 / median_depth / nmatches /
    naccepted per neighbour, exits [nneigh, n1], points)."""
    cur = int(cur)
    nb = [int(k) for k in (map.ordered[cur][:MAX_NEIGHBOURS] if neighbours is None else neighbours)]
    if len(nb) > MAX_NEIGHBOURS:
        raise GFError(-4, "at most 20 neighbours")
    if cur in nb or len(set(nb)) != len(nb):
        raise GFError(-1, "the neighbours are distinct keyframes other than the new one")
    kf = lambda k, s: (map.Tcw[k], kf_fv[k], map.kf_desc[k], map.kf_kps[k], s)  # noqa: E731
    slots = {k: map.slots[k].copy() for k in [cur] + nb}
    nmp = len(map.mps)
    rep, pts, exits = create_new_map_points_arrays(map.info, kf(cur, slots[cur]), [kf(k, slots[k]) for k in nb],
                                                   map.mps["pos"], check_ori, ctx=ctx)
    ids = []
    for r in pts:
        p = map.new_map_point(r["pos"], cur)
        k2 = nb[int(r["neighbour"])]
        map.add_observation(p, k2, int(r["idx2"]))
        map.add_observation(p, cur, int(r["idx1"]))
        map.add_map_point(cur, p, int(r["idx1"]))
        map.add_map_point(k2, p, int(r["idx2"]))
        ids.append(p)
    # the device wrote the same ids into its copies of the tables
    assert ids == list(range(nmp, nmp + len(pts)))
    for k in [cur] + nb:
        assert np.array_equal(map.slots[k], slots[k])
    map.compute_distinctive_descriptors(ids)
    map.update_normal_and_depth(ids)
    report = dict(status=rep["status"].copy(), F12=rep["F12"].reshape(-1, 3, 3).copy(),
                  median_depth=rep["median_depth"].copy(), nmatches=rep["nmatches"].copy(),
                  naccepted=rep["naccepted"].copy(), exits=exits.copy(), points=pts, neighbours=nb)
    return ids, report


def map_point_culling(map, recent, cur: int):
    """LocalMapping::MapPointCulling (:213-241) over the recent-points list
    for the current keyframe ``cur``: a bad point leaves the list; one found in
    fewer than a quarter of the frames it was visible in, or two keyframes old
    with at most two observations, is set bad and leaves; one three keyframes
    old leaves as it is. -> the new list."""
    cur_id = int(map.kf_id[int(cur)])
    out = []
    for p in recent:
        p = int(p)
        age = cur_id - int(map.first_kf[p])
        if map.mp_bad[p]:
            continue
        if map.get_found_ratio(p) < np.float32(0.25):
            map.set_bad_point(p)
        elif age >= 2 and len(map.obs[p]) <= 2:
            map.set_bad_point(p)
        elif age >= 3:
            continue
        else:
            out.append(p)
    return out
