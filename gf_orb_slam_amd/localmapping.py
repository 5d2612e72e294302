"""``LocalMapping::CreateNewMapPoints`` (src/LocalMapping.cc:243-409),
``SearchInNeighbors`` (:411-488), ``MapPointCulling`` (:213-241) and
``KeyFrameCulling`` (:562-616) on a
:class:`~gf_orb_slam_amd.loopmap.LoopMap`.

The triangulation chain runs on the device (``gf_create_new_map_points``:
set-up, then SearchForTriangulation and the triangulation kernel per
neighbour, the new keyframe's slot table carried from one neighbour to the
next); the map bookkeeping of :393-406 is done here on the host.

SearchInNeighbors searches on the device (``gf_fuse_search_dev``: every target
keyframe against the new keyframe's points in one launch, then the new
keyframe against the union of the targets' points) and takes the add / replace
decisions of ORBmatcher.cc:1690-1703 here on the live map.

KeyFrameCulling counts on the device (``gf_keyframe_culling_counts_dev``: every
candidate in one launch over flat tables of the map) and runs the decision and
``KeyFrame::SetBadFlag`` (``LoopMap.set_bad_keyframe``) here on the host.

LocalBundleAdjustment (src/Optimizer.cc:1515-1764) assembles its graph on the
device (``gf_lba_graph_dev``: the gather, the vertices and the edges from flat
tables of the map), solves it with ``gf_local_ba_stop`` and applies the outlier
erasure and the write-back of :1681-1763 here on the host.

ProcessNewKeyFrame (src/LocalMapping.cc:163-211) computes the keyframe's BoW
vectors, associates its points on the host and runs KeyFrame::UpdateConnections
(src/KeyFrame.cc:332-421) with the counting and ordering on the device
(``gf_update_connections_dev``: any number of keyframes in one launch) and the
graph updates on the host (``LoopMap.apply_connections``). :class:`LocalMapper`
strings the stages together as the body of ``LocalMapping::Run`` does.

The three stages that count or assemble over the flat tables
(:func:`culling_tables`, :func:`lba_tables`) rebuild and upload them per call,
unless the map keeps them resident (``LoopMap.attach_tables``,
``maptables.ResidentTables``): then they flush the map's journal and take the
device tables from there.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import GFError, check, lib, ptr
from .bow import BowSide, FeatureVector
from .orb import default_context

MAX_NEIGHBOURS = 20
SECOND_NEIGHBOURS = 5
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


MAX_KEYPOINTS = 4096


def culling_tables(map):
    """The flat tables ``gf_keyframe_culling_counts`` reads, of a LoopMap as
    it stands -> (kf_off, octave, slots, mp_bad, obs_off, obs_gkp, where):
    the observation rows point-major in observation-map order, an entry the
    global keypoint index ``kf_off[kf] + idx``; ``where[(p, kf)]`` = the
    entry's position."""
    n = [len(k) for k in map.kf_kps]
    if n and max(n) > MAX_KEYPOINTS:
        raise GFError(-3, "at most 4096 keypoints per keyframe")
    kf_off = np.zeros(map.nkf + 1, np.int32)
    kf_off[1:] = np.cumsum(n)
    octave = np.concatenate([np.zeros(0, np.uint8)] + [k["octave"].astype(np.uint8) for k in map.kf_kps])
    slots = np.concatenate([np.zeros(0, np.int32)] + list(map.slots)).astype(np.int32)
    rows = map.observation_rows()
    obs_off = np.zeros(len(map.mps) + 1, np.int32)
    obs_off[1:] = np.cumsum(np.bincount(rows[:, 0], minlength=len(map.mps)))
    obs_gkp = (kf_off[rows[:, 1]] + rows[:, 2]).astype(np.int32)
    where = {(int(p), int(k)): j for j, (p, k) in enumerate(rows[:, :2])}
    return kf_off, octave, slots, map.mp_bad.astype(np.uint8), obs_off, obs_gkp, where


def keyframe_culling_counts(kf_off, octave, slots, mp_bad, obs_off, obs_gkp, cand, flags=None, ctx=None):
    """``gf_keyframe_culling_counts`` on host arrays (the counting of
    LocalMapping.cc:576-611 for every candidate in one launch) -> counts
    [ncand, 2] = (nmps, nredundant). flags (uint8, one per slot of the whole
    table, optional) is written in place inside the candidates' ranges."""
    ctx = ctx or default_context()
    c = np.ascontiguousarray
    kf_off, slots, obs_off, obs_gkp, cand = (c(a, np.int32).reshape(-1) for a in (kf_off, slots, obs_off, obs_gkp, cand))
    octave, mp_bad = c(octave, np.uint8).reshape(-1), c(mp_bad, np.uint8).reshape(-1)
    if len(octave) != len(slots) or len(obs_off) != len(mp_bad) + 1:
        raise GFError(-1, "table lengths disagree")
    if flags is not None and (flags.dtype != np.uint8 or not flags.flags.c_contiguous or len(flags) != len(slots)):
        raise GFError(-1, "flags: one contiguous uint8 per slot")
    counts = np.zeros((max(len(cand), 1), 2), np.int32)
    check(lib().gf_keyframe_culling_counts(ctx.handle, len(kf_off) - 1, ptr(kf_off), ptr(octave), ptr(slots),
                                           len(mp_bad), ptr(mp_bad), ptr(obs_off), ptr(obs_gkp), len(cand), ptr(cand),
                                           ptr(counts), ptr(flags)))
    return counts[:len(cand)]


def _resident(tables, host: bool):
    """The resident tables of a map for a stage: flushed, then their sizes and
    either the host arrays (for an injected counter / assembler) or the device
    tensors. Tables kept on the host by an applier serve host callables only: a
    missing kernel path is an error, not a fallback."""
    tables.flush()
    if host:
        return tables.sizes(), tables.host_arrays()
    if tables.host:
        raise GFError(-4, "tables resident on the host (applier=) need the stage's host counter / assembler")
    return tables.sizes(), tables.arrays()


class _CullTables:
    """The five tables of :func:`culling_tables` for one KeyFrameCulling,
    resident on the device (uploaded once) unless a host ``counter`` is
    injected. After a cull only what the surgery touched is written again:
    -1 over the erased observations (the CSR is never rebuilt), the bad flags
    of the points that turned bad and -1 in the slots their SetBadFlag
    cleared. With resident tables attached to the map (``map.tables``) nothing
    is built or uploaded: the tables are flushed and taken from there, and a
    refresh is another flush, ``set_bad_keyframe`` having journalled its
    surgery."""

    NAMES = ("kf_off", "octave", "slots", "mp_bad", "obs_off", "obs_gkp")

    def __init__(self, map, ctx, counter=None):
        self.map, self.ctx, self.counter = map, ctx, counter
        self.launches = 0
        self.res = getattr(map, "tables", None)
        if counter is None:
            import torch

            self.torch = torch
            self.dev = torch.device("cuda", torch.cuda.current_device())
        if self.res is not None:
            self._take()
            return
        (self.kf_off, self.octave, self.slots, self.mp_bad, self.obs_off, self.obs_gkp,
         self.where) = culling_tables(map)
        self.n = dict(nkf=len(self.kf_off) - 1, nkp=len(self.slots), nmp=len(self.mp_bad), nobs=len(self.obs_gkp))
        if counter is None:
            self.d = [self._t(a) for a in (self.kf_off, self.octave, self.slots, self.mp_bad, self.obs_off,
                                           self.obs_gkp)]
            self.torch.cuda.current_stream().synchronize()

    def _take(self):
        """The resident tables after a flush (which may have reallocated them)."""
        self.n, arrays = _resident(self.res, self.counter is not None)
        if self.counter is not None:
            self.kf_off, self.octave, self.slots, self.mp_bad, self.obs_off, self.obs_gkp = (
                arrays[name] for name in self.NAMES)
        else:
            self.d = [arrays[name] for name in self.NAMES]

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def count(self, cand):
        """One launch over the candidates -> counts [ncand, 2]."""
        cand = np.ascontiguousarray(cand, np.int32)
        self.launches += 1
        if self.counter is not None:
            return np.asarray(self.counter(self.kf_off, self.octave, self.slots, self.mp_bad, self.obs_off,
                                           self.obs_gkp, cand), np.int32).reshape(-1, 2)
        torch = self.torch
        d_cand = self._t(cand)
        d_counts = torch.empty(len(cand) * 2, dtype=torch.int32, device=self.dev)
        torch.cuda.current_stream().synchronize()  # the uploads and refreshes ran on torch's stream
        d, n = self.d, self.n
        check(lib().gf_keyframe_culling_counts_dev(self.ctx.handle, n["nkf"], n["nkp"], ptr(d[0]), ptr(d[1]),
                                                   ptr(d[2]), n["nmp"], ptr(d[3]), ptr(d[4]), ptr(d[5]), n["nobs"],
                                                   len(cand), ptr(d_cand), ptr(d_counts), None, self.ctx.stream))
        self.ctx.sync()
        return d_counts.cpu().numpy().reshape(-1, 2)

    def refresh(self, log):
        """Point updates after ``set_bad_keyframe`` returned ``log``."""
        if self.res is not None:
            self._take()
            return
        gone = np.asarray([self.where[(p, k)] for p, k, _ in log["observations"]], np.int64)
        bad = np.asarray(log["points_bad"], np.int64)
        cleared = np.asarray([self.kf_off[k] + i for k, i in log["cleared"]], np.int64)
        self.obs_gkp[gone], self.mp_bad[bad], self.slots[cleared] = -1, 1, -1
        if self.counter is None:
            for j, rows, v in ((5, gone, -1), (3, bad, 1), (2, cleared, -1)):
                if len(rows):
                    self.d[j][self._t(rows)] = v


def keyframe_culling(map, cur: int, db=None, ctx=None, counter=None) -> dict:
    """LocalMapping::KeyFrameCulling (:562-616) on a LoopMap for the current
    keyframe ``cur``.

    The candidates are a copy of ``map.ordered[cur]`` taken once (:567), walked
    in that order, the first keyframe (mnId 0) skipped. One
    ``gf_keyframe_culling_counts_dev`` launch on device-resident tables
    (:class:`_CullTables`) counts nMPs and nRedundantObservations of every
    candidate; where nothing is culled that is all the device work. The
    decision ``nredundant > 0.9 * nmps`` is taken here in double.

    When a candidate K is culled, ``map.set_bad_keyframe(K, db)`` runs on the
    host, the device copy receives point updates only, and the candidates after
    K are counted again in one launch before the walk goes on: K's
    observations are gone from the rows of its points (fewer observations,
    fewer octave-qualified observers), and the points that fell to two
    observations turned bad and left other keyframes' nMPs. A candidate before
    K was already decided on the map of its own turn. A candidate that
    ``set_bad_keyframe`` deferred (``not_erase``) changed nothing but its
    ``to_be_erased``, so nothing is refreshed or counted again.

    counter: a callable with the signature of
    :func:`keyframe_culling_counts` used instead of the device, on host copies
    of the tables (the CPU tests inject the restatement's).

    -> report dict: ``candidates``; ``per_candidate``: a dict per candidate
    with ``kf``, ``nmps`` / ``nredundant`` (the counts of its own turn),
    ``culled``, ``deferred`` and ``recounted`` (how many times it was counted
    again); ``culled``: the culled keyframes in order; ``points_bad``;
    ``reparented``: (child, new parent) pairs; ``launches``; ``times``: seconds
    spent in uploads, launches, the host walk and the refreshes."""
    import time

    cur = int(cur)
    cand = [int(k) for k in map.ordered[cur] if map.kf_id[int(k)] != 0]
    n = len(cand)
    per = [dict(kf=k, nmps=0, nredundant=0, culled=False, deferred=False, recounted=0) for k in cand]
    rep = dict(candidates=cand, per_candidate=per, culled=[], points_bad=[], reparented=[], launches=0,
               times=dict(upload=0.0, launch=0.0, walk=0.0, refresh=0.0))
    if not n:
        return rep
    t = [time.perf_counter()]

    def lap(name):
        t.append(time.perf_counter())
        rep["times"][name] += t[-1] - t[-2]

    tables = _CullTables(map, None if counter is not None else (ctx or default_context()), counter)
    lap("upload")
    counts = tables.count(cand)
    lap("launch")
    for j, k in enumerate(cand):
        nmps, nred = int(counts[j, 0]), int(counts[j, 1])
        per[j]["nmps"], per[j]["nredundant"] = nmps, nred
        if not float(nred) > 0.9 * float(nmps):
            continue
        log = map.set_bad_keyframe(k, db)
        per[j]["deferred"], per[j]["culled"] = log["deferred"], log["erased"]
        if not log["erased"]:
            continue
        rep["culled"].append(k)
        rep["points_bad"] += log["points_bad"]
        rep["reparented"] += log["reparented"]
        lap("walk")
        tables.refresh(log)
        lap("refresh")
        if j + 1 < n:
            counts[j + 1:] = tables.count(cand[j + 1:])
            for q in per[j + 1:]:
                q["recounted"] += 1
        lap("launch")
    lap("walk")
    rep["launches"] = tables.launches
    return rep


# ------------------------------------------------ ProcessNewKeyFrame / UpdateConnections
def update_connections_counts(kf_off, slots, mp_bad, obs_off, obs_gkp, query, ctx=None):
    """``gf_update_connections`` on host arrays (the counting and ordering of
    KeyFrame.cc:332-403 for every query keyframe in one launch) -> (weights
    [nq, nkf], n_ordered [nq], ordered_kf [nq, nkf], ordered_w [nq, nkf]), all
    int32; the ordered rows hold -1 / 0 past n_ordered."""
    ctx = ctx or default_context()
    c = np.ascontiguousarray
    kf_off, slots, obs_off, obs_gkp, query = (c(a, np.int32).reshape(-1) for a in (kf_off, slots, obs_off, obs_gkp, query))
    mp_bad = c(mp_bad, np.uint8).reshape(-1)
    if len(kf_off) < 1 or len(obs_off) != len(mp_bad) + 1:
        raise GFError(-1, "table lengths disagree")
    nkf, nq = len(kf_off) - 1, len(query)
    if (nkf and kf_off[-1] != len(slots)) or obs_off[-1] != len(obs_gkp):
        raise GFError(-1, "table lengths disagree")
    weights, n_ordered = np.zeros((nq, nkf), np.int32), np.zeros(nq, np.int32)
    ordered_kf, ordered_w = np.full((nq, nkf), -1, np.int32), np.zeros((nq, nkf), np.int32)
    check(lib().gf_update_connections(ctx.handle, nkf, ptr(kf_off), ptr(slots), len(mp_bad), ptr(mp_bad), ptr(obs_off),
                                      ptr(obs_gkp), nq, ptr(query), ptr(weights) if nkf else None, ptr(n_ordered),
                                      ptr(ordered_kf) if nkf else None, ptr(ordered_w) if nkf else None))
    return weights, n_ordered, ordered_kf, ordered_w


class _CovisTables:
    """The tables of :func:`culling_tables` that UpdateConnections reads
    (``kf_off``, ``slots``, ``mp_bad``, ``obs_off``, ``obs_gkp``) for one
    ``LoopMap.connections_counts``, uploaded once unless a host ``counter`` is
    injected. With resident tables attached to the map (``map.tables``) they
    are flushed and taken from there instead."""

    NAMES = ("kf_off", "slots", "mp_bad", "obs_off", "obs_gkp")

    def __init__(self, map, ctx=None, counter=None):
        self.counter = counter
        self.nkf = map.nkf
        if counter is None:
            import torch

            self.ctx, self.torch = ctx or default_context(), torch
            self.dev = torch.device("cuda", torch.cuda.current_device())
        if getattr(map, "tables", None) is not None:
            self.n, arrays = _resident(map.tables, counter is not None)
            if counter is not None:
                self.kf_off, self.slots, self.mp_bad, self.obs_off, self.obs_gkp = (arrays[n] for n in self.NAMES)
            else:
                self.d = [arrays[n] for n in self.NAMES]
            return
        self.kf_off, _, self.slots, self.mp_bad, self.obs_off, self.obs_gkp, _ = culling_tables(map)
        self.n = dict(nkf=len(self.kf_off) - 1, nkp=len(self.slots), nmp=len(self.mp_bad), nobs=len(self.obs_gkp))
        if counter is None:
            self.d = [self._t(a) for a in (self.kf_off, self.slots, self.mp_bad, self.obs_off, self.obs_gkp)]
            self.torch.cuda.current_stream().synchronize()

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def count(self, kfs):
        """One launch over the query keyframes -> (weights [nq, nkf], per
        query ``(ordered keyframes, their weights)`` as lists)."""
        query = np.ascontiguousarray([int(k) for k in kfs], np.int32)
        nq, nkf = len(query), self.nkf
        if not nq or not nkf:
            return np.zeros((nq, nkf), np.int32), [([], []) for _ in range(nq)]
        if self.counter is not None:
            w, n, ok, ow = self.counter(self.kf_off, self.slots, self.mp_bad, self.obs_off, self.obs_gkp, query)
        else:
            torch = self.torch
            d_query = self._t(query)
            d_out = torch.empty((3 * nkf + 1) * nq, dtype=torch.int32, device=self.dev)  # weights | kf | w | n
            torch.cuda.current_stream().synchronize()  # the uploads ran on torch's stream
            d, row, n = self.d, nq * nkf, self.n
            check(lib().gf_update_connections_dev(self.ctx.handle, nkf, n["nkp"], ptr(d[0]), ptr(d[1]),
                                                  n["nmp"], ptr(d[2]), ptr(d[3]), ptr(d[4]), n["nobs"],
                                                  nq, ptr(d_query), ptr(d_out), ptr(d_out[3 * row:]),
                                                  ptr(d_out[row:]), ptr(d_out[2 * row:]), self.ctx.stream))
            self.ctx.sync()
            out = d_out.cpu().numpy()
            w, ok, ow, n = (out[:row].reshape(nq, nkf), out[row:2 * row].reshape(nq, nkf),
                            out[2 * row:3 * row].reshape(nq, nkf), out[3 * row:])
        w, n, ok, ow = (np.asarray(a, np.int32) for a in (w, n, ok, ow))
        return w.reshape(nq, nkf), [(ok.reshape(nq, nkf)[i, :n[i]].tolist(), ow.reshape(nq, nkf)[i, :n[i]].tolist())
                                    for i in range(nq)]


def process_new_keyframe(map, cur: int, voc, recent: list, levelsup: int = 4, ctx=None, counter=None) -> dict:
    """LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:163-211) on a
    LoopMap for the keyframe ``cur``, already appended with
    ``LoopMap.add_keyframe``.

    ComputeBoW (KeyFrame.cc:56-65): only when ``map.kf_bow[cur]`` or
    ``map.kf_fv[cur]`` is empty; ``voc`` is an ``ORBVocabulary`` (its
    ``transform``) or a callable ``(descriptors, levelsup) -> (words, values,
    FeatureVector or (nodes, start, feats))``; both results are stored. The
    first keyframe (mnId 0) returns after it (:172-173).

    mnId > 1 (:177-192): the slot table is copied once and walked in slot
    order; every non-NULL, non-bad point gets ``add_observation(p, cur, i)``, so
    a point in two slots ends with the later one. The reference then calls
    UpdateNormalAndDepth and ComputeDistinctiveDescriptors on the point inside
    the loop; here both run once over the distinct ids after it
    (``update_normal_and_depth_batch``, ``compute_distinctive_descriptors``).
    That is the same: each reads only its own point's observations, the
    keyframes' descriptors and poses and the point's position, and writes only
    its own point's normal, distance bounds and descriptor, which the other
    call and every other point's calls never read. A point's observations change
    inside the loop only through its own ``add_observation``, so they are
    final after its last slot, and the calls the reference makes at an earlier
    slot of the same point are recomputed from scratch at the later one. No
    pose and no keyframe descriptor changes in between.

    mnId 1 (:194-204): every non-NULL slot point, bad ones included (the test
    is on the pointer only), is appended to ``recent``
    (mlpRecentAddedMapPoints).

    UpdateConnections (:207): one ``gf_update_connections_dev`` launch for
    ``cur`` (``counter``: a host callable instead, as in
    ``LoopMap.connections_counts``), then ``map.apply_connections``.

    -> report dict: ``associated`` (the ids given an observation, in slot
    order), ``recent_added``, ``n_ordered``, ``parent`` and ``times``: seconds
    spent in bow, association, tables (build and upload), launch (and
    download) and apply."""
    import time

    cur = int(cur)
    times = dict(bow=0.0, association=0.0, tables=0.0, launch=0.0, apply=0.0)
    rep = dict(associated=[], recent_added=[], n_ordered=0, parent=int(map.parent[cur]), times=times)
    t = [time.perf_counter()]

    def lap(name):
        t.append(time.perf_counter())
        times[name] += t[-1] - t[-2]

    if map.kf_bow[cur] is None or map.kf_fv[cur] is None:
        transform = voc.transform if hasattr(voc, "transform") else voc
        words, values, fv = transform(map.kf_desc[cur], levelsup)
        map.kf_bow[cur] = (words, values)
        map.kf_fv[cur] = fv if isinstance(fv, FeatureVector) else FeatureVector(*fv)
    lap("bow")
    cur_id = int(map.kf_id[cur])
    if cur_id == 0:
        return rep
    pts = map.slots[cur].copy()  # vpMapPointMatches (:176), taken once
    if cur_id > 1:
        for i, p in enumerate(pts):
            p = int(p)
            if p < 0 or map.mp_bad[p]:
                continue
            map.add_observation(p, cur, i)
            rep["associated"].append(p)
        ids = list(dict.fromkeys(rep["associated"]))
        if counter is None:
            map.update_normal_and_depth_batch(ids, ctx)
        else:
            map.update_normal_and_depth(ids)
        map.compute_distinctive_descriptors(ids)
    else:
        rep["recent_added"] = [int(p) for p in pts if p >= 0]
        recent.extend(rep["recent_added"])
    lap("association")
    tables = _CovisTables(map, ctx, counter)
    lap("tables")
    weights, ordered = tables.count([cur])
    lap("launch")
    map.apply_connections(cur, weights[0], *ordered[0])
    lap("apply")
    rep["n_ordered"], rep["parent"] = len(ordered[0][0]), int(map.parent[cur])
    return rep


class LocalMapper:
    """The body of ``LocalMapping::Run`` (src/LocalMapping.cc:49-129) for one
    keyframe at a time on a LoopMap, without the queue and the thread: the
    caller inserts a keyframe and steps it through the stages in the
    reference's order. Holds the map, the vocabulary, mlpRecentAddedMapPoints
    (``recent``) and the context, and optionally the keyframe database ``db``
    (``loopdetect.KeyFrameDatabase``, told of culled keyframes) and the loop
    ``detector`` (``loopdetect.LoopDetector``, kept for the caller: the keyframe
    a step returns in ``to_loop_closer`` is what mpLoopCloser->InsertKeyFrame
    would receive, and calling the detector with it is the caller's business).

    counter / assembler / solver: host callables handed to the stages that
    take them (``process_new_keyframe``, ``keyframe_culling``;
    ``local_bundle_adjustment``); stages: a dict replacing stage functions by
    name (the CPU tests record the order with it). resident: attach resident
    flat tables to the map at construction (``LoopMap.attach_tables``;
    ``applier`` as there, for the host callables), unless it has some."""

    STAGES = ("process_new_keyframe", "map_point_culling", "create_new_map_points", "search_in_neighbors",
              "local_bundle_adjustment", "keyframe_culling")

    def __init__(self, map, voc, ctx=None, db=None, detector=None, levelsup=4, counter=None, cull_counter=None,
                 assembler=None, solver=None, stages=None, resident=False, applier=None):
        self.map, self.voc, self.ctx, self.db, self.detector = map, voc, ctx, db, detector
        if resident and map.tables is None:
            map.attach_tables(ctx=ctx, applier=applier)
        self.levelsup, self.recent = levelsup, []
        self.counter, self.cull_counter, self.assembler, self.solver = counter, cull_counter, assembler, solver
        self.stages = dict(process_new_keyframe=process_new_keyframe, map_point_culling=map_point_culling,
                           create_new_map_points=create_new_map_points, search_in_neighbors=search_in_neighbors,
                           local_bundle_adjustment=local_bundle_adjustment, keyframe_culling=keyframe_culling)
        self.stages.update(stages or {})

    def insert_keyframe(self, kps, desc, slots, Tcw, kf_id=None) -> int:
        """What tracking hands over (LocalMapping::InsertKeyFrame after ``new
        KeyFrame``): ``map.add_keyframe`` -> the keyframe's index."""
        return self.map.add_keyframe(kps, desc, slots, Tcw, kf_id)

    def step(self, cur: int, abort_ba: bool = False, stop_flag=None) -> dict:
        """One pass of the loop body for keyframe ``cur`` (:68-124):
        ProcessNewKeyFrame, MapPointCulling, CreateNewMapPoints (with
        ``map.kf_fv``), SearchInNeighbors and, unless ``abort_ba`` (mbAbortBA /
        stopRequested, :100), LocalBundleAdjustment (``stop_flag`` polled inside)
        and KeyFrameCulling. -> report dict: per stage run ``dict(report=the
        stage's own, seconds=host clock)``; ``order``: the stages run;
        ``to_loop_closer``: ``cur`` (:124)."""
        import time

        cur, m, s = int(cur), self.map, self.stages
        rep = dict(order=[])

        def run(name, fn):
            t0 = time.perf_counter()
            out = fn()
            rep[name] = dict(report=out, seconds=time.perf_counter() - t0)
            rep["order"].append(name)
            return out

        run("process_new_keyframe", lambda: s["process_new_keyframe"](m, cur, self.voc, self.recent, self.levelsup,
                                                                      ctx=self.ctx, counter=self.counter))
        self.recent[:] = run("map_point_culling", lambda: s["map_point_culling"](m, self.recent, cur))
        ids, _ = run("create_new_map_points", lambda: s["create_new_map_points"](m, cur, m.kf_fv, ctx=self.ctx))
        self.recent.extend(ids)  # mlpRecentAddedMapPoints.push_back (:406)
        run("search_in_neighbors", lambda: s["search_in_neighbors"](m, cur, ctx=self.ctx))
        if not abort_ba:
            run("local_bundle_adjustment", lambda: s["local_bundle_adjustment"](
                m, cur, stop_flag=stop_flag, ctx=self.ctx, assembler=self.assembler, solver=self.solver))
            run("keyframe_culling", lambda: s["keyframe_culling"](m, cur, db=self.db, ctx=self.ctx,
                                                                  counter=self.cull_counter))
        rep["to_loop_closer"] = cur
        return rep


class _DeviceMap:
    """The whole-map arrays of a LoopMap resident on the device for one
    SearchInNeighbors: positions, normals and distance bounds are uploaded
    once (nothing in :436-468 writes them), descriptor rows and bad flags again
    only where they changed since the last search; a keyframe's keypoints and
    descriptors once."""

    def __init__(self, map, ctx):
        import torch

        self.map, self.ctx, self.torch = map, ctx, torch
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.d_mps, self.d_md = self._t(map.mps.view(np.uint8)), self._t(map.mp_desc)
        self.d_bad = self._t(map.mp_bad.astype(np.uint8))
        self.epoch, self.bad = map.desc_epoch.copy(), map.mp_bad.copy()
        self.kf_bufs = {}

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _refresh(self):
        m = self.map
        rows = np.nonzero(m.desc_epoch != self.epoch)[0]
        if len(rows):
            self.d_md[self._t(rows)] = self._t(m.mp_desc[rows])
            self.epoch[rows] = m.desc_epoch[rows]
        rows = np.nonzero(m.mp_bad != self.bad)[0]
        if len(rows):
            self.d_bad[self._t(rows)] = self._t(m.mp_bad[rows].astype(np.uint8))
            self.bad[rows] = m.mp_bad[rows]

    def search(self, problems, th):
        """One ``gf_fuse_search_dev`` launch against the map as it stands.
        problems: (keyframe, candidate ids, skip bytes) per problem. -> kp per
        problem."""
        from .matcher import FuseSearchProblem, camera_center

        m, torch = self.map, self.torch
        self._refresh()
        keep, pts_bufs, probs, d_res = [], {}, [], []
        for k, pts, skip in problems:
            n = len(m.kf_kps[k])
            if k not in self.kf_bufs:  # a keyframe listed twice is uploaded once
                self.kf_bufs[k] = (self._t(m.kf_kps[k].view(np.uint8)), self._t(m.kf_desc[k])) if n else (None, None)
            if id(pts) not in pts_bufs:  # the forward problems share one candidate list
                pts_bufs[id(pts)] = self._t(np.asarray(pts, np.int32))
            d_pts, d_skip = pts_bufs[id(pts)], self._t(np.asarray(skip, np.uint8))
            r = torch.empty(len(pts) * 2, dtype=torch.int32, device=self.dev)
            keep.append(d_skip)
            d_res.append(r)
            kb = self.kf_bufs[k]
            probs.append(FuseSearchProblem.make(m.Tcw[k], camera_center(m.Tcw[k]), kb[0], kb[1], n, d_pts, d_skip,
                                                len(pts), th, r))
        arr = (FuseSearchProblem * len(probs))(*probs)
        torch.cuda.current_stream().synchronize()  # the uploads above ran on torch's stream
        check(lib().gf_fuse_search_dev(self.ctx.handle, ctypes.byref(m.info), len(probs), arr, ptr(self.d_mps),
                                       ptr(self.d_md), ptr(self.d_bad), len(m.mps), self.ctx.stream))
        self.ctx.sync()
        return [r.cpu().numpy().reshape(-1, 2)[:, 0].copy() for r in d_res]


def _in_keyframe(map, pts, k):
    """Per candidate: NULL, isBad() or IsInKeyFrame(k) (ORBmatcher.cc:1611-1615)
    on the live map."""
    return np.asarray([p < 0 or bool(map.mp_bad[p]) or map.is_in_keyframe(p, k) for p in (int(q) for q in pts)],
                      np.uint8)


def _fuse_walk(map, dmap, k, pts, kp, epoch, th, stats):
    """The candidate loop of one ``Fuse(k, pts)`` call on the live map, kp the
    search results made with the descriptors of ``epoch``. -> (rows, nFused)."""
    def search(idx, key="researched"):
        sub = np.ascontiguousarray(pts[idx])
        new = dmap.search([(k, sub, _in_keyframe(map, sub, k))], th)[0]
        stats[key] += len(idx)
        stats["changed"] += int(np.count_nonzero(new != kp[idx]))
        kp[idx] = new
        epoch[idx] = map.desc_epoch[pts[idx]]

    kp, epoch = kp.copy(), epoch.copy()
    valid = np.nonzero(pts >= 0)[0]
    stale = valid[map.desc_epoch[pts[valid]] != epoch[valid]]
    stale = stale[_in_keyframe(map, pts[stale], k) == 0]  # the others leave at :1614 whatever their descriptor
    if len(stale):
        search(stale)
    rows, nfused = [], 0
    for i in valid:
        p = int(pts[i])
        if map.mp_bad[p] or map.is_in_keyframe(p, k):  # :1614 on the live map
            continue
        if map.desc_epoch[p] != epoch[i]:       # changed inside this call: only where a slot table and an
            search(np.asarray([i]), "in_call")  # observation map disagree (see search_in_neighbors)
        if kp[i] < 0:
            continue
        idx = int(kp[i])
        occ = int(map.slots[k][idx])
        if occ >= 0:
            if not map.mp_bad[occ]:
                map.replace(p, occ)  # pMP->Replace(pMPinKF): the candidate goes, the occupant stays
                rows.append((p, idx, "replace", occ))
            else:
                rows.append((p, idx, "keep", occ))
        else:
            map.add_observation(p, k, idx)
            map.add_map_point(k, p, idx)
            rows.append((p, idx, "add", -1))
        nfused += 1
    return rows, nfused


def fuse_targets(map, cur: int):
    """vpTargetKFs of SearchInNeighbors (:414-433), stamping
    ``map.fuse_target_for`` as it goes. Only first neighbours are stamped, so a
    second neighbour can be listed more than once."""
    cur = int(cur)
    cur_id = int(map.kf_id[cur])
    targets = []
    for k in [int(k) for k in map.ordered[cur][:MAX_NEIGHBOURS]]:
        if map.kf_bad[k] or map.fuse_target_for[k] == cur_id:
            continue
        targets.append(k)
        map.fuse_target_for[k] = cur_id
        for k2 in [int(q) for q in map.ordered[k][:SECOND_NEIGHBOURS]]:
            if map.kf_bad[k2] or map.fuse_target_for[k2] == cur_id or int(map.kf_id[k2]) == cur_id:
                continue
            targets.append(k2)
    return targets


def search_in_neighbors(map, cur: int, th: float = 3.0, ctx=None) -> dict:
    """LocalMapping::SearchInNeighbors (:411-488) on a LoopMap for the new
    keyframe ``cur``, in the reference's order.

    Targets (:414-433): :func:`fuse_targets`.

    Forward (:436-444): the candidate list is ``cur``'s slot table, taken once.
    One ``gf_fuse_search_dev`` launch searches every target (duplicates
    included) against the map as it stands, ``skip`` read from the observation
    map. The targets are then walked in list order and the candidates in list
    order on the host, where ORBmatcher.cc:1690-1703 runs on the live map.

    Why the launch's results hold at a candidate's turn. A search reads the
    candidate's position, normal and distance bounds (nothing in :436-468
    writes them), the keyframe (constant) and the candidate's descriptor.
    ``MapPoint::Replace`` recomputes the survivor's descriptor and nothing else
    does, so ``LoopMap.desc_epoch`` names every search that is out of date;
    before a target's turn those candidates are searched again in one small
    call on the device-resident map (:class:`_DeviceMap`: only the descriptor
    rows and flags that changed are uploaded again). A candidate that is bad or in the keyframe at the launch is still so
    at its turn, which makes both a safe prefilter: a bad point stays bad, and
    an observation leaves a point's map only when ``Replace`` or ``SetBadFlag``
    empties the whole map and turns the point bad. Inside one ``Fuse`` call a
    descriptor changes only through ``pMP->Replace(pMPinKF)``, and the
    survivor ``pMPinKF`` sits in the keyframe's slot table: when it also is a
    later candidate of the same call it observes the keyframe and leaves at
    :1614 without a search, so no candidate's descriptor changes between the
    start of a call and its own search. That last step leans on the slot
    table and the observation map agreeing, which the map does not promise
    (docs/ORACLE_ASSUMPTIONS.md A26); the walk therefore compares the epoch
    again at the candidate's turn and searches that one candidate again if it
    moved, so the result is the serial one either way.

    Backward (:446-468): the candidates are the targets' slot tables after the
    forward walk, in list order, non-NULL, not bad, first occurrence by
    ``map.fuse_candidate_for``; one ``gf_fuse_search_dev`` problem for ``cur``
    (spread over candidate chunks), applied on the live map by the same walk. A
    later candidate that picks a slot an earlier one filled finds it as the
    occupant and is replaced by it.

    Update (:472-487): ``compute_distinctive_descriptors`` then
    ``update_normal_and_depth_batch`` once over the non-bad points of ``cur``
    instead of both per point in turn: each reads only the point's own
    observations, the keyframes' descriptors and poses and the point's
    position, and writes only the point's own descriptor, normal and distance
    bounds, which the other call on another point never reads. Then
    ``update_connections(cur)``.

    -> report dict: ``targets``; ``forward``: per target ``dict(kf, rows,
    nFused)`` with rows ``(point, kp, "add" | "replace" | "keep", other)``;
    ``researched`` / ``research_changed``: candidates searched again and how
    many of them changed kp, ``researched_in_call`` those of them searched again
    at their own turn (0 on a map whose tables and observations agree); ``candidates``, ``backward`` (``rows``,
    ``nFused``); ``updated``: the point ids of the update pass."""
    cur = int(cur)
    cur_id = int(map.kf_id[cur])
    ctx = ctx or default_context()
    stats = dict(researched=0, in_call=0, changed=0)
    targets = fuse_targets(map, cur)
    dmap = None
    # forward
    pts = map.slots[cur].astype(np.int32).copy()  # vpMapPointMatches, taken once (:438)
    forward = []
    if targets and len(pts):
        epoch = map.desc_epoch[np.maximum(pts, 0)] if len(map.mps) else np.zeros(len(pts), np.int64)
        dmap = _DeviceMap(map, ctx)
        kps = dmap.search([(k, pts, _in_keyframe(map, pts, k)) for k in targets], th)
        for k, kp in zip(targets, kps):
            rows, nf = _fuse_walk(map, dmap, k, pts, kp, epoch, th, stats)
            forward.append(dict(kf=k, rows=rows, nFused=nf))
    else:
        forward = [dict(kf=k, rows=[], nFused=0) for k in targets]
    # backward
    cand = []
    for k in targets:
        for p in map.slots[k]:
            p = int(p)
            if p < 0 or map.mp_bad[p] or map.fuse_candidate_for[p] == cur_id:
                continue
            map.fuse_candidate_for[p] = cur_id
            cand.append(p)
    cand = np.asarray(cand, np.int32)
    back_rows, back_nf = [], 0
    if len(cand):
        epoch = map.desc_epoch[cand].copy()
        dmap = dmap or _DeviceMap(map, ctx)
        kp = dmap.search([(cur, cand, _in_keyframe(map, cand, cur))], th)[0]
        back_rows, back_nf = _fuse_walk(map, dmap, cur, cand, kp, epoch, th, stats)
    # update
    ids = list(dict.fromkeys(int(p) for p in map.slots[cur] if p >= 0 and not map.mp_bad[p]))  # each once
    map.compute_distinctive_descriptors(ids)
    map.update_normal_and_depth_batch(ids, ctx)
    map.update_connections(cur)
    return dict(targets=targets, forward=forward, researched=stats["researched"] + stats["in_call"],
                researched_in_call=stats["in_call"], research_changed=stats["changed"],
                candidates=[int(p) for p in cand], backward=dict(rows=back_rows, nFused=back_nf), updated=ids)


# ------------------------------------------------ LocalBundleAdjustment on the map
class LBATables(ctypes.Structure):
    """gf_lba_tables: the flat map tables ``gf_lba_graph`` reads."""

    _fields_ = [(n, ctypes.c_int32) for n in ("nkf", "nkp", "nmp", "nobs", "nlevels", "kf0")] + [
        (n, ctypes.c_void_p) for n in ("kf_off", "octave", "slots", "kf_bad", "kp_xy", "kf_Tcw", "mp_bad", "mp_pos",
                                       "obs_off", "obs_gkp", "inv_sigma2")] + [("cam", ctypes.c_float * 4)]


class LBAGraphOut(ctypes.Structure):
    """gf_lba_graph_out: the assembled gf_ba_problem and the write-back's maps."""

    _fields_ = [(n, ctypes.c_void_p) for n in ("counts", "prob_kf", "kf_kind", "kf_Tcw", "kf_cam", "prob_pt", "pt_pos",
                                               "edge_pt", "edge_kf", "edge_z", "edge_inv_sigma2", "edge_gkp")]


# table name, dtype, elements per row, which size it follows (+1: one more row)
_LBA_TABLES = (("kf_off", np.int32, 1, "nkf+"), ("octave", np.uint8, 1, "nkp"), ("slots", np.int32, 1, "nkp"),
               ("kf_bad", np.uint8, 1, "nkf"), ("kp_xy", np.float32, 2, "nkp"), ("kf_Tcw", np.float32, 16, "nkf"),
               ("mp_bad", np.uint8, 1, "nmp"), ("mp_pos", np.float32, 3, "nmp"), ("obs_off", np.int32, 1, "nmp+"),
               ("obs_gkp", np.int32, 1, "nobs"), ("inv_sigma2", np.float32, 1, "nlevels"))
# output name, dtype, elements per row, the count it follows (0 keyframes, 1 points, 2 edges)
_LBA_OUT = (("prob_kf", np.int32, 1, 0), ("kf_kind", np.uint8, 1, 0), ("kf_Tcw", np.float32, 16, 0),
            ("kf_cam", np.float32, 4, 0), ("prob_pt", np.int32, 1, 1), ("pt_pos", np.float32, 3, 1),
            ("edge_pt", np.int32, 1, 2), ("edge_kf", np.int32, 1, 2), ("edge_z", np.float32, 2, 2),
            ("edge_inv_sigma2", np.float32, 1, 2), ("edge_gkp", np.int32, 1, 2))
MAX_LOCAL_BA_KEYFRAMES = 32


def lba_tables(map) -> dict:
    """The flat tables ``gf_lba_graph`` reads, of a LoopMap as it stands: the
    five of :func:`culling_tables` (with ``where``), the keyframes' bad flags,
    undistorted keypoint positions and poses, the points' positions,
    ``inv_sigma2`` per level, the camera and ``kf0``, the index of the keyframe
    with mnId 0 (-1 without one)."""
    kf_off, octave, slots, mp_bad, obs_off, obs_gkp, where = culling_tables(map)
    xy = [np.zeros((0, 2), np.float32)] + [np.stack([k["x"], k["y"]], axis=1).astype(np.float32) for k in map.kf_kps]
    return dict(kf_off=kf_off, octave=octave, slots=slots, mp_bad=mp_bad, obs_off=obs_off, obs_gkp=obs_gkp, where=where,
                kp_xy=np.ascontiguousarray(np.concatenate(xy)), **_lba_dense(map))


def _lba_dense(map) -> dict:
    """The small dense arrays of :func:`lba_tables` that code writes directly
    (``kf_bad``, ``kf_Tcw``, ``mp_pos``), ``inv_sigma2``, the camera and
    ``kf0``: vectorised and small, so taken whole whenever a stage asks."""
    from .optimizer import inv_level_sigma2

    first = np.nonzero(np.asarray(map.kf_id) == 0)[0]
    i = map.info
    return dict(kf_bad=map.kf_bad.astype(np.uint8), kf_Tcw=np.ascontiguousarray(map.Tcw, np.float32).reshape(-1, 16),
                mp_pos=np.ascontiguousarray(map.mps["pos"], np.float32).reshape(-1, 3),
                inv_sigma2=inv_level_sigma2(i.nlevels, i.scale_factor), cam=np.asarray([i.fx, i.fy, i.cx, i.cy], np.float32),
                kf0=int(first[0]) if len(first) else -1)


def lba_tables_resident(map) -> dict:
    """:func:`lba_tables` from the map's resident tables on the host (for an
    injected assembler): the rows carry their -1 padding, ``where`` is None."""
    n, a = _resident(map.tables, True)
    return dict({name: a[name] for name in ("kf_off", "octave", "slots", "mp_bad", "obs_off", "obs_gkp")}, where=None,
                kp_xy=a["kp_xy"].reshape(-1, 2), **_lba_dense(map))


def lba_local_keyframes(map, cur: int) -> list:
    """lLocalKeyFrames (Optimizer.cc:1520-1530): the current keyframe, then its
    ordered covisibles that are not bad."""
    return [int(cur)] + [int(k) for k in map.ordered[int(cur)] if not map.kf_bad[int(k)]]


def _lba_struct(t: dict, arrays: dict) -> LBATables:
    """The gf_lba_tables of the (host or device) ``arrays``, after checking the
    host-side lengths of ``t`` against each other."""
    n = dict(nkf=len(t["kf_off"]) - 1, nkp=len(t["octave"]), nmp=len(t["mp_bad"]), nobs=len(t["obs_gkp"]),
             nlevels=len(t["inv_sigma2"]))
    if n["nkf"] < 0 or len(np.asarray(t["cam"]).reshape(-1)) != 4:
        raise GFError(-1, "table lengths disagree")
    for name, _, per, size in _LBA_TABLES:
        want = (n[size[:-1]] + 1 if size.endswith("+") else n[size]) * per
        if _n_el(t[name]) != want:
            raise GFError(-1, f"table lengths disagree: {name} has {_n_el(t[name])} elements, not {want}")
    q = LBATables(n["nkf"], n["nkp"], n["nmp"], n["nobs"], n["nlevels"], int(t["kf0"]),
                  *[ptr(arrays[name]) if _n_el(arrays[name]) else None for name, *_ in _LBA_TABLES])
    q.cam[:] = [float(x) for x in np.asarray(t["cam"], np.float32).reshape(4)]
    return q


def _n_el(a) -> int:
    return int(a.numel()) if hasattr(a, "numel") else int(a.size)


def _lba_cut(bufs: dict, counts) -> dict:
    """The compact problem of the bound-sized output buffers (host arrays)."""
    g = dict(nkf=int(counts[0]), npts=int(counts[1]), nedges=int(counts[2]))
    for name, _, per, which in _LBA_OUT:
        a = bufs[name][:int(counts[which]) * per]
        g[name] = a.reshape(-1, per).copy() if per > 1 else a.copy()
    return g


def lba_graph_arrays(tables: dict, local, ctx=None) -> dict:
    """``gf_lba_graph`` on host arrays (Optimizer.cc:1517-1675): ``tables`` as
    :func:`lba_tables` gives them, ``local`` as :func:`lba_local_keyframes`.
    -> dict: ``nkf`` / ``npts`` / ``nedges``, the gf_ba_problem arrays
    (``kf_Tcw``, ``kf_kind``, ``kf_cam``, ``pt_pos``, ``edge_pt``, ``edge_kf``,
    ``edge_z``, ``edge_inv_sigma2``), ``prob_kf`` / ``prob_pt`` (the map index
    of every problem keyframe / point) and ``edge_gkp`` (the global keypoint
    index of every edge)."""
    ctx = ctx or default_context()
    host = {name: np.ascontiguousarray(tables[name], dt).reshape(-1) for name, dt, _, _ in _LBA_TABLES}
    q = _lba_struct(tables, host)
    local = np.ascontiguousarray(local, np.int32).reshape(-1)
    bound = (max(q.nkf, 1), max(q.nmp, 1), max(q.nobs, 1))
    bufs = {name: np.zeros(bound[which] * per, dt) for name, dt, per, which in _LBA_OUT}
    counts = np.zeros(3, np.int32)
    out = LBAGraphOut(ptr(counts), *[ptr(bufs[name]) for name, *_ in _LBA_OUT])
    check(lib().gf_lba_graph(ctx.handle, ctypes.byref(q), len(local), ptr(local), ctypes.byref(out)))
    return _lba_cut(bufs, counts)


class _LBATables:
    """The tables of :func:`lba_tables` for one LocalBundleAdjustment, resident
    on the device (uploaded once) with the bound-sized output buffers of
    ``gf_lba_graph_dev`` next to them. With resident tables attached to the
    map (``map.tables``) the big tables are flushed and taken from there and
    only the small dense arrays of :func:`_lba_dense` are uploaded; ``nobs`` is
    then the used length of ``obs_gkp``, padding included, and the bound-sized
    outputs follow it."""

    def __init__(self, map, ctx):
        import torch

        self.ctx, self.torch = ctx, torch
        self.dev = torch.device("cuda", torch.cuda.current_device())
        if getattr(map, "tables", None) is not None:
            _, arrays = _resident(map.tables, False)
            self.t = dict(arrays, **_lba_dense(map))
            self.d = {name: arrays[name] if name in arrays else
                      self._t(np.ascontiguousarray(self.t[name], dt).reshape(-1)) for name, dt, _, _ in _LBA_TABLES}
        else:
            self.t = lba_tables(map)
            self.d = {name: self._t(np.ascontiguousarray(self.t[name], dt).reshape(-1))
                      for name, dt, _, _ in _LBA_TABLES}
        self.q = _lba_struct(self.t, self.d)
        bound = (max(self.q.nkf, 1), max(self.q.nmp, 1), max(self.q.nobs, 1))
        tdt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}
        self.o = {name: torch.empty(bound[which] * per, dtype=tdt[dt], device=self.dev)
                  for name, dt, per, which in _LBA_OUT}
        self.counts = torch.zeros(3, dtype=torch.int32, device=self.dev)
        self.out = LBAGraphOut(ptr(self.counts), *[ptr(self.o[name]) for name, *_ in _LBA_OUT])
        torch.cuda.current_stream().synchronize()  # the uploads ran on torch's stream

    def _t(self, a):
        return self.torch.from_numpy(a).to(self.dev)

    def launch(self, local):
        """The assembly enqueued on the context's stream and waited for."""
        local = np.ascontiguousarray(local, np.int32).reshape(-1)
        check(lib().gf_lba_graph_dev(self.ctx.handle, ctypes.byref(self.q), len(local), ptr(local),
                                     ctypes.byref(self.out), self.ctx.stream))
        self.ctx.sync()

    def download(self) -> dict:
        """The compact problem: the counts first, then that much of every buffer."""
        counts = self.counts.cpu().numpy()
        return _lba_cut({name: self.o[name][:int(counts[which]) * per].cpu().numpy()
                         for name, _, per, which in _LBA_OUT}, counts)


def local_bundle_adjustment(map, cur: int, stop_flag=None, ctx=None, assembler=None, solver=None) -> dict:
    """Optimizer::LocalBundleAdjustment(pKF, pbStopFlag) (src/Optimizer.cc:
    1515-1764; LocalMapping.cc:108) on a LoopMap for the current keyframe
    ``cur``.

    Tables: :func:`lba_tables`, built once and uploaded once
    (:class:`_LBATables`). Assembly (:1517-1675): one ``gf_lba_graph_dev`` call
    for the local list of :func:`lba_local_keyframes`; the compact problem is
    downloaded. Solve: ``gf_local_ba_stop`` (``optimizer.local_bundle_adjustment``),
    ``stop_flag`` (a ``ctypes.c_uint8``) polled as mbAbortBA; without edges
    nothing is solved. A local point none of whose observers is alive is a
    vertex without edges: the solver accepts it and leaves it where it is.

    Write-back (:1681-1763) on the map, in the reference's order: the first
    erasure loop walks the edges in order, skips an edge whose point is bad by
    then, and on flag 1 calls ``erase_map_point_match(kf, obs[p][kf])`` then
    ``erase_observation(p, kf)``, which may turn the point bad and clear its
    other slots; the second loop does the same for flag 2; then ``set_pose`` of
    every keyframe of kind 0 or 1, the final position of every local point
    (bad ones included: SetWorldPos has no bad test) and
    ``update_normal_and_depth_batch`` of the local points.

    Two departures (docs/ORACLE_ASSUMPTIONS.md A31, A32). (a) The reference's
    first loop skips an outlier edge whose point an earlier erasure of the same
    loop turned bad, so that edge stays in optimize(10); the solver drops every
    first-round outlier. The map surgery is the same (a bad point has no
    observations left), only the second solve differs; ``stale_outliers``
    counts those edges. (b) The intermediate recover (:1700-1717) is not run:
    all it writes is written again at :1745-1763, except ``normal`` /
    ``min_dist`` / ``max_dist`` of a point that turns bad in the second loop,
    which the reference leaves at values from poses the solver does not
    expose; here they are left untouched.

    assembler(tables, local) / solver(problem): callables used instead of the
    device (the CPU tests inject the restatement's graph and the oracle's
    solver); with an assembler the final update runs on the host too.

    -> report dict: ``local_kfs`` (list order), ``fixed_kfs`` (index order),
    ``npts``, ``nedges``, ``iterations``, ``erased`` (edges erased per round),
    ``points_bad``, ``bad_round2`` (those of them from the second loop),
    ``stale_outliers``, ``graph`` (the assembled problem), ``flags`` /
    ``kf_Tcw`` / ``pt_pos`` (the solver's result, when it ran) and ``times``: seconds spent in tables, assembly, download, solve, write-back
    and update."""
    import time

    from .optimizer import local_bundle_adjustment as solve_window

    cur = int(cur)
    local = lba_local_keyframes(map, cur)
    if sum(1 for k in local if map.kf_id[k] != 0) > MAX_LOCAL_BA_KEYFRAMES:
        raise GFError(-1, "more than 32 local (non-fixed) keyframes")
    times = dict(tables=0.0, assembly=0.0, download=0.0, solve=0.0, writeback=0.0, update=0.0)
    t = [time.perf_counter()]

    def lap(name):
        t.append(time.perf_counter())
        times[name] += t[-1] - t[-2]

    if assembler is None:
        ctx = ctx or default_context()
        tables = _LBATables(map, ctx)
        lap("tables")
        tables.launch(local)
        lap("assembly")
        g = tables.download()
        lap("download")
    else:
        tables = lba_tables(map) if getattr(map, "tables", None) is None else lba_tables_resident(map)
        lap("tables")
        g = assembler(tables, local)
        lap("assembly")
    rep = dict(local_kfs=local, fixed_kfs=[int(k) for k, kind in zip(g["prob_kf"], g["kf_kind"]) if kind == 2],
               npts=g["npts"], nedges=g["nedges"], iterations=(-1, -1), erased=[0, 0], points_bad=[], bad_round2=[],
               stale_outliers=0, graph=g, flags=np.zeros(0, np.uint8), times=times)
    if not g["nedges"]:
        return rep
    if solver is None:
        T, X, flags, its = solve_window(g, ctx, stop_flag)
    else:
        T, X, flags, its = solver(g)
    lap("solve")
    rep["iterations"], rep["flags"], rep["kf_Tcw"], rep["pt_pos"] = tuple(int(i) for i in its), flags, T, X
    edge_p = g["prob_pt"][g["edge_pt"]]
    edge_k = g["prob_kf"][g["edge_kf"]]
    for rnd in (1, 2):
        for e in np.nonzero(flags == rnd)[0]:
            p, k = int(edge_p[e]), int(edge_k[e])
            if map.mp_bad[p]:
                rep["stale_outliers"] += rnd == 1
                continue
            idx = map.obs[p].get(k, -1)  # GetIndexInKeyFrame
            if idx >= 0:
                map.erase_map_point_match(k, idx)
            if map.erase_observation(p, k):
                rep["points_bad"].append(p)
                if rnd == 2:
                    rep["bad_round2"].append(p)
            rep["erased"][rnd - 1] += 1
    for q, (k, kind) in enumerate(zip(g["prob_kf"], g["kf_kind"])):
        if kind != 2:
            map.set_pose(int(k), T[q])
    map.mps["pos"][g["prob_pt"]] = np.asarray(X, np.float32).reshape(-1, 3)
    lap("writeback")
    ids = [int(p) for p in g["prob_pt"]]
    if assembler is None:
        map.update_normal_and_depth_batch(ids, ctx)
    else:
        map.update_normal_and_depth(ids)
    lap("update")
    return rep
