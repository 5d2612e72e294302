"""Local-map assembly: Tracking::UpdateReference (src/Tracking.cc:3689-3852)
over the C-ABI (gf_update_reference / gf_update_reference_dev,
include/gfslam/abi.h "local-map assembly").

A map is given as flat arrays (`CovisGraph`): keyframes in ascending
KeyFrame* order (the order Map::GetAllKeyFrames and the reference's
std::map<KeyFrame*,int> use) with their isBad flags, map-point slots
(mvpMapPoints) and ordered covisibility lists (mvpOrderedConnectedKeyFrames);
map points with isBad and their observing keyframes (mObservations).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, lib, ptr

_P = ctypes.c_void_p


class CovisMap(ctypes.Structure):
    """gf_covis_map."""

    _fields_ = [("nkf", ctypes.c_int32), ("nmp", ctypes.c_int32), ("kf_bad", _P), ("kf_mp_off", _P), ("kf_mp", _P),
                ("kf_cov_off", _P), ("kf_cov", _P), ("mp_bad", _P), ("mp_obs_off", _P), ("mp_obs", _P)]


_ARRAYS = (("kf_bad", np.uint8), ("kf_mp_off", np.int32), ("kf_mp", np.int32), ("kf_cov_off", np.int32),
           ("kf_cov", np.int32), ("mp_bad", np.uint8), ("mp_obs_off", np.int32), ("mp_obs", np.int32))


class CovisGraph:
    """Host arrays of one map (see module docstring)."""

    def __init__(self, **arrays):
        self.a = {k: np.ascontiguousarray(arrays[k], dt) for k, dt in _ARRAYS}
        self.nkf = len(self.a["kf_bad"])
        self.nmp = len(self.a["mp_bad"])
        assert len(self.a["kf_mp_off"]) == self.nkf + 1 and len(self.a["kf_cov_off"]) == self.nkf + 1
        assert len(self.a["mp_obs_off"]) == self.nmp + 1

    def struct(self) -> CovisMap:
        return CovisMap(self.nkf, self.nmp, *[self.a[k].ctypes.data if self.a[k].size else None for k, _ in _ARRAYS])

    def to_device(self, device="cuda") -> "DeviceCovisGraph":
        return DeviceCovisGraph(self, device)


class CovisOut(ctypes.Structure):
    """gf_covis_out."""

    _fields_ = [(k, _P) for k, _ in _ARRAYS]


class MapDeltaStruct(ctypes.Structure):
    """gf_map_delta."""

    _I = ctypes.c_int32
    _fields_ = [("stream", _I), ("n_new_mp", _I), ("new_mp", _P), ("new_mp_desc", _P), ("new_mp_bad", _P),
                ("n_set_mp", _I), ("set_mp_idx", _P), ("set_mp", _P), ("set_mp_desc", _P), ("n_bad_mp", _I),
                ("bad_mp", _P), ("n_new_kf", _I), ("new_kf_off", _P), ("new_kf_mp", _P), ("new_kf_bad", _P),
                ("n_bad_kf", _I), ("bad_kf", _P), ("n_slot", _I), ("slot_kf", _P), ("slot_idx", _P), ("slot_val", _P),
                ("n_obs_rows", _I), ("obs_mp", _P), ("obs_off", _P), ("obs_kf", _P), ("has_cov", _I),
                ("kf_cov_off", _P), ("kf_cov", _P)]


class MapDelta:
    """Host arrays of one stream's map delta (abi.h gf_map_delta), what the
    mapper wrote since the tracker last looked, in the front end's indices:
    new_mp / new_mp_desc / new_mp_bad: appended points; set_mp_idx / set_mp /
    set_mp_desc: rewritten points; bad_mp: points turned bad; new_kf: a list of
    slot rows, new_kf_bad: appended keyframes; bad_kf: keyframes turned bad;
    slot_kf / slot_idx / slot_val: slot writes on existing keyframes; obs_rows:
    {point: ascending observing keyframes}, the whole new row of every touched
    point; kf_cov: a list of the ordered covisible keyframes of every keyframe
    (old and appended), or None when the lists are unchanged; kf_rows: the
    appended keyframes' relocalisation database rows, for a stream whose
    database grows: a pipeline.KeyframeDB of them (offsets from 0) or a list of
    (kps, desc, words, values, FeatureVector), one per appended keyframe; None:
    the delta carries none."""

    def __init__(self, stream: int, new_mp=None, new_mp_desc=None, new_mp_bad=None, set_mp_idx=None, set_mp=None,
                 set_mp_desc=None, bad_mp=None, new_kf=None, new_kf_bad=None, bad_kf=None, slot_kf=None, slot_idx=None,
                 slot_val=None, obs_rows=None, kf_cov=None, kf_rows=None):
        from .matcher import MAP_POINT_DTYPE

        def arr(a, dt, shape=(-1,)):
            return np.ascontiguousarray(np.zeros(0, dt) if a is None else a, dt).reshape(shape)

        self.stream = int(stream)
        self.new_mp = arr(new_mp, MAP_POINT_DTYPE)
        self.new_mp_desc = arr(new_mp_desc, np.uint8, (-1, 32))
        self.new_mp_bad = (np.zeros(len(self.new_mp), np.uint8) if new_mp_bad is None
                           else arr(np.asarray(new_mp_bad).astype(np.uint8), np.uint8))
        self.set_mp_idx = arr(set_mp_idx, np.int32)
        self.set_mp = arr(set_mp, MAP_POINT_DTYPE)
        self.set_mp_desc = arr(set_mp_desc, np.uint8, (-1, 32))
        self.bad_mp, self.bad_kf = arr(bad_mp, np.int32), arr(bad_kf, np.int32)
        rows = [np.asarray(r, np.int32).reshape(-1) for r in (new_kf or [])]
        self.new_kf_off = np.zeros(len(rows) + 1, np.int32)
        self.new_kf_off[1:] = np.cumsum([len(r) for r in rows])
        self.new_kf_mp = arr(np.concatenate(rows) if rows else None, np.int32)
        self.new_kf_bad = (np.zeros(len(rows), np.uint8) if new_kf_bad is None
                           else arr(np.asarray(new_kf_bad).astype(np.uint8), np.uint8))
        self.slot_kf, self.slot_idx, self.slot_val = arr(slot_kf, np.int32), arr(slot_idx, np.int32), arr(slot_val,
                                                                                                             np.int32)
        obs_rows = obs_rows or {}
        pts = list(obs_rows)
        self.obs_mp = arr(pts, np.int32)
        orow = [np.asarray(obs_rows[p], np.int32).reshape(-1) for p in pts]
        self.obs_off = np.zeros(len(pts) + 1, np.int32)
        self.obs_off[1:] = np.cumsum([len(r) for r in orow])
        self.obs_kf = arr(np.concatenate(orow) if orow else None, np.int32)
        self.has_cov = kf_cov is not None
        crow = [np.asarray(c, np.int32).reshape(-1) for c in (kf_cov or [])]
        self.kf_cov_off = np.zeros(len(crow) + 1, np.int32)
        self.kf_cov_off[1:] = np.cumsum([len(c) for c in crow])
        self.kf_cov = arr(np.concatenate(crow) if crow else None, np.int32)
        if kf_rows is not None and not hasattr(kf_rows, "struct"):
            from .pipeline import KeyframeDB

            it = iter([(r[2], r[3], r[4]) for r in kf_rows])
            kf_rows = KeyframeDB([r[0] for r in kf_rows], [r[1] for r in kf_rows], lambda d: next(it))
        self.kf_rows = kf_rows
        if not (len(self.new_mp) == len(self.new_mp_desc) == len(self.new_mp_bad) and
                len(self.set_mp_idx) == len(self.set_mp) == len(self.set_mp_desc) and
                len(self.slot_kf) == len(self.slot_idx) == len(self.slot_val) and len(self.new_kf_bad) == len(rows)):
            raise ValueError("map delta: arrays of one item differ in length")

    def empty(self) -> bool:
        return not (len(self.new_mp) or len(self.set_mp_idx) or len(self.bad_mp) or len(self.bad_kf) or
                    len(self.new_kf_off) > 1 or len(self.slot_kf) or len(self.obs_mp) or self.has_cov)

    def struct(self) -> MapDeltaStruct:
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        return MapDeltaStruct(
            self.stream, len(self.new_mp), p(self.new_mp), p(self.new_mp_desc), p(self.new_mp_bad),
            len(self.set_mp_idx), p(self.set_mp_idx), p(self.set_mp), p(self.set_mp_desc), len(self.bad_mp),
            p(self.bad_mp), len(self.new_kf_off) - 1, self.new_kf_off.ctypes.data, p(self.new_kf_mp),
            p(self.new_kf_bad), len(self.bad_kf), p(self.bad_kf), len(self.slot_kf), p(self.slot_kf), p(self.slot_idx),
            p(self.slot_val), len(self.obs_mp), p(self.obs_mp), self.obs_off.ctypes.data, p(self.obs_kf),
            int(self.has_cov), self.kf_cov_off.ctypes.data, p(self.kf_cov))


class StreamStartStruct(ctypes.Structure):
    """gf_stream_start."""

    _fields_ = [("map", MapDeltaStruct), ("n_last", ctypes.c_int32), ("last_kps", _P), ("last_desc", _P),
                ("last_kp2mp", _P), ("Tcw", ctypes.c_float * 16), ("timestamp", ctypes.c_double),
                ("frame_id", ctypes.c_int32), ("since_reloc", ctypes.c_int32), ("ref_kf", ctypes.c_int32)]


class StreamStart:
    """One stream's beginning (abi.h gf_stream_start): ``map``, a MapDelta
    read against an empty map (appended points and keyframes, observation
    rows, covisibility lists, optionally ``kf_rows``; nothing rewritten, turned
    bad or slot-written), the frame that becomes mLastFrame (undistorted
    ``kps``, ``desc``, ``kp2mp`` into the new map with -1 for NULL, its pose
    ``Tcw``, ``timestamp`` and ``frame_id`` = mnId, ``since_reloc`` = mnId -
    mnLastRelocFrameId) and ``ref_kf``, mpReferenceKF as an index of the new
    graph (None: the newest keyframe, -1 for a map without keyframes)."""

    def __init__(self, map: MapDelta, kps=None, desc=None, kp2mp=None, Tcw=None, timestamp: float = 0.0,
                 frame_id: int = 0, since_reloc: int | None = None, ref_kf: int | None = None):
        from .orb import KEYPOINT_DTYPE

        self.map = map
        self.stream = map.stream
        self.kps = np.ascontiguousarray(np.zeros(0, KEYPOINT_DTYPE) if kps is None else kps, KEYPOINT_DTYPE).reshape(-1)
        self.desc = np.ascontiguousarray(np.zeros((0, 32), np.uint8) if desc is None else desc, np.uint8).reshape(-1, 32)
        self.kp2mp = np.ascontiguousarray(np.full(len(self.kps), -1) if kp2mp is None else kp2mp, np.int32).reshape(-1)
        if not len(self.kps) == len(self.desc) == len(self.kp2mp):
            raise ValueError("stream start: the last frame's arrays differ in length")
        self.Tcw = np.ascontiguousarray(np.eye(4) if Tcw is None else Tcw, np.float32).reshape(16)
        self.timestamp, self.frame_id = float(timestamp), int(frame_id)
        self.since_reloc = self.frame_id if since_reloc is None else int(since_reloc)  # mnLastRelocFrameId = 0
        nkf = len(map.new_kf_off) - 1
        self.ref_kf = nkf - 1 if ref_kf is None else int(ref_kf)

    @property
    def kf_rows(self):
        return self.map.kf_rows

    def struct(self) -> StreamStartStruct:
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        return StreamStartStruct(self.map.struct(), len(self.kps), p(self.kps), p(self.desc), p(self.kp2mp),
                                 (ctypes.c_float * 16)(*self.Tcw.tolist()), self.timestamp, self.frame_id,
                                 self.since_reloc, self.ref_kf)


class MapCompactStruct(ctypes.Structure):
    """gf_map_compact."""

    _fields_ = [("stream", ctypes.c_int32), ("n_drop_kf", ctypes.c_int32), ("drop_kf", _P),
                ("n_drop_mp", ctypes.c_int32), ("drop_mp", _P)]


class MapRemapStruct(ctypes.Structure):
    """gf_map_remap."""

    _fields_ = [("nkf", ctypes.c_int32), ("nmp", ctypes.c_int32), ("kf_remap", _P), ("mp_remap", _P),
                ("n_kept_kf", ctypes.c_int32), ("n_kept_mp", ctypes.c_int32)]


class MapCompact:
    """One stream's compaction request (abi.h gf_map_compact): the graph
    keyframe indices and the map indices that leave the stream's map, each
    list distinct. What frame state still holds stays (see MapRemap)."""

    def __init__(self, stream: int, drop_kf=None, drop_mp=None):
        self.stream = int(stream)
        self.drop_kf = np.ascontiguousarray([] if drop_kf is None else drop_kf, np.int32).reshape(-1)
        self.drop_mp = np.ascontiguousarray([] if drop_mp is None else drop_mp, np.int32).reshape(-1)

    def empty(self) -> bool:
        return not (len(self.drop_kf) or len(self.drop_mp))

    def struct(self) -> MapCompactStruct:
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        return MapCompactStruct(self.stream, len(self.drop_kf), p(self.drop_kf), len(self.drop_mp), p(self.drop_mp))


class MapRemap:
    """What a compaction did to one stream (abi.h gf_map_remap): the counts
    after the call, ``kf_remap`` / ``mp_remap`` (old index -> new index, -1
    dropped) over the old counts, and how many listed keyframes / points were
    pinned by frame state and stayed."""

    def __init__(self, stream: int, nkf: int, nmp: int, kf_remap, mp_remap, n_kept_kf: int = 0, n_kept_mp: int = 0):
        self.stream, self.nkf, self.nmp = int(stream), int(nkf), int(nmp)
        self.kf_remap = np.asarray(kf_remap, np.int32)
        self.mp_remap = np.asarray(mp_remap, np.int32)
        self.n_kept_kf, self.n_kept_mp = int(n_kept_kf), int(n_kept_mp)

    def identity(self) -> bool:
        return self.nkf == len(self.kf_remap) and self.nmp == len(self.mp_remap)

    @staticmethod
    def apply(remap, idx):
        """Indices through a remap table; negative ones stay as they are."""
        idx = np.asarray(idx)
        return np.where(idx >= 0, np.asarray(remap, np.int32)[np.maximum(idx, 0)], idx).astype(np.int32)


class DeviceCovisGraph:
    """The same arrays resident on the device (torch allocations as plumbing)."""

    def __init__(self, g: CovisGraph, device="cuda"):
        import torch

        self.nkf, self.nmp = g.nkf, g.nmp
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v) if v.size else np.zeros(1, v.dtype)).to(device)
                  for k, v in g.a.items()}

    def struct(self) -> CovisMap:
        return CovisMap(self.nkf, self.nmp, *[self.t[k].data_ptr() for k, _ in _ARRAYS])


def update_reference(graph: CovisGraph, frame_mps, ctx=None, kf_cap: int | None = None, mp_cap: int | None = None):
    """Tracking::UpdateReference for one frame. Returns (frame_mps with bad
    map points set to -1, local keyframes, local map points, reference
    keyframe index or -1)."""
    from .matcher import default_context

    ctx = ctx or default_context()
    fm = np.array(frame_mps, np.int32, copy=True)
    kf_cap = graph.nkf if kf_cap is None else kf_cap
    mp_cap = graph.nmp if mp_cap is None else mp_cap
    lk = np.zeros(max(kf_cap, 1), np.int32)
    lm = np.zeros(max(mp_cap, 1), np.int32)
    nk, nm, ref = ctypes.c_int(), ctypes.c_int(), ctypes.c_int32()
    m = graph.struct()
    check(lib().gf_update_reference(ctx.handle, ctypes.byref(m), ptr(fm), len(fm), ptr(lk), ctypes.byref(nk),
                                    kf_cap, ptr(lm), ctypes.byref(nm), mp_cap, ctypes.byref(ref)))
    return fm, lk[:nk.value].copy(), lm[:nm.value].copy(), int(ref.value)


def update_reference_batch(dgraph: DeviceCovisGraph, frame_mps, nkps, ctx=None, kf_cap: int | None = None,
                           mp_cap: int | None = None, stream=None):
    """gf_update_reference_dev over B frames (torch int32 tensors on the
    device: frame_mps [B][stride] updated in place, nkps [B]). Returns device
    tensors (local_kfs [B][kf_cap], n_local_kfs [B], local_mps [B][mp_cap],
    n_local_mps [B], ref_kf [B])."""
    import torch

    from .matcher import default_context

    ctx = ctx or default_context()
    B, stride = frame_mps.shape
    kf_cap = dgraph.nkf if kf_cap is None else kf_cap
    mp_cap = dgraph.nmp if mp_cap is None else mp_cap
    dev = frame_mps.device
    lk = torch.zeros((B, max(kf_cap, 1)), dtype=torch.int32, device=dev)
    lm = torch.zeros((B, max(mp_cap, 1)), dtype=torch.int32, device=dev)
    nk = torch.zeros(B, dtype=torch.int32, device=dev)
    nm = torch.zeros(B, dtype=torch.int32, device=dev)
    ref = torch.zeros(B, dtype=torch.int32, device=dev)
    m = dgraph.struct()
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    check(lib().gf_update_reference_dev(ctx.handle, ctypes.byref(m), B, _P(frame_mps.data_ptr()),
                                        _P(nkps.data_ptr()), stride, _P(lk.data_ptr()), _P(nk.data_ptr()), kf_cap,
                                        _P(lm.data_ptr()), _P(nm.data_ptr()), mp_cap, _P(ref.data_ptr()), _P(s)))
    return lk, nk, lm, nm, ref
