"""Batched tracking front end: the mirror of Tracking::GrabImage for B
independent sequences, over libgfslam's gf_frontend_* (include/gfslam/abi.h).

One `step()` tracks one frame of every stream entirely on the device
(Tracking.cc:461-917, WORKING state): ORB extraction, TrackWithMotionModel
(SearchByProjection(Cur, Last, 15) + PoseOptimization), TrackLocalMap with
the good-feature SearchReferencePointsInFrustum (updatePWLSVec,
FRAME_INFO_MATRIX, then the leftovers-only / SearchByProjection /
runActiveMapMatching branch) + PoseOptimization, the motion-model update,
the next-frame MAP_INFO_MATRIX prediction, SearchAdditionalMatchesInFrame
and the hand-over to mLastFrame. The state of every stream (last frame, pose,
velocity, map-resident observability blocks, std::rand() state) carries over
from step to step, so a stream is a tracked sequence.

PyTorch is not used here: the library owns its buffers and its stream. The
frames come from device memory (`set_source`, e.g. a rendered sequence in a
torch tensor) or from host memory (`step_host`, PCIe copy included).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import synth
from ._lib import check, lib, ptr
from .matcher import MAP_POINT_DTYPE, MP_VIEW_DTYPE
from .observability import Rng
from .orb import KEYPOINT_DTYPE, Context

RELOC_KF_DTYPE = np.dtype([("query", "<u4"), ("words", "<i4"), ("score", "<f4")])  # gf_reloc_kf

# gf_frontend field ids (abi.h GF_FE_*): name -> (id, dtype, per-stream shape
# with "cap" = keypoint capacity and "M" = map capacity)
FIELDS = {
    "kps": (0, KEYPOINT_DTYPE, ("cap",)),
    "desc": (1, np.uint8, ("cap", 32)),
    "nkp": (2, np.int32, ()),
    "Tcw": (3, np.float32, (16,)),
    "kp2mp": (4, np.int32, ("cap",)),
    "score": (5, np.int32, ("cap",)),
    "outlier": (6, np.uint8, ("cap",)),
    "last_kps": (7, KEYPOINT_DTYPE, ("cap",)),
    "last_desc": (8, np.uint8, ("cap", 32)),
    "last_nkp": (9, np.int32, ()),
    "last_kp2mp": (10, np.int32, ("cap",)),
    "last_outlier": (11, np.uint8, ("cap",)),
    "last_pos": (12, np.float32, ("cap", 3)),
    "Tcw_last": (13, np.float32, (16,)),
    "velocity": (14, np.float32, (16,)),
    "t_prev": (15, np.float64, ()),
    "t_cur": (16, np.float64, ()),
    "map": (17, MAP_POINT_DTYPE, ("M",)),
    "map_desc": (18, np.uint8, ("M", 32)),
    "nmp": (19, np.int32, ()),
    "views": (20, MP_VIEW_DTYPE, ("M",)),
    "Xv": (21, np.float64, (13,)),
    "Xv_next": (22, np.float64, (13,)),
    "base": (23, np.float64, (49,)),
    "mp_H": (24, np.float64, ("M", 14)),
    "mp_info": (25, np.float64, ("M", 49)),
    "mp_uv": (26, np.float32, ("M", 2)),
    "mp_upd": (27, np.int32, ("M",)),
    "rng": (28, np.uint8, (ctypes.sizeof(Rng),)),
    "left": (29, np.int32, ("M",)),
    "stats": (30, np.int32, None),  # [NSTAT][B]
    "hist": (31, np.int32, (8,)),  # running counters: steps per branch [0..4], steps cut by a time cap [5],
                                   # log-dets [6], local matches [7]
    "clock": (32, np.int64, ("CK",)),  # budget clock record of the last step (abi.h GF_CK_*)
    "track": (33, np.int32, (8,)),  # tracking state (abi.h GF_TR_*)
    "reloc": (34, RELOC_KF_DTYPE, (64,)),  # keyframes' relocalisation-query state (gf_reloc_kf)
}
STATS = ["m3", "found", "to_match", "branch", "in_view", "local", "inl1", "inl2", "extra", "nleft", "iter1",
         "iter2", "edges1", "edges2", "flags", "frames", "ldets", "nlocal", "ncut", "cand_last", "cand_proj",
         "tpf", "ncand", "reloc", "ransac"]
# GF_FE_TRACK columns and path codes
TR = {"state": 0, "vel": 1, "since": 2, "path": 3, "query": 4, "ok": 5, "force": 6, "force_kf": 7}
PATHS = {0: "motion model", 1: "previous frame after the motion model", 2: "previous frame", 3: "relocalisation",
         4: "none (parked)"}
STATES = {0: "WORKING", 1: "LOST", 2: "NOT_INITIALIZED"}  # GF_TR_STATE; 2: the stream is parked

NSTAT = len(STATS)

# NeedNewKeyFrame / CreateNewKeyFrame state words (abi.h GF_KF_*) and decision bits
KF = {"since": 0, "accept": 1, "stop": 2, "nkf": 3, "abort": 4, "decision": 5, "ref": 6, "ref_matches": 7,
      "inliers": 8, "seq": 9, "pending": 10, "frame": 11}
KF_N = 16
KF_BITS = {"evaluated": 1, "stop": 2, "reloc": 4, "c1a": 8, "c1b": 16, "c2": 32, "created": 64, "interrupt_ba": 128,
           "no_reference": 256}
KEYFRAME_HDR_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("frame_id", "<i4"), ("n", "<i4"),
                               ("timestamp", "<f8"), ("Tcw", "<f4", (16,))])  # gf_keyframe_hdr
assert KEYFRAME_HDR_DTYPE.itemsize == 88


class NewKfArgs(ctypes.Structure):
    """gf_newkf_args (device pointers)."""

    _fields_ = ([("B", ctypes.c_int32), ("cap", ctypes.c_int32)] +
                [(k, ctypes.c_void_p) for k in ("nkp", "kps", "desc", "kp2mp", "Tcw", "t_cur", "track", "inliers",
                                                "working", "ref_kf", "kf_count", "kf_mp_off", "kf_mp")] +
                [("off_stride", ctypes.c_int64), ("slot_stride", ctypes.c_int64)] +
                [(k, ctypes.c_void_p) for k in ("state", "out_hdr", "out_kps", "out_desc", "out_slots")] +
                [("min_frames", ctypes.c_int32), ("max_frames", ctypes.c_int32)])


def need_new_keyframe(since_kf: int, since_reloc: int, stop: bool, nkf: int, n_ref_matches: int, inliers: int,
                      accept: bool, min_frames: int, max_frames: int):
    """gf_need_new_keyframe: Tracking::NeedNewKeyFrame on scalars -> (need, GF_KF_DECISION bits)."""
    need, dec = ctypes.c_int(), ctypes.c_int()
    check(lib().gf_need_new_keyframe(int(since_kf), int(since_reloc), int(bool(stop)), int(nkf), int(n_ref_matches),
                                     int(inliers), int(bool(accept)), int(min_frames), int(max_frames),
                                     ctypes.byref(need), ctypes.byref(dec)))
    return bool(need.value), dec.value

# per-frame stage log (abi.h GF_TL_*, gf_time_rec): device-clock boundaries of a step
TL_SITES = ["begin", "extracted", "motion", "init_pose", "ref_updated", "frustum", "mat_online", "selected",
            "searched", "optimised", "end"]
TL_NSITE = 12
TIME_REC_DTYPE = np.dtype([("frame_time_stamp", np.float64), ("path", np.int32), ("branch", np.int32),
                           ("found", np.int32), ("tpf", np.int32), ("local", np.int32), ("inliers", np.int32),
                           ("extra", np.int32), ("track_map", np.int32), ("flags", np.int32), ("step", np.int32)])
# Tracking::SaveTimeLog's columns (Tracking.h:254-280), in its order
TIME_LOG_COLUMNS = ["frame_time_stamp", "time_ORB_extraction", "time_track_motion", "time_track_frame",
                    "time_track_map", "time_match", "time_select", "time_optim", "time_mat_pred", "time_mat_online",
                    "lmk_num_refTrack", "lmk_num_refInlier", "lmk_num_initTrack", "lmk_num_BA"]
TICK_S = 1e-8  # s_memrealtime: 100 MHz


def time_log_columns(stamps: np.ndarray, recs: np.ndarray) -> dict:
    """logCurrentFrame per step and stream from the device log: stamps
    [n][TL_NSITE] ticks, recs [n][B] TIME_REC_DTYPE -> {column: [n][B]}.
    Where the reference's timers sit (Tracking.cc): extraction :528;
    TrackWithMotionModel / TrackPreviousFrame :605-615 (a motion-model
    failure logs both); TrackLocalMap :672 (UpdateReference through the
    statistics); time_match = UpdateReference + SearchReferencePointsInFrustum
    (:2813); time_optim = PoseOptimization + statistics (:2814);
    time_mat_online = MAP_INFO_MATRIX (:3339); time_select =
    runActiveMapMatching (the GF selection; the reference's TrackLocalMap at
    :2745 leaves it 0, its variants at :2219 / :2705 time the selection
    there); time_mat_pred = from the motion update to the end of the step
    (:791, :913: PWLS prediction, RunMapPointsSelection,
    SearchAdditionalMatchesInFrame). Landmark counts: initTrack = the
    initial estimate's nmatches (:1635 / :1378, :1400), refTrack =
    SearchReferencePointsInFrustum's nMatched + nMatchesFound (:3409, :2808),
    refInlier = mnMatchesInliers, BA = refTrack + the additional matches
    (:3143). A boundary a stage did not reach reads 0."""
    st = stamps.astype(np.float64)
    n, B = recs.shape
    T = {k: st[:, i][:, None] * np.ones((1, B)) for i, k in enumerate(TL_SITES)}

    def dur(a, b):
        return np.where((T[a] > 0) & (T[b] > 0), (T[b] - T[a]) * TICK_S, 0.0)

    path, br, tm = recs["path"], recs["branch"], recs["track_map"] != 0
    motion = (path == 0) | (path == 1)
    prev = (path == 1) | (path == 2)
    out = {"frame_time_stamp": recs["frame_time_stamp"].copy(),
           "time_ORB_extraction": dur("begin", "extracted"),
           "time_track_motion": np.where(motion, dur("extracted", "motion"), 0.0),
           "time_track_frame": np.where(prev, dur("motion", "init_pose"), 0.0),
           "time_track_map": np.where(tm, dur("init_pose", "optimised"), 0.0),
           "time_match": np.where(tm, dur("init_pose", "searched"), 0.0),
           "time_select": np.where(tm & (br == 3), dur("mat_online", "selected"), 0.0),
           "time_optim": np.where(tm, dur("searched", "optimised"), 0.0),
           "time_mat_pred": dur("optimised", "end"),
           "time_mat_online": np.where(tm & (br == 3), dur("frustum", "mat_online"), 0.0)}
    ref = np.where(tm, recs["found"] + recs["local"], 0)
    out["lmk_num_refTrack"] = ref
    out["lmk_num_refInlier"] = np.where(tm, recs["inliers"], 0)
    out["lmk_num_initTrack"] = np.where(path == 0, recs["found"], np.where(prev, recs["tpf"], 0))
    out["lmk_num_BA"] = np.where(tm, ref + recs["extra"], 0)
    return out


# GF_FE_CLOCK layout (abi.h GF_CK_*): header words, then per-stage elapsed-time
# arrays; M = map capacity, R = max(gf_budget, 1)
CK = {"flags": 0, "match": 1, "select": 2, "viz_cut": 3, "viz_time": 4, "mat_online": 5, "am_cut": 6, "sofar": 7,
      "sa_cut": 8, "sa_sofar": 9, "budget_cut": 10}
CK_HEADER = 16
# test-clock sites (abi.h GF_CK_SITE_*)
CK_SITES = ["viz", "mi", "am_start", "am_round", "sofar", "sel", "sa", "sa_sofar", "bud"]


def ck_offsets(M: int, R: int) -> dict:
    """Offsets of the clock record's arrays: isInFrustum points, MAP_INFO
    batches (active branch), active-matching rounds, MAP_INFO batches
    (kinematic[1]), visibility-pass points, SearchByProjection_Budget points."""
    return {"viz": CK_HEADER, "mi": CK_HEADER + M, "am": CK_HEADER + M + 64, "sel": CK_HEADER + M + 64 + R,
            "sa": CK_HEADER + M + 128 + R, "bud": CK_HEADER + 2 * M + 128 + R, "words": CK_HEADER + 3 * M + 128 + R}


class FrontendParams(ctypes.Structure):
    """gf_frontend_params."""

    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fx", ctypes.c_float),
                ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("nfeatures", ctypes.c_int32), ("scale_factor", ctypes.c_float), ("nlevels", ctypes.c_int32),
                ("fast_th", ctypes.c_int32), ("batch", ctypes.c_int32), ("map_cap", ctypes.c_int32),
                ("gf_budget", ctypes.c_int32), ("gf", ctypes.c_int32), ("dt", ctypes.c_double),
                ("dist", ctypes.c_float * 5), ("max_frames", ctypes.c_int32), ("harris_score", ctypes.c_int32)]

    @classmethod
    def make(cls, camera: str, nfeatures: int, batch: int, map_cap: int, gf_budget: int, gf: bool = True,
             fps: float = 20.0, nlevels: int = 8, scale_factor: float = 1.2, fast_th: int = 20, dist=None,
             score_type: int = 1):
        """dist: Camera.k1 k2 p1 p2 [k3] (None / k1 = 0: keypoints used as extracted);
        score_type: ORBextractor.nScoreType (1 FAST_SCORE, 0 HARRIS_SCORE)."""
        w, h, fx, fy, cx, cy = synth.CAMERAS[camera]
        d = list(dist or ()) + [0.0] * (5 - len(dist or ()))
        # mMaxFrames = 18 * camera_fps / 30 (Tracking.cc:153; int of a double)
        return cls(w, h, fx, fy, cx, cy, nfeatures, scale_factor, nlevels, fast_th, batch, map_cap, gf_budget,
                   1 if gf else 0, 1.0 / fps, (ctypes.c_float * 5)(*d), int(18 * fps / 30),
                   1 if score_type == 0 else 0)


def field_shape(name: str, B: int, cap: int, M: int, R: int = 1):
    fid, dt, shp = FIELDS[name]
    if shp is None:
        return fid, dt, (NSTAT, B)
    dims = {"cap": cap, "M": M, "CK": ck_offsets(M, R)["words"]}
    return fid, dt, (B,) + tuple(dims.get(s, s) for s in shp)


class GateEvent:
    """A hipEvent_t for gf_frontend_set_gate (gf_event_create)."""

    def __init__(self, ctx: Context):
        h = ctypes.c_void_p()
        check(lib().gf_event_create(ctx.handle, ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            lib().gf_event_destroy(self.handle)
        except Exception:
            pass


def step_all(fes: list) -> None:
    """One step of every front end, from one host thread: every extraction
    is enqueued before any tracking, so a gated front end's extraction is
    never queued behind the host's launches of another's tracking."""
    for fe in fes:
        fe.step_extract()
    for fe in fes:
        fe.step_track()


class GatedRing:
    """Steps gated front ends (chain_extraction) from one host thread in the
    launch order that keeps the gate's hand-over short: front end g's
    extraction is enqueued right after g - 1's, before g - 1's tracking, and
    the last front end's tracking is held until the next step's first
    extraction is enqueued (call finish() before reading results)."""

    def __init__(self, fes: list):
        self.fes = list(fes)
        self._held = None  # the front end whose tracking is not enqueued yet

    def step(self) -> None:
        prev = self._held
        for fe in self.fes:
            if prev is fe:  # one front end: its frame is tracked before the next is extracted
                prev.step_track()
                prev = None
            fe.step_extract()
            if prev is not None:
                prev.step_track()
            prev = fe
        self._held = prev

    def finish(self) -> None:
        if self._held is not None:
            self._held.step_track()
            self._held = None


def chain_extraction(fes: list) -> list:
    """Gate the front ends' extraction stages into a ring: front end g waits
    for g - 1's extraction (g = 0 for the last one's, previous step), so the
    bandwidth-bound stages run one at a time and each front end's tracking
    overlaps the next one's extraction. Returns the events."""
    if len(fes) < 2:
        return []
    evs = [GateEvent(fe.ctx) for fe in fes]
    for g, fe in enumerate(fes):
        fe.set_gate(evs[g - 1], evs[g])
    return evs


class FrontEnd:
    """B independent streams, one frame each per step."""

    def __init__(self, camera: str = "euroc", nfeatures: int = 1000, batch: int = 1, map_size: int = 2000,
                 gf_budget: int = 100, gf: bool = True, fps: float = 20.0, ctx: Context | None = None, dist=None,
                 score_type: int = 1):
        self.params = FrontendParams.make(camera, nfeatures, batch, map_size, gf_budget, gf, fps, dist=dist,
                                          score_type=score_type)
        self.cam = synth.CAMERAS[camera]
        self.B, self.M = batch, map_size
        self.R = max(gf_budget, 1)
        if ctx is None:
            import torch

            ctx = Context(torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(lib().gf_frontend_create(ctx.handle, ctypes.byref(self.params), ctypes.byref(h)))
        self.handle = h
        c = ctypes.c_int()
        check(lib().gf_frontend_capacity(h, ctypes.byref(c)))
        self.cap = c.value
        self._keep = None

    def close(self) -> None:
        if self.handle:
            check(lib().gf_frontend_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ set-up
    def set_source(self, frames, scene_of: np.ndarray, phase: np.ndarray) -> None:
        """frames: device tensor [S][period][H][W] u8 (kept alive here);
        stream b reads scene scene_of[b] starting at phase[b]."""
        S, period, H, W = frames.shape
        assert (W, H) == tuple(self.cam[:2]) and frames.is_contiguous()
        self._keep = frames
        base = frames.data_ptr()
        fb = H * W
        bases = (ctypes.c_void_p * self.B)(*[base + int(s) * period * fb for s in scene_of])
        ph = np.ascontiguousarray(phase, np.int32)
        check(lib().gf_frontend_set_source(self.handle, bases, ptr(ph), period, fb))

    def set_map(self, stream: int, mps: np.ndarray, desc: np.ndarray) -> None:
        mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        check(lib().gf_frontend_set_map(self.handle, stream, ptr(mps), ptr(desc), len(mps)))

    def set_covis(self, stream: int, graph) -> None:
        """gf_frontend_set_covis: the keyframe graph of the stream's map
        (localmap.CovisGraph or the dict scene.build_global_map returns)."""
        from .localmap import CovisGraph

        g = graph if isinstance(graph, CovisGraph) else CovisGraph(**graph)
        self._graphs = getattr(self, "_graphs", {})
        self._graphs[stream] = g
        check(lib().gf_frontend_set_covis(self.handle, stream, ctypes.byref(g.struct())))
        getattr(self, "_kfdbs", {}).pop(stream, None)  # a database set earlier indexed the old graph: detached

    def update_maps(self, deltas) -> None:
        """gf_frontend_update_maps: apply the mapper's changes (a
        localmap.MapDelta or a list of them, one per stream at most) to the
        stream maps and keyframe graphs in place (and, for the deltas that
        carry ``kf_rows``, the appended keyframes to the stream's growable
        KeyframeDB, whose host arrays follow), behind the last step, without
        a host synchronisation; legal after capture_graph(). A refused delta
        (GFError) leaves every stream of the call untouched."""
        from .localmap import MapDelta, MapDeltaStruct

        ds = [deltas] if isinstance(deltas, MapDelta) else list(deltas)
        if not ds:
            return
        arr = (MapDeltaStruct * len(ds))(*[d.struct() for d in ds])
        if all(d.kf_rows is None for d in ds):
            check(lib().gf_frontend_update_maps(self.handle, len(ds), arr))
            return
        # the appended keyframes' database rows travel with their deltas (gf_frontend_update_maps_kfdb)
        rows = [d.kf_rows.struct() if d.kf_rows is not None else None for d in ds]
        ptrs = (ctypes.c_void_p * len(ds))(*[ctypes.addressof(r) if r is not None else None for r in rows])
        check(lib().gf_frontend_update_maps_kfdb(self.handle, len(ds), arr, ptrs))
        for d in ds:  # the host arrays follow the device
            db = getattr(self, "_kfdbs", {}).get(d.stream)
            if d.kf_rows is not None and db is not None:
                db.extend(d.kf_rows)

    def compact_maps(self, requests) -> list:
        """gf_frontend_compact_maps: drop keyframes and points from the stream
        maps and keyframe graphs in place (a localmap.MapCompact or a list of
        them, one per stream at most), renumbering every index the front end
        holds. Items frame state still holds are pinned and stay. Behind the
        last step, legal after capture_graph(); synchronises once. -> one
        localmap.MapRemap per request. A refused request (GFError) leaves
        every stream of the call untouched."""
        from .localmap import MapCompact, MapCompactStruct, MapRemap, MapRemapStruct

        rs = [requests] if isinstance(requests, MapCompact) else list(requests)
        if not rs:
            return []
        arr = (MapCompactStruct * len(rs))(*[r.struct() for r in rs])
        kf = [np.full(64, -1, np.int32) for _ in rs]
        mp = [np.full(max(self.M, 1), -1, np.int32) for _ in rs]
        out = (MapRemapStruct * len(rs))(*[MapRemapStruct(0, 0, k.ctypes.data, m.ctypes.data, 0, 0)
                                           for k, m in zip(kf, mp)])
        old = []  # the counts before the call: the lengths of the remap tables
        for r in rs:
            counts = np.zeros(5, np.int32)
            rc = lib().gf_frontend_get_covis(self.handle, r.stream, ptr(counts), None, None)
            old.append((int(counts[0]), int(counts[1])) if rc == 0 else (0, 0))  # refused below with its reason
        check(lib().gf_frontend_compact_maps(self.handle, len(rs), arr, out))
        for i, r in enumerate(rs):  # a growable database's host arrays follow the device (KeyFrameDatabase::erase)
            db = getattr(self, "_kfdbs", {}).get(r.stream)
            if db is not None and db.growable and out[i].nkf < old[i][0]:
                db.erase(kf[i][:old[i][0]])
        return [MapRemap(r.stream, o.nkf, o.nmp, kf[i][:old[i][0]].copy(), mp[i][:old[i][1]].copy(), o.n_kept_kf,
                         o.n_kept_mp) for i, (r, o) in enumerate(zip(rs, out))]

    def enable_lifecycle(self, on: bool = True) -> None:
        """gf_frontend_set_lifecycle: the reset rule of Tracking::GrabImage
        (Tracking.cc:718-726) as part of every following step's verdict: a
        stream that is LOST on a map of at most 5 keyframes is parked (state
        2, NOT_INITIALIZED) until ``start_streams`` starts it again. Also
        gives every stream without a map an empty keyframe graph in state 2,
        so that a front end can begin empty. Before capture_graph()."""
        check(lib().gf_frontend_set_lifecycle(self.handle, int(on)))

    def lifecycle(self) -> np.ndarray:
        """gf_frontend_lifecycle_read: GF_TR_STATE of every stream ([B] i32:
        0 WORKING, 1 LOST, 2 NOT_INITIALIZED / parked); synchronises."""
        st = np.zeros(self.B, np.int32)
        check(lib().gf_frontend_lifecycle_read(self.handle, ptr(st)))
        return st

    def start_streams(self, requests) -> None:
        """gf_frontend_start_streams: one stream's beginning on the device (a
        localmap.StreamStart or a list of them, one per stream at most): the
        stream then holds the request's map alone, its frame as mLastFrame,
        fresh tracking and keyframe words and, with a growable KeyframeDB
        attached, a database emptied and refilled with the request's
        ``kf_rows`` (the host arrays follow). Behind the last step, without a
        host synchronisation; legal after capture_graph(). A refused request
        (GFError) leaves every stream of the call untouched."""
        from .localmap import StreamStart, StreamStartStruct

        rs = [requests] if isinstance(requests, StreamStart) else list(requests)
        if not rs:
            return
        arr = (StreamStartStruct * len(rs))(*[r.struct() for r in rs])
        rows = [r.kf_rows.struct() if r.kf_rows is not None else None for r in rs]
        ptrs = None
        if any(r is not None for r in rows):
            ptrs = (ctypes.c_void_p * len(rs))(*[ctypes.addressof(r) if r is not None else None for r in rows])
        check(lib().gf_frontend_start_streams(self.handle, len(rs), arr, ptrs))
        for r in rs:  # the host arrays follow the device: KeyFrameDatabase::clear, then the rows
            db = getattr(self, "_kfdbs", {}).get(r.stream)
            if db is not None and db.growable:
                db.clear()
                if r.kf_rows is not None:
                    db.extend(r.kf_rows)

    def force_relocalisation(self, streams, last_kf=None) -> None:
        """gf_frontend_force_relocalisation (Tracking::ForceRelocalisation,
        Tracking.cc:4035-4045): the next step of each stream in ``streams``
        (an index or a list, each at most once) relocalises although the
        stream is WORKING, against the local window around ``last_kf`` (graph
        keyframe indices, one per stream; None or -1: the stream's newest
        keyframe that is not bad): the first 9 entries of its covisibility row,
        then the keyframe. Behind the last step, without a host
        synchronisation; legal after capture_graph(). A refused request
        (GFError) writes nothing."""
        ss = np.atleast_1d(np.asarray(streams, np.int32)).copy()
        if not len(ss):
            return
        kf = None
        if last_kf is not None:
            kf = np.atleast_1d(np.asarray(last_kf, np.int32)).copy()
            if len(kf) != len(ss):
                raise ValueError("one last_kf per stream")
        check(lib().gf_frontend_force_relocalisation(self.handle, len(ss), ptr(ss), ptr(kf) if kf is not None else None))

    def reloc_candidates(self) -> list:
        """gf_frontend_reloc_candidates_read: per stream, the relocalisation
        candidates (graph keyframe indices, in the order they were tried) of
        the last step; empty for a stream that did not relocalise.
        Synchronises."""
        c = np.zeros((self.B, 64), np.int32)
        n = np.zeros(self.B, np.int32)
        check(lib().gf_frontend_reloc_candidates_read(self.handle, ptr(c), ptr(n)))
        return [c[b, :max(int(n[b]), 0)].copy() for b in range(self.B)]

    def covis(self, stream: int) -> dict:
        """gf_frontend_get_covis: the keyframe graph the front end holds for
        the stream, as the dict of arrays set_covis takes."""
        from .localmap import _ARRAYS, CovisOut

        counts = np.zeros(5, np.int32)
        check(lib().gf_frontend_get_covis(self.handle, stream, ptr(counts), None, None))
        nkf, nmp, ns, nc, no = (int(c) for c in counts)
        size = dict(kf_bad=nkf, kf_mp_off=nkf + 1, kf_mp=ns, kf_cov_off=nkf + 1, kf_cov=nc, mp_bad=nmp,
                    mp_obs_off=nmp + 1, mp_obs=no)
        buf = {k: np.zeros(max(size[k], 1), dt) for k, dt in _ARRAYS}
        out = CovisOut(*[buf[k].ctypes.data for k, _ in _ARRAYS])
        caps = np.array([max(ns, 1), max(nc, 1), max(no, 1)], np.int32)
        check(lib().gf_frontend_get_covis(self.handle, stream, ptr(counts), ctypes.byref(out), ptr(caps)))
        return {k: buf[k][:size[k]].copy() for k, _ in _ARRAYS}

    def set_rng(self, stream: int, seed: int) -> None:
        check(lib().gf_frontend_set_rng(self.handle, stream, ctypes.c_uint32(seed)))

    def set_vocab(self, vocab) -> None:
        """gf_frontend_set_vocab: Frame::ComputeBoW's vocabulary for
        relocalisation (a bow.ORBVocabulary, kept alive here)."""
        self._vocab = vocab
        check(lib().gf_frontend_set_vocab(self.handle, vocab.handle if vocab is not None else None))

    def set_kfdb(self, stream: int, db) -> None:
        """gf_frontend_set_kfdb: the stream's keyframe database (a
        KeyframeDB over the same keyframes as its graph; None detaches)."""
        self._kfdbs = getattr(self, "_kfdbs", {})
        check(lib().gf_frontend_set_kfdb(self.handle, stream, db.device(self.ctx) if db is not None else None))
        self._kfdbs[stream] = db

    def bootstrap(self, Tcw: np.ndarray, V: np.ndarray, t0: float = 0.0) -> None:
        T = np.ascontiguousarray(Tcw, np.float32).reshape(self.B, 16)
        Vv = np.ascontiguousarray(V, np.float32).reshape(self.B, 16)
        check(lib().gf_frontend_bootstrap(self.handle, ptr(T), ptr(Vv), ctypes.c_double(t0)))

    # ------------------------------------------------------------ steps
    def step(self) -> None:
        check(lib().gf_frontend_step(self.handle))

    def step_extract(self) -> None:
        """gf_frontend_step_extract: the step's extraction gate and Frame
        construction only (step_track completes the step)."""
        check(lib().gf_frontend_step_extract(self.handle))

    def step_track(self) -> None:
        check(lib().gf_frontend_step_track(self.handle))

    def step_host(self, imgs: np.ndarray) -> None:
        imgs = np.ascontiguousarray(imgs, np.uint8)
        assert imgs.shape == (self.B, self.cam[1], self.cam[0])
        check(lib().gf_frontend_step_host(self.handle, ptr(imgs)))
        self._host_keep = imgs

    def capture_graph(self) -> None:
        check(lib().gf_frontend_capture(self.handle))

    def set_gate(self, wait_event, done_event) -> None:
        """gf_frontend_set_gate: wait for `wait_event` before extraction,
        record `done_event` after it (GateEvent or None)."""
        self._gate = (wait_event, done_event)  # keep the events alive
        check(lib().gf_frontend_set_gate(self.handle, wait_event.handle if wait_event else None,
                                         done_event.handle if done_event else None))

    def set_gate_stage(self, stage: int) -> None:
        """gf_frontend_set_gate_stage: record the gate's done event after
        extraction stage `stage` (0 resize .. 4 describe, the default)."""
        check(lib().gf_frontend_set_gate_stage(self.handle, int(stage)))

    def set_track_priority(self, priority: int = -1) -> None:
        """gf_frontend_set_track_priority: tracking kernels on a stream of HIP
        priority `priority` (lower = more urgent)."""
        check(lib().gf_frontend_set_track_priority(self.handle, priority))

    def sync(self) -> None:
        check(lib().gf_frontend_sync(self.handle))

    def set_budgets(self, match_s: float = float("inf"), select_s: float = float("inf")) -> None:
        check(lib().gf_set_budgets(self.ctx.handle, ctypes.c_double(match_s), ctypes.c_double(select_s)))

    def set_test_clock(self, sites: dict | None) -> None:
        """gf_frontend_set_test_clock (test-only): each budget check at site s
        reads base + idx * slope ticks, sites = {name: (base, slope)} over
        CK_SITES (absent sites read (0, 0)); None restores the device clock."""
        if sites is None:
            check(lib().gf_frontend_set_test_clock(self.handle, None))
            return
        bad = set(sites) - set(CK_SITES)
        if bad:
            raise ValueError(f"unknown clock sites {sorted(bad)}")
        a = np.zeros((len(CK_SITES), 2), np.int64)
        for name, (base, slope) in sites.items():
            a[CK_SITES.index(name)] = (base, slope)
        check(lib().gf_frontend_set_test_clock(self.handle, ptr(a)))

    def set_time_log(self, steps: int) -> None:
        """gf_frontend_set_time_log: keep the last `steps` steps' stage log (0: off)."""
        check(lib().gf_frontend_set_time_log(self.handle, int(steps)))

    def time_log(self) -> dict:
        """The logged steps, oldest first: {"stamps": [n][TL_NSITE] ticks,
        "recs": [n][B] TIME_REC_DTYPE, column: [n][B] for TIME_LOG_COLUMNS}."""
        cap = 4096
        st = np.zeros((cap, TL_NSITE), np.int64)
        rc = np.zeros((cap, self.B), TIME_REC_DTYPE)
        n = ctypes.c_int()
        check(lib().gf_frontend_read_time_log(self.handle, ptr(st), ptr(rc), ctypes.byref(n)))
        st, rc = st[:n.value], rc[:n.value]
        return {"stamps": st, "recs": rc, **time_log_columns(st, rc)}

    def save_time_log(self, filename: str, stream: int = 0) -> None:
        """Tracking::SaveTimeLog's file for one stream (Tracking.h:251-277)."""
        log = self.time_log()
        with open(filename, "w") as fh:
            fh.write("#frame_time_stamp time_ORB_extraction time_track_motion time_track_frame time_track_map "
                     "time_match ...\n")
            for k in range(len(log["recs"])):
                f = [f"{log[c][k, stream]:.6f}" for c in TIME_LOG_COLUMNS[:10]]
                f += [f"{int(log[c][k, stream]):d}" for c in TIME_LOG_COLUMNS[10:]]
                fh.write(" ".join(f) + "\n")

    # ------------------------------------------------------------ state
    def read(self, name: str) -> np.ndarray:
        fid, dt, shape = field_shape(name, self.B, self.cap, self.M, self.R)
        out = np.zeros(shape, dt)
        check(lib().gf_frontend_read(self.handle, fid, ptr(out), out.nbytes))
        return out

    def write(self, name: str, arr: np.ndarray) -> None:
        fid, dt, shape = field_shape(name, self.B, self.cap, self.M, self.R)
        a = np.ascontiguousarray(arr, dt).reshape(shape)
        check(lib().gf_frontend_write(self.handle, fid, ptr(a), a.nbytes))

    def stats(self) -> dict:
        s = self.read("stats")
        return {k: s[i] for i, k in enumerate(STATS)}

    # ------------------------------------------------------------ keyframes
    def enable_keyframes(self, min_frames: int = 0, max_frames: int | None = None, on: bool = True) -> None:
        """gf_frontend_set_keyframes: `if(NeedNewKeyFrame()) CreateNewKeyFrame();`
        (Tracking.cc:896-897) as a stage of every following step. min_frames =
        mMinFrames (0, :151), max_frames None = the front end's mMaxFrames.
        Needs a keyframe graph on every stream; before capture_graph()."""
        check(lib().gf_frontend_set_keyframes(self.handle, int(on), int(min_frames), int(max_frames or 0)))

    def keyframe_state(self) -> dict:
        """The GF_KF_* words: {name: [B] i32} over KF."""
        st = np.zeros((self.B, KF_N), np.int32)
        check(lib().gf_frontend_keyframe_state_read(self.handle, ptr(st), st.nbytes))
        return {k: st[:, i].copy() for k, i in KF.items()}

    def set_keyframe_state(self, stream: int | None = None, **words) -> None:
        """Write state words (names of KF) on one stream or, stream None, on all
        (a scalar or a [B] array each); the others keep their values. ACCEPT on
        a stream whose keyframe is pending is refused."""
        bad = set(words) - set(KF)
        if bad:
            raise ValueError(f"unknown keyframe state words {sorted(bad)}")
        st = np.zeros((self.B, KF_N), np.int32)
        check(lib().gf_frontend_keyframe_state_read(self.handle, ptr(st), st.nbytes))
        for k, v in words.items():
            if stream is None:
                st[:, KF[k]] = np.asarray(v, np.int32)
            else:
                st[stream, KF[k]] = int(v)
        check(lib().gf_frontend_keyframe_state_write(self.handle, ptr(st), st.nbytes))

    def take_keyframes(self, max_kf: int | None = None) -> list:
        """gf_frontend_take_keyframes: the pending keyframes (lowest streams
        first, at most max_kf), their PENDING cleared -> a list of
        dict(stream, seq, frame_id, timestamp, Tcw [4][4], kps, desc, slots);
        slots are map indices with the outliers still in place."""
        k = self.B if max_kf is None else max(0, min(int(max_kf), self.B))
        rows = k * self.cap
        hdr = np.zeros(max(k, 1), KEYFRAME_HDR_DTYPE)
        kps = np.zeros(max(rows, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(rows, 1), 32), np.uint8)
        slots = np.zeros(max(rows, 1), np.int32)
        nkf, nrows = ctypes.c_int(), ctypes.c_int()
        check(lib().gf_frontend_take_keyframes(self.handle, k, rows, ptr(hdr), ptr(kps), ptr(desc), ptr(slots),
                                               ctypes.byref(nkf), ctypes.byref(nrows)))
        out, r = [], 0
        for h in hdr[:nkf.value]:
            n = int(h["n"])
            out.append(dict(stream=int(h["stream"]), seq=int(h["seq"]), frame_id=int(h["frame_id"]),
                            timestamp=float(h["timestamp"]), Tcw=h["Tcw"].reshape(4, 4).copy(),
                            kps=kps[r:r + n].copy(), desc=desc[r:r + n].copy(), slots=slots[r:r + n].copy()))
            r += n
        return out

    def keyframes_dev(self) -> dict:
        """gf_frontend_keyframes_dev: device addresses of the state and the outbox."""
        p = [ctypes.c_void_p() for _ in range(5)]
        check(lib().gf_frontend_keyframes_dev(self.handle, *[ctypes.byref(x) for x in p]))
        return dict(zip(("state", "hdr", "kps", "desc", "slots"), (x.value for x in p)))

    # ------------------------------------------------------------ profiling
    def prof_enable(self, on: bool = True) -> None:
        check(lib().gf_prof_enable(self.ctx.handle, int(on)))

    def prof_reset(self) -> None:
        check(lib().gf_prof_reset(self.ctx.handle))

    def prof_report(self) -> dict:
        out = {}
        i = 0
        name = ctypes.create_string_buffer(64)
        while True:
            ms, cnt = ctypes.c_double(), ctypes.c_int()
            rc = lib().gf_prof_report(self.ctx.handle, i, name, 64, ctypes.byref(ms), ctypes.byref(cnt))
            if rc != 0:
                break
            out[name.value.decode()] = (ms.value, cnt.value)
            i += 1
        return out


def make_workload_frontend(camera: str, nfeatures: int, batch: int, map_size: int, gf_budget: int, workload,
                           frames, maps, seed: int = 0, ctx: Context | None = None) -> FrontEnd:
    """A FrontEnd over a scene.Workload: per-stream maps (of its scene),
    std::srand(1 + seed * 1000 + b), the source frames and the bootstrap at
    the ground-truth pose."""
    fe = FrontEnd(camera, nfeatures, batch, map_size, gf_budget, ctx=ctx)
    for b in range(batch):
        mp, d = maps[workload.scene_of[b]]
        fe.set_map(b, mp, d)
        fe.set_rng(b, 1 + seed * 1000 + b)
    fe.set_source(frames, workload.scene_of, workload.phase)
    T, V = workload.boot_state()
    fe.bootstrap(T, V, 0.0)
    return fe


class KeyframeDBArrays(ctypes.Structure):
    """gf_keyframe_db."""

    _fields_ = [("nkf", ctypes.c_int32)] + [(k, ctypes.c_void_p) for k in
                                           ("kp_off", "kps", "desc", "bow_off", "bow_words", "bow_values", "fv_off",
                                            "fv_nodes", "fv_start", "fv_feats")]


class KeyframeDB:
    """The keyframes of a map as Relocalisation reads them (abi.h
    gf_keyframe_db): per keyframe its keypoints, descriptors, BowVector and
    FeatureVector (KeyFrame::ComputeBoW, levelsup 4). `transform(desc)` gives
    (words, values, FeatureVector) — the library's ORBVocabulary.transform on
    the device, or a CPU restatement in the oracle tests.

    With ``max_kf`` and ``max_rows`` the device database grows
    (gf_kfdb_create_growable: room for max_kf keyframes and max_rows keypoints
    in total): ``append`` adds a keyframe, and a ``FrontEnd`` it is attached to
    adds the keyframes of the map deltas that carry their rows. It then belongs
    to that one stream. Without them it is fixed and can be shared."""

    _ARRAYS = ("kp_off", "kps", "desc", "bow_off", "bow_words", "bow_values", "fv_off", "fv_nodes", "fv_start",
               "fv_feats")

    def __init__(self, kf_kps: list, kf_desc: list, transform, max_kf=None, max_rows=None):
        from .orb import KEYPOINT_DTYPE

        if (max_kf is None) != (max_rows is None):
            raise ValueError("a growable database needs both max_kf and max_rows")
        self.max_kf, self.max_rows = max_kf, max_rows
        self.nkf = len(kf_kps)
        kps = [np.ascontiguousarray(k, KEYPOINT_DTYPE) for k in kf_kps]
        desc = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in kf_desc]
        self.kp_off = np.zeros(self.nkf + 1, np.int32)
        self.kp_off[1:] = np.cumsum([len(k) for k in kps])
        self.kps = np.concatenate(kps) if kps else np.zeros(0, KEYPOINT_DTYPE)
        self.desc = np.ascontiguousarray(np.concatenate(desc) if desc else np.zeros((0, 32), np.uint8))
        bw, bv, fn, fs, ff = [], [], [], [0], []
        self.bow_off = np.zeros(self.nkf + 1, np.int32)
        self.fv_off = np.zeros(self.nkf + 1, np.int32)
        for k, d in enumerate(desc):
            w, v, fv = transform(d)
            bw.append(np.asarray(w, np.int32))
            bv.append(np.asarray(v, np.float64))
            self.bow_off[k + 1] = self.bow_off[k] + len(w)
            fn.append(np.asarray(fv.nodes, np.int32))
            base = fs[-1]
            fs.extend((base + np.asarray(fv.start[1:], np.int64)).tolist())
            ff.append(np.asarray(fv.feats, np.int32))
            self.fv_off[k + 1] = self.fv_off[k] + len(fv.nodes)
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0, dt), dt)
        self.bow_words, self.bow_values = cat(bw, np.int32), cat(bv, np.float64)
        self.fv_nodes, self.fv_feats = cat(fn, np.int32), cat(ff, np.int32)
        self.fv_start = np.ascontiguousarray(fs, np.int32)
        self._dev = {}
        self._buf = None
        if self.growable:
            self.reserve()

    @property
    def growable(self) -> bool:
        return self.max_kf is not None

    def reserve(self) -> None:
        """Host arrays of a growable database at its capacities (the arrays
        become views of them), so that ``extend`` costs the new rows only."""
        K, R = int(self.max_kf), int(self.max_rows)
        cap = dict(kp_off=K + 1, kps=R, desc=R, bow_off=K + 1, bow_words=R, bow_values=R, fv_off=K + 1, fv_nodes=R,
                   fv_start=R + 1, fv_feats=R)
        self._buf = {}
        for k, n in cap.items():
            a = getattr(self, k)
            b = np.zeros((max(n, len(a)),) + a.shape[1:], a.dtype)
            b[:len(a)] = a
            self._buf[k] = b
            setattr(self, k, b[:len(a)])

    @classmethod
    def rows(cls, kps, desc, words, values, fv) -> "KeyframeDB":
        """One keyframe's rows (offsets from 0), as ``append`` and a
        ``MapDelta`` carry them."""
        return cls([kps], [desc], lambda d: (words, values, fv))

    def struct(self) -> KeyframeDBArrays:
        a = [getattr(self, k) for k in self._ARRAYS]
        return KeyframeDBArrays(self.nkf, *[x.ctypes.data if x.size else None for x in a])

    def device(self, ctx):
        """The gf_kfdb handle on ctx (created once; a fixed one is shared by
        the streams)."""
        key = id(ctx)
        if key not in self._dev:
            h = ctypes.c_void_p()
            if self.growable:
                if self._dev:
                    raise ValueError("a growable database lives on one context")
                check(lib().gf_kfdb_create_growable(ctx.handle, ctypes.byref(self.struct()), self.max_kf,
                                                    self.max_rows, ctypes.byref(h)))
            else:
                check(lib().gf_kfdb_create(ctx.handle, ctypes.byref(self.struct()), ctypes.byref(h)))
            self._dev[key] = (ctx, h)  # the context outlives the handle
        return self._dev[key][1]

    def extend(self, rows: "KeyframeDB") -> None:
        """The host arrays with the keyframes of ``rows`` behind them (what the
        device holds after a successful append)."""
        base = dict(kp_off=self.kp_off[-1], bow_off=self.bow_off[-1], fv_off=self.fv_off[-1], fv_start=self.fv_start[-1])
        for k in self._ARRAYS:
            cur, new = getattr(self, k), getattr(rows, k)
            new = new[1:] + base[k] if k in base else new
            n0, n1 = len(cur), len(cur) + len(new)
            if self._buf is not None and n1 <= len(self._buf[k]):  # in place, behind the used part
                self._buf[k][n0:n1] = new
                setattr(self, k, self._buf[k][:n1])
            else:
                self._buf = None
                setattr(self, k, np.ascontiguousarray(np.concatenate([cur, new]), cur.dtype))
        self.nkf += rows.nkf

    def clear(self) -> None:
        """KeyFrameDatabase::clear on the host arrays (what the device holds
        after ``FrontEnd.start_streams`` emptied the stream's database)."""
        for k in self._ARRAYS:
            n = 1 if k in ("kp_off", "bow_off", "fv_off", "fv_start") else 0  # the leading 0 of an offset row
            a = getattr(self, k)
            if self._buf is not None:
                self._buf[k][:n] = 0
                a = self._buf[k][:n]
            else:
                a = np.zeros((n,) + a.shape[1:], a.dtype)
            setattr(self, k, a)
        self.nkf = 0

    def erase(self, kf_remap) -> None:
        """The host arrays without the keyframes whose ``kf_remap`` entry is -1
        (what the device holds after ``FrontEnd.compact_maps`` dropped them):
        the kept keyframes' rows closed up, offsets rebased."""
        keep = np.nonzero(np.asarray(kf_remap)[:self.nkf] >= 0)[0]
        fam = dict(kp_off=("kps", "desc"), bow_off=("bow_words", "bow_values"), fv_off=("fv_nodes",))
        feat0 = self.fv_start[self.fv_off]  # the first feature of every keyframe
        new = {}
        for off, arrays in fam.items():
            o = getattr(self, off)
            rows = np.concatenate([np.arange(o[k], o[k + 1]) for k in keep]) if len(keep) else np.zeros(0, np.int64)
            for a in arrays:
                new[a] = getattr(self, a)[rows]
            n = np.zeros(len(keep) + 1, np.int32)
            n[1:] = np.cumsum((o[1:] - o[:-1])[keep])
            new[off] = n
            if off == "fv_off":  # fv_start: the nodes' offsets follow their keyframe's features down
                nf = np.zeros(len(keep) + 1, np.int64)
                nf[1:] = np.cumsum((feat0[1:] - feat0[:-1])[keep])
                shift = np.repeat(feat0[keep] - nf[:-1], (o[1:] - o[:-1])[keep])
                new["fv_start"] = np.concatenate([self.fv_start[rows] - shift, nf[-1:]]).astype(np.int32)
                frows = (np.concatenate([np.arange(feat0[k], feat0[k + 1]) for k in keep]) if len(keep)
                         else np.zeros(0, np.int64))
                new["fv_feats"] = self.fv_feats[frows]
        for k in self._ARRAYS:
            a = np.ascontiguousarray(new[k], getattr(self, k).dtype)
            if self._buf is not None:
                self._buf[k][:len(a)] = a
                a = self._buf[k][:len(a)]
            setattr(self, k, a)
        self.nkf = len(keep)

    def append(self, kps, desc=None, words=None, values=None, fv=None) -> None:
        """gf_kfdb_append: one more keyframe (index nkf) with its BowVector
        and FeatureVector, or the keyframes of a KeyframeDB of rows given as
        ``kps``. Synchronous; a database attached to a front end gets its
        keyframes through ``FrontEnd.update_maps`` instead."""
        from ._lib import GFError

        rows = kps if isinstance(kps, KeyframeDB) else KeyframeDB.rows(kps, desc, words, values, fv)
        if not self._dev and not self.growable:
            raise GFError(-1, "the keyframe database is fixed")
        for _, h in self._dev.values():
            check(lib().gf_kfdb_append(h, ctypes.byref(rows.struct())))
        self.extend(rows)

    def read(self, ctx) -> dict:
        """gf_kfdb_read: the device database and its inverted file, packed:
        the arrays of gf_keyframe_db plus inv_words / inv_off / inv_kf."""
        from .orb import KEYPOINT_DTYPE

        h = self.device(ctx)
        counts = np.zeros(6, np.int32)
        check(lib().gf_kfdb_read(h, ptr(counts), None, None, None, None, None))
        nkf, nk, nb, nn, nf, nw = (int(c) for c in counts)
        shape = dict(kp_off=(nkf + 1, np.int32), kps=(nk, KEYPOINT_DTYPE), desc=((nk, 32), np.uint8),
                     bow_off=(nkf + 1, np.int32), bow_words=(nb, np.int32), bow_values=(nb, np.float64),
                     fv_off=(nkf + 1, np.int32), fv_nodes=(nn, np.int32), fv_start=(nn + 1, np.int32),
                     fv_feats=(nf, np.int32), inv_words=(nw, np.int32), inv_off=(nw + 1, np.int32),
                     inv_kf=(nb, np.int32))
        size = lambda sh: int(np.prod(sh))  # noqa: E731
        buf = {k: np.zeros(max(size(sh), 1), dt) for k, (sh, dt) in shape.items()}
        out = KeyframeDBArrays(nkf, *[buf[k].ctypes.data for k in self._ARRAYS])
        caps = np.array([nkf, nk, nb, nn, nf, nw], np.int32)
        check(lib().gf_kfdb_read(h, ptr(counts), ctypes.byref(out), ptr(buf["inv_words"]), ptr(buf["inv_off"]),
                                 ptr(buf["inv_kf"]), ptr(caps)))
        res = {k: buf[k][:size(sh)].reshape(sh).copy() for k, (sh, dt) in shape.items()}
        res["nkf"] = nkf
        return res

    def __del__(self):
        try:
            for _, h in self._dev.values():
                lib().gf_kfdb_destroy(h)
        except Exception:
            pass
