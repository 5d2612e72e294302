"""``Tracking::CreateInitialMap`` (src/Tracking.cc:1199-1322): the link from
the monocular initialiser to a map that ``LocalMapper`` can take over.

``create_initial_maps_device`` is the batched device path: stage 1
(``gf_initial_map_points_dev``: the filter of Tracking.cc:1126-1133, the map
points, the slot tables and the graph), ``Optimizer::GlobalBundleAdjustemnt(
mpMap, 20)`` as a ``LocalBAPlan(iterations=20)`` and stage 2
(``gf_initial_map_finish_dev``: UpdateNormalAndDepth, the median depth, the
reset tests and the scaling), which reads the solver's output in place. It
chains from ``initializer.initialize_batch_device`` without host work on the
inputs; the graph arrays are downloaded once for the plan's constructor.
``create_initial_map`` is a batch of one turned into a ``LoopMap``.

Before it, ``Tracking::FirstInitialization`` / ``Tracking::Initialize``
(Tracking.cc:920-946, 988-1040, Struct_Motion): ``search_gate_initialize_device``
runs ORBmatcher::SearchForInitialization, the gate of :999-1017 and
``Initializer::Initialize`` for P sequences on device tensors without a host
step in between, ``initialize_device`` adds CreateInitialMap, and
``MonoInitializer`` is the state machine of Tracking.cc:547-569 for one
sequence, from extracted frames to a ``LoopMap``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, lib
from .initializer import INIT_RESULT_DTYPE
from .matcher import MAP_POINT_DTYPE, default_context
from .orb import KEYPOINT_DTYPE

GF_IM_OK, GF_IM_NOT_INITIALIZED, GF_IM_RESET_DEPTH, GF_IM_RESET_FEW = 0, 1, 2, 3
STATUS_NAMES = {0: "GF_IM_OK", 1: "GF_IM_NOT_INITIALIZED", 2: "GF_IM_RESET_DEPTH", 3: "GF_IM_RESET_FEW"}
THRES_INIT_MPT_NUM = 100  # include/Tracking.h
INIT_BA_ITERATIONS = 20   # Tracking.cc:1263

REPORT_DTYPE = np.dtype([("status", "i4"), ("npts", "i4"), ("tracked", "i4"), ("ba_iterations", "i4"),
                         ("median_depth", "f4"), ("Tcw", "f4", (2, 4, 4))])
assert REPORT_DTYPE.itemsize == 148

_IN_PTRS = ("kps1", "desc1", "n1", "kps2", "desc2", "n2", "matches12", "init", "p3d", "triangulated")
_PT_FIELDS = ("status", "npts", "pt_kp", "mps", "mp_desc", "slots1", "slots2", "kf_Tcw", "kf_kind", "kf_cam", "pt_pos",
              "edge_pt", "edge_kf", "edge_z", "edge_inv_sigma2")


class InitMapIn(ctypes.Structure):
    """gf_initmap_in."""

    _fields_ = [(n, ctypes.c_void_p) for n in _IN_PTRS] + [("cap1", ctypes.c_int32), ("cap2", ctypes.c_int32)]


class InitMapPoints(ctypes.Structure):
    """gf_initmap_points."""

    _fields_ = [(n, ctypes.c_void_p) for n in _PT_FIELDS]


def _alloc_points(P, cap1, cap2, dev):
    import torch

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    i32, f32, u8 = torch.int32, torch.float32, torch.uint8
    return dict(status=z(P, i32), npts=z(P, i32), pt_kp=z((P, cap1, 2), i32),
                mps=z((P, cap1, MAP_POINT_DTYPE.itemsize), u8), mp_desc=z((P, cap1, 32), u8), slots1=z((P, cap1), i32),
                slots2=z((P, cap2), i32), kf_Tcw=z((P, 2, 16), f32), kf_kind=z((P, 2), u8), kf_cam=z((P, 2, 4), f32),
                pt_pos=z((P, cap1, 3), f32), edge_pt=z((P, 2 * cap1), i32), edge_kf=z((P, 2 * cap1), i32),
                edge_z=z((P, 2 * cap1, 2), f32), edge_inv_sigma2=z((P, 2 * cap1), f32))


def _stream(dev):
    import torch

    return torch.cuda.current_stream(dev).cuda_stream


def initial_map_points_device(info, kps1, desc1, n1, kps2, desc2, n2, matches12, init, p3d, triangulated, ctx=None):
    """Stage 1 on device tensors laid out as ``initialize_batch_device`` lays
    them out: kps1 [P, cap1, 28] / kps2 [P, cap2, 28] uint8, desc1 [P, cap1,
    32] / desc2 uint8, n1 / n2 [P] int32, matches12 [P, cap1] int32, init
    [P, 200] uint8, p3d [P, cap1, 3] f32, triangulated [P, cap1] uint8.
    Enqueued on the current torch stream. -> (InitMapIn, dict of the device
    outputs named as gf_initmap_points names them)."""
    ctx = ctx or default_context()
    P, cap1, cap2 = kps1.shape[0], kps1.shape[1], kps2.shape[1]
    tens = dict(kps1=kps1, desc1=desc1, n1=n1, kps2=kps2, desc2=desc2, n2=n2, matches12=matches12, init=init, p3d=p3d,
                triangulated=triangulated)
    for k, t in tens.items():
        if not t.is_contiguous() or t.shape[0] != P:
            raise ValueError(f"{k}: a contiguous tensor with one row per problem")
    arg = InitMapIn(*[tens[k].data_ptr() for k in _IN_PTRS], cap1, cap2)
    arg._keep = tens
    out = _alloc_points(P, cap1, cap2, kps1.device)
    pts = InitMapPoints(*[out[k].data_ptr() for k in _PT_FIELDS])
    check(lib().gf_initial_map_points_dev(ctx.handle, ctypes.byref(info), P, ctypes.byref(arg), ctypes.byref(pts),
                                          _stream(kps1.device)))
    return arg, out


def initial_map_finish_device(info, arg, out, ba_Tcw_ptrs, ba_pos_ptrs, ba_iter_ptrs=None,
                              thres: int = THRES_INIT_MPT_NUM, ctx=None):
    """Stage 2: ``arg`` / ``out`` as stage 1 returned them; ba_*_ptrs: int64
    device tensors [P] holding device addresses (per problem the optimised 2 x
    16 poses, npts x 3 points, the iteration count). -> (report [P, 148] uint8,
    mps [P, cap1, 32] uint8), device tensors."""
    import torch

    ctx = ctx or default_context()
    dev = out["status"].device
    P, cap1 = out["slots1"].shape
    rep = torch.zeros((P, REPORT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    mps = torch.zeros((P, cap1, MAP_POINT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    pts = InitMapPoints(*[out[k].data_ptr() for k in _PT_FIELDS])
    check(lib().gf_initial_map_finish_dev(ctx.handle, ctypes.byref(info), P, ctypes.byref(arg), ctypes.byref(pts),
                                          ba_Tcw_ptrs.data_ptr(), ba_pos_ptrs.data_ptr(),
                                          ba_iter_ptrs.data_ptr() if ba_iter_ptrs is not None else None, int(thres),
                                          rep.data_ptr(), mps.data_ptr(), _stream(dev)))
    return rep, mps


def ba_problems(out: dict) -> list:
    """The gf_ba_problem dicts of stage 1's output (one download)."""
    h = {k: out[k].cpu().numpy() for k in ("npts", "kf_Tcw", "kf_kind", "kf_cam", "pt_pos", "edge_pt", "edge_kf",
                                           "edge_z", "edge_inv_sigma2")}
    probs = []
    for p, n in enumerate(h["npts"]):
        n = int(n)
        probs.append(dict(kf_Tcw=h["kf_Tcw"][p], kf_kind=h["kf_kind"][p], kf_cam=h["kf_cam"][p],
                          pt_pos=h["pt_pos"][p, :n], edge_pt=h["edge_pt"][p, :2 * n], edge_kf=h["edge_kf"][p, :2 * n],
                          edge_z=h["edge_z"][p, :2 * n], edge_inv_sigma2=h["edge_inv_sigma2"][p, :2 * n]))
    return probs


def create_initial_maps_device(info, kps1, desc1, n1, kps2, desc2, n2, matches12, init, p3d, triangulated,
                               thres: int = THRES_INIT_MPT_NUM, iterations: int = INIT_BA_ITERATIONS, ctx=None) -> dict:
    """CreateInitialMap for a batch (tensors as in
    :func:`initial_map_points_device`): stage 1, one
    ``LocalBAPlan(iterations=20)`` over all problems (a failed initialisation
    is an empty graph in it), stage 2 reading the plan's device results. All on
    the current torch stream. -> dict of device tensors: ``report`` [P, 148]
    uint8 (REPORT_DTYPE rows), ``mps`` [P, cap1, 32] uint8 (MAP_POINT_DTYPE
    rows), and stage 1's ``npts``, ``pt_kp``, ``mp_desc``, ``slots1``,
    ``slots2``; ``ba_steps``: the solver steps run; ``times``: host-clock
    seconds of stage 1 with the graph download (``points``), the plan's
    constructor (``plan``), the solve (``solve``) and stage 2 (``finish``)."""
    import time

    import torch

    from .optimizer import LocalBAPlan

    ctx = ctx or default_context()
    dev = kps1.device
    t = [time.perf_counter()]
    times = {}

    def lap(name):
        t.append(time.perf_counter())
        times[name] = t[-1] - t[-2]

    arg, out = initial_map_points_device(info, kps1, desc1, n1, kps2, desc2, n2, matches12, init, p3d, triangulated,
                                         ctx)
    probs = ba_problems(out)
    lap("points")
    plan = LocalBAPlan(probs, ctx, iterations=iterations)
    lap("plan")
    try:
        steps = plan.solve(_stream(dev))
        lap("solve")
        ptrs = np.asarray([plan.results_dev(p) for p in range(len(plan.arrs))], np.int64).reshape(-1, 3)
        tabs = torch.from_numpy(np.ascontiguousarray(ptrs.T)).to(dev)
        rep, mps = initial_map_finish_device(info, arg, out, tabs[0], tabs[1], tabs[2], thres, ctx)
        torch.cuda.current_stream(dev).synchronize()  # the plan's arrays are read until here
        lap("finish")
    finally:
        plan.close()
    return dict(report=rep, mps=mps, npts=out["npts"], pt_kp=out["pt_kp"], mp_desc=out["mp_desc"],
                slots1=out["slots1"], slots2=out["slots2"], ba_steps=steps, times=times)


def _dev_inputs(kps1, desc1, kps2, desc2, matches12, init, p3d, triangulated, device="cuda"):
    """One host problem as the batch-of-one device tensors."""
    import torch

    k1, k2 = np.ascontiguousarray(kps1, KEYPOINT_DTYPE), np.ascontiguousarray(kps2, KEYPOINT_DTYPE)
    n1, n2 = len(k1), len(k2)
    if n1 > 4096 or n2 > 4096:
        raise ValueError("a frame holds at most 4096 keypoints")
    c1, c2 = max(n1, 1), max(n2, 1)
    if not (np.size(matches12) == n1 and np.size(p3d) == 3 * n1 and np.size(triangulated) == n1 and
            np.size(desc1) == 32 * n1 and np.size(desc2) == 32 * n2):
        raise ValueError("matches12, p3d, triangulated and the descriptors: one row per keypoint")

    def up(a, shape, dt):
        buf = np.zeros(shape, dt)
        a = np.ascontiguousarray(a, dt).reshape(-1)
        buf.reshape(-1)[:a.size] = a
        return torch.from_numpy(buf).to(device)

    return (up(k1.view(np.uint8), (1, c1, 28), np.uint8),
            up(np.ascontiguousarray(desc1, np.uint8), (1, c1, 32), np.uint8),
            torch.tensor([n1], dtype=torch.int32, device=device),
            up(k2.view(np.uint8), (1, c2, 28), np.uint8),
            up(np.ascontiguousarray(desc2, np.uint8), (1, c2, 32), np.uint8),
            torch.tensor([n2], dtype=torch.int32, device=device),
            up(np.ascontiguousarray(matches12, np.int32), (1, c1), np.int32),
            up(np.ascontiguousarray(np.asarray(init).reshape(-1)[:1], INIT_RESULT_DTYPE).view(np.uint8), (1, 200), np.uint8),
            up(np.ascontiguousarray(p3d, np.float32), (1, c1, 3), np.float32),
            up(np.ascontiguousarray(np.asarray(triangulated).astype(np.uint8)), (1, c1), np.uint8))


def create_initial_map(info, K, kps1, desc1, kps2, desc2, matches12, init_result, p3d, triangulated, voc=None,
                       ctx=None, thres: int = THRES_INIT_MPT_NUM, levelsup: int = 4):
    """Tracking::CreateInitialMap on one initialiser output (host arrays:
    undistorted keypoints and [n, 32] descriptors of the two frames,
    mvIniMatches, the INIT_RESULT_DTYPE record, vP3D, vbTriangulated) ->
    ``(LoopMap | None, report)``.

    The map has keyframes 0 (KFini, mnId 0, identity) and 1 (KFcur, mnId 1),
    the points in index order of their KFini keypoint with ``ref_kf`` 1 and
    observations ``{0: i, 1: matches12[i]}``, both slot tables,
    ``ComputeBoW`` of both keyframes when ``voc`` is given (an
    ``ORBVocabulary`` or a callable, as ``process_new_keyframe`` takes it) and
    ``UpdateConnections`` of both (:1254-1255), median depth 1. ``None`` where
    the reference calls ``Reset()`` (or the initialiser had failed); report:
    dict with ``status`` (GF_IM_*), ``npts``, ``tracked``, ``ba_iterations``,
    ``median_depth``, ``Tcw`` [2, 4, 4] and ``times`` (host-clock seconds:
    ``upload``, the laps of :func:`create_initial_maps_device`, ``map`` for
    the download and the LoopMap, ``bow``, ``connections``). K is the calibration the
    initialiser ran with; the map's camera is ``info``'s."""
    from .bow import FeatureVector
    from .loopmap import LoopMap

    ctx = ctx or default_context()
    Kf = np.asarray(K, np.float32).reshape(3, 3)
    if not (Kf[0, 0] == np.float32(info.fx) and Kf[1, 1] == np.float32(info.fy) and Kf[0, 2] == np.float32(info.cx)
            and Kf[1, 2] == np.float32(info.cy)):
        raise ValueError("K and info describe different cameras")
    import time

    t0 = time.perf_counter()
    tens = _dev_inputs(kps1, desc1, kps2, desc2, matches12, init_result, p3d, triangulated)
    t1 = time.perf_counter()
    res = create_initial_maps_device(info, *tens, thres=thres, ctx=ctx)
    t2 = time.perf_counter()
    r = res["report"].cpu().numpy().view(REPORT_DTYPE)[0, 0]
    times = dict(upload=t1 - t0, **res["times"])
    report = dict(status=int(r["status"]), npts=int(r["npts"]), tracked=int(r["tracked"]),
                  ba_iterations=int(r["ba_iterations"]), median_depth=np.float32(r["median_depth"]),
                  Tcw=r["Tcw"].copy(), times=times)
    if report["status"] != GF_IM_OK:
        return None, report
    n, n1, n2 = report["npts"], len(kps1), len(kps2)
    mps = res["mps"].cpu().numpy().reshape(-1).view(MAP_POINT_DTYPE)[:n].copy()
    pt_kp = res["pt_kp"].cpu().numpy()[0, :n]
    m = LoopMap(info, [kps1, kps2], [desc1, desc2],
                [res["slots1"].cpu().numpy()[0, :n1], res["slots2"].cpu().numpy()[0, :n2]], mps,
                res["mp_desc"].cpu().numpy()[0, :n], observations=[{0: int(a), 1: int(b)} for a, b in pt_kp],
                kf_Tcw=report["Tcw"], ref_kf=np.ones(n, np.int32), kf_id=[0, 1])
    t3 = time.perf_counter()
    times["map"] = t3 - t2
    if voc is not None:
        transform = voc.transform if hasattr(voc, "transform") else voc
        for k in (0, 1):
            words, values, fv = transform(m.kf_desc[k], levelsup)
            m.kf_bow[k] = (words, values)
            m.kf_fv[k] = fv if isinstance(fv, FeatureVector) else FeatureVector(*fv)
    t4 = time.perf_counter()
    m.update_connections_batch([0, 1], ctx)
    times["bow"], times["connections"] = t4 - t3, time.perf_counter() - t4
    return m, report


# ------------------------------------------------ Tracking::Initialize
GF_SI_OK, GF_SI_FEW_KEYPOINTS, GF_SI_FEW_MATCHES = 0, 1, 2
SRH_WINDOW_SIZE_INIT = 100  # include/Tracking.h
NOT_INITIALIZED, INITIALIZING, WORKING = "NOT_INITIALIZED", "INITIALIZING", "WORKING"


def search_for_initialization_device(info, kps1, desc1, n1, kps2, desc2, n2, prev_matched,
                                     window: int = SRH_WINDOW_SIZE_INIT, nnratio: float = 0.9, check_ori: bool = True,
                                     flags: int = 0, ctx=None):
    """``gf_search_for_initialization_batch_dev`` on device tensors laid out
    as :func:`initial_map_points_device` takes them; prev_matched [P, cap1, 2]
    f32 is updated in place. -> (matches12 [P, cap1] int32, nmatches [P]
    int32). Enqueued on the current torch stream."""
    import torch

    ctx = ctx or default_context()
    P, cap1, cap2 = kps1.shape[0], kps1.shape[1], kps2.shape[1]
    for k, t in dict(kps1=kps1, desc1=desc1, n1=n1, kps2=kps2, desc2=desc2, n2=n2, prev_matched=prev_matched).items():
        if not t.is_contiguous() or t.shape[0] != P:
            raise ValueError(f"{k}: a contiguous tensor with one row per problem")
    if prev_matched.dtype != torch.float32 or prev_matched.numel() != 2 * P * cap1:
        raise ValueError("prev_matched: float32 [P, cap1, 2]")
    dev = kps1.device
    m12 = torch.empty((P, cap1), dtype=torch.int32, device=dev)
    nm = torch.zeros(P, dtype=torch.int32, device=dev)
    check(lib().gf_search_for_initialization_batch_dev(
        ctx.handle, ctypes.byref(info), P, kps1.data_ptr(), desc1.data_ptr(), cap1, n1.data_ptr(), kps2.data_ptr(),
        desc2.data_ptr(), cap2, n2.data_ptr(), int(window), ctypes.c_float(nnratio), int(bool(check_ori)), int(flags),
        prev_matched.data_ptr(), m12.data_ptr(), nm.data_ptr(), _stream(dev)))
    return m12, nm


def search_gate_initialize_device(info, K, kps1, desc1, n1, kps2, desc2, n2, prev_matched, rng_states,
                                  thres: int = THRES_INIT_MPT_NUM, flags: int = 0, ctx=None) -> dict:
    """Tracking::Initialize (Tracking.cc:999-1023) for P sequences in one set
    of launches: the matcher with ORBmatcher(0.9, true) and window 100, the
    gate, ``Initializer(frame, 1.0, 200)::Initialize`` on each problem's own
    rand() state (rng_states [P, 132] uint8, advanced in place where the
    initialiser runs). prev_matched [P, cap1, 2] is updated in place as the
    reference updates mvbPrevMatched. -> dict of device tensors: ``status``
    (GF_SI_*), ``nmatches``, ``matches12`` (mvIniMatches as the matcher or the
    gate left them), ``init_matches12`` (what the initialiser saw), ``init``
    [P, 200] uint8, ``p3d``, ``triangulated``."""
    import torch

    from .initializer import initialize_batch_device

    ctx = ctx or default_context()
    dev = kps1.device
    P, cap1 = kps1.shape[0], kps1.shape[1]
    before = prev_matched.clone()
    m12, nm = search_for_initialization_device(info, kps1, desc1, n1, kps2, desc2, n2, prev_matched, flags=flags,
                                               ctx=ctx)
    status = torch.zeros(P, dtype=torch.int32, device=dev)
    init_m = torch.empty((P, cap1), dtype=torch.int32, device=dev)
    check(lib().gf_tracking_initialize_gate_dev(ctx.handle, P, n2.data_ptr(), cap1, int(thres), before.data_ptr(),
                                                prev_matched.data_ptr(), m12.data_ptr(), nm.data_ptr(),
                                                status.data_ptr(), init_m.data_ptr(), _stream(dev)))
    res, p3d, tri = initialize_batch_device(ctx, K, kps1, n1, kps2, n2, init_m, rng_states)
    return dict(status=status, nmatches=nm, matches12=m12, init_matches12=init_m, init=res, p3d=p3d, triangulated=tri,
                _keep=before)


def initialize_device(info, K, kps1, desc1, n1, kps2, desc2, n2, prev_matched, rng_states,
                      thres: int = THRES_INIT_MPT_NUM, flags: int = 0, ctx=None) -> dict:
    """The batched chain search -> gate -> Initializer -> CreateInitialMap on
    device tensors (see :func:`search_gate_initialize_device` and
    :func:`create_initial_maps_device`). -> the dicts of both merged, plus
    ``states``: per problem NOT_INITIALIZED (the gate failed or CreateInitialMap
    reset), INITIALIZING (the initialiser failed) or WORKING, and
    ``ini_matches`` [P, cap1] int32: mvIniMatches after the untriangulated
    filter of Tracking.cc:1025-1032 where the initialiser succeeded."""
    import torch

    a = search_gate_initialize_device(info, K, kps1, desc1, n1, kps2, desc2, n2, prev_matched, rng_states, thres,
                                      flags, ctx)
    b = create_initial_maps_device(info, kps1, desc1, n1, kps2, desc2, n2, a["init_matches12"], a["init"], a["p3d"],
                                   a["triangulated"], thres=thres, ctx=ctx)
    ok = a["init"].view(torch.int32)[:, 0] != 0
    m = a["matches12"]
    drop = ok[:, None] & (m >= 0) & (a["triangulated"] == 0)
    ini = torch.where(drop, torch.full_like(m, -1), m)
    st = a["status"].cpu().numpy()
    im = b["report"].cpu().numpy().view(REPORT_DTYPE).reshape(-1)["status"]
    okh = ok.cpu().numpy()
    states = [NOT_INITIALIZED if s != GF_SI_OK else INITIALIZING if not o else WORKING if i == GF_IM_OK
              else NOT_INITIALIZED for s, o, i in zip(st, okh, im)]
    return dict(a, **b, states=states, ini_matches=ini)


class MonoInitializer:
    """The tracker's start for one monocular sequence (Tracking.cc:547-569):
    NOT_INITIALIZED -> FirstInitialization (:920-946), INITIALIZING ->
    Initialize (:988-1040, Struct_Motion), WORKING once CreateInitialMap has
    made a map. ``feed(kps, desc)`` takes one extracted frame (undistorted
    keypoints, [n, 32] descriptors) and returns ``(state, map, report)``: the
    ``LoopMap`` and CreateInitialMap's report when the state became WORKING,
    else ``None`` and a dict with what was reached (``status`` of the gate,
    ``nmatches``, ``init`` the initialiser's record, ``im_status``). A reset
    status of CreateInitialMap returns the tracker to NOT_INITIALIZED, where
    Reset() leaves mState (:4092); a failed initialiser leaves INITIALIZING
    with mvbPrevMatched as the matcher updated it. ``rng`` is the caller's
    rand() state (a ``pnp.Rand`` or its RNG_DTYPE record), advanced in place."""

    def __init__(self, info, K, rng, voc=None, ctx=None, thres: int = THRES_INIT_MPT_NUM, levelsup: int = 4):
        self.info, self.K, self.voc = info, np.asarray(K, np.float32).reshape(3, 3), voc
        self.rng_state = rng.state if hasattr(rng, "state") else rng  # RNG_DTYPE [1], advanced in place
        self.ctx = ctx or default_context()
        self.thres, self.levelsup = int(thres), int(levelsup)
        self.mState = NOT_INITIALIZED
        self.mInitialFrame = None    # (keypoints, descriptors)
        self.mvbPrevMatched = None   # float32 [n1, 2]
        self.mvIniMatches = None     # int32 [n1]
        self.times = {}

    def feed(self, kps, desc):
        import time

        import torch

        k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(len(k), 32)
        if len(k) > 4096:
            raise ValueError("a frame holds at most 4096 keypoints")
        if self.mState == WORKING:
            raise RuntimeError("the map exists: the frame belongs to the tracking front end")
        if self.mState == NOT_INITIALIZED:  # FirstInitialization
            if len(k) > self.thres:
                self.mInitialFrame = (k, d)
                self.mvbPrevMatched = np.ascontiguousarray(np.stack([k["x"], k["y"]], 1), np.float32)
                self.mvIniMatches = np.full(len(k), -1, np.int32)
                self.mState = INITIALIZING
            return self.mState, None, dict(status=None)
        t0 = time.perf_counter()
        k1, d1 = self.mInitialFrame
        n1, n2 = len(k1), len(k)
        c2 = max(n2, 1)
        dev = "cuda"

        def up(a, shape, dt):
            buf = np.zeros(shape, dt)
            a = np.ascontiguousarray(a, dt).reshape(-1)
            buf.reshape(-1)[:a.size] = a
            return torch.from_numpy(buf).to(dev)

        tens = (up(k1.view(np.uint8), (1, n1, 28), np.uint8), up(d1, (1, n1, 32), np.uint8),
                torch.tensor([n1], dtype=torch.int32, device=dev), up(k.view(np.uint8), (1, c2, 28), np.uint8),
                up(d, (1, c2, 32), np.uint8), torch.tensor([n2], dtype=torch.int32, device=dev))
        prev = torch.from_numpy(self.mvbPrevMatched.reshape(1, n1, 2)).to(dev)
        rs = torch.from_numpy(self.rng_state.view(np.uint8).reshape(1, -1).copy()).to(dev)
        t1 = time.perf_counter()
        a = search_gate_initialize_device(self.info, self.K, *tens, prev, rs, self.thres, ctx=self.ctx)
        status = int(a["status"].cpu()[0])
        t2 = time.perf_counter()
        self.mvbPrevMatched = prev.cpu().numpy().reshape(n1, 2)
        self.mvIniMatches = a["matches12"].cpu().numpy().reshape(n1).copy()
        self.rng_state.view(np.uint8).reshape(-1)[:] = rs.cpu().numpy().reshape(-1)
        rep = dict(status=status, nmatches=int(a["nmatches"].cpu()[0]))
        self.times = dict(upload=t1 - t0, search_gate_initialize=t2 - t1)
        if status != GF_SI_OK:
            self.mState = NOT_INITIALIZED
            return self.mState, None, rep
        init = a["init"].cpu().numpy().reshape(-1).view(INIT_RESULT_DTYPE).copy()
        rep["init"] = init
        if not int(init["ok"][0]):
            return self.mState, None, rep
        p3d = a["p3d"].cpu().numpy().reshape(n1, 3)
        tri = a["triangulated"].cpu().numpy().reshape(n1)
        t3 = time.perf_counter()
        m, irep = create_initial_map(self.info, self.K, k1, d1, k, d, self.mvIniMatches, init, p3d, tri, voc=self.voc,
                                     ctx=self.ctx, thres=self.thres, levelsup=self.levelsup)
        self.mvIniMatches[(self.mvIniMatches >= 0) & (tri == 0)] = -1  # Tracking.cc:1025-1032
        self.times.update(download=t3 - t2, create_initial_map=time.perf_counter() - t3, **{
            "map_" + k_: v for k_, v in irep["times"].items()})
        irep.update(rep, im_status=irep["status"], status=status)
        self.mState = WORKING if irep["im_status"] == GF_IM_OK else NOT_INITIALIZED
        return self.mState, m, irep


# ------------------------------------------------ NeedNewKeyFrame / CreateNewKeyFrame -> LocalMapping
def loopmap_from_global_map(info, gm, voc=None, ctx=None, levelsup: int = 4, counter=None):
    """A ``LoopMap`` over a ``scene.build_global_map`` entry ``gm``, the map a
    front-end stream tracks (``FrontEnd.set_map`` / ``set_covis`` of the same
    entry): point id = map index, keyframe index = graph index, the slot
    tables from the graph's CSR, the poses ``gm["kf_Tcw"]``. With ``voc``
    every keyframe gets its ``ComputeBoW`` (what CreateNewMapPoints reads of
    the neighbours); the covisibility graph is ``UpdateConnections`` of every
    keyframe, in index order (``counter``: as ``LoopMap.update_connections_batch``
    takes it, the device's by default)."""
    from .bow import FeatureVector
    from .loopmap import LoopMap

    g = gm["graph"]
    off = np.asarray(g["kf_mp_off"], np.int64)
    kf_mp = [np.asarray(g["kf_mp"][off[k]:off[k + 1]], np.int32) for k in range(len(off) - 1)]
    m = LoopMap(info, gm["kf_kps"], gm["kf_desc"], kf_mp, gm["mp"], gm["desc"], mp_bad=g["mp_bad"], kf_bad=g["kf_bad"],
                kf_Tcw=np.asarray(gm["kf_Tcw"], np.float32))
    if voc is not None:
        transform = voc.transform if hasattr(voc, "transform") else voc
        for k in range(m.nkf):
            words, values, fv = transform(m.kf_desc[k], levelsup)
            m.kf_bow[k] = (words, values)
            m.kf_fv[k] = fv if isinstance(fv, FeatureVector) else FeatureVector(*fv)
    m.update_connections_batch(range(m.nkf), ctx, counter)
    return m


# ------------------------------------------------ LocalMapping -> the tracker's map
def _csr(rows, dtype=np.int32):
    off = np.zeros(len(rows) + 1, np.int32)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, dtype).reshape(-1) for r in rows]) if rows else np.zeros(0, dtype)
    return off, np.ascontiguousarray(flat, dtype)


def covis_graph_from_loopmap(m) -> dict:
    """The ``gf_covis_map`` arrays of a ``LoopMap`` (the dict
    ``FrontEnd.set_covis`` takes), point id = map index and keyframe index =
    graph index: the slot tables, the observation maps as rows of ascending
    keyframe index, ``kf_cov`` the ordered connected keyframes
    (mvpOrderedConnectedKeyFrames). The inverse of
    :func:`loopmap_from_global_map`."""
    kf_mp_off, kf_mp = _csr([np.asarray(s, np.int32) for s in m.slots])
    kf_cov_off, kf_cov = _csr([np.asarray(o, np.int32) for o in m.ordered])
    mp_obs_off, mp_obs = _csr([np.asarray(sorted(o), np.int32) for o in m.obs])
    return dict(kf_bad=np.asarray(m.kf_bad).astype(np.uint8), kf_mp_off=kf_mp_off, kf_mp=kf_mp, kf_cov_off=kf_cov_off,
                kf_cov=kf_cov, mp_bad=np.asarray(m.mp_bad).astype(np.uint8), mp_obs_off=mp_obs_off, mp_obs=mp_obs)


def _changed_rows(off_a, flat_a, off_b, flat_b, n: int) -> np.ndarray:
    """Rows < n of two CSR tables that differ in length or content."""
    la, lb = np.diff(off_a[:n + 1]), np.diff(off_b[:n + 1])
    diff = la != lb
    same = np.nonzero(~diff & (la > 0))[0]
    if len(same):
        ln = la[same]
        row = np.repeat(np.arange(len(same)), ln)
        within = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        ne = flat_a[off_a[same][row] + within] != flat_b[off_b[same][row] + within]
        bad = np.zeros(len(same), bool)
        np.logical_or.at(bad, row, ne)
        diff[same[bad]] = True
    return np.nonzero(diff)[0]


def restrict_graph(g, kf_remap, mp_remap) -> dict:
    """The ``gf_covis_map`` arrays restricted to the kept keyframes and points
    (remap tables: new index, -1 dropped) and renumbered, as
    ``FrontEnd.compact_maps`` leaves them on the device: slot rows of dropped
    keyframes gone, a slot that named a dropped point -1, observation rows and
    covisibility lists filtered in order."""
    kf_remap, mp_remap = np.asarray(kf_remap, np.int32), np.asarray(mp_remap, np.int32)
    keep_kf, keep_mp = kf_remap >= 0, mp_remap >= 0
    nkf, n = len(keep_kf), len(keep_mp)

    def off_of(lens):
        off = np.zeros(len(lens) + 1, np.int32)
        off[1:] = np.cumsum(lens)
        return off

    srow = np.repeat(np.arange(nkf), np.diff(g["kf_mp_off"]))
    sm = keep_kf[srow]
    sv = g["kf_mp"][sm]
    kf_mp = np.where(sv >= 0, mp_remap[np.maximum(sv, 0)], -1).astype(np.int32) if n else sv.astype(np.int32)
    crow = np.repeat(np.arange(nkf), np.diff(g["kf_cov_off"]))
    cm = keep_kf[crow] & keep_kf[g["kf_cov"]] if nkf else np.zeros(0, bool)
    orow = np.repeat(np.arange(n), np.diff(g["mp_obs_off"]))
    om = keep_mp[orow] & keep_kf[g["mp_obs"]] if nkf else np.zeros(len(orow), bool)
    return dict(kf_bad=np.asarray(g["kf_bad"])[keep_kf].astype(np.uint8),
                kf_mp_off=off_of(np.diff(g["kf_mp_off"])[keep_kf]), kf_mp=kf_mp,
                kf_cov_off=off_of(np.bincount(crow[cm], minlength=nkf)[keep_kf]),
                kf_cov=kf_remap[g["kf_cov"][cm]].astype(np.int32),
                mp_bad=np.asarray(g["mp_bad"])[keep_mp].astype(np.uint8),
                mp_obs_off=off_of(np.bincount(orow[om], minlength=n)[keep_mp]),
                mp_obs=kf_remap[g["mp_obs"][om]].astype(np.int32))


def _graph_through(m, mp_id, kf_id) -> dict:
    """:func:`covis_graph_from_loopmap` of the points ``mp_id`` and keyframes
    ``kf_id`` of a ``LoopMap`` (ascending ids), in their positions: what a
    front end that holds exactly those holds."""
    mp_index, kf_index = np.full(len(m.mps), -1, np.int32), np.full(m.nkf, -1, np.int32)
    mp_index[mp_id] = np.arange(len(mp_id), dtype=np.int32)
    kf_index[kf_id] = np.arange(len(kf_id), dtype=np.int32)

    def through(ids, index):
        ids = np.asarray(ids, np.int32).reshape(-1)
        return np.where(ids >= 0, index[np.maximum(ids, 0)], -1).astype(np.int32) if len(index) else ids

    kf_mp_off, kf_mp = _csr([through(m.slots[k], mp_index) for k in kf_id])
    cov = [through(m.ordered[k], kf_index) for k in kf_id]
    kf_cov_off, kf_cov = _csr([c[c >= 0] for c in cov])
    obs = [through(sorted(m.obs[p]), kf_index) for p in mp_id]  # ascending ids stay ascending: the remap is monotone
    mp_obs_off, mp_obs = _csr([o[o >= 0] for o in obs])
    return dict(kf_bad=np.asarray(m.kf_bad)[kf_id].astype(np.uint8), kf_mp_off=kf_mp_off, kf_mp=kf_mp,
                kf_cov_off=kf_cov_off, kf_cov=kf_cov, mp_bad=np.asarray(m.mp_bad)[mp_id].astype(np.uint8),
                mp_obs_off=mp_obs_off, mp_obs=mp_obs)


class MapFeedback:
    """Carries a ``LocalMapper``'s result back into the map a front-end stream
    tracks (``FrontEnd.update_maps``): a host shadow of what the front end
    holds for the stream (points, descriptors, bad flags, slot rows,
    observation rows, covisibility lists), ``delta()`` the difference between
    the ``LoopMap`` and the shadow as a ``localmap.MapDelta``, ``commit()``
    the shadow advanced after the update succeeded. When the stream has a
    growable ``KeyframeDB``, the delta carries the new keyframes' database rows
    (``kf_kps`` / ``kf_desc`` / ``kf_bow`` / ``kf_fv`` of the LoopMap).

    The id mapping starts as the identity: the LoopMap's point id is the map
    index, its keyframe index the graph index, and both only grow. Anything
    else (a map smaller than the shadow, an existing keyframe whose slot count
    changed, a bad point or keyframe that is good again) raises ``ValueError``.
    ``compact()`` drops keyframes and points from the front end's map
    (``FrontEnd.compact_maps``) while the LoopMap never shrinks; from then on
    ``mp_index`` / ``kf_index`` (LoopMap id -> front-end index, -1 = not held)
    and their inverses ``mp_id`` / ``kf_id`` carry the mapping, and ``delta()``
    goes through them.

    The shadow starts from the front end's own state (``fe.read`` /
    ``fe.covis``), or from ``shadow`` = dict(mp, desc, graph) when given."""

    def __init__(self, fe, stream: int, loopmap, shadow=None):
        self.fe, self.stream, self.map = fe, int(stream), loopmap
        if shadow is None:
            n = int(fe.read("nmp")[stream])
            shadow = dict(mp=fe.read("map")[stream][:n], desc=fe.read("map_desc")[stream][:n], graph=fe.covis(stream))
        self.mp = np.ascontiguousarray(shadow["mp"], MAP_POINT_DTYPE).copy()
        self.desc = np.ascontiguousarray(shadow["desc"], np.uint8).reshape(-1, 32).copy()
        self.graph = {k: np.array(v, copy=True) for k, v in shadow["graph"].items()}
        if len(self.graph["mp_bad"]) != len(self.mp):
            raise ValueError("the shadow's graph and points differ in size")
        self.mp_id = np.arange(len(self.mp), dtype=np.int32)  # front-end index -> LoopMap id
        self.kf_id = np.arange(len(self.graph["kf_bad"]), dtype=np.int32)
        self.mp_index, self.kf_index = self.mp_id.copy(), self.kf_id.copy()  # LoopMap id -> front-end index, -1 not held
        self._identity = True
        self._next = None
        self.delta()  # raises where the map and the front end cannot share indices
        self._next = None

    @staticmethod
    def empty_shadow() -> dict:
        """The shadow of a stream that holds no map: no points, the empty graph."""
        g = {k: np.zeros(1 if k.endswith("_off") else 0, np.uint8 if k.endswith("_bad") else np.int32)
             for k in ("kf_bad", "kf_mp_off", "kf_mp", "kf_cov_off", "kf_cov", "mp_bad", "mp_obs_off", "mp_obs")}
        return dict(mp=np.zeros(0, MAP_POINT_DTYPE), desc=np.zeros((0, 32), np.uint8), graph=g)

    @classmethod
    def starting(cls, fe, stream: int, loopmap) -> "MapFeedback":
        """A feedback for a stream that is about to be started on ``loopmap``
        (:meth:`start`): its shadow is the empty map, whatever the front end
        holds for the stream now."""
        return cls(fe, stream, loopmap, shadow=cls.empty_shadow())

    def start(self, frame_kps, frame_desc, frame_id: int, timestamp: float, since_reloc=None):
        """The ``localmap.StreamStart`` that begins this stream on its LoopMap
        (as ``create_initial_map`` returns it; Tracking.cc:1302-1321), for
        ``FrontEnd.start_streams``: the whole map as a delta against the empty
        map (through ``covis_graph_from_loopmap``; with a growable KeyframeDB
        on the stream, the keyframes' database rows from ``kf_bow`` /
        ``kf_fv``), the given frame (the newest keyframe's: undistorted
        keypoints and descriptors, its mnId and timestamp) as mLastFrame with
        the newest keyframe's slot table as its map points and the newest
        keyframe's pose, and the newest keyframe as mpReferenceKF. The id maps
        and the shadow are then "the front end holds exactly this map": send
        the request; if it is refused, make a new feedback.

        A frame with more keypoints than the front end's capacity (the
        initialiser's extractor asks for 2000, Tracking.cc:218) is reduced to
        the keypoints that hold a map point, in order: SearchByProjection(Cur,
        Last) (ORBmatcher.cc:2096-2098) and TrackPreviousFrame's WindowSearch
        and SearchByProjection(F1, F2) (ORBmatcher.cc:995-998, 1101-1104) walk
        mLastFrame.mvpMapPoints and skip NULL, so the dropped keypoints are
        never read. If even those exceed the
        capacity: GFError GF_ERR_CAP."""
        from ._lib import GFError
        from .localmap import StreamStart

        m = self.map
        if m.nkf < 1:
            raise ValueError("the map holds no keyframe to start from")
        shadow = self.empty_shadow()
        self.mp, self.desc, self.graph = shadow["mp"], shadow["desc"], shadow["graph"]
        self._set_ids(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0)
        self._identity = True
        d = self.delta()
        cur = m.nkf - 1
        kps = np.ascontiguousarray(frame_kps, KEYPOINT_DTYPE).reshape(-1)
        desc = np.ascontiguousarray(frame_desc, np.uint8).reshape(-1, 32)
        kp2mp = np.asarray(m.slots[cur], np.int32).reshape(-1)
        if not len(kps) == len(desc) == len(kp2mp):
            self.discard()
            raise ValueError("the frame and the newest keyframe differ in keypoints")
        if len(kps) > self.fe.cap:
            keep = np.nonzero(kp2mp >= 0)[0]
            if len(keep) > self.fe.cap:
                self.discard()
                raise GFError(-3, f"the initial frame holds {len(keep)} matched keypoints, the front end {self.fe.cap}")
            kps, desc, kp2mp = kps[keep], desc[keep], kp2mp[keep]
        req = StreamStart(d, kps, desc, kp2mp, np.asarray(m.Tcw[cur], np.float32), timestamp, frame_id,
                          since_reloc, ref_kf=cur)
        self.commit()
        return req

    def delta(self):
        """The ``MapDelta`` that takes the front end from the shadow to the
        LoopMap as it stands."""
        from .localmap import MapDelta

        m, g0 = self.map, self.graph
        if len(m.mps) < len(self.mp_index) or m.nkf < len(self.kf_index):
            raise ValueError("the map holds fewer points or keyframes than the front end: not the identity mapping")
        # what the front end will hold: what it holds, then the LoopMap's new points and keyframes in id order
        mp_id = np.concatenate([self.mp_id, np.arange(len(self.mp_index), len(m.mps), dtype=np.int32)])
        kf_id = np.concatenate([self.kf_id, np.arange(len(self.kf_index), m.nkf, dtype=np.int32)])
        g1 = covis_graph_from_loopmap(m) if self._identity else _graph_through(m, mp_id, kf_id)
        n0, n1, k0, k1 = len(self.mp), len(mp_id), len(g0["kf_bad"]), len(kf_id)
        ns0 = int(g0["kf_mp_off"][k0])
        if not np.array_equal(g1["kf_mp_off"][:k0 + 1], g0["kf_mp_off"]):
            raise ValueError("an existing keyframe changed its slot count: not the identity mapping")
        if np.any(g0["mp_bad"].astype(bool) & ~g1["mp_bad"][:n0].astype(bool)) or \
                np.any(g0["kf_bad"].astype(bool) & ~g1["kf_bad"][:k0].astype(bool)):
            raise ValueError("a bad point or keyframe is good again")
        mp1 = np.ascontiguousarray(np.asarray(m.mps)[mp_id], MAP_POINT_DTYPE)
        desc1 = np.ascontiguousarray(np.asarray(m.mp_desc).reshape(-1, 32)[mp_id], np.uint8)
        rows = lambda a: a.view(np.uint8).reshape(len(a), a.dtype.itemsize)  # noqa: E731
        ch = np.nonzero(np.any(rows(mp1[:n0]) != rows(self.mp), axis=1) | np.any(desc1[:n0] != self.desc, axis=1))[0]
        bad_mp = np.nonzero(g1["mp_bad"][:n0].astype(bool) & ~g0["mp_bad"].astype(bool))[0]
        bad_kf = np.nonzero(g1["kf_bad"][:k0].astype(bool) & ~g0["kf_bad"].astype(bool))[0]
        pos = np.nonzero(g1["kf_mp"][:ns0] != g0["kf_mp"][:ns0])[0]
        skf = np.searchsorted(g0["kf_mp_off"], pos, side="right") - 1
        touched = _changed_rows(g1["mp_obs_off"], g1["mp_obs"], g0["mp_obs_off"], g0["mp_obs"], n0)
        o1 = g1["mp_obs_off"]
        grown = n0 + np.nonzero(np.diff(o1[n0:]) > 0)[0]
        obs_rows = {int(p): g1["mp_obs"][o1[p]:o1[p + 1]] for p in np.concatenate([touched, grown])}
        same_cov = (np.array_equal(g1["kf_cov_off"][:k0 + 1], g0["kf_cov_off"]) and
                    np.array_equal(g1["kf_cov"], g0["kf_cov"]) and int(g1["kf_cov_off"][k1]) == len(g0["kf_cov"]))
        co = g1["kf_cov_off"]
        # a stream whose database grows: the new keyframes join it with the graph (KeyFrameDatabase::add)
        db = getattr(self.fe, "_kfdbs", {}).get(self.stream)
        kf_rows = None
        if k1 > k0 and db is not None and db.growable:
            for k in kf_id[k0:]:
                if m.kf_bow[k] is None or m.kf_fv[k] is None:
                    raise ValueError(f"keyframe {k} has no BoW yet: it cannot join the keyframe database")
            kf_rows = [(m.kf_kps[k], m.kf_desc[k], m.kf_bow[k][0], m.kf_bow[k][1], m.kf_fv[k]) for k in kf_id[k0:]]
        d = MapDelta(self.stream, new_mp=mp1[n0:], new_mp_desc=desc1[n0:], new_mp_bad=g1["mp_bad"][n0:],
                     set_mp_idx=ch, set_mp=mp1[ch], set_mp_desc=desc1[ch], bad_mp=bad_mp,
                     new_kf=[g1["kf_mp"][g1["kf_mp_off"][k]:g1["kf_mp_off"][k + 1]] for k in range(k0, k1)],
                     new_kf_bad=g1["kf_bad"][k0:],
                     bad_kf=bad_kf, slot_kf=skf, slot_idx=pos - g0["kf_mp_off"][skf], slot_val=g1["kf_mp"][pos],
                     obs_rows=obs_rows, kf_rows=kf_rows,
                     kf_cov=None if same_cov else [g1["kf_cov"][co[k]:co[k + 1]] for k in range(k1)])
        self._next = dict(mp=mp1.copy(), desc=desc1.copy(), graph=g1, mp_id=mp_id, kf_id=kf_id, n_mp=len(m.mps),
                          n_kf=m.nkf)
        return d

    def commit(self) -> None:
        """The shadow becomes the map of the last :meth:`delta`."""
        if self._next is None:
            raise RuntimeError("no delta to commit")
        nx = self._next
        self.mp, self.desc, self.graph = nx["mp"], nx["desc"], nx["graph"]
        self._set_ids(nx["mp_id"], nx["kf_id"], nx["n_mp"], nx["n_kf"])
        self._next = None

    def discard(self) -> None:
        """Forget the last :meth:`delta` without committing it (it was not sent)."""
        self._next = None

    def _set_ids(self, mp_id, kf_id, n_mp: int, n_kf: int) -> None:
        """The maps from the front end's indices to the LoopMap's ids (of n_mp
        points and n_kf keyframes known so far) and their inverses."""
        self.mp_id, self.kf_id = np.asarray(mp_id, np.int32), np.asarray(kf_id, np.int32)
        self.mp_index, self.kf_index = np.full(n_mp, -1, np.int32), np.full(n_kf, -1, np.int32)
        self.mp_index[self.mp_id] = np.arange(len(self.mp_id), dtype=np.int32)
        self.kf_index[self.kf_id] = np.arange(len(self.kf_id), dtype=np.int32)

    def default_drops(self, keep_kf=None):
        """The default policy on what the front end holds (the shadow), in its
        indices -> (drop_kf, drop_mp): every bad keyframe goes; if more than
        ``keep_kf`` good keyframes remain, the newest keyframe stays, then its
        ordered covisibility list in order, then the rest by recency, up to
        ``keep_kf``; a bad point in no kept keyframe's slot goes, and so does a
        good point that no kept keyframe observes. On a stream with a fixed
        keyframe database attached every keyframe is kept (dropping one is
        refused there), so the request is points-only; a growable database
        follows the graph."""
        g = self.graph
        nkf, n = len(g["kf_bad"]), len(self.mp)
        good = np.nonzero(~g["kf_bad"].astype(bool))[0]
        kept = good
        db = getattr(self.fe, "_kfdbs", {}).get(self.stream)
        if db is not None and not getattr(db, "growable", False):
            # a fixed keyframe database is attached: its keyframes cannot leave (GF_ERR_UNSUPPORTED), points can
            kept = np.arange(nkf)
        elif keep_kf is not None and len(good) > keep_kf:
            newest = int(good[-1])
            cov = g["kf_cov"][g["kf_cov_off"][newest]:g["kf_cov_off"][newest + 1]]
            order = [newest] + [int(c) for c in cov if not g["kf_bad"][c]] + [int(k) for k in good[::-1]]
            kept = np.sort(np.asarray(list(dict.fromkeys(order))[:max(int(keep_kf), 1)], np.int64))
        keep_mask = np.zeros(nkf, bool)
        keep_mask[kept] = True
        srow = np.repeat(np.arange(nkf), np.diff(g["kf_mp_off"]))
        in_slot = np.zeros(n, bool)
        v = g["kf_mp"][keep_mask[srow]]
        in_slot[v[v >= 0]] = True
        orow = np.repeat(np.arange(n), np.diff(g["mp_obs_off"]))
        seen = np.zeros(n, bool)
        seen[orow[keep_mask[g["mp_obs"]]]] = True
        bad = g["mp_bad"].astype(bool)
        drop_mp = np.nonzero((bad & ~in_slot) | (~bad & ~seen))[0]
        return np.nonzero(~keep_mask)[0].astype(np.int32), drop_mp.astype(np.int32)

    def compact(self, drop_kf=None, drop_mp=None, keep_kf=None):
        """Drop keyframes and points (front-end indices; both None: the default
        policy of :meth:`default_drops`) from the front end's map with
        ``FrontEnd.compact_maps``, and apply the returned remaps to the shadow
        and the id maps. What frame state still holds is pinned and stays. The
        LoopMap itself never shrinks. The shadow must be current (no delta
        waiting for its commit). -> the ``localmap.MapRemap``."""
        from .localmap import MapCompact

        if self._next is not None:
            raise RuntimeError("a delta waits for its commit")
        if drop_kf is None and drop_mp is None:
            drop_kf, drop_mp = self.default_drops(keep_kf)
        rm = self.fe.compact_maps([MapCompact(self.stream, drop_kf, drop_mp)])[0]
        if rm.identity():
            return rm
        keep_mp, keep_k = rm.mp_remap >= 0, rm.kf_remap >= 0
        self.mp, self.desc = self.mp[keep_mp], self.desc[keep_mp]
        self.graph = restrict_graph(self.graph, rm.kf_remap, rm.mp_remap)
        self._set_ids(self.mp_id[keep_mp], self.kf_id[keep_k], len(self.mp_index), len(self.kf_index))
        self._identity = False
        return rm


class KeyFrameInserter:
    """The half of ``LocalMapping``'s interface that faces tracking, without
    the thread: ``InsertKeyFrame`` (LocalMapping.cc:149-155), the queue
    ``mlNewKeyFrames`` with ``CheckNewKeyFrames`` (:158-162), ``SetAcceptKeyFrames``
    (:70, :116-117), ``mbAbortBA`` (:98, :100, :153) and ``RequestStop`` /
    ``Release`` (:132-141), between a ``pipeline.FrontEnd`` whose keyframe stage
    is on and one ``LocalMapper`` per stream (a dict or a list; a stream
    without a mapper is left alone).

    point_ids[stream] (optional) maps the front end's map index to the
    mapper's point id (identity by default; -1 stays -1). A stream with a
    ``MapFeedback`` translates through the feedback's ``mp_id`` instead, which
    follows the compactions of the front end's map.

    feedback (optional): a ``MapFeedback`` per stream (a dict or a list) over
    the stream's mapper's map; ``feed_back()`` then carries the mappers' results
    back into the front end's maps. Off without it; a stream with ``point_ids``
    cannot have one (the feedback keeps the id mapping itself)."""

    def __init__(self, fe, mappers, point_ids=None, feedback=None):
        self.fe = fe
        self.mappers = dict(mappers) if isinstance(mappers, dict) else dict(enumerate(mappers))
        self.point_ids = dict(point_ids or {})
        self.queue = {b: [] for b in self.mappers}       # mlNewKeyFrames: keyframe indices
        self.stop_flags = {b: ctypes.c_uint8(0) for b in self.mappers}  # the byte LocalBundleAdjustment polls
        self.stop_requested = {b: False for b in self.mappers}
        self.taken = []  # every keyframe handed over, in order: (stream, keyframe index, header fields)
        fb = feedback or {}
        self.feedback = dict(fb) if isinstance(fb, dict) else dict(enumerate(fb))
        for b in self.feedback:
            if self.point_ids.get(b) is not None:
                raise ValueError(f"stream {b}: map feedback needs the identity id mapping")
        self._ran = set()  # streams whose mapper ran since the last feed_back
        self._parked = set()  # streams poll_resets has reported and start has not started again

    def start(self, stream: int, loopmap, frame_kps, frame_desc, frame_id: int, timestamp: float, since_reloc=None,
              mapper=None, voc=None):
        """Begin ``stream`` on ``loopmap`` (a ``MonoInitializer``'s map, as
        ``create_initial_map`` returns it) while the other streams keep
        running: a ``MapFeedback`` whose shadow is this map, a ``LocalMapper``
        over it (``mapper``, or one made with ``voc``), and the
        ``FrontEnd.start_streams`` call with the initial frame as mLastFrame
        (``MapFeedback.start``). A refused start (GFError) leaves the stream
        and the inserter as they were. mbAcceptKeyFrames of the stream comes
        back afterwards, as LocalMapping::ResetIfRequested leaves an idle
        mapper. -> the ``localmap.StreamStart`` sent."""
        from ._lib import GFError

        stream = int(stream)
        fb = MapFeedback.starting(self.fe, stream, loopmap)
        req = fb.start(frame_kps, frame_desc, frame_id, timestamp, since_reloc)
        self.fe.start_streams([req])
        if mapper is None:
            from .localmapping import LocalMapper

            mapper = LocalMapper(loopmap, voc)
        self.mappers[stream], self.feedback[stream] = mapper, fb
        self.point_ids.pop(stream, None)
        self.queue[stream] = []
        self.stop_flags[stream] = ctypes.c_uint8(0)
        self.stop_requested[stream] = False
        self._ran.discard(stream)
        self._parked.discard(stream)
        try:
            self.fe.set_keyframe_state(stream, accept=1, stop=0)
        except GFError:  # the keyframe stage is off: no words to set
            pass
        return req

    def poll_resets(self) -> list:
        """``FrontEnd.lifecycle()``: every mapped stream that is newly parked
        (state 2: it lost track on a map of at most 5 keyframes, the reset rule
        of Tracking.cc:718-726) loses its mapper, its feedback and its queued
        keyframes (LocalMapping::RequestReset / ResetIfRequested, LocalMapping.cc:625-655). -> their
        indices, for the caller to run a ``MonoInitializer`` on them again and
        :meth:`start` them."""
        st = self.fe.lifecycle()
        out = []
        for b in sorted(set(self.mappers) | set(self.feedback)):
            if int(st[b]) != 2 or b in self._parked:
                continue
            self.mappers.pop(b, None)
            self.feedback.pop(b, None)
            self.point_ids.pop(b, None)
            self.queue.pop(b, None)
            self.stop_flags.pop(b, None)
            self.stop_requested.pop(b, None)
            self._ran.discard(b)
            self._parked.add(b)
            out.append(b)
        return out

    def pump(self) -> list:
        """Take the pending keyframes of the mapped streams' front end, insert
        each into its stream's map and queue it; raise the stop byte of a
        stream whose ABORT word the device set. -> [(stream, keyframe index)]."""
        abort = self.fe.keyframe_state()["abort"]
        for b in self.mappers:
            if abort[b]:
                self.stop_flags[b].value = 1  # mbAbortBA as LocalBundleAdjustment's pbStopFlag sees it
        out = []
        for kf in self.fe.take_keyframes():
            b = kf["stream"]
            if b not in self.mappers:
                continue
            slots = kf["slots"]
            ids = self.feedback[b].mp_id if b in self.feedback else self.point_ids.get(b)
            if ids is not None:
                ids = np.asarray(ids, np.int32)
                slots = np.where(slots >= 0, ids[np.maximum(slots, 0)], -1).astype(np.int32)
            k = self.mappers[b].insert_keyframe(kf["kps"], kf["desc"], slots, kf["Tcw"])
            self.queue[b].append(k)
            self.taken.append((b, k, {x: kf[x] for x in ("seq", "frame_id", "timestamp")}))
            out.append((b, k))
        return out

    def run_mapper(self, stream: int):
        """One pass of LocalMapping::Run's body (:58-124) for the stream's
        oldest queued keyframe -> the ``LocalMapper.step`` report, or None with
        an empty queue. mbAbortBA is cleared first (:98); local BA is skipped
        when more keyframes wait or a stop was requested (:100); ACCEPT comes
        back when the queue is empty (:116-117)."""
        q = self.queue[stream]
        if not q:
            return None
        cur = q.pop(0)
        self.fe.set_keyframe_state(stream, abort=0)
        self.stop_flags[stream].value = 0
        abort_ba = bool(q) or self.stop_requested[stream]
        rep = self.mappers[stream].step(cur, abort_ba=abort_ba, stop_flag=self.stop_flags[stream])
        self._ran.add(stream)
        if not q:
            self.fe.set_keyframe_state(stream, accept=1)
        return rep

    def _passes(self, fb, d, lim) -> bool:
        """The front end's counts after delta ``d`` pass a limit of ``lim``
        (keyframes, points, slots, observations; the nkf^2 covisibility
        capacity cannot be passed below the keyframe limit)."""
        g = fb.graph
        nkf = len(g["kf_bad"]) + len(d.new_kf_off) - 1
        slots = len(g["kf_mp"]) + len(d.new_kf_mp)
        old = np.diff(g["mp_obs_off"])
        obs = len(g["mp_obs"]) + len(d.obs_kf) - int(old[d.obs_mp[d.obs_mp < len(old)]].sum())
        return (nkf > lim["kf"] or len(fb.mp) + len(d.new_mp) > lim["mp"] or slots > lim["slots"] or obs > lim["slots"])

    def feed_back(self, streams=None, compact_at=None) -> list:
        """The maps of the streams whose mapper ran since the last call (or of
        ``streams``) back into the front end: their ``MapFeedback.delta()``s in
        one ``FrontEnd.update_maps`` call, the shadows committed after it. In
        the reference this is no step at all: Tracking reads what LocalMapping
        wrote through its pointers, under the map mutex. -> the deltas sent.

        compact_at (optional): dict(kf=, mp=, slots=, keep_kf=) of limits, each
        defaulting to the front end's capacity (64 keyframes, map_cap points,
        64 x keypoint-capacity slots and observations). A stream whose delta
        would pass one is compacted first (``MapFeedback.compact`` with the
        default policy and ``keep_kf``, by default half the keyframe limit),
        and its delta is taken again through the new id maps."""
        which = sorted(self._ran if streams is None else streams)
        fbs = [self.feedback[b] for b in which if b in self.feedback]
        deltas = [fb.delta() for fb in fbs]
        if compact_at is not None:
            lim = dict(kf=64, mp=self.fe.M, slots=64 * self.fe.cap)
            lim.update({k: v for k, v in compact_at.items() if k != "keep_kf"})
            for i, fb in enumerate(fbs):
                if self._passes(fb, deltas[i], lim):
                    fb.discard()  # the delta is taken again after the compaction
                    fb.compact(keep_kf=compact_at.get("keep_kf", max(lim["kf"] // 2, 1)))
                    deltas[i] = fb.delta()
        live = [(fb, d) for fb, d in zip(fbs, deltas) if not d.empty()]
        if live:
            self.fe.update_maps([d for _, d in live])
        for fb in fbs:
            fb.commit()
        self._ran -= set(which)
        return [d for _, d in live]

    def request_stop(self, stream: int) -> None:
        """LocalMapping::RequestStop (:132-135): the stream inserts no keyframe
        (Tracking.cc:3042) and its next mapper pass skips local BA."""
        self.stop_requested[stream] = True
        self.fe.set_keyframe_state(stream, stop=1)

    def release(self, stream: int) -> None:
        """LocalMapping::Release (:138-141)."""
        self.stop_requested[stream] = False
        self.fe.set_keyframe_state(stream, stop=0)

    def loop_corrected(self, stream: int, last_kf=None) -> int:
        """The arrow from the loop closer to the tracker
        (``mpTracker->ForceRelocalisation()``, LoopClosing.cc:554): the
        stream's corrected map goes to the front end (``feed_back([stream])``:
        every moved, replaced and bad point, the slot writes, the changed
        observation rows and covisibility lists), then
        ``FrontEnd.force_relocalisation`` makes the stream's next step
        relocalise against the local window around ``last_kf``, a keyframe id
        of the stream's ``LoopMap`` (mpLastKeyFrame; default: the highest id
        the front end holds that is not bad), translated through the
        feedback's ``kf_index``. A refused update (GFError) sends no request.
        -> the graph keyframe index sent."""
        stream = int(stream)
        fb = self.feedback[stream]
        self.feed_back([stream])
        m = fb.map
        if last_kf is None:
            held = [int(k) for k in fb.kf_id if not m.kf_bad[int(k)]]
            if not held:
                raise ValueError(f"stream {stream}: the front end holds no good keyframe of the map")
            last_kf = max(held)
        last_kf = int(last_kf)
        if not 0 <= last_kf < len(fb.kf_index) or fb.kf_index[last_kf] < 0:
            raise ValueError(f"stream {stream}: the front end does not hold keyframe {last_kf}")
        idx = int(fb.kf_index[last_kf])
        self.fe.force_relocalisation([stream], [idx])
        return idx

    def correct_loop(self, stream: int, cur_kf, matched_kf, gScw, current_matched_points, loop_points, last_kf=None,
                     ctx=None) -> dict:
        """LoopClosing::CorrectLoop (LoopClosing.cc:426-560) for a tracked
        stream: ``request_stop`` (:430), ``sim3.correct_loop`` on the stream's
        mapper's map, :meth:`loop_corrected`, ``release`` (:559). The reference
        raises the flag before OptimizeEssentialGraph while its tracker runs on
        a thread of its own; here the whole correction is applied before the
        next step sees any of it. -> ``sim3.correct_loop``'s report."""
        from . import sim3

        stream = int(stream)
        self.request_stop(stream)
        try:
            rep = sim3.correct_loop(self.mappers[stream].map, cur_kf, matched_kf, gScw, current_matched_points,
                                    loop_points, ctx)
            self.loop_corrected(stream, last_kf)
        finally:
            self.release(stream)
        return rep
