"""ctypes wrapper of tests/helpers/libinitmapref.so: the serial CPU restatement
of Tracking::CreateInitialMap around the solver (tests/helpers/initmap_ref.cpp).
``points`` is everything before the bundle adjustment, ``finish`` everything
after it; ``create`` chains them through the CPU oracle's BundleAdjustment
(``oracle_lib.local_ba(p, its=(20, 0))``)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
OK, NOT_INITIALIZED, RESET_DEPTH, RESET_FEW = 0, 1, 2, 3


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libinitmapref.so"))
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def points(info, kps1, desc1, kps2, desc2, matches12, init, p3d, tri) -> dict:
    """Stage 1 for one problem. init: one INIT_RESULT_DTYPE record. -> dict
    with status, npts, pt_kp, mps, mp_desc, slots1, slots2 and ``ba``, the
    gf_ba_problem arrays."""
    k1, k2 = np.ascontiguousarray(kps1, KEYPOINT_DTYPE), np.ascontiguousarray(kps2, KEYPOINT_DTYPE)
    n1, n2 = len(k1), len(k2)
    d1 = np.ascontiguousarray(desc1, np.uint8).reshape(n1, 32)
    d2 = np.ascontiguousarray(desc2, np.uint8).reshape(n2, 32)
    m = np.ascontiguousarray(matches12, np.int32).reshape(n1)
    X = np.ascontiguousarray(p3d, np.float32).reshape(n1, 3)
    t = np.ascontiguousarray(np.asarray(tri).astype(np.uint8)).reshape(n1)
    r = np.asarray(init).reshape(-1)[0]
    R21, t21 = np.ascontiguousarray(r["R21"], np.float32), np.ascontiguousarray(r["t21"], np.float32)
    cam = np.array([info.fx, info.fy, info.cx, info.cy], np.float32)
    c = max(n1, 1)
    status = np.zeros(1, np.int32)
    pt_kp, mps, mp_desc = np.full((c, 2), -9, np.int32), np.zeros(c, MAP_POINT_DTYPE), np.zeros((c, 32), np.uint8)
    s1, s2 = np.full(max(n1, 1), -9, np.int32), np.full(max(n2, 1), -9, np.int32)
    kf_Tcw, kf_kind, kf_cam = np.zeros((2, 4, 4), np.float32), np.zeros(2, np.uint8), np.zeros((2, 4), np.float32)
    pt_pos = np.zeros((c, 3), np.float32)
    e_pt, e_kf = np.zeros(2 * c, np.int32), np.zeros(2 * c, np.int32)
    e_z, e_w = np.zeros((2 * c, 2), np.float32), np.zeros(2 * c, np.float32)
    n = lib().imr_points(_p(cam), int(info.nlevels), ctypes.c_float(info.scale_factor), _p(k1), _p(d1), n1, _p(k2),
                         _p(d2), n2, _p(m), int(r["ok"]), _p(R21), _p(t21), _p(X), _p(t), _p(status), _p(pt_kp),
                         _p(mps), _p(mp_desc), _p(s1), _p(s2), _p(kf_Tcw), _p(kf_kind), _p(kf_cam), _p(pt_pos),
                         _p(e_pt), _p(e_kf), _p(e_z), _p(e_w))
    ba = dict(kf_Tcw=kf_Tcw.reshape(2, 16), kf_kind=kf_kind, kf_cam=kf_cam, pt_pos=pt_pos[:n], edge_pt=e_pt[:2 * n],
              edge_kf=e_kf[:2 * n], edge_z=e_z[:2 * n], edge_inv_sigma2=e_w[:2 * n])
    return dict(status=int(status[0]), npts=n, pt_kp=pt_kp[:n], mps=mps[:n], mp_desc=mp_desc[:n], slots1=s1[:n1],
                slots2=s2[:n2], ba=ba, kps1=k1, kps2=k2)


def finish(info, st1: dict, ba_Tcw, ba_pos, thres: int = 100) -> dict:
    """Stage 2 on the result of :func:`points` and the solver's output."""
    if st1["status"] == NOT_INITIALIZED:
        return dict(status=NOT_INITIALIZED, npts=0, tracked=0, median=np.float32(0), Tcw=st1["ba"]["kf_Tcw"].reshape(2, 4, 4),
                    mps=np.zeros(0, MAP_POINT_DTYPE))
    n = st1["npts"]
    T = np.ascontiguousarray(ba_Tcw, np.float32).reshape(2, 16)
    X = np.ascontiguousarray(np.asarray(ba_pos, np.float32).reshape(-1, 3)[:n])
    if not n:
        X = np.zeros((1, 3), np.float32)
    k1, k2 = st1["kps1"], st1["kps2"]
    pk = np.ascontiguousarray(st1["pt_kp"], np.int32) if n else np.zeros((1, 2), np.int32)
    s1 = np.ascontiguousarray(st1["slots1"], np.int32) if len(k1) else np.zeros(1, np.int32)
    s2 = np.ascontiguousarray(st1["slots2"], np.int32) if len(k2) else np.zeros(1, np.int32)
    tracked, median = np.zeros(1, np.int32), np.zeros(1, np.float32)
    Tout, mps = np.zeros((2, 4, 4), np.float32), np.zeros(max(n, 1), MAP_POINT_DTYPE)
    kk1 = k1 if len(k1) else np.zeros(1, KEYPOINT_DTYPE)
    kk2 = k2 if len(k2) else np.zeros(1, KEYPOINT_DTYPE)
    st = lib().imr_finish(int(info.nlevels), ctypes.c_float(info.scale_factor), _p(kk1), len(k1), _p(kk2), len(k2), n,
                          _p(pk), _p(s1), _p(s2), _p(T), _p(X), int(thres), _p(tracked), _p(median), _p(Tout), _p(mps))
    return dict(status=int(st), npts=n, tracked=int(tracked[0]), median=median[0], Tcw=Tout, mps=mps[:n])


def oracle_ba(ba: dict, iterations: int = 20):
    """Optimizer::BundleAdjustment on the CPU oracle: optimize(iterations) then
    optimize(0) -> (kf_Tcw, pt_pos, iterations run)."""
    import oracle_lib as O

    T, X, _, its = O.local_ba(ba, its=(iterations, 0))
    return T, X, its[0]


def create(info, kps1, desc1, kps2, desc2, matches12, init, p3d, tri, thres: int = 100):
    """Restatement + oracle BA end to end -> (stage-1 dict, stage-2 dict with
    ``ba_iterations`` and the unscaled ``ba_Tcw`` / ``ba_pos``)."""
    a = points(info, kps1, desc1, kps2, desc2, matches12, init, p3d, tri)
    if a["status"] == NOT_INITIALIZED:
        return a, finish(info, a, None, None, thres)
    T, X, it = oracle_ba(a["ba"])
    b = finish(info, a, T, X, thres)
    b.update(ba_iterations=it, ba_Tcw=T, ba_pos=X)
    return a, b
