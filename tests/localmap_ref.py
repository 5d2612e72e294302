"""ctypes wrapper of tests/helpers/liblocalmapref.so, the serial CPU restatement
of LocalMapping::CreateNewMapPoints (tests/helpers/localmap_ref.cpp), and the
neighbour loop around it: set-up, the CPU oracle's SearchForTriangulation,
the per-match body with its slot updates, then the reference's bookkeeping."""
from __future__ import annotations

import ctypes
import os

import numpy as np

import oracle_lib as O
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

EXITS = ("parallax", "w0", "z1", "z2", "reproj1", "reproj2", "dist0", "scale", "accepted")
X = {n: i for i, n in enumerate(EXITS)}
STATUS = ("ok", "baseline", "nodepth")
NEWPOINT_DTYPE = np.dtype([("neighbour", np.int32), ("idx1", np.int32), ("idx2", np.int32), ("pos", np.float32, 3)])
CULL = ("kept", "erased_bad", "bad_ratio", "bad_obs", "erased_old")


class Camera(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("scale_factor", ctypes.c_float), ("nlevels", ctypes.c_int32)]

    @classmethod
    def of(cls, info):
        return cls(info.fx, info.fy, info.cx, info.cy, info.scale_factor, info.nlevels)


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "liblocalmapref.so"))
        _lib.lm_median_of.restype = ctypes.c_float
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _T(T):
    return np.ascontiguousarray(T, np.float32).reshape(16)


def svd4(A):
    """cv::SVD::compute of a 4x4 CV_32F -> (w, vt)."""
    A = np.ascontiguousarray(A, np.float32).reshape(16)
    w, vt = np.zeros(4, np.float32), np.zeros(16, np.float32)
    lib().lm_svd4(_p(A), _p(w), _p(vt))
    return w, vt.reshape(4, 4)


def compute_f12(info, T1, T2):
    F = np.zeros(9, np.float32)
    cam, a, b = Camera.of(info), _T(T1), _T(T2)
    lib().lm_compute_f12(ctypes.byref(cam), _p(a), _p(b), _p(F))
    return F.reshape(3, 3)


def median_depth(Tcw, slots, mp_pos):
    """ComputeSceneMedianDepth(2) -> (the depth list in slot order, the median or None)."""
    s = np.ascontiguousarray(slots, np.int32)
    pos = np.ascontiguousarray(mp_pos, np.float32).reshape(-1, 3)
    d, med, T = np.zeros(max(len(s), 1), np.float32), ctypes.c_float(), _T(Tcw)
    n = lib().lm_median_depth(_p(T), _p(s), len(s), _p(pos), len(pos), _p(d), ctypes.byref(med))
    return d[:n].copy(), (np.float32(med.value) if n else None)


def median_of(depths):
    d = np.ascontiguousarray(depths, np.float32)
    return np.float32(lib().lm_median_of(_p(d), len(d)))


def setup(info, T1, T2, slots2, mp_pos):
    """:270-284 for one neighbour -> (status, F12 [3, 3], median depth)."""
    s = np.ascontiguousarray(slots2, np.int32)
    pos = np.ascontiguousarray(mp_pos, np.float32).reshape(-1, 3)
    F, med, cam, a, b = np.zeros(9, np.float32), ctypes.c_float(), Camera.of(info), _T(T1), _T(T2)
    st = lib().lm_setup(ctypes.byref(cam), _p(a), _p(b), _p(s), len(s), _p(pos), len(pos), _p(F), ctypes.byref(med))
    return st, F.reshape(3, 3), np.float32(med.value)


def match_body(info, T1, T2, kp1, kp2):
    """One match of :307-390 -> (exit, x3D)."""
    k1 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE).reshape(1)
    k2 = np.ascontiguousarray(kp2, KEYPOINT_DTYPE).reshape(1)
    x, cam, a, b = np.zeros(3, np.float32), Camera.of(info), _T(T1), _T(T2)
    e = lib().lm_match_body(ctypes.byref(cam), _p(a), _p(b), _p(k1), _p(k2), _p(x))
    return e, x


def triangulate(info, T1, T2, kps1, kps2, matches12, neighbour, slots1, slots2, next_id):
    """:307-407 for one neighbour; slots1 / slots2 are updated in place.
    -> (records, exits [n1], nmatches)."""
    k1, k2 = np.ascontiguousarray(kps1, KEYPOINT_DTYPE), np.ascontiguousarray(kps2, KEYPOINT_DTYPE)
    m = np.ascontiguousarray(matches12, np.int32)
    assert slots1.dtype == np.int32 and slots2.dtype == np.int32 and slots1.flags.c_contiguous
    exits = np.full(max(len(k1), 1), -1, np.int32)
    out = np.zeros(max(len(k1), 1), NEWPOINT_DTYPE)
    nm, cam, a, b = ctypes.c_int(), Camera.of(info), _T(T1), _T(T2)
    na = lib().lm_triangulate(ctypes.byref(cam), _p(a), _p(b), _p(k1), len(k1), _p(k2), len(k2), _p(m), int(neighbour),
                              _p(slots1), _p(slots2), int(next_id), _p(exits), _p(out), ctypes.byref(nm))
    return out[:na].copy(), exits[:len(k1)].copy(), nm.value


def create_new_map_points(scene, chain=1, check_ori=False):
    """The neighbour loop of CreateNewMapPoints on a scene of
    localmap_scenes.scene(): chain=1 is the reference (every neighbour is
    matched against the slot table the previous ones left); chain=0 matches
    every neighbour against the starting table of the new keyframe (the slot
    writes still happen). -> dict status, F12, median, nmatches, naccepted
    (per neighbour), exits [nneigh, n1], points (records in creation order),
    slots (the final tables of every keyframe)."""
    info, cur, neigh = scene["info"], scene["cur"], scene["neighbours"]
    slots = [s.copy() for s in scene["slots"]]
    start1 = slots[cur].copy()
    nmp = len(scene["mps"])
    pos = np.ascontiguousarray(scene["mps"]["pos"], np.float32)
    kps, desc, fv, Tcw = scene["kps"], scene["desc"], scene["fv"], scene["Tcw"]
    n1 = len(kps[cur])
    sigma2 = (info.scale_factors() * info.scale_factors()).astype(np.float32)
    rep = dict(status=[], F12=[], median=[], nmatches=[], naccepted=[])
    exits = np.full((len(neigh), n1), -1, np.int32)
    points = []
    total = 0
    side = lambda k, s: ((fv[k].nodes, fv[k].start, fv[k].feats), desc[k], kps[k], s)  # noqa: E731
    for i, k2 in enumerate(neigh):
        st, F, med = setup(info, Tcw[cur], Tcw[k2], slots[k2], pos)
        rep["status"].append(st)
        rep["F12"].append(F)
        rep["median"].append(med)
        if st != 0:
            rep["nmatches"].append(0)
            rep["naccepted"].append(0)
            continue
        _, m12 = O.search_triangulation(check_ori, side(cur, slots[cur] if chain else start1), side(k2, slots[k2]), F,
                                        sigma2)
        recs, ex, nm = triangulate(info, Tcw[cur], Tcw[k2], kps[cur], kps[k2], m12, i, slots[cur], slots[k2],
                                   nmp + total)
        exits[i] = ex
        points.append(recs)
        total += len(recs)
        rep["nmatches"].append(nm)
        rep["naccepted"].append(len(recs))
    rep = {k: np.asarray(v) for k, v in rep.items()}
    rep["F12"] = rep["F12"].astype(np.float32).reshape(-1, 3, 3)
    rep["median"] = rep["median"].astype(np.float32)
    pts = np.concatenate(points) if points else np.zeros(0, NEWPOINT_DTYPE)
    return dict(rep, exits=exits, points=pts, slots=slots)


def bookkeeping(scene, res):
    """:393-406 on the restatement's world after create_new_map_points: the
    observations of the new points (kf2 first, then the new keyframe), their
    descriptors (ComputeDistinctiveDescriptors on the CPU oracle, rows in
    keyframe-index order), their normal and depth (the loop-fusion
    restatement's UpdateNormalAndDepth) and the recent list.
    -> dict ids, obs_rows, mp_desc, geometry [n, 8], recent."""
    import loopfuse_ref as LF
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE

    cur, neigh, pts = scene["cur"], scene["neighbours"], res["points"]
    nmp, n = len(scene["mps"]), len(res["points"])
    ids = np.arange(nmp, nmp + n, dtype=np.int32)
    mps = np.zeros(nmp + n, MAP_POINT_DTYPE)
    mps[:nmp] = scene["mps"]
    mps["pos"][nmp:] = pts["pos"]
    mp_desc = np.zeros((nmp + n, 32), np.uint8)
    mp_desc[:nmp] = scene["mp_desc"]
    obs = [dict(o) for o in scene["obs"]] + [{int(neigh[r["neighbour"]]): int(r["idx2"]), cur: int(r["idx1"])}
                                            for r in pts]
    rows, offs = [], [0]
    for o in obs[nmp:]:
        rows += [scene["desc"][kf][o[kf]] for kf in sorted(o)]
        offs.append(len(rows))
    if n:
        mp_desc[nmp:] = O.distinctive_descriptors(np.asarray(rows, np.uint8), np.asarray(offs, np.int32))[1]
    world = LF.RefMap(scene["info"], scene["kps"], scene["desc"], res["slots"], mps, mp_desc, observations=obs)
    for k, T in enumerate(scene["Tcw"]):
        world.set_pose(k, T)
    for p in range(nmp):
        world.set_ref(p, int(scene["ref_kf"][p]))
    for p in ids:
        world.set_ref(int(p), cur)
    world.update_normal_and_depth(ids)
    return dict(ids=ids, obs_rows=world.observation_rows(), mp_desc=mp_desc, geometry=world.geometry(),
                recent=[int(p) for p in ids])


def map_point_culling(bad, found, visible, first_kf_id, nobs, cur_kf_id):
    """MapPointCulling over a recent list given as arrays -> action per entry (CULL)."""
    c = np.ascontiguousarray
    b, f, v = c(np.asarray(bad).astype(np.uint8)), c(found, np.int32), c(visible, np.int32)
    k, o = c(first_kf_id, np.int64), c(nobs, np.int32)
    act = np.zeros(max(len(b), 1), np.int32)
    lib().lm_map_point_culling(len(b), _p(b), _p(f), _p(v), _p(k), _p(o), ctypes.c_int64(int(cur_kf_id)), _p(act))
    return act[:len(b)]
