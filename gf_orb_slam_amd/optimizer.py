"""Host-side mirror of ORB_SLAM::Optimizer::PoseOptimization (include/Optimizer.h:53,
src/Optimizer.cc:279-413) over libgfslam's C-ABI. The LM runs on the GPU
(csrc/poseopt.hip); this module only packs the Frame's matched keypoints into
edges and writes the results back, as the reference does.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, lib, ptr
from .orb import default_context

POSE_EDGE_DTYPE = np.dtype([("X", "<f4", 3), ("z", "<f4", 2), ("inv_sigma2", "<f4")])
assert POSE_EDGE_DTYPE.itemsize == 24


def inv_level_sigma2(nlevels: int = 8, scale_factor: float = 1.2) -> np.ndarray:
    """Frame::mvInvLevelSigma2 = 1 / (scale^level)^2 in float (ORBextractor.cc:443-452)."""
    s = [np.float32(1.0)]
    for _ in range(1, nlevels):
        s.append(np.float32(s[-1] * np.float32(scale_factor)))
    s = np.array(s, np.float32)
    return (np.float32(1.0) / (s * s)).astype(np.float32)


class Optimizer:
    @staticmethod
    def PoseOptimization(pFrame, map_pos: np.ndarray | None = None, ctx=None) -> int:
        """Motion-only BA of pFrame.mTcw against its matched map points.

        Edges are the keypoints with mvpMapPoints[i] >= 0, in keypoint order.
        Map-point world positions come from map_pos[mvpMapPoints[i]] when given,
        else from pFrame.mp_pos[i]. Updates pFrame.mTcw and pFrame.mvbOutlier
        (matched keypoints only) and returns the number of inliers.
        """
        ctx = ctx or default_context()
        idx = np.nonzero(pFrame.mvpMapPoints >= 0)[0]
        n = len(idx)
        edges = np.zeros(max(n, 1), POSE_EDGE_DTYPE)
        if n:
            mp = pFrame.mvpMapPoints[idx]
            edges["X"][:n] = (np.asarray(map_pos, np.float32)[mp] if map_pos is not None else pFrame.mp_pos[idx])
            kps = pFrame.mvKeysUn[idx]
            edges["z"][:n, 0] = kps["x"]
            edges["z"][:n, 1] = kps["y"]
            invs = inv_level_sigma2(pFrame.info.nlevels, pFrame.info.scale_factor)
            edges["inv_sigma2"][:n] = invs[kps["octave"]]
        Tin = np.ascontiguousarray(pFrame.mTcw, np.float32)
        Tout = np.zeros((4, 4), np.float32)
        outl = np.zeros(max(n, 1), np.uint8)
        ninl = ctypes.c_int32()
        fi = pFrame.info
        check(lib().gf_pose_opt(ctx.handle, ptr(Tin), ptr(edges), n, ctypes.c_float(fi.fx), ctypes.c_float(fi.fy),
                                ctypes.c_float(fi.cx), ctypes.c_float(fi.cy), ptr(Tout), ptr(outl),
                                ctypes.byref(ninl), None))
        pFrame.mTcw = Tout
        if n:
            pFrame.mvbOutlier[idx] = outl[:n]
        return int(ninl.value)

    @staticmethod
    def pose_opt_edges(Tcw, edges: np.ndarray, fx, fy, cx, cy, ctx=None):
        """Raw edge-list form: returns (Tcw_out, outlier[n], ninliers, iterations)."""
        ctx = ctx or default_context()
        edges = np.ascontiguousarray(edges, POSE_EDGE_DTYPE)
        n = len(edges)
        Tin = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4)
        Tout = np.zeros((4, 4), np.float32)
        outl = np.zeros(max(n, 1), np.uint8)
        ninl, iters = ctypes.c_int32(), ctypes.c_int32()
        check(lib().gf_pose_opt(ctx.handle, ptr(Tin), ptr(edges) if n else None, n, ctypes.c_float(fx),
                                ctypes.c_float(fy), ctypes.c_float(cx), ctypes.c_float(cy), ptr(Tout), ptr(outl),
                                ctypes.byref(ninl), ctypes.byref(iters)))
        return Tout, outl[:n].copy(), int(ninl.value), int(iters.value)

    @staticmethod
    def pose_opt_batch_dev(d_Tcw, d_edges, d_nedges, edge_stride: int, fx, fy, cx, cy, d_outlier, d_ninliers,
                           d_iterations=None, ctx=None, stream=None) -> None:
        """Batched device form: torch tensors (or raw pointers) already on the GPU."""
        ctx = ctx or default_context()
        nprob = int(d_nedges.numel()) if hasattr(d_nedges, "numel") else int(len(d_nedges))
        check(lib().gf_pose_opt_batch_dev(ctx.handle, nprob, ptr(d_Tcw), ptr(d_edges), ptr(d_nedges),
                                          int(edge_stride), ctypes.c_float(fx), ctypes.c_float(fy),
                                          ctypes.c_float(cx), ctypes.c_float(cy), ptr(d_outlier), ptr(d_ninliers),
                                          ptr(d_iterations), stream if stream is not None else ctx.stream))

    @staticmethod
    def OptimizeSim3(kf1, kf2, matches1, S12, mp_pos, mp_bad=None, th2=10, ctx=None):
        """Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2)
        (Optimizer.cc:2019-2215). kf1 / kf2: ``sim3.Sim3KeyFrame``; matches1:
        per KF1 keypoint the id of the KF2 map point matched to it (-1 = NULL);
        S12: the estimate, ``(s, R, t)`` as the Sim3Solver hands it over (float;
        the quaternion is Quaterniond(Matrix3d) of R, as ``g2o::Sim3(R, t, s)``
        builds it) or the 8 doubles ``qx qy qz qw tx ty tz s`` of a g2o::Sim3;
        mp_pos: [n_mp, 3] world positions; mp_bad: isBad(). The pair list is
        the reference's (:2072-2111): pairs with a NULL or bad point or with
        ``GetIndexInKeyFrame(pKF2) < 0`` are skipped and keep their match.
        -> (nIn, S12 as 8 doubles, matches1 with the rejected matches cleared)."""
        from .sim3 import _to_camera

        m1 = np.asarray(matches1, np.int32).copy()
        mp_pos = np.asarray(mp_pos, np.float32).reshape(-1, 3)
        bad = np.zeros(len(mp_pos), bool) if mp_bad is None else np.asarray(mp_bad, bool)
        idx, X1, X2, z1, z2, w1, w2 = [], [], [], [], [], [], []
        for i in range(len(m1)):
            mp2 = int(m1[i])
            if mp2 < 0:
                continue
            mp1 = int(kf1.mp_ids[i])
            i2 = kf2.index_of(mp2)
            if mp1 < 0 or bad[mp1] or bad[mp2] or i2 < 0:
                continue
            idx.append(i)
            X1.append(_to_camera(kf1.Tcw, mp_pos[mp1]))
            X2.append(_to_camera(kf2.Tcw, mp_pos[mp2]))
            z1.append((kf1.kps["x"][i], kf1.kps["y"][i]))
            z2.append((kf2.kps["x"][i2], kf2.kps["y"][i2]))
            # invSigma2 of KF1's level; sigma2 of KF2's: GetSigma2 at :2140
            w1.append(np.float32(1.0) / np.float32(kf1.level_sigma2[kf1.kps["octave"][i]]))
            w2.append(np.float32(kf2.level_sigma2[kf2.kps["octave"][i2]]))
        nin, S, inl, _ = Optimizer.optimize_sim3_pairs(X1, X2, z1, z2, w1, w2, kf1.K, kf2.K, S12, th2, ctx)
        m1[np.asarray(idx, np.int64)[~inl.astype(bool)]] = -1
        return nin, S, m1

    @staticmethod
    def optimize_sim3_pairs(X1, X2, z1, z2, w1, w2, K1, K2, S12, th2=10, ctx=None):
        """Raw pair-list form of OptimizeSim3 over ``gf_optimize_sim3`` (see
        abi.h for the arrays). -> (nIn, S12 as 8 doubles, inlier[n], stats[4] =
        iterations of the two rounds, LM trials of the two)."""
        ctx = ctx or default_context()
        c = lambda a, k: np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, k))  # noqa: E731
        X1, X2, z1, z2 = c(X1, 3), c(X2, 3), c(z1, 2), c(z2, 2)
        w1, w2 = np.ascontiguousarray(w1, np.float32).reshape(-1), np.ascontiguousarray(w2, np.float32).reshape(-1)
        n = len(X1)
        assert len(X2) == len(z1) == len(z2) == len(w1) == len(w2) == n
        S = sim3_to_g2o(S12)
        inl = np.zeros(max(n, 1), np.uint8)
        nin = ctypes.c_int32()
        stats = np.zeros(4, np.int32)
        # held in names: a temporary would be freed before the call reads it
        k1 = np.ascontiguousarray(K1, np.float32).reshape(4)
        k2 = np.ascontiguousarray(K2, np.float32).reshape(4)
        p = (lambda a: ptr(a) if n else None)
        check(lib().gf_optimize_sim3(ctx.handle, n, p(X1), p(X2), p(z1), p(z2), p(w1), p(w2), ptr(k1), ptr(k2),
                                     ctypes.c_float(th2), ptr(S), p(inl), ctypes.byref(nin), ptr(stats)))
        return int(nin.value), S, inl[:n].copy(), stats

    @staticmethod
    def optimize_sim3_batch_dev(d_X1, d_X2, d_z1, d_z2, d_w1, d_w2, d_offsets, d_K, d_th2, d_S12, d_inlier, d_nin,
                                d_stats=None, ctx=None, stream=None) -> None:
        """Ragged batched device form (``gf_optimize_sim3_dev``): torch tensors
        (or raw pointers) already on the GPU; problem p's pairs are rows
        [d_offsets[p], d_offsets[p + 1])."""
        ctx = ctx or default_context()
        nprob = (int(d_nin.numel()) if hasattr(d_nin, "numel") else int(len(d_nin)))
        check(lib().gf_optimize_sim3_dev(ctx.handle, nprob, ptr(d_X1), ptr(d_X2), ptr(d_z1), ptr(d_z2), ptr(d_w1),
                                         ptr(d_w2), ptr(d_offsets), ptr(d_K), ptr(d_th2), ptr(d_S12), ptr(d_inlier),
                                         ptr(d_nin), ptr(d_stats), stream if stream is not None else ctx.stream))

    @staticmethod
    def OptimizeEssentialGraph(map, loop_kf, cur_kf, Scurw, NonCorrectedSim3, CorrectedSim3, LoopConnections,
                               ctx=None) -> dict:
        """Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, Scurw,
        NonCorrectedSim3, CorrectedSim3, LoopConnections) (Optimizer.cc:1768-2017)
        on the GPU (csrc/essgraph.hip). Arguments keep the reference's meaning
        (``EssGraphArrays`` for the containers; Scurw is unused, as in the
        reference). -> dict: Tcw [N, 4, 4], pos [M, 3], iterations, trials,
        stop, chi2_initial, chi2_final and the trial trace."""
        ctx = ctx or default_context()
        arr = EssGraphArrays(map, loop_kf, cur_kf, NonCorrectedSim3, CorrectedSim3, LoopConnections)
        check(lib().gf_optimize_essential_graph(ctx.handle, ctypes.byref(arr.problem), ctypes.byref(arr.result)))
        return arr.out()


def quat_from_R(R) -> np.ndarray:
    """Eigen's Quaterniond(Matrix3d) (the trace-branch algorithm, no
    normalisation) of a rotation given in any float type -> (x, y, z, w)."""
    m = np.asarray(R, np.float64).reshape(3, 3)
    t = m[0, 0] + (m[1, 1] + m[2, 2])
    q = np.zeros(4, np.float64)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def sim3_to_g2o(S12) -> np.ndarray:
    """``(s, R, t)`` (g2o::Sim3(Matrix3d, Vector3d, double) of the float values)
    or 8 doubles -> qx qy qz qw tx ty tz s as a fresh float64 array."""
    if isinstance(S12, (tuple, list)) and len(S12) == 3:
        s, R, t = S12
        out = np.zeros(8, np.float64)
        out[:4] = quat_from_R(np.asarray(R, np.float32))
        out[4:7] = np.asarray(t, np.float32).reshape(3).astype(np.float64)
        out[7] = np.float64(np.float32(s))
        return out
    return np.ascontiguousarray(S12, np.float64).reshape(8).copy()


def _quat_rotate(q, v):
    """Eigen's quaternion * vector: v + w*uv + q x uv with uv = 2 (q x v)."""
    x, y, z, w = (float(c) for c in q)
    uv = [y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]]
    uv = [u + u for u in uv]
    c = [y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]]
    return [v[0] + w * uv[0] + c[0], v[1] + w * uv[1] + c[1], v[2] + w * uv[2] + c[2]]


def sim3_mul(A, B) -> np.ndarray:
    """g2o::Sim3::operator* (sim3.h:266-272) on two 8-double similarities."""
    ax, ay, az, aw = (float(c) for c in A[:4])
    bx, by, bz, bw = (float(c) for c in B[:4])
    out = np.zeros(8, np.float64)
    out[0] = aw * bx + ax * bw + ay * bz - az * by
    out[1] = aw * by + ay * bw + az * bx - ax * bz
    out[2] = aw * bz + az * bw + ax * by - ay * bx
    out[3] = aw * bw - ax * bx - ay * by - az * bz
    rt = _quat_rotate(A[:4], [float(c) for c in B[4:7]])
    s = float(A[7])
    for i in range(3):
        out[4 + i] = s * rt[i] + float(A[4 + i])
    out[7] = s * float(B[7])
    return out


def sim3_from_g2o(S) -> tuple:
    """8 doubles -> (s, R [3, 3], t [3]) in double: Quaterniond::toRotationMatrix."""
    x, y, z, w = (float(v) for v in S[:4])
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, 1 - (txx + tyy)]], np.float64)
    return float(S[7]), R, np.asarray(S[4:7], np.float64).copy()


# ---------------------------------------------------------------- local BA (B1)
BA_LOCAL, BA_LOCAL_FIXED, BA_FIXED = 0, 1, 2


class BAProblem(ctypes.Structure):
    """gf_ba_problem (include/gfslam/abi.h): the graph LocalBundleAdjustment builds."""

    _fields_ = [("nkf", ctypes.c_int32), ("npts", ctypes.c_int32), ("nedges", ctypes.c_int32),
                ("kf_Tcw", ctypes.c_void_p), ("kf_kind", ctypes.c_void_p), ("kf_cam", ctypes.c_void_p),
                ("pt_pos", ctypes.c_void_p), ("edge_pt", ctypes.c_void_p), ("edge_kf", ctypes.c_void_p),
                ("edge_z", ctypes.c_void_p), ("edge_inv_sigma2", ctypes.c_void_p)]


class BAResult(ctypes.Structure):
    _fields_ = [("kf_Tcw", ctypes.c_void_p), ("pt_pos", ctypes.c_void_p), ("edge_outlier", ctypes.c_void_p),
                ("iterations", ctypes.c_int32 * 2)]


_BA_FIELDS = (("kf_Tcw", np.float32), ("kf_kind", np.uint8), ("kf_cam", np.float32), ("pt_pos", np.float32),
              ("edge_pt", np.int32), ("edge_kf", np.int32), ("edge_z", np.float32),
              ("edge_inv_sigma2", np.float32))


class BAArrays:
    """Keeps the numpy arrays of one problem alive next to its ctypes views."""

    def __init__(self, prob: dict):
        self.a = {k: np.ascontiguousarray(prob[k], dt) for k, dt in _BA_FIELDS}
        self.nkf, self.npts, self.nedges = len(self.a["kf_kind"]), len(self.a["pt_pos"]), len(self.a["edge_pt"])
        self.problem = BAProblem(self.nkf, self.npts, self.nedges,
                                 *[self.a[k].ctypes.data if self.a[k].size else None for k, _ in _BA_FIELDS])
        self.kf_Tcw = np.zeros((self.nkf, 4, 4), np.float32)
        self.pt_pos = np.zeros((self.npts, 3), np.float32)
        self.outlier = np.zeros(max(self.nedges, 1), np.uint8)
        self.result = BAResult(self.kf_Tcw.ctypes.data, self.pt_pos.ctypes.data, self.outlier.ctypes.data)

    def out(self):
        """(kf_Tcw [nkf,4,4], pt_pos [npts,3], edge_outlier [nedges], iterations (it5, it10))."""
        return (self.kf_Tcw.copy(), self.pt_pos.copy(), self.outlier[:self.nedges].copy(),
                tuple(int(i) for i in self.result.iterations))


def local_bundle_adjustment(prob: dict, ctx=None, stop_flag=None):
    """Optimizer::LocalBundleAdjustment(pKF, pbStopFlag) (Optimizer.cc:1515-1764)
    on one local window (dict with the gf_ba_problem arrays, e.g.
    synth.synth_lba_problem). stop_flag: optional ctypes.c_uint8 polled as
    mbAbortBA. Returns (kf_Tcw, pt_pos, edge_outlier, iterations)."""
    ctx = ctx or default_context()
    arr = BAArrays(prob)
    check(lib().gf_local_ba_stop(ctx.handle, ctypes.byref(arr.problem), ctypes.byref(arr.result),
                                 ctypes.byref(stop_flag) if stop_flag is not None else None))
    return arr.out()


def bundle_adjustment(prob: dict, iterations: int, ctx=None, stop_flag=None):
    """Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag)
    (Optimizer.cc:36-142) on one graph (dict with the gf_ba_problem arrays):
    one optimize(iterations), no outlier pass. stop_flag: optional
    ctypes.c_uint8. Returns (kf_Tcw, pt_pos, edge_outlier (all zero),
    iterations (run, -1))."""
    ctx = ctx or default_context()
    arr = BAArrays(prob)
    check(lib().gf_bundle_adjustment(ctx.handle, ctypes.byref(arr.problem), int(iterations),
                                     ctypes.byref(arr.result),
                                     ctypes.byref(stop_flag) if stop_flag is not None else None))
    return arr.out()


def global_bundle_adjustment(map, iterations: int = 20, stop_flag=None, ctx=None) -> dict:
    """Optimizer::GlobalBundleAdjustemnt(pMap, nIterations, pbStopFlag)
    (Optimizer.cc:28-142) on a ``loopmap.LoopMap``. The graph is assembled on
    the host (it runs once per map): the non-bad keyframes in index order
    (fixed when mnId == 0), the non-bad points in id order, each point's
    observations in keyframe-index order with bad keyframes skipped
    (docs/ORACLE_ASSUMPTIONS.md A26). Solved by ``gf_bundle_adjustment``, which
    raises above 32 free keyframes; the poses are written back with
    ``set_pose``, the positions into ``map.mps`` and the points get the batched
    UpdateNormalAndDepth (:139). -> dict: ``iterations`` (run; -1 when the
    graph has no edge), ``keyframes`` and ``points``, the indices written."""
    ctx = ctx or default_context()
    kfs = [k for k in range(map.nkf) if not map.kf_bad[k]]
    col = {k: j for j, k in enumerate(kfs)}
    pts = [p for p in range(len(map.mps)) if not map.mp_bad[p]]
    invs = inv_level_sigma2(map.info.nlevels, map.info.scale_factor)
    e_pt, e_kf, e_z, e_w = [], [], [], []
    for j, p in enumerate(pts):
        for kf in sorted(map.obs[p]):
            if kf not in col:
                continue
            kp = map.kf_kps[kf][map.obs[p][kf]]
            e_pt.append(j)
            e_kf.append(col[kf])
            e_z.append((kp["x"], kp["y"]))
            e_w.append(invs[int(kp["octave"])])
    cam = np.array([map.info.fx, map.info.fy, map.info.cx, map.info.cy], np.float32)
    prob = dict(kf_Tcw=np.asarray(map.Tcw, np.float32).reshape(-1, 16)[kfs].reshape(-1, 16),
                kf_kind=np.asarray([BA_LOCAL_FIXED if map.kf_id[k] == 0 else BA_LOCAL for k in kfs], np.uint8),
                kf_cam=np.tile(cam, (len(kfs), 1)), pt_pos=map.mps["pos"][pts].reshape(-1, 3),
                edge_pt=np.asarray(e_pt, np.int32), edge_kf=np.asarray(e_kf, np.int32),
                edge_z=np.asarray(e_z, np.float32).reshape(-1, 2), edge_inv_sigma2=np.asarray(e_w, np.float32))
    T, X, _, its = bundle_adjustment(prob, iterations, ctx, stop_flag)
    for j, k in enumerate(kfs):
        map.set_pose(k, T[j])
    if pts:
        map.mps["pos"][pts] = X
        map.update_normal_and_depth_batch(pts, ctx)
    return dict(iterations=its[0], keyframes=kfs, points=pts)


class LocalBAPlan:
    """Batched device path: nprob local windows uploaded once, solved together
    (gf_ba_plan_create / _solve / _results). iterations=None: the
    LocalBundleAdjustment schedule (optimize(5), outlier pass, optimize(10),
    outlier pass); iterations=n: BundleAdjustment's one optimize(n) without
    outlier passes (gf_ba_plan_create_iters)."""

    def __init__(self, probs: list, ctx=None, iterations=None):
        self.ctx = ctx or default_context()
        self.arrs = [BAArrays(p) for p in probs]
        ps = (BAProblem * len(probs))(*[a.problem for a in self.arrs])
        self.handle = ctypes.c_void_p()
        if iterations is None:
            check(lib().gf_ba_plan_create(self.ctx.handle, len(probs), ps, ctypes.byref(self.handle)))
        else:
            check(lib().gf_ba_plan_create_iters(self.ctx.handle, len(probs), ps, int(iterations),
                                                ctypes.byref(self.handle)))

    def results_dev(self, p: int):
        """gf_ba_plan_results_dev: (kf_Tcw, pt_pos, iterations) device
        addresses of problem p's outputs (nkf x 16 and npts x 3 floats, 2
        int32), valid after solve() for work on the same stream."""
        T, X, I = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().gf_ba_plan_results_dev(self.handle, int(p), ctypes.byref(T), ctypes.byref(X), ctypes.byref(I)))
        return T.value, X.value, I.value

    def solve(self, stream=None, stop_flag=None) -> int:
        """gf_ba_plan_solve_stop (gf_ba_plan_solve is the same call with a null
        flag). stop_flag: optional ctypes.c_uint8 standing for mbAbortBA. The
        host reads it through its address before every chunk of steps, so the
        caller keeps the object alive until solve() returns; another thread
        may set it meanwhile. Returns the steps enqueued."""
        steps = ctypes.c_int()
        check(lib().gf_ba_plan_solve_stop(self.handle, stream if stream is not None else self.ctx.stream,
                                          ctypes.byref(stop_flag) if stop_flag is not None else None,
                                          ctypes.byref(steps)))
        return steps.value

    def results(self) -> list:
        rs = (BAResult * len(self.arrs))(*[a.result for a in self.arrs])
        check(lib().gf_ba_plan_results(self.handle, rs))
        for a, r in zip(self.arrs, rs):
            a.result.iterations[:] = r.iterations[:]
        return [a.out() for a in self.arrs]

    def close(self) -> None:
        if self.handle:
            lib().gf_ba_plan_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------- essential graph (loop correction)
class EssGraphArrays:
    """One map as ``gf_essgraph_problem`` (include/gfslam/abi.h), its numpy
    arrays kept alive next to the ctypes view, and the result buffers.

    ``map``: dict with kf_id [N], Tcw [N, 4, 4], parent [N] (-1 = none), cov
    (per keyframe a pair (neighbours, weights) in mvpOrderedConnectedKeyFrames
    order), loop_edges (per keyframe the GetLoopEdges() indices), pos [M, 3],
    bad [M], ref [M], corrected_ref [M]. NonCorrectedSim3 / CorrectedSim3:
    dicts keyframe index -> 8 doubles (qx qy qz qw tx ty tz s) over the same
    keys; LoopConnections: dict keyframe index -> iterable of indices."""

    def __init__(self, map, loop_kf, cur_kf, NonCorrectedSim3, CorrectedSim3, LoopConnections):
        from ._lib import ESSGRAPH_TRACE, EssGraphProblem, EssGraphResult

        i32 = lambda a: np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1), np.int32)  # noqa: E731
        N = len(map["kf_id"])

        def csr(rows):
            start = np.zeros(len(rows) + 1, np.int32)
            start[1:] = np.cumsum([len(r) for r in rows])
            flat = [v for r in rows for v in r]
            return start, i32(flat)

        assert sorted(CorrectedSim3) == sorted(NonCorrectedSim3), "CorrectedSim3 / NonCorrectedSim3 keys differ"
        keys = sorted(CorrectedSim3)
        lck = sorted(LoopConnections)
        a = {}
        a["kf_id"] = i32(map["kf_id"])
        a["kf_Tcw"] = np.ascontiguousarray(map["Tcw"], np.float32).reshape(N, 16)
        a["parent"] = i32(map["parent"])
        a["cov_start"], a["cov_nbr"] = csr([list(c[0]) for c in map["cov"]])
        a["cov_weight"] = i32([w for c in map["cov"] for w in c[1]])
        a["le_start"], a["le_nbr"] = csr([list(r) for r in map["loop_edges"]])
        a["lc_key"] = i32(lck)
        a["lc_start"], a["lc_nbr"] = csr([list(LoopConnections[k]) for k in lck])
        a["corr_idx"] = i32(keys)
        a["corrected"] = np.ascontiguousarray([CorrectedSim3[k] for k in keys], np.float64).reshape(-1, 8)
        a["noncorrected"] = np.ascontiguousarray([NonCorrectedSim3[k] for k in keys], np.float64).reshape(-1, 8)
        a["pt_pos"] = np.ascontiguousarray(map["pos"], np.float32).reshape(-1, 3)
        M = len(a["pt_pos"])
        a["pt_bad"] = np.ascontiguousarray(np.asarray(map["bad"]).astype(np.uint8)).reshape(-1)
        a["pt_ref"] = i32(map["ref"])
        a["pt_corrected_ref"] = i32(map["corrected_ref"])
        assert len(a["pt_bad"]) == len(a["pt_ref"]) == len(a["pt_corrected_ref"]) == M
        self.a, self.N, self.M = a, N, M
        order = ("kf_id", "kf_Tcw", "parent", "cov_start", "cov_nbr", "cov_weight", "le_start", "le_nbr", "lc_key",
                 "lc_start", "lc_nbr", "corr_idx", "corrected", "noncorrected", "pt_pos", "pt_bad", "pt_ref",
                 "pt_corrected_ref")
        self.problem = EssGraphProblem(N, M, len(keys), len(lck), int(loop_kf), int(cur_kf),
                                       *[a[k].ctypes.data if a[k].size else None for k in order])
        self.Tcw = np.zeros((N, 4, 4), np.float32)
        self.pos = np.zeros((M, 3), np.float32)
        self.trace_lambda = np.zeros(ESSGRAPH_TRACE, np.float64)
        self.trace_chi2 = np.zeros(ESSGRAPH_TRACE, np.float64)
        self.trace_accepted = np.zeros(ESSGRAPH_TRACE, np.uint8)
        self.result = EssGraphResult()
        self.result.kf_Tcw = self.Tcw.ctypes.data
        self.result.pt_pos = self.pos.ctypes.data if M else None
        self.result.trace_lambda = self.trace_lambda.ctypes.data
        self.result.trace_chi2 = self.trace_chi2.ctypes.data
        self.result.trace_accepted = self.trace_accepted.ctypes.data

    def out(self, stats=None) -> dict:
        st = stats if stats is not None else self.result.stats
        n = int(st.ntrace)
        return dict(Tcw=self.Tcw.copy(), pos=self.pos.copy(), iterations=int(st.iterations), trials=int(st.trials),
                    stop=int(st.stop), chi2_initial=float(st.chi2_initial), chi2_final=float(st.chi2_final),
                    trace_lambda=self.trace_lambda[:n].copy(), trace_chi2=self.trace_chi2[:n].copy(),
                    trace_accepted=self.trace_accepted[:n].astype(bool))


class EssentialGraphPlan:
    """A ragged batch of maps (gf_essgraph_plan_*). ``problems``: a list of
    argument tuples (map, loop_kf, cur_kf, NonCorrectedSim3, CorrectedSim3,
    LoopConnections)."""

    def __init__(self, problems: list, ctx=None):
        from ._lib import EssGraphProblem

        self.ctx = ctx or default_context()
        self.arrs = [p if isinstance(p, EssGraphArrays) else EssGraphArrays(*p) for p in problems]
        ps = (EssGraphProblem * len(self.arrs))(*[a.problem for a in self.arrs])
        self.handle = ctypes.c_void_p()
        check(lib().gf_essgraph_plan_create(self.ctx.handle, len(self.arrs), ps, ctypes.byref(self.handle)))

    def edges(self, p: int) -> np.ndarray:
        """The edge rows (i, j, kind) of problem p."""
        n = ctypes.c_int()
        check(lib().gf_essgraph_plan_edges(self.handle, p, None, 0, ctypes.byref(n)))
        rows = np.zeros((max(n.value, 1), 3), np.int32)
        check(lib().gf_essgraph_plan_edges(self.handle, p, ptr(rows), n.value, ctypes.byref(n)))
        return rows[:n.value].copy()

    def solve(self, stream=None) -> None:
        check(lib().gf_essgraph_plan_solve(self.handle, stream if stream is not None else self.ctx.stream))

    def results(self) -> list:
        from ._lib import EssGraphResult

        rs = (EssGraphResult * len(self.arrs))(*[a.result for a in self.arrs])
        check(lib().gf_essgraph_plan_results(self.handle, rs))
        return [a.out(r.stats) for a, r in zip(self.arrs, rs)]

    def close(self) -> None:
        if self.handle:
            lib().gf_essgraph_plan_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def optimize_essential_graph_batch(problems: list, ctx=None) -> list:
    """OptimizeEssentialGraph over a list of maps -> one result dict per map."""
    plan = EssentialGraphPlan(problems, ctx)
    try:
        plan.solve()
        return plan.results()
    finally:
        plan.close()


def correct_loop_points(pos, bad, sel, Sfrom, Sto, ctx=None) -> np.ndarray:
    """``gf_correct_loop_points``: point m with sel[m] = c >= 0 becomes
    Sto[c].inverse().map(Sfrom[c].map(pos[m])) (LoopClosing.cc:462-491)."""
    ctx = ctx or default_context()
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    bad = np.ascontiguousarray(np.asarray(bad).astype(np.uint8)).reshape(-1)
    sel = np.ascontiguousarray(sel, np.int32).reshape(-1)
    a = np.ascontiguousarray(Sfrom, np.float64).reshape(-1, 8)
    b = np.ascontiguousarray(Sto, np.float64).reshape(-1, 8)
    assert len(bad) == len(sel) == len(pos) and len(a) == len(b)
    out = np.zeros_like(pos)
    p = (lambda x: ptr(x) if x.size else None)
    check(lib().gf_correct_loop_points(ctx.handle, len(pos), p(pos), p(bad), p(sel), len(a), p(a), p(b), p(out)))
    return out
