"""ctypes wrapper of tests/helpers/libloopfuseref.so: the serial CPU restatement
of Fuse(pKF, Scw, ...), SearchAndFuse and the MapPoint / KeyFrame calls they
make (tests/helpers/loopfuse_ref.cpp)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

EXITS = ("fused", "bad", "found", "depth", "image", "range", "angle", "window", "level", "dist")
X = {n: i for i, n in enumerate(EXITS)}
ACTIONS = ("none", "add", "replace", "keep")


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libloopfuseref.so"))
        _lib.lf_create.restype = ctypes.c_void_p
        _lib.lf_counter.restype = ctypes.c_long
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class RefMap:
    """The restatement's world, built from the arrays a LoopMap is built from."""

    def __init__(self, info, kf_kps, kf_desc, kf_mp, mps, mp_desc, mp_bad=None, observations=None, kf_bad=None):
        c = np.ascontiguousarray
        self.nkf, self.nmp = len(kf_kps), len(mps)
        self.kf_n = [len(k) for k in kf_kps]
        off = np.zeros(self.nkf + 1, np.int32)
        off[1:] = np.cumsum(self.kf_n)
        cat = lambda xs, dt, shape: c(np.concatenate([np.asarray(x, dt).reshape(shape) for x in xs])  # noqa: E731
                                      if xs else np.zeros(shape, dt))
        kx = cat([k["x"] for k in kf_kps], np.float32, (-1,))
        ky = cat([k["y"] for k in kf_kps], np.float32, (-1,))
        ko = cat([k["octave"] for k in kf_kps], np.int32, (-1,))
        kd = cat(kf_desc, np.uint8, (-1, 32))
        sl = cat(kf_mp, np.int32, (-1,))
        if observations is None:
            observations = [dict() for _ in range(self.nmp)]
            for k, s in enumerate(kf_mp):
                for idx in np.nonzero(np.asarray(s) >= 0)[0]:
                    observations[int(s[idx])][k] = int(idx)
        rows = np.asarray([(p, kf, o[kf]) for p, o in enumerate(observations) for kf in sorted(o)],
                          np.int32).reshape(-1, 3)
        bounds = np.array([info.min_x, info.max_x, info.min_y, info.max_y], np.int32)
        K = np.array([info.fx, info.fy, info.cx, info.cy], np.float32)
        sc = c(info.scale_factors(), np.float32)
        kb = None if kf_bad is None else c(np.asarray(kf_bad).astype(np.uint8))
        mb = None if mp_bad is None else c(np.asarray(mp_bad).astype(np.uint8))
        pos, nrm = c(mps["pos"], np.float32), c(mps["normal"], np.float32)
        mind, maxd = c(mps["min_dist"], np.float32), c(mps["max_dist"], np.float32)
        md = c(mp_desc, np.uint8)
        op, ok, os_ = c(rows[:, 0]), c(rows[:, 1]), c(rows[:, 2])
        self.h = ctypes.c_void_p(lib().lf_create(_p(bounds), _p(K), len(sc), _p(sc), self.nkf, _p(off), _p(kx), _p(ky),
                                                 _p(ko), _p(kd), _p(sl), _p(kb), self.nmp, _p(pos), _p(nrm), _p(mind),
                                                 _p(maxd), _p(md), _p(mb), len(rows), _p(op), _p(ok), _p(os_)))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.lf_destroy(self.h)
            self.h = None

    def fuse(self, kf, Scw, points, th=4.0, apply=False):
        """One Fuse call -> dict kp, dist, exit, action, replaced, nFused."""
        pts = np.ascontiguousarray(points, np.int32).reshape(-1)
        m = len(pts)
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        o = {k: np.zeros(max(m, 1), np.int32) for k in ("kp", "dist", "exit", "action", "replaced")}
        nf = lib().lf_fuse(self.h, int(kf), _p(S), _p(pts), m, ctypes.c_float(th), int(apply), _p(o["kp"]),
                           _p(o["dist"]), _p(o["exit"]), _p(o["action"]), _p(o["replaced"]))
        o = {k: v[:m] for k, v in o.items()}
        o["nFused"] = nf
        return o

    def search_and_fuse(self, kfs, Scw, points, th=4.0):
        """SearchAndFuse over kfs (index order) -> dict of [nk, m] arrays kp,
        dist, exit, action, replaced, stale_kp and nFused [nk]."""
        kfs = np.ascontiguousarray(kfs, np.int32)
        pts = np.ascontiguousarray(points, np.int32).reshape(-1)
        nk, m = len(kfs), len(pts)
        S = np.ascontiguousarray(np.asarray(Scw, np.float32).reshape(nk, 16))
        o = {k: np.zeros((nk, max(m, 1)), np.int32) for k in ("kp", "dist", "exit", "action", "replaced", "stale_kp")}
        if m:
            nf = np.zeros(nk, np.int32)
            lib().lf_search_and_fuse(self.h, nk, _p(kfs), _p(S), _p(pts), m, ctypes.c_float(th), _p(o["kp"]),
                                     _p(o["dist"]), _p(o["exit"]), _p(o["action"]), _p(o["replaced"]),
                                     _p(o["stale_kp"]), _p(nf))
        else:
            nf = np.zeros(nk, np.int32)
        o = {k: v[:, :m] for k, v in o.items()}
        o["nFused"] = nf
        return o

    def replace(self, a, b):
        lib().lf_replace(self.h, int(a), int(b))

    def add_observation(self, p, kf, slot):
        lib().lf_add_observation(self.h, int(p), int(kf), int(slot))

    def add_map_point(self, kf, p, slot):
        lib().lf_add_map_point(self.h, int(kf), int(p), int(slot))

    def set_scale_factor(self, f):
        lib().lf_set_scale_factor(self.h, ctypes.c_float(f))

    def set_pose(self, kf, T):
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        lib().lf_set_pose(self.h, int(kf), _p(T))

    def set_ref(self, p, ref):
        lib().lf_set_ref(self.h, int(p), int(ref))

    def set_pos(self, p, x):
        x = np.ascontiguousarray(x, np.float32).reshape(3)
        lib().lf_set_pos(self.h, int(p), _p(x))

    def update_normal_and_depth(self, ids):
        for p in ids:
            lib().lf_update_normal_and_depth(self.h, int(p))

    def geometry(self):
        """-> MAP_POINT_DTYPE-shaped float rows [M, 8]: pos, normal, min_dist, max_dist."""
        out = np.zeros((max(self.nmp, 1), 8), np.float32)
        lib().lf_get_geometry(self.h, _p(out))
        return out[:self.nmp]

    def update_connections(self, kf):
        lib().lf_update_connections(self.h, int(kf))

    def connections(self, kf):
        """-> (ordered covisibles, their weights, the weight map as a dict, parent)."""
        o, w, n = np.zeros((self.nkf + 1, 2), np.int32), np.zeros((self.nkf + 1, 2), np.int32), np.zeros(3, np.int32)
        lib().lf_get_connections(self.h, int(kf), self.nkf + 1, _p(o), _p(w), _p(n))
        return ([int(x) for x in o[:n[0], 0]], [int(x) for x in o[:n[0], 1]],
                {int(a): int(b) for a, b in w[:n[1]]}, int(n[2]))

    def loop_fusion(self, cur, matched):
        m = np.ascontiguousarray(matched, np.int32)
        lib().lf_loop_fusion(self.h, int(cur), _p(m), len(m))

    def loop_connections(self, connected):
        """-> dict keyframe -> sorted list of its new neighbours."""
        c = np.ascontiguousarray(connected, np.int32)
        cap = self.nkf * self.nkf + 1
        out = np.zeros((cap, 2), np.int32)
        n = lib().lf_loop_connections(self.h, len(c), _p(c), cap, _p(out))
        lc = {int(k): [] for k in c}
        for a, b in out[:n]:
            lc[int(a)].append(int(b))
        return lc

    def counter(self, name):
        return int(lib().lf_counter(self.h, {"erase_branch": 0, "same_id": 1}[name]))

    def slots(self):
        out = np.zeros(max(sum(self.kf_n), 1), np.int32)
        lib().lf_get_slots(self.h, _p(out))
        return np.split(out[:sum(self.kf_n)], np.cumsum(self.kf_n)[:-1]) if self.nkf else []

    def points(self):
        bad, desc = np.zeros(max(self.nmp, 1), np.uint8), np.zeros((max(self.nmp, 1), 32), np.uint8)
        lib().lf_get_points(self.h, _p(bad), _p(desc))
        return bad[:self.nmp].astype(bool), desc[:self.nmp]

    def observation_rows(self):
        n = lib().lf_get_obs(self.h, 0, None)
        out = np.zeros((max(n, 1), 3), np.int32)
        lib().lf_get_obs(self.h, n, _p(out))
        return out[:n]
