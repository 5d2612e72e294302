"""ctypes wrapper of tests/helpers/libneighborsref.so: the serial CPU
restatement of LocalMapping::SearchInNeighbors, plain ORBmatcher::Fuse and the
MapPoint / KeyFrame calls they make (tests/helpers/neighbors_ref.cpp)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

EXITS = ("fused", "null", "bad", "inkf", "depth", "image", "range", "angle", "window", "level", "dist")
X = {n: i for i, n in enumerate(EXITS)}
BEFORE_DESCRIPTORS = tuple(X[n] for n in ("null", "bad", "inkf", "depth", "image", "range", "angle", "window"))
ACTIONS = ("none", "add", "replace", "keep")
_FIELDS = ("targets", "nfused", "f_kp", "f_dist", "f_exit", "f_action", "f_other", "f_stale", "cand", "b_kp",
           "b_dist", "b_exit", "b_action", "b_other", "b_stale", "updated", "scalars", "f_exit0", "b_exit0")


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libneighborsref.so"))
        _lib.nr_create.restype = ctypes.c_void_p
        _lib.nr_counter.restype = ctypes.c_long
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class RefWorld:
    """The restatement's world, built from the arrays a LoopMap is built from
    (plus the poses, the reference keyframes and the keyframe ids)."""

    def __init__(self, info, kf_kps, kf_desc, kf_mp, mps, mp_desc, mp_bad=None, observations=None, kf_bad=None,
                 kf_Tcw=None, ref_kf=None, kf_id=None):
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
        if ref_kf is None:
            ref_kf = [min(o) if o else -1 for o in observations]
        bounds = np.array([info.min_x, info.max_x, info.min_y, info.max_y], np.int32)
        K = np.array([info.fx, info.fy, info.cx, info.cy], np.float32)
        sc = c(info.scale_factors(), np.float32)
        kb = None if kf_bad is None else c(np.asarray(kf_bad).astype(np.uint8))
        mb = None if mp_bad is None else c(np.asarray(mp_bad).astype(np.uint8))
        T = (np.tile(np.eye(4, dtype=np.float32), (self.nkf, 1, 1)) if kf_Tcw is None
             else c(np.asarray(kf_Tcw, np.float32).reshape(self.nkf, 16)))
        ids = c(np.arange(self.nkf) if kf_id is None else kf_id, np.int32)
        rk = c(np.asarray(ref_kf, np.int32).reshape(-1))
        pos, nrm = c(mps["pos"], np.float32), c(mps["normal"], np.float32)
        mind, maxd = c(mps["min_dist"], np.float32), c(mps["max_dist"], np.float32)
        md = c(mp_desc, np.uint8)
        op, ok, os_ = c(rows[:, 0]), c(rows[:, 1]), c(rows[:, 2])
        self.h = ctypes.c_void_p(lib().nr_create(
            _p(bounds), _p(K), len(sc), _p(sc), ctypes.c_float(info.scale_factor), self.nkf, _p(off), _p(kx), _p(ky),
            _p(ko), _p(kd), _p(sl), _p(kb), _p(T), _p(ids), self.nmp, _p(pos), _p(nrm), _p(mind), _p(maxd), _p(md),
            _p(mb), _p(rk), len(rows), _p(op), _p(ok), _p(os_)))

    @classmethod
    def from_loopmap(cls, m):
        """A world equal to the LoopMap ``m`` as it stands (the covisibility
        graph is not copied: run update_connections on both)."""
        return cls(m.info, m.kf_kps, m.kf_desc, m.slots, m.mps, m.mp_desc, m.mp_bad, m.obs, m.kf_bad, m.Tcw, m.ref_kf,
                   m.kf_id)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.nr_destroy(self.h)
            self.h = None

    def fuse(self, kf, points, th=3.0, apply=False):
        """One Fuse call -> dict kp, dist, exit, action, other, nFused."""
        pts = np.ascontiguousarray(points, np.int32).reshape(-1)
        m = len(pts)
        o = {k: np.zeros(max(m, 1), np.int32) for k in ("kp", "dist", "exit", "action", "other")}
        nf = lib().nr_fuse(self.h, int(kf), _p(pts), m, ctypes.c_float(th), int(apply), _p(o["kp"]), _p(o["dist"]),
                           _p(o["exit"]), _p(o["action"]), _p(o["other"]))
        o = {k: v[:m] for k, v in o.items()}
        o["nFused"] = nf
        return o

    def replace(self, a, b):
        lib().nr_replace(self.h, int(a), int(b))

    def set_bad_kf(self, kf, bad=True):
        lib().nr_set_bad_kf(self.h, int(kf), int(bad))

    def update_normal_and_depth(self, ids):
        for p in ids:
            lib().nr_update_normal_and_depth(self.h, int(p))

    def update_connections(self, kf):
        lib().nr_update_connections(self.h, int(kf))

    def _field(self, name):
        i = _FIELDS.index(name)
        n = lib().nr_report(self.h, i, None)
        out = np.zeros(max(n, 1), np.int32)
        lib().nr_report(self.h, i, _p(out))
        return out[:n]

    def search_in_neighbors(self, cur, th=3.0):
        """-> dict: targets, nfused [nt]; kp / dist / exit / action / other /
        stale_kp [nt, m] of the forward calls (m = the new keyframe's slots);
        cand and b_* [nc] of the backward call, b_nfused; updated;
        skipped_bad_kf; f_exit0 / b_exit0: the exits on the map as it stood
        when the forward calls / the backward call began."""
        lib().nr_search_in_neighbors(self.h, int(cur), ctypes.c_float(th))
        r = {n: self._field(n) for n in _FIELDS}
        m, r["b_nfused"], r["skipped_bad_kf"] = (int(x) for x in r.pop("scalars"))
        nt = len(r["targets"])
        for n in ("f_kp", "f_dist", "f_exit", "f_action", "f_other", "f_stale", "f_exit0"):
            r[n] = r[n].reshape(nt, m)
        return r

    def counter(self, name):
        return int(lib().nr_counter(self.h, {"erase_branch": 0, "same_id": 1}[name]))

    def geometry(self):
        """-> float rows [M, 8]: pos, normal, min_dist, max_dist."""
        out = np.zeros((max(self.nmp, 1), 8), np.float32)
        lib().nr_get_geometry(self.h, _p(out))
        return out[:self.nmp]

    def connections(self, kf):
        """-> (ordered covisibles, their weights, the weight map as a dict, parent)."""
        o, w, n = np.zeros((self.nkf + 1, 2), np.int32), np.zeros((self.nkf + 1, 2), np.int32), np.zeros(3, np.int32)
        lib().nr_get_connections(self.h, int(kf), self.nkf + 1, _p(o), _p(w), _p(n))
        return ([int(x) for x in o[:n[0], 0]], [int(x) for x in o[:n[0], 1]],
                {int(a): int(b) for a, b in w[:n[1]]}, int(n[2]))

    def slots(self):
        out = np.zeros(max(sum(self.kf_n), 1), np.int32)
        lib().nr_get_slots(self.h, _p(out))
        return np.split(out[:sum(self.kf_n)], np.cumsum(self.kf_n)[:-1]) if self.nkf else []

    def points(self):
        bad, desc = np.zeros(max(self.nmp, 1), np.uint8), np.zeros((max(self.nmp, 1), 32), np.uint8)
        lib().nr_get_points(self.h, _p(bad), _p(desc))
        return bad[:self.nmp].astype(bool), desc[:self.nmp]

    def markers(self):
        """-> (mnFuseTargetForKF per keyframe, mnFuseCandidateForKF per point)."""
        a, b = np.zeros(max(self.nkf, 1), np.int64), np.zeros(max(self.nmp, 1), np.int64)
        lib().nr_get_markers(self.h, _p(a), _p(b))
        return a[:self.nkf], b[:self.nmp]

    def observation_rows(self):
        n = lib().nr_get_obs(self.h, 0, None)
        out = np.zeros((max(n, 1), 3), np.int32)
        lib().nr_get_obs(self.h, n, _p(out))
        return out[:n]
