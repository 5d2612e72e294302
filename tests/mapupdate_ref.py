"""ctypes wrapper of tests/helpers/libmapupdateref.so: the serial CPU
restatement of ``gf_frontend_update_maps`` for one stream
(tests/helpers/mapupdate_ref.cpp). ``State`` holds one stream's flat arrays
laid out as the front end's slabs (map capacity M, 64 keyframes, 64 x
keypoint-capacity slots and observations); ``State.apply(delta)`` gives the
verdict (0, -1 GF_ERR_ARG, -3 GF_ERR_CAP, -4 GF_ERR_UNSUPPORTED) and, on 0,
applies the ``localmap.MapDelta`` in place."""
from __future__ import annotations

import copy
import ctypes
import os

import numpy as np

from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, MP_VIEW_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
KC = 64
GRAPH_KEYS = ("kf_bad", "kf_mp_off", "kf_mp", "kf_cov_off", "kf_cov", "mp_bad", "mp_obs_off", "mp_obs")


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libmapupdateref.so"))
        _lib.mu_apply.restype = _lib.mu_check.restype = ctypes.c_int
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class State:
    """One stream: the map fields (full slabs of M rows, so that rows past the
    used part can hold sentinels), the graph slabs, the last frame's cache."""

    def __init__(self, M: int, cap: int, mp, desc, graph, views=None, upd=None, last_kp2mp=None, last_nkp: int = 0,
                 last_pos=None, has_db: bool = False, tail=None):
        """mp / desc: the stream's points (n rows) or full slabs (M rows) with
        graph["mp_bad"] giving n; graph: the compact gf_covis_map arrays;
        tail: byte the unused rows of the graph slabs are filled with."""
        self.M, self.cap, self.slot_cap, self.has_db = int(M), int(cap), KC * int(cap), bool(has_db)
        g = {k: np.asarray(graph[k]) for k in GRAPH_KEYS}
        n, nkf = len(g["mp_bad"]), len(g["kf_bad"])
        self.counts = np.array([n, nkf], np.int32)

        def slab(a, rows, dt, width=()):
            out = np.zeros((rows,) + width, dt)
            if tail is not None:
                out.view(np.uint8)[...] = tail
            a = np.ascontiguousarray(a, dt).reshape((-1,) + width)
            out[:len(a)] = a
            return out

        self.map = slab(mp, M, MAP_POINT_DTYPE)
        self.desc = slab(desc, M, np.uint8, (32,))
        self.pos = np.ascontiguousarray(self.map["pos"], np.float32).copy()
        self.views = slab(np.zeros(0, MP_VIEW_DTYPE) if views is None else views, M, MP_VIEW_DTYPE)
        self.upd = slab(np.full(M, -1000, np.int32) if upd is None else upd, M, np.int32)
        self.mp_bad = slab(g["mp_bad"], M, np.uint8)
        self.kf_bad = slab(g["kf_bad"], KC, np.uint8)
        self.kf_mp_off = slab(g["kf_mp_off"] if nkf else [0], KC + 1, np.int32)
        self.kf_mp = slab(g["kf_mp"], self.slot_cap, np.int32)
        self.kf_cov_off = slab(g["kf_cov_off"] if nkf else [0], KC + 1, np.int32)
        self.kf_cov = slab(g["kf_cov"], KC * KC, np.int32)
        self.mp_obs_off = slab(g["mp_obs_off"] if n else [0], M + 1, np.int32)
        self.mp_obs = slab(g["mp_obs"], self.slot_cap, np.int32)
        self.last_kp2mp = slab(np.full(cap, -1, np.int32) if last_kp2mp is None else last_kp2mp, cap, np.int32)
        self.last_nkp = int(last_nkp)
        self.last_pos = slab(np.zeros((cap, 3), np.float32) if last_pos is None else last_pos, cap, np.float32, (3,))

    @property
    def nmp(self) -> int:
        return int(self.counts[0])

    @property
    def nkf(self) -> int:
        return int(self.counts[1])

    def copy(self) -> "State":
        return copy.deepcopy(self)

    def graph(self) -> dict:
        """The compact gf_covis_map arrays."""
        n, k = self.nmp, self.nkf
        ns, nc = (int(self.kf_mp_off[k]), int(self.kf_cov_off[k])) if k else (0, 0)
        no = int(self.mp_obs_off[n]) if n else 0
        zero = np.zeros(1, np.int32)
        return dict(kf_bad=self.kf_bad[:k].copy(), kf_mp_off=self.kf_mp_off[:k + 1].copy() if k else zero.copy(),
                    kf_mp=self.kf_mp[:ns].copy(), kf_cov_off=self.kf_cov_off[:k + 1].copy() if k else zero.copy(),
                    kf_cov=self.kf_cov[:nc].copy(), mp_bad=self.mp_bad[:n].copy(),
                    mp_obs_off=self.mp_obs_off[:n + 1].copy() if n else zero.copy(), mp_obs=self.mp_obs[:no].copy())

    def check(self, delta) -> int:
        s = delta.struct()
        return lib().mu_check(self.M, KC, self.slot_cap, int(self.has_db), self.nmp, self.nkf, _p(self.kf_mp_off),
                              _p(self.mp_obs_off), ctypes.byref(s))

    def apply(self, delta) -> int:
        s = delta.struct()
        return lib().mu_apply(self.M, KC, self.slot_cap, self.cap, int(self.has_db), _p(self.counts), _p(self.map),
                              _p(self.desc), _p(self.pos), _p(self.upd), _p(self.views), _p(self.mp_bad),
                              _p(self.kf_bad), _p(self.kf_mp_off), _p(self.kf_mp), _p(self.kf_cov_off),
                              _p(self.kf_cov), _p(self.mp_obs_off), _p(self.mp_obs), _p(self.last_kp2mp),
                              self.last_nkp, _p(self.last_pos), ctypes.byref(s))


def same_graph(a: dict, b: dict) -> list:
    """Names of the graph arrays that differ (byte equality)."""
    return [k for k in GRAPH_KEYS
            if np.asarray(a[k]).astype(np.int64).tobytes() != np.asarray(b[k]).astype(np.int64).tobytes()]
