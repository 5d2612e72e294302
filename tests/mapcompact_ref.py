"""ctypes wrapper of tests/helpers/libmapcompactref.so: the serial CPU
restatement of ``gf_frontend_compact_maps`` for one stream
(tests/helpers/mapcompact_ref.cpp). ``State`` holds one stream's flat arrays
laid out as the front end's slabs (map capacity M, 64 keyframes, 64 x
keypoint-capacity slots and observations) and the index holders;
``State.apply(request)`` gives the verdict (0, -1 GF_ERR_ARG, -4
GF_ERR_UNSUPPORTED) and, on 0, restricts the state in place and returns the
``localmap.MapRemap``."""
from __future__ import annotations

import copy
import ctypes
import os

import numpy as np

from gf_orb_slam_amd.localmap import MapRemap

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
KC = 64
GRAPH_KEYS = ("kf_bad", "kf_mp_off", "kf_mp", "kf_cov_off", "kf_cov", "mp_bad", "mp_obs_off", "mp_obs")
_P, _I = ctypes.c_void_p, ctypes.c_int32


class _Request(ctypes.Structure):
    _fields_ = [("n_drop_kf", _I), ("drop_kf", _P), ("n_drop_mp", _I), ("drop_mp", _P)]


class _Stream(ctypes.Structure):
    _fields_ = [("M", _I), ("KC", _I), ("slot_cap", _I), ("cap", _I), ("counts", _P), ("n_point_rows", _I),
                ("point_rows", _P), ("point_row_bytes", _P), ("n_kf_rows", _I), ("kf_rows", _P), ("kf_row_bytes", _P),
                ("kf_mp_off", _P), ("kf_mp", _P), ("kf_cov_off", _P), ("kf_cov", _P), ("mp_obs_off", _P),
                ("mp_obs", _P), ("kp2mp", _P), ("nkp", _I), ("last_kp2mp", _P), ("last_nkp", _I), ("left", _P),
                ("nleft", _I), ("out_slots", _P), ("out_n", _I), ("pending", _I), ("ref_kf", _P), ("state_ref", _P)]


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libmapcompactref.so"))
        _lib.mc_apply.restype = _lib.mc_check.restype = ctypes.c_int
        _lib.mc_apply.argtypes = [_P, ctypes.c_int, _P, _P, _P, _P]
        _lib.mc_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]
    return _lib


def _request(req):
    kf = np.ascontiguousarray(req.drop_kf, np.int32)
    mp = np.ascontiguousarray(req.drop_mp, np.int32)
    r = _Request(len(kf), kf.ctypes.data if kf.size else None, len(mp), mp.ctypes.data if mp.size else None)
    return r, (kf, mp)


class State:
    """One stream. point_rows / kf_rows: {name: slab} whose row i belongs to
    point / keyframe i (full slabs of M / 64 rows, so that rows past the used
    part can hold sentinels); graph: the compact gf_covis_map arrays (its
    mp_bad / kf_bad join the row slabs); holders: kp2mp, nkp, last_kp2mp,
    last_nkp, left, nleft, out_slots, out_n, pending, ref_kf, state_ref (None:
    no keyframe stage)."""

    def __init__(self, M: int, cap: int, graph, point_rows=None, kf_rows=None, has_db: bool = False, tail=None,
                 **holders):
        self.M, self.cap, self.slot_cap, self.has_db = int(M), int(cap), KC * int(cap), bool(has_db)
        g = {k: np.asarray(graph[k]) for k in GRAPH_KEYS}
        n, nkf = len(g["mp_bad"]), len(g["kf_bad"])
        self.counts = np.array([n, nkf], np.int32)

        def slab(a, rows, dt):
            out = np.zeros(rows, dt)
            if tail is not None:
                out.view(np.uint8)[...] = tail
            a = np.ascontiguousarray(a, dt).reshape(-1)
            out[:len(a)] = a
            return out

        self.point_rows = {k: np.ascontiguousarray(v).copy() for k, v in (point_rows or {}).items()}
        self.kf_rows = {k: np.ascontiguousarray(v).copy() for k, v in (kf_rows or {}).items()}
        assert all(len(v) == M for v in self.point_rows.values()) and all(len(v) == KC for v in self.kf_rows.values())
        self.point_rows["mp_bad"] = slab(g["mp_bad"], M, np.uint8)
        self.kf_rows["kf_bad"] = slab(g["kf_bad"], KC, np.uint8)
        self.kf_mp_off = slab(g["kf_mp_off"] if nkf else [0], KC + 1, np.int32)
        self.kf_mp = slab(g["kf_mp"], self.slot_cap, np.int32)
        self.kf_cov_off = slab(g["kf_cov_off"] if nkf else [0], KC + 1, np.int32)
        self.kf_cov = slab(g["kf_cov"], KC * KC, np.int32)
        self.mp_obs_off = slab(g["mp_obs_off"] if n else [0], M + 1, np.int32)
        self.mp_obs = slab(g["mp_obs"], self.slot_cap, np.int32)
        h = holders

        def held(key, rows):
            a = np.full(rows, -1, np.int32)
            if h.get(key) is not None:
                a[:] = np.asarray(h[key], np.int32).reshape(-1)
            return a

        self.kp2mp, self.nkp = held("kp2mp", cap), int(h.get("nkp", 0))
        self.last_kp2mp, self.last_nkp = held("last_kp2mp", cap), int(h.get("last_nkp", 0))
        self.left, self.nleft = held("left", M), int(h.get("nleft", 0))
        self.out_slots, self.out_n = held("out_slots", cap), int(h.get("out_n", 0))
        self.pending = int(h.get("pending", 0))
        self.ref_kf = np.array([h.get("ref_kf", -1)], np.int32)
        self.state_ref = None if h.get("state_ref") is None else np.array([h["state_ref"]], np.int32)

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
        return dict(kf_bad=self.kf_rows["kf_bad"][:k].copy(), kf_mp_off=self.kf_mp_off[:k + 1].copy() if k else zero.copy(),
                    kf_mp=self.kf_mp[:ns].copy(), kf_cov_off=self.kf_cov_off[:k + 1].copy() if k else zero.copy(),
                    kf_cov=self.kf_cov[:nc].copy(), mp_bad=self.point_rows["mp_bad"][:n].copy(),
                    mp_obs_off=self.mp_obs_off[:n + 1].copy() if n else zero.copy(), mp_obs=self.mp_obs[:no].copy())

    def check(self, req) -> int:
        r, _keep = _request(req)
        return lib().mc_check(self.nmp, self.nkf, int(self.has_db), ctypes.addressof(r))

    def apply(self, req):
        """-> (verdict, MapRemap or None)."""
        r, _keep = _request(req)
        prow, krow = list(self.point_rows.values()), list(self.kf_rows.values())
        pp = (ctypes.c_void_p * max(len(prow), 1))(*[a.ctypes.data for a in prow])
        kp = (ctypes.c_void_p * max(len(krow), 1))(*[a.ctypes.data for a in krow])
        pb = np.array([a.strides[0] for a in prow] or [0], np.int32)
        kb = np.array([a.strides[0] for a in krow] or [0], np.int32)
        p = lambda a: a.ctypes.data  # noqa: E731
        s = _Stream(self.M, KC, self.slot_cap, self.cap, p(self.counts), len(prow), ctypes.addressof(pp), p(pb),
                    len(krow), ctypes.addressof(kp), p(kb), p(self.kf_mp_off), p(self.kf_mp), p(self.kf_cov_off),
                    p(self.kf_cov), p(self.mp_obs_off), p(self.mp_obs), p(self.kp2mp), self.nkp, p(self.last_kp2mp),
                    self.last_nkp, p(self.left), self.nleft, p(self.out_slots), self.out_n, self.pending,
                    p(self.ref_kf), None if self.state_ref is None else p(self.state_ref))
        n0, k0 = self.nmp, self.nkf
        kf_remap, mp_remap = np.full(max(k0, 1), -1, np.int32), np.full(max(n0, 1), -1, np.int32)
        kept = np.zeros(2, np.int32)
        rc = lib().mc_apply(ctypes.addressof(s), int(self.has_db), ctypes.addressof(r), p(kf_remap), p(mp_remap), p(kept))
        if rc:
            return rc, None
        return 0, MapRemap(req.stream, self.nkf, self.nmp, kf_remap[:k0], mp_remap[:n0], int(kept[0]), int(kept[1]))


def same_graph(a: dict, b: dict) -> list:
    """Names of the graph arrays that differ (byte equality)."""
    return [k for k in GRAPH_KEYS
            if np.asarray(a[k]).astype(np.int64).tobytes() != np.asarray(b[k]).astype(np.int64).tobytes()]
