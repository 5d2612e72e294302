"""ctypes wrapper of tests/helpers/libsearchinitref.so: the serial CPU
restatement of ORBmatcher::SearchForInitialization and of the gate and state
machine of Tracking::Initialize (tests/helpers/searchinit_ref.cpp).

``search`` is the matcher; ``RefInitializer`` is the CPU chain of one sequence:
the restatement's FirstInitialization / gate -> ``oracle_lib.initialize`` ->
``initmap_ref.create``."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
COUNTERS = ("steals", "filtered", "ratio_equal", "hist_removed", "stale")
OK, FEW_KEYPOINTS, FEW_MATCHES = 0, 1, 2
NOT_INITIALIZED, INITIALIZING, WORKING = "NOT_INITIALIZED", "INITIALIZING", "WORKING"


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libsearchinitref.so"))
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _bounds(info):
    return np.array([info.min_x, info.max_x, info.min_y, info.max_y], np.int32)


def _frame(kps, desc):
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    d = np.ascontiguousarray(desc, np.uint8).reshape(len(k), 32)
    if not len(k):  # a valid address for the empty frame
        return np.zeros(1, KEYPOINT_DTYPE), np.zeros((1, 32), np.uint8), 0
    return k, d, len(k)


def search(info, kps1, desc1, kps2, desc2, prev_matched, window=100, nnratio=0.9, check_ori=True):
    """-> (nmatches, matches12 [n1], prev_matched after [n1, 2], counters dict).
    ``prev_matched`` is not modified."""
    k1, d1, n1 = _frame(kps1, desc1)
    k2, d2, n2 = _frame(kps2, desc2)
    prev = np.zeros((max(n1, 1), 2), np.float32)
    prev[:n1] = np.asarray(prev_matched, np.float32).reshape(n1, 2)
    m12 = np.full(max(n1, 1), -9, np.int32)
    cnt = np.zeros(len(COUNTERS), np.int64)
    nm = lib().sir_search(_p(_bounds(info)), _p(k1), _p(d1), n1, _p(k2), _p(d2), n2, int(window),
                          ctypes.c_float(nnratio), int(bool(check_ori)), _p(prev), _p(m12), _p(cnt))
    return int(nm), m12[:n1], prev[:n1], dict(zip(COUNTERS, (int(c) for c in cnt)))


def gate(info, kps1, desc1, kps2, desc2, prev_matched, ini_matches, thres=100):
    """Tracking::Initialize up to the initialiser -> (status, nmatches,
    mvIniMatches, mvbPrevMatched), the inputs not modified."""
    k1, d1, n1 = _frame(kps1, desc1)
    k2, d2, n2 = _frame(kps2, desc2)
    prev = np.zeros((max(n1, 1), 2), np.float32)
    prev[:n1] = np.asarray(prev_matched, np.float32).reshape(n1, 2)
    m = np.full(max(n1, 1), -1, np.int32)
    m[:n1] = np.asarray(ini_matches, np.int32).reshape(n1)
    nm = np.zeros(1, np.int32)
    cnt = np.zeros(len(COUNTERS), np.int64)
    st = lib().sir_initialize_gate(_p(_bounds(info)), _p(k1), _p(d1), n1, _p(k2), _p(d2), n2, int(thres), _p(prev),
                                   _p(m), _p(nm), _p(cnt))
    return int(st), int(nm[0]), m[:n1], prev[:n1]


def first_initialization(kps, thres=100):
    """-> mvbPrevMatched [n, 2] when the frame becomes the initial frame, else None."""
    k, _, n = _frame(kps, np.zeros((len(kps), 32), np.uint8))
    prev = np.zeros((max(n, 1), 2), np.float32)
    ok = lib().sir_first_initialization(_p(k), n, int(thres), _p(prev))
    return prev[:n] if ok else None


class RefInitializer:
    """The CPU chain for one sequence (Tracking.cc:547-569): feed(kps, desc)
    -> state. After a feed: ``status`` (gate status or None), ``nmatches``,
    ``ini_matches`` (mvIniMatches), ``prev_matched``, ``init`` (the
    initialiser's record or None), ``map`` (initmap_ref.create's pair or
    None)."""

    def __init__(self, info, K, rng_state, thres=100):
        self.info, self.K, self.rng, self.thres = info, np.asarray(K, np.float32).reshape(3, 3), rng_state, thres
        self.state = NOT_INITIALIZED
        self.ini = self.prev_matched = self.ini_matches = None
        self.status = self.init = self.map = None
        self.nmatches = 0

    def feed(self, kps, desc):
        import initmap_ref
        import oracle_lib as O

        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(len(kps), 32)
        self.status = self.init = self.map = None
        if self.state == NOT_INITIALIZED:
            prev = first_initialization(kps, self.thres)
            if prev is not None:
                self.ini, self.prev_matched = (kps, desc), prev
                self.ini_matches = np.full(len(kps), -1, np.int32)
                self.state = INITIALIZING
            return self.state
        assert self.state == INITIALIZING
        k1, d1 = self.ini
        self.status, self.nmatches, self.ini_matches, self.prev_matched = gate(
            self.info, k1, d1, kps, desc, self.prev_matched, self.ini_matches, self.thres)
        if self.status != OK:
            self.state = NOT_INITIALIZED
            return self.state
        rc, res, p3d, tri = O.initialize(self.K, k1, kps, self.ini_matches, self.rng)
        assert rc == 0
        self.init, self.p3d, self.tri = res, p3d, tri
        if not int(res["ok"][0]):
            return self.state
        a, b = initmap_ref.create(self.info, k1, d1, kps, desc, self.ini_matches, res, p3d, tri, self.thres)
        m = self.ini_matches.copy()
        m[(m >= 0) & (tri == 0)] = -1  # Tracking.cc:1025-1032
        self.ini_matches = m
        self.map = (a, b)
        self.state = WORKING if b["status"] == initmap_ref.OK else NOT_INITIALIZED
        return self.state
