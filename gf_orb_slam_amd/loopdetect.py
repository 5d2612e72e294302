"""Host-side mirror of loop detection: ORB_SLAM::KeyFrameDatabase
(src/KeyFrameDatabase.cc:32-196) over libgfslam's growable device database
(abi.h gf_loopdb_*, gf_detect_loop_candidates; csrc/loopdetect.hip) and
LoopClosing::DetectLoop (src/LoopClosing.cc:111-238) on top of it. The
BowVectors stay on the device; a query intersects every listed vector with the
query's, scores the survivors and orders the candidates in three kernels. The
consistent-group bookkeeping runs on the host, as sim3.loop_fusion /
loop_connections do."""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, lib, ptr
from .orb import default_context


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _pp(a):
    return ptr(a) if a.size else None


def bow_score(v1, v2, scoring: int = 0) -> float:
    """TemplatedVocabulary::score(v1, v2) = L1Scoring::score
    (ScoringObject.cpp:23-68) of two BowVectors (words ascending, values), in
    double on the host. scoring: the vocabulary's ScoringType (0 = L1_NORM,
    the only one implemented)."""
    w1, x1 = _i32(v1[0]), np.ascontiguousarray(v1[1], np.float64).reshape(-1)
    w2, x2 = _i32(v2[0]), np.ascontiguousarray(v2[1], np.float64).reshape(-1)
    if len(w1) != len(x1) or len(w2) != len(x2):
        raise ValueError("a BowVector is (words, values) of equal length")
    s = ctypes.c_double()
    check(lib().gf_bow_score(int(scoring), _pp(w1), _pp(x1), len(w1), _pp(w2), _pp(x2), len(w2), ctypes.byref(s)))
    return s.value


def covisibles_csr(ordered) -> tuple[np.ndarray, np.ndarray]:
    """mvpOrderedConnectedKeyFrames per keyframe (a list of lists) as the
    (cov_off, cov) arrays the queries take."""
    off = np.zeros(len(ordered) + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in ordered])
    cov = np.asarray([k for o in ordered for k in o], np.int32).reshape(-1)
    return off, cov


class KeyFrameDatabase:
    """KeyFrameDatabase on the device. A keyframe is a slot, numbered from 0 in
    insert order; insert() stores its BowVector, add() / erase() list and
    unlist it in the inverted file's order (an add sequence number per slot)."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.handle = ctypes.c_void_p()
        check(lib().gf_loopdb_create(self.ctx.handle, ctypes.byref(self.handle)))

    def _size(self):
        n, m = ctypes.c_int(), ctypes.c_int()
        check(lib().gf_loopdb_size(self.handle, ctypes.byref(n), ctypes.byref(m)))
        return n.value, m.value

    @property
    def nslots(self) -> int:
        return self._size()[0]

    @property
    def nlisted(self) -> int:
        return self._size()[1]

    def insert(self, words, values) -> int:
        """Store a keyframe's BowVector (not listed yet) -> its slot."""
        w, v = _i32(words), np.ascontiguousarray(values, np.float64).reshape(-1)
        if len(w) != len(v):
            raise ValueError("words and values differ in length")
        slot = ctypes.c_int()
        check(lib().gf_loopdb_insert(self.handle, _pp(w), _pp(v), len(w), ctypes.byref(slot)))
        return slot.value

    def insert_dev(self, d_words, d_values, d_nwords, cap: int, frame: int, stream=None) -> int:
        """The same for frame `frame` of the device arrays gf_bow_transform_dev
        wrote (strided by cap), on `stream`, without synchronising."""
        slot = ctypes.c_int()
        check(lib().gf_loopdb_insert_dev(self.handle, ptr(d_words), ptr(d_values), ptr(d_nwords), int(cap), int(frame),
                                         ctypes.c_void_p(stream or 0), ctypes.byref(slot)))
        return slot.value

    def add(self, slot: int) -> None:
        """KeyFrameDatabase::add (:39-45)."""
        check(lib().gf_loopdb_add(self.handle, int(slot)))

    def erase(self, slot: int) -> None:
        """KeyFrameDatabase::erase (:47-66)."""
        check(lib().gf_loopdb_erase(self.handle, int(slot)))

    def clear(self) -> None:
        """KeyFrameDatabase::clear (:68-72): every keyframe unlisted."""
        check(lib().gf_loopdb_clear(self.handle))

    def score_against(self, query: int, slots) -> np.ndarray:
        """(float) mpORBVocabulary->score(query's BowVec, slot's BowVec) for
        each slot (LoopClosing.cc:142), listed or not."""
        s = _i32(slots)
        out = np.zeros(len(s), np.float32)
        check(lib().gf_loopdb_scores(self.handle, int(query), _pp(s), len(s), _pp(out)))
        return out

    def detect_loop_candidates(self, query: int, connected, cov_off, cov, min_score: float, full: bool = False):
        """DetectLoopCandidates(pKF, minScore) (:75-196) -> the candidate slots
        in the reference's order. connected: GetConnectedKeyFrames() of the
        query; cov_off / cov: the ordered covisibles of every slot
        (covisibles_csr). full: -> dict with ``cands``, ``words`` (mnLoopWords
        per slot), ``score`` (mLoopScore, valid where words > min_common) and
        ``min_common``."""
        n = self.nslots
        c, co, cv = _i32(sorted(connected)), _i32(cov_off), _i32(cov)
        if len(co) != n + 1:
            raise ValueError(f"cov_off needs {n + 1} entries")
        words, score = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
        cands = np.zeros(max(n, 1), np.int32)
        mc, nc = ctypes.c_int(), ctypes.c_int()
        check(lib().gf_detect_loop_candidates(self.handle, int(query), _pp(c), len(c), ptr(co), _pp(cv),
                                              ctypes.c_float(min_score), ptr(words), ptr(score), ctypes.byref(mc),
                                              ptr(cands), ctypes.byref(nc)))
        out = cands[:nc.value].copy()
        if not full:
            return out
        return dict(cands=out, words=words[:n].copy(), score=score[:n].copy(), min_common=mc.value)

    def close(self) -> None:
        if self.handle:
            lib().gf_loopdb_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LoopDetector:
    """LoopClosing::DetectLoop (LoopClosing.cc:111-238), one call per keyframe
    taken from the loop queue.

    db: a :class:`KeyFrameDatabase` (or any object with its ``score_against``,
    ``detect_loop_candidates`` and ``add``) holding every keyframe's BowVector
    at the slot equal to its index in ``map``. map: the covisibility graph, a
    :class:`loopmap.LoopMap` or anything with ``ordered[kf]``
    (GetVectorCovisibleKeyFrames), ``kf_bad[kf]``, ``kf_id[kf]`` (mnId) and
    ``get_connected_keyframes(kf)``.

    State: ``last_loop_kf_id`` (mLastLoopKFid; CorrectLoop's caller sets it to
    the current keyframe's mnId) and ``consistent_groups`` (mvConsistentGroups:
    a list of (set of keyframes, consistency counter))."""

    def __init__(self, db, map, consistency_th: int = 3):
        self.db, self.map = db, map
        self.consistency_th = int(consistency_th)  # mnCovisibilityConsistencyTh
        self.last_loop_kf_id = 0
        self.consistent_groups: list[tuple[set, int]] = []
        self.min_score = None  # of the last call that reached the query

    def detect_loop(self, kf: int):
        """-> (detected, mvpEnoughConsistentCandidates). The current keyframe
        is added to the database on every path. The returned list is what
        :func:`sim3.compute_sim3_loop` takes as ``candidates`` once each
        keyframe index is replaced by its (Sim3KeyFrame, descriptors,
        FeatureVector) triple."""
        kf = int(kf)
        m = self.map
        if int(m.kf_id[kf]) < self.last_loop_kf_id + 10:
            self.db.add(kf)
            return False, []
        # the lowest score to a connected keyframe in the covisibility graph
        cov = [int(k) for k in m.ordered[kf] if not m.kf_bad[k]]
        min_score = np.float32(1)
        if cov:
            s = self.db.score_against(kf, cov)
            for x in s:
                if x < min_score:
                    min_score = x
        self.min_score = float(min_score)
        cov_off, cov_all = covisibles_csr(m.ordered)
        cands = [int(c) for c in self.db.detect_loop_candidates(kf, m.get_connected_keyframes(kf), cov_off, cov_all,
                                                                float(min_score))]
        if not cands:
            self.db.add(kf)
            self.consistent_groups = []
            return False, []
        enough = []
        current = []
        seen = [False] * len(self.consistent_groups)  # vbConsistentGroup
        for c in cands:
            group = set(int(k) for k in m.get_connected_keyframes(c))
            group.add(c)
            enough_consistent = False
            consistent_for_some = False
            for g, (prev, n_prev) in enumerate(self.consistent_groups):
                if group.isdisjoint(prev):
                    continue
                consistent_for_some = True
                n_cur = n_prev + 1
                if not seen[g]:
                    current.append((group, n_cur))
                    seen[g] = True  # the same previous group extends once
                if n_cur >= self.consistency_th and not enough_consistent:
                    enough.append(c)
                    enough_consistent = True  # the same candidate enters once
            if not consistent_for_some:
                current.append((group, 0))
        self.consistent_groups = current
        self.db.add(kf)
        return bool(enough), enough
