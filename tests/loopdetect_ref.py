"""ctypes wrapper of tests/helpers/libloopdetectref.so: the serial CPU
restatement of KeyFrameDatabase::add / erase / clear / DetectLoopCandidates,
L1Scoring::score and LoopClosing::DetectLoop
(tests/helpers/loopdetect_ref.cpp)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

TRACE_FIELDS = ("sharing", "max_common", "min_common", "scored", "passed", "at_min_score", "best_differs", "retained",
                "dropped", "duplicates", "at_min_common", "just_above", "neigh_summed", "neigh_skipped", "eleventh",
                "same_first_word")
PATHS = ("early", "no_candidate", "not_consistent", "detected")


class Trace(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in TRACE_FIELDS]

    def as_dict(self):
        return {n: getattr(self, n) for n in TRACE_FIELDS}


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libloopdetectref.so"))
        _lib.ld_create.restype = ctypes.c_void_p
        _lib.ld_score.restype = ctypes.c_double
        _lib.ld_score_vectors.restype = ctypes.c_double
        _lib.ld_set_last_loop.argtypes = [ctypes.c_void_p, ctypes.c_long]
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a.size else None


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def score_vectors(v1, v2) -> float:
    w1, x1, w2, x2 = _i32(v1[0]), np.ascontiguousarray(v1[1], np.float64), _i32(v2[0]), \
        np.ascontiguousarray(v2[1], np.float64)
    return lib().ld_score_vectors(_p(w1), _p(x1), len(w1), _p(w2), _p(x2), len(w2))


class RefWorld:
    """The restatement's keyframes, inverted file and DetectLoop state."""

    def __init__(self, consistency_th: int = 3):
        self.h = ctypes.c_void_p(lib().ld_create(int(consistency_th)))
        self.n = 0

    def __del__(self):
        if getattr(self, "h", None):
            lib().ld_destroy(self.h)
            self.h = None

    def insert(self, words, values) -> int:
        w, v = _i32(words), np.ascontiguousarray(values, np.float64).reshape(-1)
        self.n += 1
        return lib().ld_insert(self.h, _p(w), _p(v), len(w))

    def set_graph(self, kf, ordered, connected) -> None:
        o, c = _i32(list(ordered)), _i32(sorted(connected))
        lib().ld_set_graph(self.h, int(kf), _p(o), len(o), _p(c), len(c))

    def set_bad(self, kf, bad=True) -> None:
        lib().ld_set_bad(self.h, int(kf), int(bad))

    def add(self, kf) -> None:
        lib().ld_add(self.h, int(kf))

    def erase(self, kf) -> None:
        lib().ld_erase(self.h, int(kf))

    def clear(self) -> None:
        lib().ld_clear(self.h)

    def word_list(self, word) -> list:
        out = np.zeros(max(self.n, 1), np.int32)
        n = lib().ld_word_list(self.h, int(word), _p(out), len(out))
        return out[:n].tolist()

    def score(self, a, b) -> float:
        return lib().ld_score(self.h, int(a), int(b))

    def detect_candidates(self, kf, min_score) -> dict:
        words, score = np.zeros(self.n, np.int32), np.zeros(self.n, np.float32)
        cands = np.zeros(self.n, np.int32)
        tr = Trace()
        n = lib().ld_detect_candidates(self.h, int(kf), ctypes.c_float(min_score), _p(words), _p(score), _p(cands),
                                       ctypes.byref(tr))
        return dict(cands=cands[:n].copy(), words=words, score=score, min_common=tr.min_common, trace=tr.as_dict())

    def set_last_loop(self, kf_id) -> None:
        lib().ld_set_last_loop(self.h, int(kf_id))

    def detect_loop(self, kf):
        """-> (path name, minScore or None, mvpEnoughConsistentCandidates)."""
        ms = ctypes.c_float(-1)
        enough = np.zeros(self.n, np.int32)
        ne = ctypes.c_int32()
        path = lib().ld_detect_loop(self.h, int(kf), ctypes.byref(ms), _p(enough), ctypes.byref(ne))
        return PATHS[path], (None if path == 0 else ms.value), enough[:ne.value].tolist()

    def groups(self) -> list:
        """mvConsistentGroups as [(set of keyframes, counter)]."""
        cap_g, cap_m = 4 * self.n + 4, 4 * self.n * self.n + 4
        cnt, siz, mem = np.zeros(cap_g, np.int32), np.zeros(cap_g, np.int32), np.zeros(cap_m, np.int32)
        g = lib().ld_groups(self.h, _p(cnt), _p(siz), _p(mem), cap_g, cap_m)
        assert g >= 0
        out, o = [], 0
        for i in range(g):
            out.append((set(mem[o:o + siz[i]].tolist()), int(cnt[i])))
            o += siz[i]
        return out


class RefDatabase:
    """A CPU stand-in for loopdetect.KeyFrameDatabase over a second
    restatement world: the scoring and candidate functions a LoopDetector
    takes from its database."""

    def __init__(self):
        self.world = RefWorld()
        self.ordered = []

    def insert(self, words, values) -> int:
        return self.world.insert(words, values)

    def add(self, slot) -> None:
        self.world.add(slot)

    def erase(self, slot) -> None:
        self.world.erase(slot)

    def score_against(self, query, slots) -> np.ndarray:
        return np.asarray([np.float32(self.world.score(query, s)) for s in slots], np.float32)

    def detect_loop_candidates(self, query, connected, cov_off, cov, min_score, full=False):
        for k in range(self.world.n):
            self.world.set_graph(k, cov[cov_off[k]:cov_off[k + 1]], connected if k == query else ())
        r = self.world.detect_candidates(query, min_score)
        return r if full else r["cands"]
