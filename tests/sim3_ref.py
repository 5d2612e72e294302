"""ctypes loader of tests/helpers/libsim3ref.so, the tests' CPU restatement of
Sim3Solver (tests/helpers/sim3_ref.cpp). std::rand() values are pre-drawn with
gf_rng_next and handed over as an array."""
import ctypes
import os

import numpy as np

from gf_orb_slam_amd._lib import check, lib, ptr
from gf_orb_slam_amd.pnp import RNG_DTYPE
from gf_orb_slam_amd.sim3 import SIM3_STATE_DTYPE, sim3_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ref = None


def ref():
    global _ref
    if _ref is None:
        _ref = ctypes.CDLL(os.path.join(ROOT, "tests", "helpers", "libsim3ref.so"))
    return _ref


def rand_values(seed, count):
    """The first `count` std::rand() values after std::srand(seed)."""
    g = np.zeros(1, RNG_DTYPE)
    check(lib().gf_rng_seed(ptr(g), ctypes.c_uint32(seed)))
    out = np.zeros(max(count, 1), np.int32)
    if count:
        check(lib().gf_rng_next(ptr(g), ptr(out), count))
    return out


def init(n, **kw):
    st = np.zeros(1, SIM3_STATE_DTYPE)
    assert ref().sim3ref_init(int(n), ptr(sim3_params(**kw)), ptr(st)) == 0
    return st


class RefSolver:
    """One restated solver over several iterate() calls; `rand` is a shared
    [values, cursor] pair so that several solvers can interleave one stream."""

    def __init__(self, X1, X2, s1, s2, K1, K2, rand, **params):
        self.X1 = np.ascontiguousarray(X1, np.float32).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X2, np.float32).reshape(-1, 3)
        self.s1 = np.ascontiguousarray(s1, np.float32)
        self.s2 = np.ascontiguousarray(s2, np.float32)
        self.K1 = np.asarray(K1, np.float32).reshape(4)
        self.K2 = np.asarray(K2, np.float32).reshape(4)
        self.n = len(self.X1)
        self.state = init(self.n, **params)
        self.best_mask = np.zeros(max(self.n, 1), np.uint8)
        self.rand = rand

    def iterate(self, n_iterations):
        """-> (T12[16], inliers[n], ninliers, flags, rand() values consumed so far)"""
        T = np.zeros(16, np.float32)
        inl = np.zeros(max(self.n, 1), np.uint8)
        ni = np.zeros(1, np.int32)
        fl = np.zeros(1, np.int32)
        cur = np.array([self.rand[1]], np.int32)
        vals = self.rand[0]
        assert ref().sim3ref_iterate(ptr(self.X1), ptr(self.X2), ptr(self.s1), ptr(self.s2), ptr(self.K1),
                                     ptr(self.K2), ptr(self.state), ptr(self.best_mask), int(n_iterations),
                                     ptr(vals), len(vals), ptr(cur), ptr(T), ptr(inl), ptr(ni), ptr(fl)) == 0
        assert cur[0] <= len(vals), "pre-drawn rand() values exhausted"
        self.rand[1] = int(cur[0])
        return T, inl[:self.n].copy(), int(ni[0]), int(fl[0]), int(cur[0])


def search_by_sim3(info, T1, kps1, desc1, ids1, T2, kps2, desc2, ids2, mps, mp_desc, mp_bad, matches12, s12, R12, t12,
                   th):
    """The restated ORBmatcher::SearchBySim3 -> (matches12, nfound)."""
    c = np.ascontiguousarray
    m12 = c(matches12, np.int32).copy()
    T1, T2 = c(T1, np.float32).reshape(16), c(T2, np.float32).reshape(16)
    kps1, kps2, desc1, desc2 = c(kps1), c(kps2), c(desc1, np.uint8), c(desc2, np.uint8)
    ids1, ids2 = c(ids1, np.int32), c(ids2, np.int32)
    mps, mp_desc = c(mps), c(mp_desc, np.uint8)
    bad = None if mp_bad is None else c(np.asarray(mp_bad).astype(np.uint8))
    R, t = c(R12, np.float32).reshape(9), c(t12, np.float32).reshape(3)
    f = ref().sim3ref_search_by_sim3
    f.restype = ctypes.c_int
    nf = f(ctypes.byref(info), ptr(T1), ptr(kps1), ptr(desc1), len(kps1), ptr(ids1), ptr(T2), ptr(kps2), ptr(desc2),
           len(kps2), ptr(ids2), ptr(mps), ptr(mp_desc), ptr(bad), ptr(m12), ctypes.c_float(s12), ptr(R), ptr(t),
           ctypes.c_float(th))
    return m12, int(nf)


def run(X1, X2, s1, s2, K1, K2, seed, calls, **params):
    """A fresh solver, `calls` successive iterate() counts -> list of
    (T12, inliers, ninliers, flags, draws, state copy, best_mask copy)."""
    rand = [rand_values(seed, 3 * (sum(calls) + 1)), 0]
    s = RefSolver(X1, X2, s1, s2, K1, K2, rand, **params)
    out = []
    for c in calls:
        r = s.iterate(c)
        out.append(r + (s.state.copy(), s.best_mask[:s.n].copy()))
    return out
