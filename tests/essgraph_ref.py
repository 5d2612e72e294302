"""ctypes loader of tests/helpers/libessgraphref.so, the tests' CPU restatement
of Optimizer::OptimizeEssentialGraph (tests/helpers/essgraph_ref.cpp)."""
import ctypes
import os

import numpy as np

from gf_orb_slam_amd._lib import ESSGRAPH_TRACE, EssGraphStats, ptr
from gf_orb_slam_amd.optimizer import EssGraphArrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLT, LDLT = 0, 1
_ref = None


def ref():
    global _ref
    if _ref is None:
        _ref = ctypes.CDLL(os.path.join(ROOT, "tests", "helpers", "libessgraphref.so"))
        for f in ("egref_exp", "egref_log", "egref_mul", "egref_inverse", "egref_from_pose", "egref_edge_error",
                  "egref_edge_jacobian"):
            getattr(_ref, f).restype = None
        _ref.egref_edges.restype = ctypes.c_int
        _ref.egref_solve.restype = ctypes.c_int
    return _ref


def _d(a, n):
    return np.ascontiguousarray(a, np.float64).reshape(n)


def sim_exp(u):
    S, u = np.zeros(8), _d(u, 7)
    ref().egref_exp(ptr(u), ptr(S))
    return S


def sim_log(S):
    u, S = np.zeros(7), _d(S, 8)
    ref().egref_log(ptr(S), ptr(u))
    return u


def sim_mul(a, b):
    r, a, b = np.zeros(8), _d(a, 8), _d(b, 8)
    ref().egref_mul(ptr(a), ptr(b), ptr(r))
    return r


def sim_inverse(a):
    r, a = np.zeros(8), _d(a, 8)
    ref().egref_inverse(ptr(a), ptr(r))
    return r


def sim_from_pose(T):
    S = np.zeros(8)
    T = np.ascontiguousarray(T, np.float32).reshape(16)
    ref().egref_from_pose(ptr(T), ptr(S))
    return S


def edge_error(C, v1, v2):
    e, C, v1, v2 = np.zeros(7), _d(C, 8), _d(v1, 8), _d(v2, 8)
    ref().egref_edge_error(ptr(C), ptr(v1), ptr(v2), ptr(e))
    return e


def edge_jacobian(C, v1, v2):
    """BaseBinaryEdge's central differences of one EdgeSim3 -> (Ji, Jj), 7 x 7 each (row = error component)."""
    Ji, Jj = np.zeros((7, 7)), np.zeros((7, 7))
    C, v1, v2 = _d(C, 8), _d(v1, 8), _d(v2, 8)
    ref().egref_edge_jacobian(ptr(C), ptr(v1), ptr(v2), ptr(Ji), ptr(Jj))
    return Ji, Jj


def edges(args) -> np.ndarray:
    """The restatement's edge rows (i, j, kind) of one problem (the argument tuple of EssGraphArrays)."""
    arr = args if isinstance(args, EssGraphArrays) else EssGraphArrays(*args)
    n = ref().egref_edges(ctypes.byref(arr.problem), None, 0)
    rows = np.zeros((max(n, 1), 3), np.int32)
    ref().egref_edges(ctypes.byref(arr.problem), ptr(rows), n)
    return rows[:n].copy()


def solve(args, solver=LLT, reverse=False, jac_edge=-1) -> dict:
    """The restated OptimizeEssentialGraph -> the dict of EssGraphArrays.out(), plus J (2, 7, 7) of jac_edge."""
    arr = args if isinstance(args, EssGraphArrays) else EssGraphArrays(*args)
    st = EssGraphStats()
    J = np.zeros((2, 7, 7))
    assert arr.trace_lambda.size == ESSGRAPH_TRACE
    pos = arr.pos if arr.M else np.zeros((1, 3), np.float32)
    ref().egref_solve(ctypes.byref(arr.problem), int(solver), int(bool(reverse)), ptr(arr.Tcw), ptr(pos),
                      ctypes.byref(st), ptr(arr.trace_lambda), ptr(arr.trace_chi2), ptr(arr.trace_accepted),
                      int(jac_edge), ptr(J))
    out = arr.out(st)
    out["J"] = J
    return out
