"""ctypes wrapper of tests/helpers/libmaptablesref.so: the serial CPU
restatement of ``gf_map_tables_apply`` / ``gf_map_tables_move``
(tests/helpers/maptables_ref.cpp), with the signatures of
``maptables.tables_apply`` / ``maptables.tables_move`` so that the pair
``APPLIER`` can stand in for the device in ``ResidentTables(applier=...)``."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
MT_ROW = 1024


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libmaptablesref.so"))
        _lib.mr_apply.restype = _lib.mr_move.restype = None
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def apply(kf_off, slots, mp_bad, obs_off, obs_gkp, slot_g, slot_v, bad_p, row_ids, row_op_off, ops, ctx=None,
          row_max=MT_ROW):
    """The journal applied in place to ``slots`` / ``mp_bad`` / ``obs_gkp``
    (contiguous int32 / uint8 / int32) -> status [2]."""
    for a, dt in ((slots, np.int32), (mp_bad, np.uint8), (obs_gkp, np.int32)):
        assert a.dtype == dt and a.flags.c_contiguous
    kf_off, obs_off, slot_g, slot_v, bad_p, row_ids, row_op_off, ops = (
        _i32(a) for a in (kf_off, obs_off, slot_g, slot_v, bad_p, row_ids, row_op_off, ops))
    assert len(obs_off) == len(mp_bad) + 1 and len(slot_g) == len(slot_v) and len(ops) % 3 == 0
    assert len(row_op_off) == len(row_ids) + 1 or (len(row_ids) == 0 and len(row_op_off) == 0)
    if not len(row_op_off):
        row_op_off = np.zeros(1, np.int32)
    status = np.full(2, -9, np.int32)
    lib().mr_apply(len(kf_off) - 1, _p(kf_off), _p(slots), len(mp_bad), _p(mp_bad), _p(obs_off), _p(obs_gkp),
                   len(slot_g), _p(slot_g), _p(slot_v), len(bad_p), _p(bad_p), len(row_ids), _p(row_ids),
                   _p(row_op_off), len(ops) // 3, _p(ops), int(row_max), _p(status))
    return status


def move(old_off, old_gkp, new_off, new_gkp, ctx=None):
    """The regrow into ``new_gkp`` (contiguous int32, every entry written) ->
    status [1]."""
    assert new_gkp.dtype == np.int32 and new_gkp.flags.c_contiguous
    old_off, old_gkp, new_off = _i32(old_off), _i32(old_gkp), _i32(new_off)
    assert len(old_off) == len(new_off)
    status = np.full(1, -9, np.int32)
    lib().mr_move(max(len(old_off) - 1, 0), _p(old_off), _p(old_gkp), _p(new_off), _p(new_gkp), _p(status))
    return status


APPLIER = (apply, move)
