"""ctypes wrapper of tests/helpers/libcovisref.so: the serial CPU restatement
of KeyFrame::UpdateConnections over raw flat tables and on a small world, and
of the index state of LocalMapping::ProcessNewKeyFrame
(tests/helpers/covis_ref.cpp)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_FIELDS = ("slots", "obs", "weights", "ordered", "parent", "first_connection", "recent", "associated", "bow_computed")
STATE = _FIELDS[:6]


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libcovisref.so"))
        _lib.cr_create.restype = ctypes.c_void_p
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _u8(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.uint8)).reshape(-1)


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, _i32([v for x in lists for v in x])


def counts(kf_off, slots, mp_bad, obs_off, obs_gkp, query, ctx=None):
    """The restatement's counting and ordering over the flat tables of
    ``gf_update_connections``, with the signature of
    ``localmapping.update_connections_counts`` -> (weights [nq, nkf],
    n_ordered [nq], ordered_kf [nq, nkf], ordered_w [nq, nkf])."""
    kf_off, slots, obs_off, obs_gkp, query = (_i32(a) for a in (kf_off, slots, obs_off, obs_gkp, query))
    mp_bad = _u8(mp_bad)
    nkf, nq = len(kf_off) - 1, len(query)
    w, n = np.full((nq, nkf), -9, np.int32), np.full(nq, -9, np.int32)
    ok, ow = np.full((nq, nkf), -9, np.int32), np.full((nq, nkf), -9, np.int32)
    lib().cr_counts(nkf, _p(kf_off), _p(slots), len(mp_bad), _p(mp_bad), _p(obs_off), _p(obs_gkp), nq, _p(query),
                    _p(w), _p(n), _p(ok), _p(ow))
    return w, n, ok, ow


def loopmap_state(m) -> dict:
    """The fields of :meth:`RefWorld.state` read off a LoopMap."""
    rows = lambda t: np.asarray(t, np.int32).reshape(-1, 3)  # noqa: E731
    return dict(slots=np.concatenate([np.zeros(0, np.int32)] + list(m.slots)).astype(np.int32),
                obs=m.observation_rows(),
                weights=rows([(k, o, w[o]) for k, w in enumerate(m.weights) for o in sorted(w)]),
                ordered=rows([(k, o, w) for k in range(m.nkf) for o, w in zip(m.ordered[k], m.ordered_w[k])]),
                parent=np.asarray(m.parent, np.int32), first_connection=np.asarray(m.first_connection, np.int32))


def assert_same_state(m, w):
    """A LoopMap against the restatement's world, field by field."""
    a, b = loopmap_state(m), w.state()
    for name in STATE:
        assert np.array_equal(a[name], b[name]), name


def assert_same_maps(a, b):
    """Two LoopMaps, every index field and every array, bit for bit."""
    x, y = loopmap_state(a), loopmap_state(b)
    for name in STATE:
        assert np.array_equal(x[name], y[name]), name
    assert a.nkf == b.nkf and len(a.mps) == len(b.mps)
    for name in ("kf_bad", "mp_bad", "kf_id", "ref_kf", "first_kf", "found", "visible", "fuse_target_for",
                 "fuse_candidate_for", "not_erase", "to_be_erased", "desc_epoch"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.mps.tobytes() == b.mps.tobytes(), "mps"
    assert a.mp_desc.tobytes() == b.mp_desc.tobytes(), "mp_desc"
    assert a.Tcw.tobytes() == b.Tcw.tobytes(), "Tcw"
    assert a.loop_edges == b.loop_edges


class RefWorld:
    """The restatement's world: slot tables, mnIds, bad flags, observation
    maps, the recent list and the covisibility graph with parents."""

    def __init__(self, h):
        self.h = ctypes.c_void_p(h)

    @classmethod
    def from_loopmap(cls, m, recent=()):
        """A world equal to the LoopMap ``m`` as it stands, graph included."""
        off = np.zeros(m.nkf + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in m.slots])
        slots = _i32(np.concatenate([np.zeros(0, np.int32)] + list(m.slots)))
        rows = m.observation_rows()
        op, ok, oi = _i32(rows[:, 0]), _i32(rows[:, 1]), _i32(rows[:, 2])
        w_off, w_kf = _csr([sorted(w) for w in m.weights])
        w_w = _i32([w[o] for w in m.weights for o in sorted(w)])
        o_off, o_kf = _csr(m.ordered)
        o_w = _i32([x for l in m.ordered_w for x in l])
        ids, par, fc = _i32(m.kf_id), _i32(m.parent), _u8(m.first_connection)
        bow = _u8([b is not None and f is not None for b, f in zip(m.kf_bow, m.kf_fv)])
        mb = _u8(m.mp_bad)
        w = cls(lib().cr_create(m.nkf, _p(off), _p(slots), _p(ids), _p(par), _p(fc), _p(bow), _p(w_off), _p(w_kf),
                                _p(w_w), _p(o_off), _p(o_kf), _p(o_w), len(m.mps), _p(mb), len(rows), _p(op), _p(ok),
                                _p(oi)))
        w.set_recent(recent)
        return w

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.cr_destroy(self.h)
            self.h = None

    def _field(self, name):
        i = _FIELDS.index(name)
        n = lib().cr_get(self.h, i, None)
        out = np.zeros(max(n, 1), np.int32)
        lib().cr_get(self.h, i, _p(out))
        return out[:n]

    def state(self) -> dict:
        s = {n: self._field(n) for n in STATE}
        for n in ("obs", "weights", "ordered"):
            s[n] = s[n].reshape(-1, 3)
        return s

    def add_keyframe(self, slots, kf_id) -> int:
        s = _i32(slots)
        return lib().cr_add_keyframe(self.h, len(s), _p(s), int(kf_id))

    def set_recent(self, ids):
        ids = _i32(list(ids))
        lib().cr_set_recent(self.h, len(ids), _p(ids))

    def update_connections(self, kf):
        lib().cr_update_connections(self.h, int(kf))

    def process_new_keyframe(self, kf) -> dict:
        """-> dict: associated (ids in slot order), recent (the whole list
        afterwards), bow_computed (per keyframe, how often ComputeBoW worked)."""
        lib().cr_process_new_keyframe(self.h, int(kf))
        return dict(associated=self._field("associated").tolist(), recent=self._field("recent").tolist(),
                    bow_computed=self._field("bow_computed").tolist())
