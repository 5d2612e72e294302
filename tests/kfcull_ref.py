"""ctypes wrapper of tests/helpers/libkfcullref.so: the serial CPU restatement
of LocalMapping::KeyFrameCulling, KeyFrame::SetBadFlag and the KeyFrame /
MapPoint calls it makes (tests/helpers/kfcull_ref.cpp)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_FIELDS = ("kf_bad", "mp_bad", "slots", "obs", "ref_kf", "parent", "weights", "ordered", "to_be_erased", "not_erase",
           "cand", "nmps", "nred", "culled_at", "deferred_at", "culled", "points_bad", "reparented", "flags",
           "children")
STATE = _FIELDS[:10]


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libkfcullref.so"))
        _lib.kr_create.restype = ctypes.c_void_p
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


def counts(kf_off, octave, slots, mp_bad, obs_off, obs_gkp, cand, flags=None, ctx=None):
    """The restatement's counting over the flat tables of
    ``gf_keyframe_culling_counts``, with the signature of
    ``localmapping.keyframe_culling_counts`` -> counts [ncand, 2]."""
    kf_off, slots, obs_off, obs_gkp, cand = (_i32(a) for a in (kf_off, slots, obs_off, obs_gkp, cand))
    octave, mp_bad = _u8(octave), _u8(mp_bad)
    out = np.zeros((max(len(cand), 1), 2), np.int32)
    if flags is not None:
        assert flags.dtype == np.uint8 and flags.flags.c_contiguous and len(flags) == len(slots)
    lib().kr_counts_arrays(len(kf_off) - 1, _p(kf_off), _p(octave), _p(slots), len(mp_bad), _p(mp_bad), _p(obs_off),
                           _p(obs_gkp), len(cand), _p(cand), _p(out), _p(flags))
    return out[:len(cand)]


def loopmap_state(m) -> dict:
    """The fields of :meth:`RefWorld.state` read off a LoopMap."""
    rows = lambda t: np.asarray(t, np.int32).reshape(-1, 3)  # noqa: E731
    return dict(kf_bad=m.kf_bad.astype(np.int32), mp_bad=m.mp_bad.astype(np.int32),
                slots=np.concatenate([np.zeros(0, np.int32)] + list(m.slots)).astype(np.int32),
                obs=m.observation_rows(), ref_kf=m.ref_kf.astype(np.int32), parent=np.asarray(m.parent, np.int32),
                weights=rows([(k, o, w[o]) for k, w in enumerate(m.weights) for o in sorted(w)]),
                ordered=rows([(k, o, w) for k in range(m.nkf) for o, w in zip(m.ordered[k], m.ordered_w[k])]),
                to_be_erased=m.to_be_erased.astype(np.int32), not_erase=m.not_erase.astype(np.int32))


def assert_same_state(m, w):
    """A LoopMap against the restatement's world, field by field."""
    a, b = loopmap_state(m), w.state()
    for name in STATE:
        assert np.array_equal(a[name], b[name]), name


class RefWorld:
    """The restatement's world: slot tables, octaves, observation maps,
    reference keyframes, the covisibility graph, the spanning tree, the loop
    edges and the erase flags."""

    def __init__(self, h, kf_n):
        self.h, self.kf_n = ctypes.c_void_p(h), list(kf_n)

    @classmethod
    def from_loopmap(cls, m):
        """A world equal to the LoopMap ``m`` as it stands, graph included."""
        kf_n = [len(k) for k in m.kf_kps]
        off = np.zeros(m.nkf + 1, np.int32)
        off[1:] = np.cumsum(kf_n)
        octave = _i32(np.concatenate([np.zeros(0, np.int32)] + [k["octave"] for k in m.kf_kps]))
        slots = _i32(np.concatenate([np.zeros(0, np.int32)] + list(m.slots)))
        rows = m.observation_rows()
        op, ok, oi = _i32(rows[:, 0]), _i32(rows[:, 1]), _i32(rows[:, 2])
        w_off, w_kf = _csr([sorted(w) for w in m.weights])
        w_w = _i32([w[o] for w in m.weights for o in sorted(w)])
        o_off, o_kf = _csr(m.ordered)
        o_w = _i32([x for l in m.ordered_w for x in l])
        le_off, le_kf = _csr(m.loop_edges)
        kb, mb, ne, tbe = _u8(m.kf_bad), _u8(m.mp_bad), _u8(m.not_erase), _u8(m.to_be_erased)
        ids, ref, par = _i32(m.kf_id), _i32(m.ref_kf), _i32(m.parent)
        h = lib().kr_create(m.nkf, _p(off), _p(octave), _p(slots), _p(kb), _p(ids), len(m.mps), _p(mb), _p(ref),
                            len(rows), _p(op), _p(ok), _p(oi), _p(par), _p(w_off), _p(w_kf), _p(w_w), _p(o_off),
                            _p(o_kf), _p(o_w), _p(le_off), _p(le_kf), _p(ne), _p(tbe))
        return cls(h, kf_n)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.kr_destroy(self.h)
            self.h = None

    def _field(self, name):
        i = _FIELDS.index(name)
        n = lib().kr_get(self.h, i, None)
        out = np.zeros(max(n, 1), np.int32)
        lib().kr_get(self.h, i, _p(out))
        return out[:n]

    def state(self) -> dict:
        s = {n: self._field(n) for n in STATE}
        for n in ("obs", "weights", "ordered"):
            s[n] = s[n].reshape(-1, 3)
        return s

    def log(self) -> dict:
        """points_bad and reparented [(child, new parent)] since the last
        clear_log / keyframe_culling."""
        return dict(points_bad=self._field("points_bad").tolist(),
                    reparented=[tuple(r) for r in self._field("reparented").reshape(-1, 2).tolist()])

    def clear_log(self):
        lib().kr_clear_log(self.h)

    def children(self, kf) -> set:
        rows = self._field("children").reshape(-1, 2)
        return set(int(c) for k, c in rows if k == kf)

    def set_bad_keyframe(self, kf) -> int:
        """-> 1 erased, 2 deferred, 0 returned (mnId 0)."""
        return lib().kr_set_bad_keyframe(self.h, int(kf))

    def erase_observation(self, p, kf):
        lib().kr_erase_observation(self.h, int(p), int(kf))

    def set_not_erase(self, kf):
        lib().kr_set_not_erase(self.h, int(kf))

    def set_erase(self, kf) -> int:
        return lib().kr_set_erase(self.h, int(kf))

    def count(self, kf):
        """-> (nmps, nredundant, flags of the keyframe's slots) on the world as it stands."""
        out, fl = np.zeros(2, np.int32), np.zeros(max(self.kf_n[kf], 1), np.int32)
        lib().kr_count(self.h, int(kf), _p(out), _p(fl))
        return int(out[0]), int(out[1]), fl[:self.kf_n[kf]].astype(np.uint8)

    def keyframe_culling(self, cur) -> dict:
        """-> dict: candidates; nmps / nredundant / culled / deferred per
        candidate and flags (a list of planes) at the candidate's turn; culled,
        points_bad, reparented in order."""
        lib().kr_keyframe_culling(self.h, int(cur))
        cand = self._field("cand").tolist()
        flat = self._field("flags").astype(np.uint8)
        cuts = np.cumsum([self.kf_n[k] for k in cand])[:-1] if cand else []
        r = dict(candidates=cand, nmps=self._field("nmps").tolist(), nredundant=self._field("nred").tolist(),
                 culled_at=self._field("culled_at").astype(bool).tolist(),
                 deferred_at=self._field("deferred_at").astype(bool).tolist(),
                 flags=np.split(flat, cuts) if cand else [], culled=self._field("culled").tolist())
        r.update(self.log())
        return r
