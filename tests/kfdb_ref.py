"""ctypes wrapper of tests/helpers/libkfdbref.so, the serial CPU restatement of
the relocalisation keyframe database that grows (tests/helpers/kfdb_ref.cpp),
and the small database builders the tests share. A database is a
``pipeline.KeyframeDB`` (host arrays); its packed form is the dict
``KeyframeDB.read`` returns: the arrays of gf_keyframe_db plus inv_words /
inv_off / inv_kf and nkf."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from gf_orb_slam_amd.bow import FeatureVector
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
from gf_orb_slam_amd.pipeline import KeyframeDB, KeyframeDBArrays

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
ROW_KEYS = KeyframeDB._ARRAYS
KEYS = ROW_KEYS + ("inv_words", "inv_off", "inv_kf")


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libkfdbref.so"))
        for f in (_lib.kr_check, _lib.kr_build, _lib.kr_append):
            f.restype = ctypes.c_int
        _lib.kr_check.argtypes = [ctypes.c_void_p]
        _lib.kr_build.argtypes = [ctypes.c_void_p] * 5
        _lib.kr_append.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 2
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def check(db: KeyframeDB) -> int:
    return lib().kr_check(ctypes.byref(db.struct()))


def build(db: KeyframeDB):
    """KeyFrameDatabase::add for every keyframe of ``db`` in index order ->
    the packed database, or the verdict (< 0)."""
    nb = max(len(db.bow_words), 1)
    iw, io, ik = np.zeros(nb, np.int32), np.zeros(nb + 1, np.int32), np.zeros(nb, np.int32)
    sizes = np.zeros(4, np.int32)
    nw = lib().kr_build(ctypes.byref(db.struct()), _p(iw), _p(io), _p(ik), _p(sizes))
    if nw < 0:
        return nw
    out = {k: np.array(getattr(db, k), copy=True) for k in ROW_KEYS}
    out.update(inv_words=iw[:nw].copy(), inv_off=io[:nw + 1].copy(), inv_kf=ik[:int(sizes[1])].copy(), nkf=db.nkf)
    return out


class RefDB:
    """A database held at its capacities, as the device holds a growable one;
    ``append(rows)`` gives the verdict (0, -1, -3) and applies on 0."""

    def __init__(self, db: KeyframeDB, max_kf: int, max_rows: int, fill: int = 0):
        self.max_kf, self.max_rows = int(max_kf), int(max_rows)
        K, R = self.max_kf, max(self.max_rows, 1)
        shape = dict(kp_off=(K + 1, np.int32), kps=(R, KEYPOINT_DTYPE), desc=((R, 32), np.uint8),
                     bow_off=(K + 1, np.int32), bow_words=(R, np.int32), bow_values=(R, np.float64),
                     fv_off=(K + 1, np.int32), fv_nodes=(R, np.int32), fv_start=(R + 1, np.int32),
                     fv_feats=(R, np.int32), inv_words=(R, np.int32), inv_off=(R + 1, np.int32), inv_kf=(R, np.int32))
        self.a = {}
        for k, (sh, dt) in shape.items():
            self.a[k] = np.zeros(sh, dt)
            self.a[k].view(np.uint8)[...] = fill
        for k in ("kp_off", "bow_off", "fv_off", "fv_start", "inv_off"):
            self.a[k][0] = 0
        self.counts = np.zeros(6, np.int32)
        if db.nkf:
            rc = self.append(db)
            if rc:
                raise ValueError(f"the initial database is refused: {rc}")

    def _struct(self):
        return KeyframeDBArrays(int(self.counts[0]), *[self.a[k].ctypes.data for k in ROW_KEYS])

    def append(self, rows: KeyframeDB) -> int:
        st = self._struct()
        return lib().kr_append(ctypes.byref(st), _p(self.a["inv_words"]), _p(self.a["inv_off"]), _p(self.a["inv_kf"]),
                               _p(self.counts), ctypes.byref(rows.struct()), self.max_kf, self.max_rows)

    def packed(self) -> dict:
        nkf, nk, nb, nn, nf, nw = (int(c) for c in self.counts)
        n = dict(kp_off=nkf + 1, kps=nk, desc=nk, bow_off=nkf + 1, bow_words=nb, bow_values=nb, fv_off=nkf + 1,
                 fv_nodes=nn, fv_start=nn + 1, fv_feats=nf, inv_words=nw, inv_off=nw + 1, inv_kf=nb)
        out = {k: self.a[k][:n[k]].copy() for k in KEYS}
        out["nkf"] = nkf
        return out


def same(a: dict, b: dict) -> list:
    """The keys at which two packed databases differ in a byte."""
    bad = [k for k in KEYS if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
    return bad + (["nkf"] if int(a["nkf"]) != int(b["nkf"]) else [])


# ---------------------------------------------------------------- builders
def keyframe(rng, nkp: int, words, nodes_per: int = 3):
    """One keyframe's rows with the BowVector words given: random keypoints,
    descriptors and values, a FeatureVector that spreads the keypoints over a
    few ascending nodes. -> (kps, desc, words, values, FeatureVector)."""
    words = np.asarray(words, np.int32)
    kps = np.zeros(nkp, KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 700, nkp), rng.uniform(0, 400, nkp)
    kps["octave"] = rng.integers(0, 8, nkp)
    desc = rng.integers(0, 256, (nkp, 32), dtype=np.uint8)
    values = rng.uniform(0.01, 1.0, len(words))
    nn = min(nodes_per, nkp)
    nodes = np.sort(rng.choice(1000, nn, replace=False)).astype(np.int32) if nn else np.zeros(0, np.int32)
    cuts = np.sort(rng.integers(0, nkp + 1, max(nn - 1, 0)))
    start = np.concatenate([[0], cuts, [nkp]]).astype(np.int32) if nn else np.zeros(1, np.int32)
    feats = rng.permutation(nkp).astype(np.int32) if nn else np.zeros(0, np.int32)
    return kps, desc, words, values, FeatureVector(nodes, start, feats)


def db_of(kfs, max_kf=None, max_rows=None) -> KeyframeDB:
    """A KeyframeDB over the keyframes ``kfs`` (tuples of :func:`keyframe`)."""
    it = iter([(k[2], k[3], k[4]) for k in kfs])
    return KeyframeDB([k[0] for k in kfs], [k[1] for k in kfs], lambda d: next(it), max_kf=max_kf, max_rows=max_rows)


def random_keyframes(seed: int, nkf: int, nkp=(0, 12), vocab: int = 30):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nkf):
        n = int(rng.integers(nkp[0], nkp[1] + 1))
        nw = int(rng.integers(0, min(n, vocab) + 1))
        out.append(keyframe(rng, n, np.sort(rng.choice(vocab, nw, replace=False))))
    return out
