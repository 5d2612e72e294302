"""ctypes wrapper of tests/helpers/libnewkeyframeref.so: the serial CPU
restatement of Tracking::NeedNewKeyFrame / CreateNewKeyFrame,
KeyFrame::TrackedMapPoints, the KeyFrame snapshot, the flag effects of
LocalMapping::InsertKeyFrame / InterruptBA / SetAcceptKeyFrames and the packed
hand-over (tests/helpers/newkeyframe_ref.cpp)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

WORDS = ("since", "accept", "stop", "nkf", "abort", "decision", "ref", "ref_matches", "inliers", "seq", "pending",
         "frame")
W = {k: i for i, k in enumerate(WORDS)}
NWORDS = 16
BITS = dict(evaluated=1, stop=2, reloc=4, c1a=8, c1b=16, c2=32, created=64, interrupt_ba=128, no_reference=256)
HDR_DTYPE = np.dtype([("stream", "<i4"), ("seq", "<i4"), ("frame_id", "<i4"), ("n", "<i4"), ("timestamp", "<f8"),
                      ("Tcw", "<f4", (16,))])
KP_BYTES = 28


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(_HERE, "helpers", "libnewkeyframeref.so"))
        _lib.nk_stage.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 +
                                  [ctypes.c_void_p] * 4 + [ctypes.c_double] + [ctypes.c_void_p] * 4)
        _lib.nk_take.argtypes = ([ctypes.c_int] * 2 + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 2 +
                                 [ctypes.c_void_p] * 6)
        _lib.nk_tracked_map_points.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.nk_set_accept.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return _lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def rule(since_kf, since_reloc, stop, nkf, n_ref, inliers, accept, min_frames, max_frames) -> int:
    """The decision bits of NeedNewKeyFrame on scalars (n_ref < 0: no reference keyframe)."""
    return lib().nk_rule(int(since_kf), int(since_reloc), int(stop), int(nkf), int(n_ref), int(inliers), int(accept),
                         int(min_frames), int(max_frames))


def tracked_map_points(slots) -> int:
    s = np.ascontiguousarray(slots, np.int32)
    return lib().nk_tracked_map_points(_p(s) if len(s) else None, len(s))


def new_state(B: int) -> np.ndarray:
    """The state after the stage is switched on: SINCE 0, ACCEPT 1, NKF -1."""
    st = np.zeros((B, NWORDS), np.int32)
    st[:, W["accept"]] = 1
    st[:, W["nkf"]] = -1
    return st


def set_accept(state_row: np.ndarray, flag: bool) -> int:
    return lib().nk_set_accept(_p(state_row), int(flag))


class Outbox:
    """[B] headers and [B][cap] rows, pre-filled with a sentinel."""

    def __init__(self, B: int, cap: int, sentinel: int = 0xA5):
        self.B, self.cap = B, cap
        self.hdr = np.frombuffer(bytes([sentinel]) * (HDR_DTYPE.itemsize * B), HDR_DTYPE).copy()
        self.kps = np.full((B, cap, KP_BYTES), sentinel, np.uint8)
        self.desc = np.full((B, cap, 32), sentinel, np.uint8)
        self.slots = np.frombuffer(bytes([sentinel]) * (4 * B * cap), np.int32).reshape(B, cap).copy()


def stage(state, box: Outbox, b, working, ref, kf_count, kf_off, kf_mp, since_reloc, frame_id, inliers, min_frames,
          max_frames, n, kps, desc, kp2mp, Tcw, timestamp) -> bool:
    """One stream's stage of one step on state[b] and box slot b (arrays of
    this stream: kf_off / kf_mp its graph's slot CSR; kps as [n][28] bytes or
    a KEYPOINT_DTYPE array)."""
    kf_off, kf_mp = np.ascontiguousarray(kf_off, np.int32), np.ascontiguousarray(kf_mp, np.int32)
    kps = np.ascontiguousarray(kps).view(np.uint8).reshape(-1)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1)
    kp2mp = np.ascontiguousarray(kp2mp, np.int32)
    Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    assert len(kps) >= n * KP_BYTES and len(desc) >= 32 * n and len(kp2mp) >= n
    row = state[b]
    assert row.flags["C_CONTIGUOUS"]
    return bool(lib().nk_stage(_p(row), int(b), int(bool(working)), int(ref), int(kf_count), _p(kf_off),
                               _p(kf_mp) if len(kf_mp) else None, int(since_reloc), int(frame_id), int(inliers),
                               int(min_frames), int(max_frames), int(n), _p(kps) if len(kps) else None,
                               _p(desc) if len(desc) else None, _p(kp2mp) if len(kp2mp) else None, _p(Tcw),
                               float(timestamp), _p(box.hdr[b:b + 1]), _p(box.kps[b]), _p(box.desc[b]),
                               _p(box.slots[b])))


def take(state, box: Outbox, max_kf: int, rows_cap: int):
    """The packed hand-over -> (rc, hdr [nkf], kps [nrows][28], desc, slots, nrows
    reported); PENDING of the taken streams is cleared in state."""
    B, cap = box.B, box.cap
    k = max(max_kf, 1)
    r = max(rows_cap, 1)
    hdr = np.zeros(k, HDR_DTYPE)
    kps, desc, slots = np.zeros((r, KP_BYTES), np.uint8), np.zeros((r, 32), np.uint8), np.zeros(r, np.int32)
    nkf, nrows = ctypes.c_int(), ctypes.c_int()
    assert state.flags["C_CONTIGUOUS"] and state.shape == (B, NWORDS)
    rc = lib().nk_take(B, cap, _p(state), _p(box.hdr), _p(box.kps), _p(box.desc), _p(box.slots), int(max_kf),
                       int(rows_cap), _p(hdr), _p(kps), _p(desc), _p(slots), ctypes.byref(nkf), ctypes.byref(nrows))
    n = nrows.value if rc == 0 else 0
    return rc, hdr[:nkf.value], kps[:n], desc[:n], slots[:n], nrows.value
