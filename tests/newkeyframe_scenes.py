"""Inputs of the NeedNewKeyFrame / CreateNewKeyFrame tests: problems for one
``gf_need_new_keyframe_dev`` launch as host arrays (``Problem``), the
restatement run over them (``run_ref``) and the device run (``run_dev``)."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np

import newkeyframe_ref as R

MAXF = 12  # mMaxFrames of the synthetic problems (18 * 20 fps / 30)
SENTINEL = 0xA5


class Problem:
    """B streams: frames (rows of 28-byte keypoints, descriptors, map point per
    keypoint), tracking words, per-stream graphs (slot CSR) and state."""

    def __init__(self, B, cap, off_stride, slot_stride, min_frames=0, max_frames=MAXF, seed=0):
        rng = np.random.default_rng(seed)
        self.B, self.cap, self.off_stride, self.slot_stride = B, cap, off_stride, slot_stride
        self.min_frames, self.max_frames = min_frames, max_frames
        self.nkp = rng.integers(0, cap + 1, B).astype(np.int32)
        self.kps = rng.integers(0, 256, (B, cap, R.KP_BYTES), dtype=np.uint8)
        self.desc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
        self.kp2mp = rng.integers(-1, 500, (B, cap)).astype(np.int32)
        self.Tcw = rng.standard_normal((B, 16)).astype(np.float32)
        self.t_cur = rng.uniform(0, 100, B)
        self.track = np.zeros((B, 8), np.int32)
        self.track[:, 2] = 1 << 30               # GF_TR_SINCE: no relocalisation so far
        self.track[:, 4] = rng.integers(1, 10000, B)  # GF_TR_QUERY: mnId
        self.inliers = np.full(B, 100, np.int32)
        self.working = np.ones(B, np.int32)
        self.ref_kf = np.zeros(B, np.int32)
        self.kf_count = np.ones(B, np.int32)
        self.kf_mp_off = np.zeros((B, off_stride), np.int32)
        self.kf_mp = np.full((B, max(slot_stride, 1)), -7, np.int32)  # outside the rows: not -1, so a stray read counts
        self.state = R.new_state(B)
        self.state[:, R.W["since"]] = 1000       # long since the last keyframe

    def set_row(self, b, length, fill, ref=0, start=0, nkf=None):
        """Reference keyframe `ref` of stream b gets a slot row of `length`
        starting at CSR offset `start`; fill: array or scalar."""
        nkf = ref + 1 if nkf is None else nkf
        off = self.kf_mp_off[b]
        off[:] = start + length          # the keyframes after it are empty
        off[:ref + 1] = start            # those before it too, but keyframe 0, which owns [0, start)
        if ref:
            off[0] = 0
        self.kf_mp[b, start:start + length] = fill
        self.ref_kf[b], self.kf_count[b] = ref, nkf


def truth_table(min_frames=0, seed=1) -> Problem:
    """Every combination of WORKING / not, STOP, relocalisation gate, SINCE
    around mMaxFrames, ACCEPT, inliers 15 / 16 and reference / none."""
    since = (0, MAXF - 2, MAXF - 1, MAXF)  # the frame's value is + 1: both sides of c1a, and of c1b's min_frames
    combos = list(itertools.product((1, 0), (0, 1), (0, 1), since, (1, 0), (15, 16), (0, -1)))
    B = len(combos)
    p = Problem(B, 70, 4, 64, min_frames=min_frames, seed=seed)
    for b, (working, stop, gate, s, accept, inl, ref) in enumerate(combos):
        p.working[b] = working
        p.state[b, R.W["stop"]] = stop
        # :3046 refuses when mnId < mnLastRelocFrameId + mMaxFrames and KeyFramesInMap() > mMaxFrames
        p.track[b, 2] = MAXF - 1 if gate else MAXF
        p.state[b, R.W["nkf"]] = MAXF + 1 if gate else (-1 if b % 2 else MAXF)
        p.state[b, R.W["since"]] = s
        p.state[b, R.W["accept"]] = accept
        p.inliers[b] = inl
        p.set_row(b, 40, np.where(np.arange(40) % 5 == 0, -1, 3), ref=1, start=3, nkf=2)  # 32 tracked: 0.9 * 32 = 28.8
        p.ref_kf[b] = 1 if ref == 0 else -1
    return p


def c2_boundary(seed=2) -> Problem:
    """Every nRef in 0..1030 with inliers floor(0.9 nRef) - 1, floor, + 1."""
    cases = [(n, (9 * n) // 10 + d) for n in range(1031) for d in (-1, 0, 1)]
    p = Problem(len(cases), 8, 2, 1032, seed=seed)
    for b, (n, inl) in enumerate(cases):
        p.set_row(b, n, 5, ref=0, start=b % 2)
        p.inliers[b] = inl
    return p


COUNT_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)


def count_rows(cap=1030, seed=3) -> Problem:
    """Reference rows of the listed lengths and `cap` at odd CSR offsets
    (every 16-byte phase of the row's start occurs: the stream stride is odd),
    filled all NULL, all set, mixed."""
    rng = np.random.default_rng(seed)
    cases = [(n, f) for n in COUNT_LENGTHS + (cap,) for f in range(3)]
    p = Problem(len(cases), 16, 4, cap + 9, seed=seed)
    for b, (n, f) in enumerate(cases):
        fill = (np.full(n, -1), rng.integers(0, 2000, n), np.where(rng.random(n) < 0.4, -1, rng.integers(0, 2000, n)))[f]
        p.set_row(b, n, fill, ref=2, start=1 + 2 * (b % 4), nkf=3)
        p.inliers[b] = 16
    return p


SNAP_N = (0, 1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 1030)


def snapshot(cap=1030, seed=4) -> Problem:
    """Creating streams with the listed N, then three that do not create (not
    WORKING, stopped, mapper busy)."""
    B = len(SNAP_N) + 3
    p = Problem(B, cap, 2, 64, seed=seed)
    p.kp2mp = np.random.default_rng(seed).integers(-1, 2600, (B, cap)).astype(np.int32)
    for b in range(B):
        p.set_row(b, 60, 9)
        p.inliers[b] = 30
    p.nkp[:len(SNAP_N)] = SNAP_N
    p.nkp[len(SNAP_N):] = 500
    p.working[len(SNAP_N)] = 0
    p.state[len(SNAP_N) + 1, R.W["stop"]] = 1
    p.state[len(SNAP_N) + 2, R.W["accept"]] = 0
    return p


def run_ref(p: Problem, state=None, box=None):
    """The restatement over every stream -> (state [B][16], Outbox)."""
    st = p.state.copy() if state is None else state
    box = R.Outbox(p.B, p.cap, SENTINEL) if box is None else box
    for b in range(p.B):
        R.stage(st, box, b, p.working[b], p.ref_kf[b], p.kf_count[b], p.kf_mp_off[b], p.kf_mp[b], p.track[b, 2],
                p.track[b, 4], p.inliers[b], p.min_frames, p.max_frames, p.nkp[b], p.kps[b], p.desc[b], p.kp2mp[b],
                p.Tcw[b], p.t_cur[b])
    return st, box


def run_dev(p: Problem, ctx, state_ptr=None, box_ptrs=None):
    """One gf_need_new_keyframe_dev launch. Without state_ptr / box_ptrs the
    state and a sentinel-filled outbox are uploaded and read back ->
    (state, Outbox); with them (device addresses, e.g. a front end's) nothing
    is returned."""
    import torch

    from gf_orb_slam_amd._lib import check, lib
    from gf_orb_slam_amd.pipeline import NewKfArgs

    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    names = ("nkp", "kps", "desc", "kp2mp", "Tcw", "t_cur", "track", "inliers", "working", "ref_kf", "kf_count",
             "kf_mp_off", "kf_mp")
    t = {k: up(getattr(p, k)) for k in names}
    own = state_ptr is None
    if own:
        ref_box = R.Outbox(p.B, p.cap, SENTINEL)
        t["state"] = up(p.state)
        t["out_hdr"], t["out_kps"] = up(ref_box.hdr.view(np.uint8)), up(ref_box.kps)
        t["out_desc"], t["out_slots"] = up(ref_box.desc), up(ref_box.slots)
        out = {k: t[k].data_ptr() for k in ("state", "out_hdr", "out_kps", "out_desc", "out_slots")}
    else:
        out = dict(state=state_ptr, out_hdr=box_ptrs["hdr"], out_kps=box_ptrs["kps"], out_desc=box_ptrs["desc"],
                   out_slots=box_ptrs["slots"])
    a = NewKfArgs(p.B, p.cap, *[t[k].data_ptr() for k in names], p.off_stride, p.kf_mp.shape[1], out["state"],
                  out["out_hdr"], out["out_kps"], out["out_desc"], out["out_slots"], p.min_frames, p.max_frames)
    check(lib().gf_need_new_keyframe_dev(ctx.handle, ctypes.byref(a), None))
    torch.cuda.synchronize()
    if not own:
        return None
    box = R.Outbox(p.B, p.cap, SENTINEL)
    box.hdr = t["out_hdr"].cpu().numpy().view(R.HDR_DTYPE).reshape(-1).copy()
    box.kps, box.desc, box.slots = (t[k].cpu().numpy() for k in ("out_kps", "out_desc", "out_slots"))
    return t["state"].cpu().numpy(), box


def assert_same(dev, ref, what=""):
    """(state, Outbox) pairs, every word and every byte."""
    sd, bd = dev
    sr, br = ref
    for k, i in R.W.items():
        bad = np.nonzero(sd[:, i] != sr[:, i])[0]
        assert not len(bad), f"{what}state word {k} differs on streams {bad[:8].tolist()}: " \
                             f"{sd[bad[:8], i].tolist()} vs {sr[bad[:8], i].tolist()}"
    assert np.array_equal(sd, sr), what + "state padding words differ"
    assert bd.hdr.tobytes() == br.hdr.tobytes(), what + "outbox headers differ"
    for k in ("kps", "desc", "slots"):
        a, b = getattr(bd, k), getattr(br, k)
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        assert not len(bad), f"{what}outbox {k} differ on streams {bad.tolist()}"
