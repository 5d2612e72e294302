"""Stream start without a GPU: the restatement (tests/streamstart_ref.py)
against a hand-written table, its verdicts on every refusal,
tracking.MapFeedback.start / KeyFrameInserter.start / poll_resets against a
stub front end, and the reduced last frame: two oracle chains loaded with the
full and with the reduced mLastFrame give equal steps."""
from types import SimpleNamespace

import numpy as np
import pytest

import mapupdate_ref as MR
import mapupdate_scenes as S
import oracle_chain as C
import oracle_lib as O
import streamstart_ref as R
import streamstart_scenes as SS
from gf_orb_slam_amd import tracking
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.bow import FeatureVector
from gf_orb_slam_amd.localmap import MapDelta, StreamStart
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, MP_VIEW_DTYPE
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
from gf_orb_slam_amd.pipeline import KF, RELOC_KF_DTYPE, TR


def _before(cap, M, seed=0):
    """A stream that holds sentinels everywhere."""
    rng = np.random.default_rng(seed)
    z = lambda shape, dt: np.full(shape, 0, dt)  # noqa: E731
    st = dict(map=z(M, MAP_POINT_DTYPE), map_desc=z((M, 32), np.uint8), views=z(M, MP_VIEW_DTYPE), mp_upd=z(M, np.int32),
              last_kps=z(cap, KEYPOINT_DTYPE), last_desc=z((cap, 32), np.uint8), last_kp2mp=z(cap, np.int32),
              last_outlier=z(cap, np.uint8), last_pos=z((cap, 3), np.float32), kp2mp=z(cap, np.int32),
              outlier=z(cap, np.uint8), reloc=z(64, RELOC_KF_DTYPE))
    for a in st.values():
        a.view(np.uint8)[...] = S.SENTINEL
    st.update(nmp=np.int32(3), last_nkp=np.int32(2), Tcw_last=rng.normal(size=16).astype(np.float32),
              t_prev=np.float64(7.5), t_cur=np.float64(7.55), track=np.array([2, 1, 9, 4, 77, 0, 5, 6], np.int32),
              Xv=rng.normal(size=13), Xv_next=rng.normal(size=13), base=rng.normal(size=49),
              mp_H=rng.normal(size=(M, 14)), velocity=rng.normal(size=16).astype(np.float32), nleft=4,
              graph=SS.EMPTY["graph"], kf={w: 3 for w in KF})
    return st


def test_restatement_against_a_hand_written_table():
    """Two points, one keyframe of three slots, a last frame of two keypoints."""
    M, cap = 3, 3
    mp = np.zeros(2, MAP_POINT_DTYPE)
    mp["pos"] = [[1, 2, 3], [4, 5, 6]]
    desc = np.arange(64, dtype=np.uint8).reshape(2, 32)
    d = MapDelta(1, new_mp=mp, new_mp_desc=desc, new_mp_bad=[0, 1], new_kf=[[1, -1, 0]], obs_rows={0: [0], 1: [0]},
                 kf_cov=[[]])
    kps = SS.keypoints(np.random.default_rng(0), 2)
    fdesc = np.full((2, 32), 9, np.uint8)
    Tcw = np.arange(16, dtype=np.float32)
    req = StreamStart(d, kps, fdesc, [1, -1], Tcw, timestamp=2.25, frame_id=11, since_reloc=4)
    assert req.ref_kf == 0 and req.stream == 1
    b = _before(cap, M)
    a = R.start(b, req)
    sent = lambda x: np.all(np.asarray(x).view(np.uint8) == S.SENTINEL)  # noqa: E731
    assert a["nmp"] == 2 and a["map"][:2].tobytes() == mp.tobytes() and sent(a["map"][2:])
    assert np.array_equal(a["map_desc"][:2], desc) and sent(a["map_desc"][2:])
    assert a["mp_upd"][:2].tolist() == [-1000, -1000] and sent(a["mp_upd"][2:])
    assert not a["views"][:2].view(np.uint8).any() and sent(a["views"][2:])
    g = a["graph"]
    assert g["kf_bad"].tolist() == [0] and g["kf_mp_off"].tolist() == [0, 3] and g["kf_mp"].tolist() == [1, -1, 0]
    assert g["mp_bad"].tolist() == [0, 1] and g["mp_obs_off"].tolist() == [0, 1, 2] and g["mp_obs"].tolist() == [0, 0]
    assert g["kf_cov_off"].tolist() == [0, 0] and len(g["kf_cov"]) == 0
    assert a["last_nkp"] == 2 and a["last_kps"][:2].tobytes() == kps.tobytes() and sent(a["last_kps"][2:])
    assert np.array_equal(a["last_desc"][:2], fdesc) and a["last_kp2mp"][:2].tolist() == [1, -1]
    assert a["last_outlier"][:2].tolist() == [0, 0] and a["last_pos"][:2].tolist() == [[4, 5, 6], [0, 0, 0]]
    assert sent(a["last_pos"][2:]) and sent(a["last_kp2mp"][2:]) and sent(a["last_outlier"][2:])
    assert np.array_equal(a["Tcw_last"], Tcw) and a["t_prev"] == 2.25 == a["t_cur"]
    assert a["kp2mp"].tolist() == [-1] * 3 and a["outlier"].tolist() == [0] * 3 and a["nleft"] == 0
    assert a["track"].tolist() == [0, 0, 4, 2, 11, 1, 5, 6]
    assert a["kf"] == dict(b["kf"], since=0, pending=0, abort=0, decision=0, ref=0)
    assert not a["Xv"].any() and not a["Xv_next"].any() and not a["base"].any() and not a["reloc"].view(np.uint8).any()
    assert a["mp_H"].tobytes() == b["mp_H"].tobytes() and a["velocity"].tobytes() == b["velocity"].tobytes()
    assert sent(b["map"]) and b["track"][0] == 2, "the restatement wrote into its input"


def _transform(voc):
    def t(d):
        w, v, (nodes, start, feats) = O.bow_transform(voc, d, 4)
        return w, v, FeatureVector(nodes, start, feats)
    return t


def test_every_refusal_has_its_verdict():
    from gf_orb_slam_amd import synth

    cap, M = 1100, 1400
    bad, good, m = SS.refusal_cases(cap, M, _transform(synth.synth_vocabulary_fast(11, k=10, L=5)))
    kinds = {0: None, 1: (4, 200), 2: "fixed", 3: None}
    for name, (r, code) in bad.items():
        named = [0] if name == "stream named twice" else []
        assert R.verdict(r, cap, M, named=named, nstreams=4, db=kinds.get(r.stream)) == code, name
    for r in good:
        assert R.verdict(r, cap, M, nstreams=4, db=kinds[r.stream]) == 0


class _StubFrontEnd:
    """start_streams through the restatement's verdict; the lifecycle words are set by the test."""

    def __init__(self, B=3, M=256, cap=32, dbs=None):
        self.B, self.M, self.cap = B, M, cap
        self._kfdbs = dict(dbs or {})
        self.started, self.words = [], []
        self.state = np.full(B, 2, np.int32)

    def start_streams(self, reqs):
        reqs = [reqs] if isinstance(reqs, StreamStart) else list(reqs)
        for i, r in enumerate(reqs):
            db = self._kfdbs.get(r.stream)
            rc = R.verdict(r, self.cap, self.M, named=[q.stream for q in reqs[:i]], nstreams=self.B,
                           db=None if db is None else (db.max_kf, db.max_rows) if db.growable else "fixed")
            if rc:
                raise GFError(rc, "refused")
        self.started += reqs
        for r in reqs:
            self.state[r.stream] = 0

    def set_keyframe_state(self, stream=None, **words):
        self.words.append((stream, words))

    def lifecycle(self):
        return self.state.copy()


def _loopmap(m, n_slots_last, seed=0):
    """What MapFeedback.start reads of a LoopMap, over a scenes map whose
    newest keyframe has n_slots_last keypoints."""
    rng = np.random.default_rng(seed)
    g = m["graph"]
    nkf = len(g["kf_bad"])
    slots = [r.copy() for r in S.rows_of(g["kf_mp_off"], g["kf_mp"])]
    kps = [SS.keypoints(rng, len(s)) for s in slots]
    desc = [rng.integers(0, 256, (len(s), 32), dtype=np.uint8) for s in slots]
    bow = [(np.arange(3, dtype=np.int32) + k, np.full(3, 1 / 3)) for k in range(nkf)]
    fv = [FeatureVector(np.array([0], np.int32), np.array([0, len(s)], np.int32), np.arange(len(s), dtype=np.int32))
          for s in slots]
    assert len(slots[-1]) == n_slots_last
    return SimpleNamespace(mps=m["mp"].copy(), mp_desc=m["desc"].copy(), nkf=nkf, slots=slots,
                           ordered=[r.tolist() for r in S.rows_of(g["kf_cov_off"], g["kf_cov"])],
                           obs=[set(r.tolist()) for r in S.rows_of(g["mp_obs_off"], g["mp_obs"])],
                           kf_bad=np.asarray(g["kf_bad"]).astype(bool).copy(),
                           mp_bad=np.asarray(g["mp_bad"]).astype(bool).copy(), kf_kps=kps, kf_desc=desc, kf_bow=bow,
                           kf_fv=fv, Tcw=np.stack([SS.pose(rng) for _ in range(nkf)]))


def _map_with_last(seed, nmp, nkf, n_last, matched):
    """A scenes map whose newest keyframe has n_last slots, `matched` of them holding a point."""
    m = SS.graph_map(seed, nmp, nkf, slots=(3, 9))
    rows = S.rows_of(m["graph"]["kf_mp_off"], m["graph"]["kf_mp"])
    rng = np.random.default_rng(seed)
    last = np.full(n_last, -1, np.int32)
    last[rng.choice(n_last, matched, replace=False)] = rng.choice(nmp, matched, replace=False)
    rows[-1] = last
    g = m["graph"]
    m["graph"] = S.graph_of(rows, g["kf_bad"], S.rows_of(g["kf_cov_off"], g["kf_cov"]), g["mp_bad"],
                            S.rows_of(g["mp_obs_off"], g["mp_obs"]))
    return m


def test_mapfeedback_start_builds_the_request_and_resets_the_id_maps():
    from gf_orb_slam_amd.pipeline import KeyframeDB

    m = _map_with_last(1, 60, 4, 20, 12)
    lm = _loopmap(m, 20)
    db = KeyframeDB([], [], lambda d: None, max_kf=64, max_rows=500)
    fe = _StubFrontEnd(dbs={1: db})
    fb = tracking.MapFeedback.starting(fe, 1, lm)
    assert len(fb.mp) == 0 and len(fb.kf_id) == 0
    req = fb.start(lm.kf_kps[3], lm.kf_desc[3], frame_id=1, timestamp=0.05)
    d = req.map
    # the whole map as a delta against the empty map
    got = dict(mp=d.new_mp, desc=d.new_mp_desc, graph=R.graph_of_delta(d))
    assert S.same_map(got, m) == [] and MR.same_graph(got["graph"], tracking.covis_graph_from_loopmap(lm)) == []
    assert not (len(d.set_mp_idx) or len(d.bad_mp) or len(d.bad_kf) or len(d.slot_kf))
    # the last frame: the newest keyframe's keypoints, slot table and pose; mpReferenceKF the newest keyframe
    assert req.kps.tobytes() == lm.kf_kps[3].tobytes() and np.array_equal(req.desc, lm.kf_desc[3])
    assert np.array_equal(req.kp2mp, lm.slots[3]) and np.array_equal(req.Tcw.reshape(4, 4), lm.Tcw[3])
    assert (req.ref_kf, req.frame_id, req.since_reloc, req.timestamp, req.stream) == (3, 1, 1, 0.05, 1)
    # the database rows of every keyframe, as delta() makes them
    rows = req.kf_rows
    assert rows.nkf == 4 and np.array_equal(np.diff(rows.kp_off), np.diff(d.new_kf_off))
    assert rows.kps.tobytes() == np.concatenate(lm.kf_kps).tobytes() and np.array_equal(rows.bow_words[:3], [0, 1, 2])
    assert R.verdict(req, fe.cap, fe.M, nstreams=3, db=(64, 500)) == 0
    # the id maps and the shadow: the front end holds exactly this map
    assert np.array_equal(fb.mp_id, np.arange(60)) and np.array_equal(fb.kf_id, np.arange(4))
    assert np.array_equal(fb.mp_index, np.arange(60)) and np.array_equal(fb.kf_index, np.arange(4)) and fb._identity
    assert S.same_map(dict(mp=fb.mp, desc=fb.desc, graph=fb.graph), m) == [] and fb.delta().empty()
    fb.discard()
    # since_reloc given; a second start of the same feedback gives the same request again
    again = fb.start(lm.kf_kps[3], lm.kf_desc[3], frame_id=9, timestamp=0.5, since_reloc=3)
    assert again.since_reloc == 3 and again.map.new_mp.tobytes() == d.new_mp.tobytes() and again.kf_rows.nkf == 4
    # without a growable database the request carries no rows
    assert tracking.MapFeedback.starting(_StubFrontEnd(), 0, lm).start(lm.kf_kps[3], lm.kf_desc[3], 1, 0.0).kf_rows is None


def test_a_frame_above_the_capacity_is_reduced_to_its_matched_keypoints():
    m = _map_with_last(2, 80, 2, 50, 30)  # 50 keypoints, the stub front end holds 32
    lm = _loopmap(m, 50)
    fe = _StubFrontEnd()
    req = tracking.MapFeedback.starting(fe, 0, lm).start(lm.kf_kps[1], lm.kf_desc[1], 1, 0.0)
    keep = np.nonzero(lm.slots[1] >= 0)[0]
    assert len(keep) == 30 == len(req.kps) and np.array_equal(req.kp2mp, lm.slots[1][keep])
    assert req.kps.tobytes() == lm.kf_kps[1][keep].tobytes() and np.array_equal(req.desc, lm.kf_desc[1][keep])
    assert len(req.map.new_kf_mp) == len(np.concatenate(lm.slots)), "the keyframe itself keeps every slot"
    # even the matched keypoints exceed the capacity
    m = _map_with_last(3, 80, 2, 50, 33)
    lm = _loopmap(m, 50)
    fb = tracking.MapFeedback.starting(fe, 0, lm)
    with pytest.raises(GFError) as e:
        fb.start(lm.kf_kps[1], lm.kf_desc[1], 1, 0.0)
    assert e.value.code == -3 and fb._next is None


def test_inserter_start_and_poll_resets():
    m = _map_with_last(4, 60, 2, 20, 12)
    lm = _loopmap(m, 20)
    fe = _StubFrontEnd(B=3)
    ins = tracking.KeyFrameInserter(fe, {})
    assert ins.poll_resets() == []  # parked from the beginning, never mapped: nothing to drop
    mapper = SimpleNamespace(map=lm)
    req = ins.start(1, lm, lm.kf_kps[1], lm.kf_desc[1], frame_id=1, timestamp=0.0, mapper=mapper)
    assert fe.started == [req] and fe.words == [(1, dict(accept=1, stop=0))]
    assert ins.mappers[1] is mapper and ins.feedback[1].map is lm and ins.queue[1] == [] and fe.state[1] == 0
    assert ins.poll_resets() == []
    ins.queue[1].append(7)
    fe.state[1] = 2  # the device parked it: LOST on at most 5 keyframes
    assert ins.poll_resets() == [1] and 1 not in ins.mappers and 1 not in ins.feedback and 1 not in ins.queue
    assert ins.poll_resets() == [], "reported once"
    ins.start(1, lm, lm.kf_kps[1], lm.kf_desc[1], frame_id=1, timestamp=0.0, mapper=mapper)
    fe.state[1] = 2
    assert ins.poll_resets() == [1], "started again, parked again: reported again"
    # a refused start leaves the inserter as it was
    big = _loopmap(_map_with_last(5, 300, 2, 20, 12), 20)
    with pytest.raises(GFError):
        ins.start(2, big, big.kf_kps[1], big.kf_desc[1], 1, 0.0, mapper=mapper)  # 300 points, map_cap 256
    assert 2 not in ins.mappers and 2 not in ins.feedback and len(fe.started) == 2


def test_two_chains_with_the_full_and_the_reduced_last_frame_step_equally():
    """mLastFrame with its NULL keypoints dropped (what MapFeedback.start
    sends when the initial frame exceeds the capacity) gives the same steps:
    SearchByProjection(Cur, Last) and TrackPreviousFrame's searches walk
    mLastFrame.mvpMapPoints and skip NULL. With a velocity (the motion model)
    and without (as after a start)."""
    from gf_orb_slam_amd import scene

    W = scene.Workload("euroc", 1, n_scenes=1, period=8, seed=9, tex_size=256)
    fr = W.render_all("cpu").numpy()
    mp, desc = W.build_maps(lambda im: O.extract(im), 1500)[W.scene_of[0]]
    T, V = W.boot_state()
    ch = C.Chain("euroc", 1000, 1500, 100)
    ch.set_map(mp, desc)
    ch.set_rng(3)
    ch.bootstrap(fr[W.scene_of[0], W.phase[0] % 8], T[0], V[0])
    ch.step(fr[W.scene_of[0], (W.phase[0] + 1) % 8])
    st = {k: ch.read(k)[None] for k in C.Chain.STATE}
    st["stats"] = ch.read("stats")[:, None]
    n = int(st["last_nkp"][0])
    keep = np.nonzero(st["last_kp2mp"][0][:n] >= 0)[0]
    assert 50 < len(keep) < n, (len(keep), n)
    red = {k: v.copy() for k, v in st.items()}
    for k in ("last_kps", "last_desc", "last_kp2mp", "last_outlier", "last_pos"):
        red[k][0, :len(keep)] = st[k][0][keep]
    red["last_nkp"][0] = len(keep)
    for vel in (1, 0):
        out = []
        for s in (st, red):
            s = {k: v.copy() for k, v in s.items()}
            s["track"][0, TR["vel"]] = vel
            c = C.Chain("euroc", 1000, 1500, 100)
            c.set_map(mp, desc)
            c.load_from(s, 0)
            steps = []
            for k in (2, 3):
                c.step(fr[W.scene_of[0], (W.phase[0] + k) % 8])
                steps.append({f: c.read(f) for f in C.FIELDS if f not in ("clock", "hist")})
            out.append(steps)
        path = int(out[0][0]["track"][TR["path"]])
        assert path == (0 if vel else 2), path
        for i, (a, b) in enumerate(zip(*out)):
            assert int(a["track"][TR["state"]]) == 0, "the full chain lost track"
            for f in a:
                assert a[f].tobytes() == b[f].tobytes(), f"velocity {vel}: step {i}: {f}"
