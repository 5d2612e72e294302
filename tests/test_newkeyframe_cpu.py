"""NeedNewKeyFrame / CreateNewKeyFrame without a GPU: the CPU restatement
(tests/helpers/newkeyframe_ref.cpp) against hand-written cases with literal
outcomes, the library's scalar rule against the same table, and
tracking.KeyFrameInserter's queue and flag sequence over a fake front end and
stub mapper stages."""
import numpy as np
import pytest

import newkeyframe_ref as R
import newkeyframe_scenes as S
from gf_orb_slam_amd import pipeline, tracking
from gf_orb_slam_amd.localmapping import LocalMapper

BIG = 1 << 30
# (since_kf, since_reloc, stop, nkf, n_ref, inliers, accept, min_frames, max_frames) -> decision bits, by hand:
# 1 evaluated, 2 stop, 4 relocalisation, 8 c1a, 16 c1b, 32 c2, 64 created, 128 InterruptBA, 256 no reference
RULE_CASES = [
    ("stopped", (100, BIG, 1, 20, 100, 50, 1, 0, 12), 1 | 2),
    ("not stopped", (100, BIG, 0, 20, 100, 50, 1, 0, 12), 1 | 8 | 16 | 32 | 64),
    ("just relocalised, large map", (100, 11, 0, 13, 100, 50, 1, 0, 12), 1 | 4),
    ("relocalised mMaxFrames ago", (100, 12, 0, 13, 100, 50, 1, 0, 12), 1 | 8 | 16 | 32 | 64),
    ("just relocalised, map of mMaxFrames keyframes", (100, 11, 0, 12, 100, 50, 1, 0, 12), 1 | 8 | 16 | 32 | 64),
    ("no reference keyframe", (100, BIG, 0, 20, -1, 50, 1, 0, 12), 1 | 256),
    ("stop wins over the missing reference", (100, BIG, 1, 20, -1, 50, 1, 0, 12), 1 | 2),
    ("c1a at mMaxFrames, mapper busy: InterruptBA", (12, BIG, 0, 20, 100, 50, 0, 0, 12), 1 | 8 | 32 | 128),
    ("one frame short of c1a, mapper busy", (11, BIG, 0, 20, 100, 50, 0, 0, 12), 1 | 32),
    ("c1b at mMinFrames, idle", (5, BIG, 0, 20, 100, 50, 1, 5, 12), 1 | 16 | 32 | 64),
    ("one frame short of c1b", (4, BIG, 0, 20, 100, 50, 1, 5, 12), 1 | 32),
    ("c1b needs the idle mapper", (5, BIG, 0, 20, 100, 50, 0, 5, 12), 1 | 32),
    ("15 inliers: not enough", (100, BIG, 0, 20, 100, 15, 1, 0, 12), 1 | 8 | 16),
    ("16 inliers", (100, BIG, 0, 20, 100, 16, 1, 0, 12), 1 | 8 | 16 | 32 | 64),
    ("inliers equal to 90 % of the reference", (100, BIG, 0, 20, 20, 18, 1, 0, 12), 1 | 8 | 16),
    ("inliers just below 90 % of the reference", (100, BIG, 0, 20, 20, 17, 1, 0, 12), 1 | 8 | 16 | 32 | 64),
    ("90 % is not an integer: 0.9 * 21 = 18.9", (100, BIG, 0, 20, 21, 18, 1, 0, 12), 1 | 8 | 16 | 32 | 64),
    ("0.9 * 21 = 18.9 < 19", (100, BIG, 0, 20, 21, 19, 1, 0, 12), 1 | 8 | 16),
    ("c2 without c1: nothing happens", (3, BIG, 0, 20, 100, 50, 0, 0, 12), 1 | 32),
    ("c1 without c2, busy mapper: no InterruptBA", (100, BIG, 0, 20, 100, 95, 0, 0, 12), 1 | 8),
    ("empty reference keyframe", (100, BIG, 0, 20, 0, 50, 1, 0, 12), 1 | 8 | 16),
]


@pytest.mark.parametrize("name,args,bits", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_rule_restatement_against_table(name, args, bits):
    assert R.rule(*args) == bits


@pytest.mark.parametrize("name,args,bits", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_rule_library_scalar_against_table(name, args, bits):
    need, dec = pipeline.need_new_keyframe(*args)
    assert dec == bits and need == bool(bits & 64)


def test_tracked_map_points_counts_non_null_slots():
    assert R.tracked_map_points([]) == 0
    assert R.tracked_map_points([-1, -1]) == 0
    assert R.tracked_map_points([4, -1, 0, 7, -1, 7]) == 4  # a point twice counts twice, as two pointers do


def test_stage_creates_and_snapshots():
    # 16 inliers against a reference keyframe of 10 tracked points (0.9 * 10 = 9): no weak frame, nothing written
    q = S.Problem(1, 6, 3, 40, seed=5)
    q.set_row(0, 10, 1, ref=1, start=3, nkf=2)
    q.nkp[0], q.inliers[0], q.track[0, 4] = 4, 16, 321
    q.state[0, R.W["since"]] = 4
    st, box = S.run_ref(q)
    assert st[0, :12].tolist() == [5, 1, 0, -1, 0, 1 | 16, 1, 10, 16, 0, 0, 0]
    assert np.all(box.kps == S.SENTINEL) and np.all(box.slots.view(np.uint8) == S.SENTINEL)
    assert np.all(box.hdr.view(np.uint8) == S.SENTINEL)
    # the creating case: 16 inliers against a reference of 30 tracked points
    q.set_row(0, 30, 1, ref=1, start=3, nkf=2)
    st, box = S.run_ref(q)
    # SINCE 0, ACCEPT cleared, ABORT raised, decision: evaluated c1b c2 created, what it read, SEQ 1, PENDING, FRAME
    assert st[0, :12].tolist() == [0, 0, 0, -1, 1, 1 | 16 | 32 | 64, 1, 30, 16, 1, 1, 321]
    h = box.hdr[0]
    assert (h["stream"], h["seq"], h["frame_id"], h["n"]) == (0, 1, 321, 4) and h["timestamp"] == q.t_cur[0]
    assert np.array_equal(h["Tcw"], q.Tcw[0])
    assert np.array_equal(box.kps[0, :4], q.kps[0, :4]) and np.array_equal(box.desc[0, :4], q.desc[0, :4])
    assert np.array_equal(box.slots[0, :4], q.kp2mp[0, :4])
    assert np.all(box.kps[0, 4:] == S.SENTINEL) and np.all(box.desc[0, 4:] == S.SENTINEL)  # rows >= N untouched
    # the next frame: the mapper has not taken it, so the mapper reads as busy and nothing is created
    st2, box2 = S.run_ref(q, st.copy(), box)
    assert st2[0, R.W["decision"]] == 1 | 32 and st2[0, R.W["since"]] == 1 and st2[0, R.W["seq"]] == 1
    # ACCEPT is refused while the keyframe waits, and comes back after the hand-over
    assert R.set_accept(st2[0], True) == -1
    rc, hdr, kps, desc, slots, nrows = R.take(st2, box2, 1, 6)
    assert rc == 0 and len(hdr) == 1 and nrows == 4 and st2[0, R.W["pending"]] == 0
    assert np.array_equal(slots, q.kp2mp[0, :4])
    assert R.set_accept(st2[0], True) == 0 and st2[0, R.W["accept"]] == 1


def test_stage_interrupt_ba_and_since_saturates():
    q = S.Problem(1, 6, 3, 40, seed=6)
    q.set_row(0, 30, 1, ref=1, start=3, nkf=2)
    q.inliers[0] = 16
    q.state[0, R.W["since"]], q.state[0, R.W["accept"]] = BIG, 0
    st, box = S.run_ref(q)
    assert st[0, R.W["since"]] == BIG and st[0, R.W["decision"]] == 1 | 8 | 32 | 128
    assert st[0, R.W["abort"]] == 1 and st[0, R.W["pending"]] == 0 and st[0, R.W["seq"]] == 0
    q.working[0] = 0  # a frame that did not end WORKING: not evaluated, SINCE still counts
    q.state[0, R.W["since"]] = 6
    st, _ = S.run_ref(q)
    assert st[0, :12].tolist() == [7, 0, 0, -1, 0, 0, -1, 0, 0, 0, 0, 0]


def test_take_packs_ascending_and_respects_the_caps():
    p = S.snapshot(cap=40)
    p.nkp[:] = [0, 1, 7, 40, 3, 0, 40, 12, 5, 9, 11, 20, 20, 20]
    st, box = S.run_ref(p)
    pending = np.nonzero(st[:, R.W["pending"]])[0].tolist()
    assert pending == list(range(len(S.SNAP_N)))
    need = int(p.nkp[:3].sum())
    rc, hdr, *_, nrows = R.take(st.copy(), box, 3, need - 1)
    assert rc == -3 and nrows == need and len(hdr) == 0
    st3 = st.copy()
    rc, hdr, kps, desc, slots, nrows = R.take(st3, box, 3, need)
    assert rc == 0 and hdr["stream"].tolist() == [0, 1, 2] and hdr["n"].tolist() == [0, 1, 7] and nrows == 8
    assert np.array_equal(slots, np.concatenate([p.kp2mp[1, :1], p.kp2mp[2, :7]]))
    assert np.array_equal(kps, np.concatenate([p.kps[1, :1], p.kps[2, :7]]))
    assert np.nonzero(st3[:, R.W["pending"]])[0].tolist() == pending[3:]


# ---------------------------------------------------------------- KeyFrameInserter
class _FakeFrontEnd:
    def __init__(self, B):
        self.B = B
        self.words = {k: np.zeros(B, np.int32) for k in pipeline.KF}
        self.outbox = []
        self.log = []

    def keyframe_state(self):
        return {k: v.copy() for k, v in self.words.items()}

    def set_keyframe_state(self, stream=None, **words):
        for k, v in words.items():
            assert not (k == "accept" and v and self.words["pending"][stream]), "ACCEPT while pending"
            self.words[k][stream] = v
            self.log.append((stream, k, v))

    def create(self, stream, slots):
        n = len(slots)
        self.words["pending"][stream], self.words["accept"][stream], self.words["abort"][stream] = 1, 0, 1
        self.outbox.append(dict(stream=stream, seq=1, frame_id=7, timestamp=0.5, Tcw=np.eye(4, dtype=np.float32),
                                kps=np.zeros(n, pipeline.KEYPOINT_DTYPE), desc=np.zeros((n, 32), np.uint8),
                                slots=np.asarray(slots, np.int32)))

    def take_keyframes(self, max_kf=None):
        out, self.outbox = sorted(self.outbox, key=lambda k: k["stream"]), []
        for k in out:
            self.words["pending"][k["stream"]] = 0
        return out


class _FakeMap:
    tables = None
    kf_fv = None

    def __init__(self):
        self.kfs = []

    def add_keyframe(self, kps, desc, slots, Tcw, kf_id=None):
        self.kfs.append(np.asarray(slots).copy())
        return 10 + len(self.kfs) - 1


def _mapper(seen):
    def stage(name, ret=None):
        def fn(*a, **kw):
            seen.append((name, kw.get("stop_flag").value if kw.get("stop_flag") is not None else None))
            return ret
        return fn

    stages = dict(process_new_keyframe=stage("pnk"), map_point_culling=stage("mpc", []),
                  create_new_map_points=stage("cnmp", ([], None)), search_in_neighbors=stage("sin"),
                  local_bundle_adjustment=stage("lba"), keyframe_culling=stage("kfc"))
    return LocalMapper(_FakeMap(), None, stages=stages)


def test_inserter_two_queued_keyframes_skip_ba_once():
    fe, seen = _FakeFrontEnd(2), []
    lm = _mapper(seen)
    ins = tracking.KeyFrameInserter(fe, {1: lm}, point_ids={1: np.array([5, 6, 7, 8])})
    fe.create(1, [0, -1, 3])
    fe.create(0, [1])  # a stream without a mapper: left alone
    assert ins.pump() == [(1, 10)]
    assert lm.map.kfs[0].tolist() == [5, -1, 8]  # translated, NULL stays NULL
    assert ins.stop_flags[1].value == 1           # the device's ABORT word, seen at pump()
    fe.create(1, [2])
    assert ins.pump() == [(1, 11)] and ins.queue[1] == [10, 11]
    rep = ins.run_mapper(1)
    assert rep["to_loop_closer"] == 10 and "local_bundle_adjustment" not in rep["order"]  # LocalMapping.cc:100
    assert fe.words["abort"][1] == 0 and fe.words["accept"][1] == 0  # a keyframe still waits: not idle yet
    rep = ins.run_mapper(1)
    assert rep["to_loop_closer"] == 11 and rep["order"][-2:] == ["local_bundle_adjustment", "keyframe_culling"]
    assert ("lba", 0) in seen  # mbAbortBA was cleared before the pass (:98)
    assert fe.words["accept"][1] == 1 and ins.run_mapper(1) is None
    assert [e for e in fe.log if e[1] == "accept"] == [(1, "accept", 1)]  # only once, with the queue empty


def test_inserter_stop_request_skips_ba_and_sets_the_word():
    fe, seen = _FakeFrontEnd(1), []
    ins = tracking.KeyFrameInserter(fe, [_mapper(seen)])
    ins.request_stop(0)
    assert fe.words["stop"][0] == 1
    fe.create(0, [0])
    ins.pump()
    rep = ins.run_mapper(0)
    assert rep["order"] == ["process_new_keyframe", "map_point_culling", "create_new_map_points",
                            "search_in_neighbors"]
    ins.release(0)
    assert fe.words["stop"][0] == 0 and fe.words["accept"][0] == 1
    fe.create(0, [0])
    ins.pump()
    assert "local_bundle_adjustment" in ins.run_mapper(0)["order"]
