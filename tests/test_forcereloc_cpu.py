"""Forced relocalisation without a GPU: the premise of the GPU parity tests
pinned with the oracle chain alone (forcereloc_scenes.py), the numpy
restatement of the forced candidate list on hand-written rows, and
``KeyFrameInserter.correct_loop`` / ``loop_corrected`` on a stub front end that
records calls."""
from types import SimpleNamespace

import numpy as np
import pytest

import forcereloc_scenes as FS
from gf_orb_slam_amd import tracking
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.pipeline import TR


# ---------------------------------------------------------------- the premise
def test_the_edited_row_turns_the_database_list_into_the_forced_list():
    """At steps 3, 6 and 8 the LOST-at-k chain's candidates are the pinned
    lists, giving the row of C[-1] the entries C[:-1] leaves them unchanged
    (so the forced list of the edited graph is C), and each chain relocalises.
    At step 3 the first candidate has fewer than 15 SearchByBoW matches: the
    second one wins. Keyframe 0 shares no match with frame 4 (the failure
    test's last_kf)."""
    sc = FS.cpu_scene()
    g = sc["m1"]["graph"]
    assert len(g["kf_bad"]) == 24 and len(sc["m1"]["mp"]) == 2600
    for k, want in FS.CANDS.items():
        ch, cands = FS.lost_at(sc, k)
        assert cands == want, (k, cands)
        me = FS.edited(sc["m1"], cands)
        che, cands_e = FS.lost_at(sc, k, me)
        assert cands_e == want, (k, cands_e)
        assert FS.forced_list(me["graph"]["kf_cov_off"], me["graph"]["kf_cov"], want[-1]) == want
        for c in (ch, che):
            assert c.stats()["flags"] & 32768 and int(c.read("track")[TR["state"]]) == 0, (k, "did not relocalise")
        assert ch.stats()["ransac"] == 1 and che.stats()["ransac"] == 1
        n = int(ch.read("nkp"))
        nm = [FS.bow_matches(sc["rows"], g, c, ch.read("desc")[:n], ch.read("kps")[:n], sc["voc"]) for c in want]
        print(f"step {k}: candidates {cands}, SearchByBoW matches {nm}, nGood {ch.stats()['reloc']}")
        if k == 3:
            assert nm[0] < 15 <= nm[1], nm
        if k == 8:
            assert min(nm) >= 15, nm
    # the natural list and the failing one of step 4
    ch, cands = FS.lost_at(sc, 4)
    assert cands == [23]
    n = int(ch.read("nkp"))
    assert FS.bow_matches(sc["rows"], g, 0, ch.read("desc")[:n], ch.read("kps")[:n], sc["voc"]) == 0
    assert g["kf_cov_off"][1] - g["kf_cov_off"][0] == 0, "keyframe 0 has covisible keyframes"
    assert g["kf_cov_off"][24] - g["kf_cov_off"][23] == 11, "keyframe 23's covisibility row"
    nodb, _ = FS.lost_at(sc, 4, db=None)
    assert int(nodb.read("track")[TR["state"]]) == 1 and not nodb.read("track")[TR["vel"]]


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n", [0, 1, 9, 10, 11])
def test_forced_list_on_hand_written_rows(n):
    rows = [[], list(range(20, 20 + n)), [5]]
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    cov = np.array([c for r in rows for c in r], np.int32)
    got = FS.forced_list(off, cov, 1)
    assert got == list(range(20, 20 + min(n, 9))) + [1]
    assert len(got) == min(n, 9) + 1
    assert FS.forced_list(off, cov, 0) == [0] and FS.forced_list(off, cov, 2) == [5, 2]


# ---------------------------------------------------------------- the host side
class _StubFE:
    """Records the calls a KeyFrameInserter makes."""

    def __init__(self, refuse_update=False):
        self.calls, self.refuse_update, self._kfdbs = [], refuse_update, {}

    def set_keyframe_state(self, stream, **kw):
        self.calls.append(("kf_state", stream, kw))

    def update_maps(self, deltas):
        if self.refuse_update:
            raise GFError(-3, "refused")
        self.calls.append(("update", [d.stream for d in deltas]))

    def force_relocalisation(self, streams, last_kf=None):
        self.calls.append(("force", list(streams), list(last_kf)))


def _stub_map(nkf=5):
    """A LoopMap stand-in of nkf keyframes without slots and one point."""
    return SimpleNamespace(nkf=nkf, mps=np.zeros(1, tracking.MAP_POINT_DTYPE), mp_desc=np.zeros((1, 32), np.uint8),
                           kf_bad=np.zeros(nkf, bool), moved=False)


def _graph(m):
    n = m.nkf
    mp_bad = np.array([1 if m.moved else 0], np.uint8)  # something for the delta to carry once the map has moved
    return dict(kf_bad=np.asarray(m.kf_bad).astype(np.uint8), kf_mp_off=np.zeros(n + 1, np.int32),
                kf_mp=np.zeros(0, np.int32), kf_cov_off=np.zeros(n + 1, np.int32), kf_cov=np.zeros(0, np.int32),
                mp_bad=mp_bad, mp_obs_off=np.zeros(2, np.int32), mp_obs=np.zeros(0, np.int32))


@pytest.fixture
def stubbed(monkeypatch):
    from gf_orb_slam_amd import sim3

    log = []

    def fake_correct_loop(map, cur_kf, matched_kf, gScw, cmp_, lp, ctx=None):
        log.append(("correct", cur_kf, matched_kf))
        map.moved = True
        return dict(report=1)

    monkeypatch.setattr(sim3, "correct_loop", fake_correct_loop)
    monkeypatch.setattr(tracking, "covis_graph_from_loopmap", _graph)
    monkeypatch.setattr(tracking, "_graph_through", lambda m, mp_id, kf_id: {
        k: (v[kf_id] if k == "kf_bad" else v[:len(kf_id) + 1] if k in ("kf_mp_off", "kf_cov_off") else v)
        for k, v in _graph(m).items()})
    return log


def _inserter(fe, m):
    shadow = dict(mp=m.mps.copy(), desc=m.mp_desc.copy(), graph=_graph(m))
    fb = tracking.MapFeedback(fe, 0, m, shadow=shadow)
    return tracking.KeyFrameInserter(fe, {0: SimpleNamespace(map=m)}, feedback={0: fb}), fb


def test_correct_loop_order_and_default_keyframe(stubbed):
    fe, m = _StubFE(), _stub_map()
    m.kf_bad[4] = True  # the newest keyframe is bad: the default is the one before
    ins, fb = _inserter(fe, m)
    rep = ins.correct_loop(0, 4, 1, np.zeros(8), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert rep == dict(report=1)
    names = [c[0] for c in fe.calls]
    assert names == ["kf_state", "update", "force", "kf_state"], fe.calls
    assert fe.calls[0][2] == dict(stop=1) and fe.calls[3][2] == dict(stop=0)
    assert stubbed == [("correct", 4, 1)]
    assert fe.calls[2] == ("force", [0], [3])
    assert not ins.stop_requested[0]


def test_last_kf_goes_through_kf_index_after_a_remap(stubbed):
    fe, m = _StubFE(), _stub_map(6)
    ins, fb = _inserter(fe, m)
    # a compaction dropped keyframes 0 and 2: the front end holds LoopMap keyframes 1, 3, 4, 5 as 0 .. 3
    fb.graph = {k: (v[[1, 3, 4, 5]] if k == "kf_bad" else v[:5] if k in ("kf_mp_off", "kf_cov_off") else v)
                for k, v in fb.graph.items()}
    fb._identity = False
    fb._set_ids(fb.mp_id, np.array([1, 3, 4, 5], np.int32), 1, 6)
    m.moved = True
    assert ins.loop_corrected(0, last_kf=4) == 2
    assert fe.calls[-1] == ("force", [0], [2])
    assert ins.loop_corrected(0) == 3 and fe.calls[-1] == ("force", [0], [3])  # the default: the highest id held
    with pytest.raises(ValueError):
        ins.loop_corrected(0, last_kf=2)  # not held
    assert fe.calls[-1] == ("force", [0], [3])


def test_a_refused_update_sends_no_request(stubbed):
    fe, m = _StubFE(refuse_update=True), _stub_map()
    ins, fb = _inserter(fe, m)
    with pytest.raises(GFError):
        ins.correct_loop(0, 4, 1, np.zeros(8), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert [c[0] for c in fe.calls] == ["kf_state", "kf_state"], fe.calls  # stop, release; no update landed, no force
    assert not ins.stop_requested[0]
