"""The serial restatement of gf_frontend_compact_maps
(tests/helpers/mapcompact_ref.cpp) against a hand-written table and against
the map built from scratch from the kept items, and the algebra of the
restriction: two compactions equal one with the union, an empty request is
the identity; then tracking.MapFeedback's id maps, default policy and
KeyFrameInserter.feed_back(compact_at=...) against a stub front end that
compacts through the restatement."""
import numpy as np
import pytest

import mapcompact_ref as R
import mapcompact_scenes as CS
import mapupdate_scenes as S
from gf_orb_slam_amd.localmap import MapCompact, MapRemap


def _tiny():
    """Four points, three keyframes."""
    mp, desc = S.points(np.random.default_rng(0), 4)
    g = S.graph_of(kf_rows=[[0, -1, 1], [2, 3], [1, 3, -1, 0]], kf_bad=[0, 1, 0], cov_rows=[[2, 1], [0], [1, 0]],
                   mp_bad=[0, 0, 1, 0], obs_rows=[[0, 2], [0, 2], [1], [1, 2]])
    return dict(mp=mp, desc=desc, graph=g)


def test_hand_written_table():
    m = _tiny()
    st = CS.state_of_map(1, m, 6, 5, holders=False)
    # the last frame still holds point 2: listed, it stays; keyframe 1 and point 0 go
    st.last_kp2mp[:3] = [2, -1, 3]
    st.last_nkp = 3
    st.left[:3] = [0, 3, 1]
    st.nleft = 3
    st.ref_kf[0] = 2
    before = st.copy()
    rc, rm = st.apply(MapCompact(0, drop_kf=[1], drop_mp=[0, 2]))
    assert rc == 0
    assert (rm.nkf, rm.nmp, rm.n_kept_kf, rm.n_kept_mp) == (2, 3, 0, 1)
    assert rm.kf_remap.tolist() == [0, -1, 1] and rm.mp_remap.tolist() == [-1, 0, 1, 2]
    g = st.graph()
    assert g["kf_bad"].tolist() == [0, 0] and g["mp_bad"].tolist() == [0, 1, 0]
    assert g["kf_mp_off"].tolist() == [0, 3, 7] and g["kf_mp"].tolist() == [-1, -1, 0, 0, 2, -1, -1]
    assert g["kf_cov_off"].tolist() == [0, 1, 2] and g["kf_cov"].tolist() == [1, 0]
    assert g["mp_obs_off"].tolist() == [0, 2, 2, 3] and g["mp_obs"].tolist() == [0, 1, 1]  # point 2 keeps an empty row
    assert st.last_kp2mp[:3].tolist() == [1, -1, 2] and st.left[:3].tolist() == [-1, 2, 0] and st.ref_kf[0] == 1
    for k, a in st.point_rows.items():
        assert a[:3].tobytes() == before.point_rows[k][[1, 2, 3]].tobytes(), k
        assert a[3:].tobytes() == before.point_rows[k][3:].tobytes(), f"{k}: rows past the count changed"
    assert st.kf_rows["reloc"][:2].tobytes() == before.kf_rows["reloc"][[0, 2]].tobytes()


def test_verdicts():
    st = CS.state_of_map(2, _tiny(), 6, 5)
    for req, code in ((MapCompact(0, drop_mp=[4]), -1), (MapCompact(0, drop_mp=[-1]), -1),
                      (MapCompact(0, drop_mp=[1, 1]), -1), (MapCompact(0, drop_kf=[3]), -1),
                      (MapCompact(0, drop_kf=[0, 2, 0]), -1), (MapCompact(0, drop_kf=[0], drop_mp=[3]), 0)):
        assert st.check(req) == code, (req.drop_kf, req.drop_mp)
    st.has_db = True
    assert st.check(MapCompact(0, drop_kf=[0])) == -4 and st.check(MapCompact(0, drop_mp=[0])) == 0
    before = st.copy()
    assert st.apply(MapCompact(0, drop_kf=[0]))[0] == -4
    assert R.same_graph(st.graph(), before.graph()) == [] and st.nmp == before.nmp


def _pinned_masks(st, req):
    """What the request keeps, pins included, stated on the State's holders."""
    keep_mp, keep_kf = np.ones(st.nmp, bool), np.ones(st.nkf, bool)
    keep_mp[req.drop_mp] = False
    keep_kf[req.drop_kf] = False
    held = np.concatenate([st.kp2mp[:st.nkp], st.last_kp2mp[:st.last_nkp], st.out_slots[:st.out_n] if st.pending else []])
    keep_mp[held[held >= 0].astype(np.int64)] = True
    if st.ref_kf[0] >= 0:
        keep_kf[st.ref_kf[0]] = True
    return keep_kf, keep_mp


@pytest.mark.parametrize("seed,nmp,nkf,pat_kf,pat_mp,holders", [
    (0, 70, 9, "first", "first", False), (1, 70, 9, "last", "last", True), (2, 64, 5, "alternate", "alternate", True),
    (3, 65, 64, "random", "random", True), (4, 1, 1, "all", "all", False), (5, 130, 12, "all", "all", True),
    (6, 50, 0, "none", "random", False), (7, 90, 7, "random", "none", True), (8, 0, 3, "first", "none", False)])
def test_equals_the_graph_built_from_the_kept_items(seed, nmp, nkf, pat_kf, pat_mp, holders):
    rng = np.random.default_rng(100 + seed)
    m = S.random_map(seed, nmp, nkf, slots=(0, 12), odd_offsets=True)
    st = CS.state_of_map(seed, m, nmp + 7, 20, holders=holders)
    if holders and nkf:
        st.ref_kf[0] = int(rng.integers(0, nkf))
        st.pending, st.out_n = 1, 9
        st.out_slots[:9] = rng.integers(-1, nmp, 9)
    req = MapCompact(0, CS.drops(pat_kf, nkf, rng), CS.drops(pat_mp, nmp, rng))
    keep_kf, keep_mp = _pinned_masks(st, req)
    want, new_kf, new_mp = CS.restrict(m, keep_kf, keep_mp)
    before = st.copy()
    rc, rm = st.apply(req)
    assert rc == 0
    assert np.array_equal(rm.kf_remap, new_kf) and np.array_equal(rm.mp_remap, new_mp)
    assert S.same_map(CS.map_of_state(st), want) == []
    assert rm.n_kept_mp == int(keep_mp[req.drop_mp].sum()) and rm.n_kept_kf == int(keep_kf[req.drop_kf].sum())
    for k, a in st.point_rows.items():
        assert a[:st.nmp].tobytes() == before.point_rows[k][:nmp][keep_mp].tobytes(), k
    for name, n in (("kp2mp", st.nkp), ("last_kp2mp", st.last_nkp), ("left", st.nleft)):
        assert np.array_equal(getattr(st, name)[:n], MapRemap.apply(new_mp, getattr(before, name)[:n])), name
        assert np.array_equal(getattr(st, name)[n:], getattr(before, name)[n:]), name
    if holders and nmp:
        assert np.all(st.kp2mp[:st.nkp][before.kp2mp[:st.nkp] >= 0] >= 0), "a held point was dropped"


def test_two_compactions_equal_one_with_the_union():
    rng = np.random.default_rng(5)
    m = S.random_map(11, 120, 20, slots=(0, 15))
    a, b = CS.state_of_map(3, m, 128, 24), CS.state_of_map(3, m, 128, 24)
    kf1, mp1 = CS.drops("random", 20, rng), CS.drops("random", 120, rng)
    rc, r1 = a.apply(MapCompact(0, kf1, mp1))
    assert rc == 0
    # the second request, stated in the old indices and sent in the new ones
    kf2 = np.setdiff1d(CS.drops("random", 20, rng), kf1)
    mp2 = np.setdiff1d(CS.drops("random", 120, rng), mp1)
    kf2n, mp2n = r1.kf_remap[kf2], r1.mp_remap[mp2]
    rc, r2 = a.apply(MapCompact(0, kf2n[kf2n >= 0], mp2n[mp2n >= 0]))
    assert rc == 0
    rc, ru = b.apply(MapCompact(0, np.concatenate([kf1, kf2]), np.concatenate([mp1, mp2])))
    assert rc == 0
    assert S.same_map(CS.map_of_state(a), CS.map_of_state(b)) == []
    assert np.array_equal(MapRemap.apply(r2.mp_remap, r1.mp_remap), ru.mp_remap)
    assert np.array_equal(MapRemap.apply(r2.kf_remap, r1.kf_remap), ru.kf_remap)
    for k in a.point_rows:
        assert a.point_rows[k][:a.nmp].tobytes() == b.point_rows[k][:b.nmp].tobytes(), k
    assert np.array_equal(a.kp2mp, b.kp2mp) and np.array_equal(a.last_kp2mp, b.last_kp2mp)


def test_an_empty_request_is_the_identity():
    m = S.random_map(12, 40, 6)
    st = CS.state_of_map(4, m, 48, 16)
    before = st.copy()
    rc, rm = st.apply(MapCompact(0))
    assert rc == 0 and rm.identity() and rm.n_kept_kf == rm.n_kept_mp == 0
    assert rm.mp_remap.tolist() == list(range(40)) and rm.kf_remap.tolist() == list(range(6))
    assert R.same_graph(st.graph(), before.graph()) == []
    for k in st.point_rows:
        assert st.point_rows[k].tobytes() == before.point_rows[k].tobytes(), k
    assert np.array_equal(st.kp2mp, before.kp2mp) and np.array_equal(st.left, before.left)


# ---------------------------------------------------------------- MapFeedback's id maps
class _StubFrontEnd:
    """compact_maps through the restatement, nothing held by frame state."""

    def __init__(self, m, M=256, cap=32):
        self.M, self.cap, self.B = M, cap, 1
        self.st = CS.state_of_map(0, m, M, cap, holders=False)
        self.requests = []

    def compact_maps(self, reqs):
        self.requests += reqs
        out = []
        for r in reqs:
            rc, rm = self.st.apply(r)
            assert rc == 0
            out.append(rm)
        return out


def _loopmap_of(m):
    """What MapFeedback reads of a LoopMap, over a scenes map (ids = indices)."""
    from types import SimpleNamespace

    g = m["graph"]
    return SimpleNamespace(mps=m["mp"].copy(), mp_desc=m["desc"].copy(), nkf=len(g["kf_bad"]),
                           slots=[r.copy() for r in S.rows_of(g["kf_mp_off"], g["kf_mp"])],
                           ordered=[r.tolist() for r in S.rows_of(g["kf_cov_off"], g["kf_cov"])],
                           obs=[set(r.tolist()) for r in S.rows_of(g["mp_obs_off"], g["mp_obs"])],
                           kf_bad=np.asarray(g["kf_bad"]).astype(bool).copy(),
                           mp_bad=np.asarray(g["mp_bad"]).astype(bool).copy())


def test_map_feedback_id_maps_after_compact():
    from gf_orb_slam_amd import tracking

    m = S.random_map(21, 150, 14, slots=(3, 20))
    lm, fe = _loopmap_of(m), _StubFrontEnd(m)
    fb = tracking.MapFeedback(fe, 0, lm, shadow=m)
    assert fb.delta().empty() and np.array_equal(fb.mp_index, np.arange(150)) and np.array_equal(fb.kf_id, np.arange(14))
    fb.commit()
    drop_kf, drop_mp = np.array([0, 5, 13]), np.arange(0, 150, 3)
    rm = fb.compact(drop_kf, drop_mp)
    want, new_kf, new_mp = CS.restrict(m, rm.kf_remap >= 0, rm.mp_remap >= 0)
    assert rm.nmp == 100 and rm.nkf == 11 and np.array_equal(fb.mp_index, new_mp) and np.array_equal(fb.kf_index, new_kf)
    assert np.array_equal(fb.mp_id, np.nonzero(new_mp >= 0)[0]) and np.array_equal(fb.kf_id, np.nonzero(new_kf >= 0)[0])
    assert S.same_map(dict(mp=fb.mp, desc=fb.desc, graph=fb.graph), want) == []
    assert S.same_map(CS.map_of_state(fe.st), want) == []
    assert len(lm.mps) == 150 and lm.nkf == 14  # the LoopMap never shrinks
    # the unchanged LoopMap through the id maps is what the front end holds
    d = fb.delta()
    assert d.empty(), "the delta of an unchanged map is not empty after a compaction"
    fb.commit()
    # a new point takes the next front-end index; a dropped point that comes back into a slot stays out
    kf = int(fb.kf_id[2])
    lm.mps = np.concatenate([lm.mps, lm.mps[:1]])
    lm.mp_desc = np.concatenate([lm.mp_desc, lm.mp_desc[:1]])
    lm.mp_bad = np.concatenate([lm.mp_bad, [False]])
    lm.obs.append({kf, 5})  # keyframe 5 is not held
    lm.slots[kf][0] = 150
    lm.slots[kf][1] = 3     # point 3 was dropped
    d = fb.delta()
    assert len(d.new_mp) == 1 and d.new_mp.tobytes() == lm.mps[150:].tobytes()
    assert d.obs_mp.tolist() == [100] and d.obs_kf.tolist() == [2]
    assert (d.slot_kf == 2).all() and 0 in d.slot_idx.tolist()
    assert d.slot_val[d.slot_idx.tolist().index(0)] == 100
    if 1 in d.slot_idx.tolist():
        assert d.slot_val[d.slot_idx.tolist().index(1)] == -1
    fb.commit()
    assert fb.mp_index[150] == 100 and fb.mp_id[100] == 150 and fb.mp_index[3] == -1
    # the errors of the identity mapping stay
    lm.mps = lm.mps[:120]
    with pytest.raises(ValueError):
        fb.delta()


def test_map_feedback_default_policy():
    from gf_orb_slam_amd import tracking

    m = S.random_map(22, 80, 10, slots=(3, 12))
    g = m["graph"]
    g["kf_bad"][:] = 0
    g["kf_bad"][[2, 7]] = 1
    lm, fe = _loopmap_of(m), _StubFrontEnd(m)
    fb = tracking.MapFeedback(fe, 0, lm, shadow=m)
    drop_kf, drop_mp = fb.default_drops()
    assert drop_kf.tolist() == [2, 7]
    # with a window of four: the newest, its covisibles in order, then by recency
    drop_kf, drop_mp = fb.default_drops(keep_kf=4)
    cov = [int(c) for c in S.rows_of(g["kf_cov_off"], g["kf_cov"])[9] if not g["kf_bad"][c]]
    order = list(dict.fromkeys([9] + cov + [k for k in range(9, -1, -1) if not g["kf_bad"][k]]))[:4]
    assert sorted(set(range(10)) - set(drop_kf.tolist())) == sorted(order)
    kept = np.zeros(10, bool)
    kept[order] = True
    slots, obs = S.rows_of(g["kf_mp_off"], g["kf_mp"]), S.rows_of(g["mp_obs_off"], g["mp_obs"])
    in_slot = set(int(v) for k in order for v in slots[k] if v >= 0)
    for p in range(80):
        if g["mp_bad"][p]:
            assert (p in drop_mp) == (p not in in_slot), p
        else:
            assert (p in drop_mp) == (not any(kept[k] for k in obs[p])), p
    rm = fb.compact(keep_kf=4)
    assert rm.nkf == 4 and rm.nmp == 80 - len(drop_mp) and fb.delta().empty()


def test_feed_back_compacts_before_a_delta_that_passes_a_capacity():
    from gf_orb_slam_amd import tracking

    m = S.random_map(23, 60, 63, slots=(2, 6))
    g = m["graph"]
    g["kf_bad"][:] = 0
    g["kf_bad"][5:45] = 1
    lm, fe = _loopmap_of(m), _StubFrontEnd(m, M=64)
    fe.sent = []
    fe.update_maps = lambda ds: fe.sent.extend(ds)
    fb = tracking.MapFeedback(fe, 0, lm, shadow=m)
    ins = tracking.KeyFrameInserter(fe, {}, feedback={0: fb})
    for _ in range(2):  # two keyframes leave the mapper: 65 in all
        lm.slots.append(np.array([1, -1, 2], np.int32))
        lm.ordered.append([62])
        lm.kf_bad = np.concatenate([lm.kf_bad, [False]])
        lm.nkf += 1
    # without compact_at the delta goes out as it is (the front end would answer GF_ERR_CAP)
    d = fb.delta()
    assert len(d.new_kf_off) - 1 == 2 and len(fb.graph["kf_bad"]) + 2 > 64
    fb.discard()
    sent = ins.feed_back(streams=[0], compact_at=dict(keep_kf=30))
    assert len(fe.requests) == 1 and fe.requests[0].drop_kf.tolist() == list(range(5, 45))
    assert len(sent) == 1 and len(sent[0].new_kf_off) - 1 == 2 and fe.sent == sent
    assert len(fb.graph["kf_bad"]) == 25 and fb.kf_id.tolist() == [*range(5), *range(45, 65)]
    assert sent[0].new_kf_mp.tolist() == [int(fb.mp_index[1]), -1, int(fb.mp_index[2])] * 2
    assert fb.delta().empty()


def test_default_policy_is_points_only_with_a_database_attached():
    from gf_orb_slam_amd import tracking

    m = S.random_map(24, 80, 10, slots=(3, 12))
    m["graph"]["kf_bad"][[2, 7]] = 1
    lm, fe = _loopmap_of(m), _StubFrontEnd(m)
    fe._kfdbs = {0: object()}  # dropping a keyframe would be GF_ERR_UNSUPPORTED on this stream
    fb = tracking.MapFeedback(fe, 0, lm, shadow=m)
    drop_kf, drop_mp = fb.default_drops(keep_kf=4)
    assert len(drop_kf) == 0 and len(drop_mp) > 0
    rm = fb.compact(keep_kf=4)
    assert rm.nkf == 10 and rm.nmp == 80 - len(drop_mp) and len(fe.requests[0].drop_kf) == 0
