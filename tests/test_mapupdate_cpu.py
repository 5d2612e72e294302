"""Map feedback without a GPU: the serial restatement of
gf_frontend_update_maps (tests/helpers/mapupdate_ref.cpp) against a
hand-written table and against randomised maps, the verdicts of refused deltas,
``tracking.covis_graph_from_loopmap`` as the inverse of
``loopmap_from_global_map``, and ``tracking.MapFeedback.delta()`` on a LoopMap
driven through its mutators. Every comparison is byte equality."""
import numpy as np
import pytest

import covis_ref
import mapupdate_ref as R
import mapupdate_scenes as S
import maptables_scenes
from gf_orb_slam_amd import tracking
from gf_orb_slam_amd.localmap import MapDelta
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE


def _hand_map():
    mp = np.zeros(5, MAP_POINT_DTYPE)
    mp["pos"] = np.arange(15, dtype=np.float32).reshape(5, 3)
    mp["min_dist"], mp["max_dist"] = 1, 9
    desc = np.arange(5 * 32, dtype=np.uint8).reshape(5, 32)
    g = S.graph_of([[0, 1, -1], [1, 2, 3, 4]], [0, 0], [[1], [0]], [0] * 5, [[0], [0, 1], [1], [1], [1]])
    return dict(mp=mp, desc=desc, graph=g)


def test_restatement_on_a_hand_written_table():
    """Two keyframes, five points, one of each delta item."""
    m0 = _hand_map()
    new = np.zeros(1, MAP_POINT_DTYPE)
    new["pos"], new["normal"], new["min_dist"], new["max_dist"] = (7, 8, 9), (0, 0, 1), 2, 5
    p2 = m0["mp"][2:3].copy()
    p2["pos"] += 1
    d2 = (m0["desc"][2:3] ^ 0xFF).astype(np.uint8)
    d = MapDelta(0, new_mp=new, new_mp_desc=np.full((1, 32), 77, np.uint8), set_mp_idx=[2], set_mp=p2, set_mp_desc=d2,
                 bad_mp=[3], new_kf=[[5, 0]], bad_kf=[0], slot_kf=[1], slot_idx=[2], slot_val=[-1],
                 obs_rows={0: [0, 2], 3: [], 5: [2]}, kf_cov=[[1, 2], [2, 0], [1]])
    st = R.State(8, 4, m0["mp"], m0["desc"], m0["graph"], last_kp2mp=[2, -1, 0, 4], last_nkp=3,
                 last_pos=np.full((4, 3), 100, np.float32), upd=np.arange(8), tail=S.SENTINEL)
    views0 = st.views.copy()
    assert st.apply(d) == 0
    g = st.graph()
    assert (st.nmp, st.nkf) == (6, 3)
    assert g["kf_bad"].tolist() == [1, 0, 0]
    assert g["kf_mp_off"].tolist() == [0, 3, 7, 9] and g["kf_mp"].tolist() == [0, 1, -1, 1, 2, -1, 4, 5, 0]
    assert g["kf_cov_off"].tolist() == [0, 2, 4, 5] and g["kf_cov"].tolist() == [1, 2, 2, 0, 1]
    assert g["mp_bad"].tolist() == [0, 0, 0, 1, 0, 0]
    assert g["mp_obs_off"].tolist() == [0, 2, 4, 5, 5, 6, 7] and g["mp_obs"].tolist() == [0, 2, 0, 1, 1, 1, 2]
    want = np.concatenate([m0["mp"], new])
    want[2] = p2[0]
    assert st.map[:6].tobytes() == want.tobytes() and np.array_equal(st.pos[:6], want["pos"])
    assert np.array_equal(st.desc[5], np.full(32, 77)) and np.array_equal(st.desc[2], d2[0])
    assert np.array_equal(st.desc[[0, 1, 3, 4]], m0["desc"][[0, 1, 3, 4]])
    # a fresh point's state; every other state row as it was
    assert st.upd.tolist() == [0, 1, 2, 3, 4, -1000, 6, 7]
    assert not st.views[5:6].view(np.uint8).any() and st.views[:5].tobytes() == views0[:5].tobytes()
    assert st.views[6:].tobytes() == views0[6:].tobytes() and np.all(st.map[6:].view(np.uint8) == S.SENTINEL)
    # the last frame's points read the new positions; a NULL match and rows >= N stay
    assert st.last_pos.tolist() == [want["pos"][2].tolist(), [100] * 3, want["pos"][0].tolist(), [100] * 3]
    # nothing of the slabs past the used part moved
    assert np.all(st.kf_mp[9:].view(np.uint8) == S.SENTINEL) and np.all(st.mp_obs[7:].view(np.uint8) == S.SENTINEL)
    assert np.all(st.kf_cov[5:].view(np.uint8) == S.SENTINEL) and np.all(st.mp_bad[6:] == S.SENTINEL)
    # an empty delta changes nothing
    before = st.copy()
    assert MapDelta(0).empty() and st.apply(MapDelta(0)) == 0
    assert all(np.array_equal(getattr(st, k), getattr(before, k)) for k in vars(st) if isinstance(getattr(st, k), np.ndarray))


CASES = [dict(nmp=60, nkf=5, new_mp=7, new_kf=1, rewrite=9, bad_mp=3, bad_kf=1, slot_writes=11),
         dict(nmp=0, nkf=0, new_mp=1, new_kf=1, obs="grow"),
         dict(nmp=300, nkf=20, new_mp=0, new_kf=0, rewrite=40, obs="none", cov=False),
         dict(nmp=300, nkf=20, new_mp=33, new_kf=0, obs="none", cov=False),
         dict(nmp=257, nkf=63, new_mp=0, new_kf=1, obs="all"),
         dict(nmp=100, nkf=9, new_mp=5, new_kf=2, obs="shrink", slot_writes=50),
         dict(nmp=100, nkf=9, new_mp=5, new_kf=0, obs="ends"),
         dict(nmp=700, nkf=12, new_mp=30, new_kf=1, obs=1024), dict(nmp=700, nkf=12, new_mp=30, new_kf=1, obs=1025)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_restatement_of_the_diff_reproduces_the_map(case):
    kw = dict(CASES[case])
    m0 = S.random_map(100 + case, kw.pop("nmp"), kw.pop("nkf"), odd_offsets=True)
    m1 = S.evolve(200 + case, m0, **kw)
    d = S.diff(0, m0, m1)
    st = R.State(len(m1["mp"]) + 3, 64, m0["mp"], m0["desc"], m0["graph"], tail=S.SENTINEL)
    assert st.check(d) == 0 and st.apply(d) == 0
    assert S.same_map(S.map_of_state(st), m1) == []
    if isinstance(CASES[case].get("obs"), int):
        assert len(m1["graph"]["mp_obs"]) == CASES[case]["obs"]


def test_refusals_write_nothing():
    m0 = S.random_map(5, 40, 6, odd_offsets=True)
    full = S.random_map(6, 40, 64, slots=(0, 3))
    good = S.diff(0, m0, S.evolve(7, m0, new_mp=2, rewrite=3))

    def refused(m, d, want, M=48, has_db=False):
        st = R.State(M, 64, m["mp"], m["desc"], m["graph"], has_db=has_db, tail=S.SENTINEL)
        before = st.copy()
        assert st.check(d) == want and st.apply(d) == want
        assert all(np.array_equal(getattr(st, k), getattr(before, k)) for k in vars(st)
                   if isinstance(getattr(st, k), np.ndarray))

    refused(full, S.diff(0, full, S.evolve(8, full, new_kf=1, cov=False, obs="none")), -3)  # 65 keyframes
    refused(m0, S.diff(0, m0, S.evolve(9, m0, new_mp=9, cov=False, obs="none")), -3)        # map_cap + 1 points
    refused(m0, MapDelta(0, slot_kf=[1], slot_idx=[0], slot_val=[40]), -1)                  # slot value out of range
    refused(m0, MapDelta(0, obs_rows={3: [2, 1]}), -1)                                      # row not ascending
    refused(m0, MapDelta(0, obs_rows={3: [1, 1]}), -1)
    refused(m0, MapDelta(0, obs_rows={3: [6]}), -1)                                         # keyframe >= nkf
    refused(m0, MapDelta(0, slot_kf=[1, 1], slot_idx=[0, 0], slot_val=[2, 3]), -1)          # a slot written twice
    refused(m0, MapDelta(0, set_mp_idx=[40], set_mp=m0["mp"][:1], set_mp_desc=m0["desc"][:1]), -1)
    refused(m0, MapDelta(0, bad_mp=[40]), -1)
    refused(m0, MapDelta(0, new_kf=[[0, 1]]), -4, has_db=True)                              # a database is attached
    st = R.State(48, 64, m0["mp"], m0["desc"], m0["graph"], has_db=True)
    assert st.apply(good) == 0  # a delta that appends no keyframe passes with a database


def _global_map_like(seed, nkf=6, window=90, stride=30):
    """A map in the form of scene.build_global_map: keyframe k sees the points
    [stride k, stride k + window), so every pair that shares a point shares 15
    or more; the graph by build_global_map's rule."""
    rng = np.random.default_rng(seed)
    nmp = stride * (nkf - 1) + window
    mp, desc = S.points(rng, nmp)
    kf_mp, kf_kps, kf_desc = [], [], []
    for k in range(nkf):
        ids = np.arange(stride * k, stride * k + window, dtype=np.int32)
        row = np.full(window + 10, -1, np.int32)
        row[rng.permutation(window + 10)[:window]] = ids
        kf_mp.append(row)
        kp = np.zeros(len(row), KEYPOINT_DTYPE)
        kp["x"], kp["y"], kp["octave"] = rng.uniform(0, 700, len(row)), rng.uniform(0, 400, len(row)), 1
        kf_kps.append(kp)
        kf_desc.append(rng.integers(0, 256, (len(row), 32), dtype=np.uint8))
    obs = [[k for k in range(nkf) if p in set(kf_mp[k].tolist())] for p in range(nmp)]
    shared = np.zeros((nkf, nkf), np.int64)
    for o in obs:
        for a in o:
            for b in o:
                if a != b:
                    shared[a, b] += 1
    cov = [sorted([b for b in range(nkf) if b != a and shared[a, b] >= 15], key=lambda b: (-shared[a, b], -b))
           for a in range(nkf)]
    assert shared[shared > 0].min() >= 15
    g = S.graph_of(kf_mp, np.zeros(nkf), cov, np.zeros(nmp), obs)
    return dict(mp=mp, desc=desc, graph=g, kf_Tcw=np.tile(np.eye(4, dtype=np.float32), (nkf, 1, 1)), kf_kps=kf_kps,
                kf_desc=kf_desc)


def test_covis_graph_from_loopmap_inverts_loopmap_from_global_map():
    info = FrameInfo.make(752, 480, 458.654, 457.296, 367.215, 248.375)
    for seed in (1, 2):
        gm = _global_map_like(seed)
        m = tracking.loopmap_from_global_map(info, gm, counter=covis_ref.counts)
        assert R.same_graph(tracking.covis_graph_from_loopmap(m), gm["graph"]) == []


def test_mapfeedback_delta_reproduces_a_driven_loopmap():
    m = maptables_scenes.thin_map(30, distinctive=maptables_scenes.keep_descriptors)
    rng = np.random.default_rng(3)
    m.mps["pos"] = rng.normal(size=(len(m.mps), 3)).astype(np.float32)
    start = dict(mp=m.mps.copy(), desc=m.mp_desc.copy(), graph=tracking.covis_graph_from_loopmap(m))
    fb = tracking.MapFeedback(None, 2, m, shadow=start)
    assert fb.delta().empty()
    cap = 64
    total = dict()
    for rnd in range(3):
        n0 = len(m.mps)
        shadow = dict(mp=fb.mp.copy(), desc=fb.desc.copy(), graph={k: v.copy() for k, v in fb.graph.items()})
        done = maptables_scenes.random_walk(m, 150, 40 + rnd)
        for k, v in done.items():
            total[k] = total.get(k, 0) + v
        moved = rng.choice(n0, 12, replace=False)  # SetWorldPos of local BA
        m.mps["pos"][moved] += np.float32(0.25)
        for k in range(0, m.nkf, 3):  # UpdateConnections: new ordered lists
            m.update_connections(k)
        d = fb.delta()
        assert d.stream == 2 and not d.empty()
        st = R.State(len(m.mps) + 1, cap, shadow["mp"], shadow["desc"], shadow["graph"], tail=S.SENTINEL)
        assert st.apply(d) == 0
        now = dict(mp=m.mps, desc=m.mp_desc, graph=tracking.covis_graph_from_loopmap(m))
        assert S.same_map(S.map_of_state(st), now) == []
        assert set(moved.tolist()) <= set(d.set_mp_idx.tolist())
        fb.commit()
        assert fb.delta().empty()
    for kind in ("new_map_point", "replace", "set_bad_point", "set_bad_keyframe", "add_keyframe"):
        assert total.get(kind, 0) > 0, kind
    # not the identity mapping: a map that lost a point, a keyframe whose slots changed in number
    m.slots[1] = m.slots[1][:-1]
    with pytest.raises(ValueError):
        fb.delta()
