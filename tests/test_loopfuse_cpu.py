"""SearchAndFuse without a GPU: the conditions the synthetic maps must meet (on
the serial restatement's trace), the restatement against hand-computed tiny
cases, LoopMap's host surgery against the restatement, and search_and_fuse's
skip rule on a map that leaves nothing to search."""
import numpy as np
import pytest

import loopfuse_ref as R
import loopfuse_scenes as S
import oracle_lib as O
from gf_orb_slam_amd.loopmap import LoopMap
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE


def cpu_distinctive(desc, offsets, current):
    """ComputeDistinctiveDescriptors on the CPU oracle, in the shape LoopMap asks for."""
    best, out = O.distinctive_descriptors(desc, offsets)
    return best, np.where((best >= 0)[:, None], out, current)


def _run_ref(sc):
    ref = R.RefMap(*S.map_args(sc))
    kfs = sc["cur"]
    return ref, ref.search_and_fuse(kfs, np.stack([sc["corrected"][k] for k in kfs]), sc["loop_points"], 4.0)


def test_small_scene_meets_its_conditions():
    sc = S.small()
    assert len(sc["kf_kps"]) == 6 and len(sc["cur"]) == 3
    for k in sc["cur"]:  # scale != 1: sqrt(row0 . row0) of Scw
        assert abs(np.linalg.norm(sc["corrected"][k][0, :3]) - 1.3) < 1e-5
    pts, bad0, slots0 = sc["loop_points"], sc["mp_bad"].copy(), [s.copy() for s in sc["kf_mp"]]
    ref, o = _run_ref(sc)
    nk = len(sc["cur"])
    # (a) a slot chosen by at least three candidates in one call
    assert max(np.bincount(o["kp"][j][o["kp"][j] >= 0]).max() for j in range(nk)) >= 3
    # (b) a bad occupant
    assert (o["action"] == R.ACTIONS.index("keep")).any()
    # (c) an empty slot taken, then chosen again in the same call
    hit = False
    for j in range(nk):
        added = set(o["kp"][j][o["action"][j] == R.ACTIONS.index("add")])
        for i in np.nonzero(o["action"][j] == R.ACTIONS.index("replace"))[0]:
            hit |= o["kp"][j][i] in added and slots0[sc["cur"][j]][o["kp"][j][i]] < 0
    assert hit
    # (d) Replace's erase branch
    assert ref.counter("erase_branch") > 0
    # (e) a loop point skipped because an earlier call made it bad
    assert any(((o["exit"][j] == R.X["bad"]) & ~bad0[pts]).any() for j in range(1, nk))
    # (f) one skipped because an earlier Replace put it into the keyframe
    assert any(((o["exit"][j] == R.X["found"]) & ~np.isin(pts, slots0[sc["cur"][j]])).any() for j in range(1, nk))
    # (g) a recomputed descriptor picks another keypoint than the launch-time one would
    g = (o["exit"] == R.X["fused"]) & (o["stale_kp"] >= 0) & (o["stale_kp"] != o["kp"])
    assert g[1:].any()
    # (h) every geometric exit
    for name in ("depth", "image", "range", "angle", "window", "level", "dist"):
        assert (o["exit"] == R.X[name]).any(), name
    # at least 20 % of the loop points fuse somewhere
    assert (o["exit"] == R.X["fused"]).any(0).mean() >= 0.2


def test_edge_scene_shapes():
    sc = S.edges()
    assert len(sc["kf_kps"][0]) == 1000 and len(sc["kf_kps"][1]) == 0 and len(sc["loop_points"]) == 1500
    ref = R.RefMap(*S.map_args(sc))
    o = ref.fuse(0, sc["corrected"][0], sc["loop_points"], 4.0)
    assert (o["kp"] >= 0).mean() >= 0.2
    o = ref.fuse(1, sc["corrected"][1], sc["loop_points"], 4.0)
    assert (o["kp"] == -1).all() and o["nFused"] == 0


def _tiny():
    """Camera at the origin, Scw = 2 * I. Keypoint 0 at the principal point
    (descriptor zeros, slot: point 2), keypoint 1 far away. Points 0 and 1 are
    loop points on the optical axis at depth 4 with 3 and 5 bits set; point 2
    is the keyframe's own, also seen by keyframe 1 at slot 0."""
    info = FrameInfo.make(752, 480, 400.0, 400.0, 376.0, 240.0)
    k0 = np.zeros(2, KEYPOINT_DTYPE)
    k0["x"], k0["y"] = [376.0, 100.0], [240.0, 100.0]
    k1 = np.zeros(1, KEYPOINT_DTYPE)
    k1["x"], k1["y"] = 50.0, 60.0
    d0 = np.zeros((2, 32), np.uint8)
    d0[1] = 0xFF
    d1 = np.full((1, 32), 0x0F, np.uint8)
    mps = np.zeros(3, MAP_POINT_DTYPE)
    mps["pos"], mps["normal"] = [0, 0, 4], [0, 0, 1]
    mps["min_dist"], mps["max_dist"] = 4, 20  # ratio 1: level 0, radius 4
    md = np.zeros((3, 32), np.uint8)
    md[0, 0], md[1, 0], md[2] = 0b111, 0b11111, 0xAA
    S2 = np.diag([2, 2, 2, 1]).astype(np.float32)
    return info, [k0, k1], [d0, d1], [np.array([2, -1], np.int32), np.array([2], np.int32)], mps, md, S2


def test_restatement_on_a_hand_computed_chain():
    info, kps, desc, slots, mps, md, S2 = _tiny()
    ref = R.RefMap(info, kps, desc, slots, mps, md)
    # search only: both points reach keypoint 0 at Hamming distance 3 and 5
    o = ref.fuse(0, S2, [0, 1], 4.0, apply=False)
    assert list(o["kp"]) == [0, 0] and list(o["dist"]) == [3, 5] and o["nFused"] == 2
    assert np.array_equal(ref.slots()[0], [2, -1])
    # the chain: 2 is replaced by 0, then 0 by 1; both slots of 2 follow
    o = ref.fuse(0, S2, [0, 1], 4.0, apply=True)
    assert [R.ACTIONS[a] for a in o["action"]] == ["replace", "replace"] and list(o["replaced"]) == [2, 0]
    sl = ref.slots()
    assert np.array_equal(sl[0], [1, -1]) and np.array_equal(sl[1], [1])
    bad, d = ref.points()
    assert list(bad) == [True, False, True]
    assert np.array_equal(ref.observation_rows(), [[1, 0, 0], [1, 1, 0]])
    # two rows: both medians are the self distance 0, the first row (keyframe 0's, zeros) wins
    assert not d[1].any() and not d[0].any()
    # a second call finds point 1 in the keyframe and point 0 bad
    o = ref.fuse(0, S2, [0, 1], 4.0, apply=True)
    assert [R.EXITS[e] for e in o["exit"]] == ["bad", "found"] and o["nFused"] == 0


def test_restatement_scale_and_exits_by_hand():
    info, kps, desc, slots, mps, md, S2 = _tiny()
    ref = R.RefMap(info, kps, desc, slots, mps, md)
    # without the division by scw the camera centre would move; with t = (0, 0, 2) * 2 the point sits at depth 6
    S = S2.copy()
    S[2, 3] = 4.0  # tcw = (0, 0, 2): dist3D = 6, ratio 1.5 -> level 3, radius 4 * 1.728
    assert R.EXITS[ref.fuse(0, S, [0], 4.0)["exit"][0]] == "level"  # keypoint 0 is at octave 0
    S[2, 3] = -10.0  # behind the camera
    assert R.EXITS[ref.fuse(0, S, [0], 4.0)["exit"][0]] == "depth"
    S[2, 3], S[0, 3] = 0.0, 16.0  # tcw = (8, 0, 0): u = 376 + 400 * 2
    assert R.EXITS[ref.fuse(0, S, [0], 4.0)["exit"][0]] == "image"


def _compare(lm, ref):
    for a, b in zip(lm.slots, ref.slots()):
        assert np.array_equal(a, b)
    bad, d = ref.points()
    assert np.array_equal(lm.mp_bad, bad) and np.array_equal(lm.mp_desc, d)
    assert np.array_equal(lm.observation_rows(), ref.observation_rows())


def test_loopmap_surgery_equals_restatement():
    sc = S.small()
    lm = LoopMap(*S.map_args(sc), distinctive=cpu_distinctive)
    ref = R.RefMap(*S.map_args(sc))
    _compare(lm, ref)
    rng = np.random.default_rng(0)
    n = len(sc["mps"])
    erased0 = ref.counter("erase_branch")
    for step in range(400):
        if step % 4 == 3:  # AddObservation overwrites; AddMapPoint may give a point a second slot
            p, kf = int(rng.integers(n)), int(rng.integers(len(lm.slots)))
            idx = int(rng.integers(len(lm.slots[kf])))
            lm.add_observation(p, kf, idx), ref.add_observation(p, kf, idx)
            lm.add_map_point(kf, p, idx), ref.add_map_point(kf, p, idx)
        else:
            a, b = (int(x) for x in rng.integers(n, size=2))
            if step % 50 == 0:
                b = a  # the same-id return
            lm.replace(a, b), ref.replace(a, b)
    _compare(lm, ref)
    assert ref.counter("erase_branch") > erased0 and ref.counter("same_id") > 0
    assert lm.mp_bad.sum() > sc["mp_bad"].sum() and lm.desc_epoch.any()


def _same_graph(lm, ref):
    for k in range(lm.nkf):
        o, w, wm, parent = ref.connections(k)
        assert lm.ordered[k] == o and lm.ordered_w[k] == w and lm.weights[k] == wm and lm.parent[k] == parent, k


def test_update_connections_equals_restatement():
    """On the small map, in an order that makes AddConnection rebuild lists that
    UpdateConnections wrote, before and after the fusion changed the slots."""
    from gf_orb_slam_amd.sim3 import loop_connections, loop_fusion

    sc = S.small()
    lm = LoopMap(*S.map_args(sc), distinctive=cpu_distinctive)
    ref = R.RefMap(*S.map_args(sc))
    for k in (2, 0, 4, 1, 3, 5, 2):
        lm.update_connections(k), ref.update_connections(k)
    _same_graph(lm, ref)
    assert all(lm.ordered[k] for k in range(lm.nkf)) and lm.parent[0] == -1 and lm.parent[3] >= 0
    # the loop fusion block: matches of the current keyframe (2) with loop points it does not hold
    rng = np.random.default_rng(1)
    matched = np.full(len(lm.slots[2]), -1, np.int32)
    idx = rng.permutation(len(matched))[:60]
    matched[idx] = rng.permutation(sc["n_loop_points"])[:60]
    assert (lm.slots[2][idx] >= 0).any() and (lm.slots[2][idx] < 0).any()
    loop_fusion(lm, 2, matched), ref.loop_fusion(2, matched)
    _compare(lm, ref)
    # SearchAndFuse as the restatement does it, mirrored into the LoopMap by its actions
    kfs = sc["cur"]
    o = ref.search_and_fuse(kfs, np.stack([sc["corrected"][k] for k in kfs]), sc["loop_points"], 4.0)
    for j, k in enumerate(kfs):
        for i in np.nonzero(o["action"][j])[0]:
            p, kp, act = int(sc["loop_points"][i]), int(o["kp"][j][i]), R.ACTIONS[o["action"][j][i]]
            if act == "replace":
                lm.replace(int(o["replaced"][j][i]), p)
            elif act == "add":
                lm.add_observation(p, k, kp), lm.add_map_point(k, p, kp)
    _compare(lm, ref)
    connected = lm.ordered[2] + [2]
    got, want = loop_connections(lm, connected), ref.loop_connections(connected)
    assert got == want
    _same_graph(lm, ref)
    assert any(got.values())  # the fusion tied the two sides of the loop together


def test_update_connections_weight_map_and_ordered_list_by_hand():
    """Keyframe 0 shares 20 points with keyframe 1 and 3 with keyframe 2: its
    weight map gets both, its ordered list only keyframe 1; keyframe 2, below
    the threshold everywhere, lists its single heaviest neighbour and tells it,
    and an AddConnection with a new weight rebuilds keyframe 0's list from every weight."""
    info = FrameInfo.make(752, 480, 400.0, 400.0, 376.0, 240.0)
    kps = [np.zeros(23, KEYPOINT_DTYPE), np.zeros(20, KEYPOINT_DTYPE), np.zeros(4, KEYPOINT_DTYPE)]
    desc = [np.zeros((len(k), 32), np.uint8) for k in kps]
    slots = [np.arange(23, dtype=np.int32), np.arange(20, dtype=np.int32),
             np.array([20, 21, 22, 23], np.int32)]  # point 23 is seen by keyframe 2 alone
    mps = np.zeros(24, MAP_POINT_DTYPE)
    lm = LoopMap(info, kps, desc, slots, mps, np.zeros((24, 32), np.uint8), distinctive=cpu_distinctive)
    ref = R.RefMap(info, kps, desc, slots, mps, np.zeros((24, 32), np.uint8))
    lm.update_connections(0), ref.update_connections(0)
    assert lm.weights[0] == {1: 20, 2: 3} and lm.ordered[0] == [1] and lm.ordered_w[0] == [20]
    assert lm.weights[1] == {0: 20} and lm.ordered[1] == [0] and lm.weights[2] == {}
    assert lm.get_connected_keyframes(0) == {1, 2} and lm.parent[0] == -1  # keyframe 0 never gets a parent
    _same_graph(lm, ref)
    lm.update_connections(2), ref.update_connections(2)
    assert lm.weights[2] == {0: 3} and lm.ordered[2] == [0] and lm.parent[2] == 0
    assert lm.ordered[0] == [1]  # AddConnection(2, 3) found the same weight in the map and returned
    _same_graph(lm, ref)
    for m in (lm, ref):  # one more shared point: the weight changes, and the list is rebuilt from every weight
        m.add_map_point(2, 19, 3), m.add_observation(19, 2, 3)
        m.update_connections(2)
    assert lm.weights[2] == {0: 4, 1: 1} and lm.ordered[2] == [0] and lm.ordered_w[2] == [4]
    assert lm.ordered[0] == [1, 2] and lm.ordered_w[0] == [20, 4] and lm.weights[1] == {0: 20}
    _same_graph(lm, ref)


def test_update_normal_and_depth_bit_equal_to_restatement():
    """Same stated float order on both sides: equal to the bit. Poses away from
    the identity, a reference keyframe that does not observe the point
    (observations[pRefKF] inserts slot 0), a bad point and one without
    observations."""
    from gf_orb_slam_amd import synth

    sc = S.small()
    rng = np.random.default_rng(2)
    T = np.stack([synth.look_pose(rng, 0.5, 20.0) for _ in range(6)])
    lm = LoopMap(*S.map_args(sc), distinctive=cpu_distinctive, kf_Tcw=T)
    ref = R.RefMap(*S.map_args(sc))
    ref.set_scale_factor(sc["info"].scale_factor)
    n = len(sc["mps"])
    lm.ref_kf[5], lm.obs[6] = next(k for k in range(6) if k not in lm.obs[5]), {}
    for k in range(6):
        ref.set_pose(k, T[k])
    for p in range(n):
        ref.set_ref(p, lm.ref_kf[p])
    before = lm.mps.copy()
    ids = np.arange(n)
    lm.update_normal_and_depth(ids), ref.update_normal_and_depth([p for p in ids if p != 6])
    g = ref.geometry()
    keep = np.ones(n, bool)
    keep[6] = False
    for name, cols in (("pos", slice(0, 3)), ("normal", slice(3, 6)), ("min_dist", 6), ("max_dist", 7)):
        assert lm.mps[name][keep].tobytes() == np.ascontiguousarray(g[keep][:, cols]).tobytes(), name
    changed = np.any(lm.mps["normal"] != before["normal"], axis=1)
    assert changed[5] and changed.sum() > n // 2
    assert not changed[sc["mp_bad"]].any() and not changed[6]
    assert np.allclose(np.linalg.norm(lm.mps["normal"][changed], axis=1), 1, atol=0.2)
    assert (lm.mps["max_dist"][changed] > lm.mps["min_dist"][changed]).all()


def test_distinctive_leaves_bad_and_unobserved_points():
    sc = S.small()
    bad = sc["mp_bad"].copy()
    bad[0] = True
    lm = LoopMap(*S.map_args(sc)[:6], bad, distinctive=cpu_distinctive)
    lm.obs[1] = {}
    before = lm.mp_desc.copy()
    lm.compute_distinctive_descriptors([0, 1])
    assert np.array_equal(lm.mp_desc, before) and not lm.desc_epoch.any()


def test_search_and_fuse_fuses_nothing_when_every_point_is_in_every_keyframe():
    """Identity scale, CorrectedSim3 == NonCorrectedSim3 (the poses themselves),
    every loop point in every searched keyframe: :1739 skips them all, so no
    device is needed to say so."""
    from gf_orb_slam_amd.sim3 import search_and_fuse, sim3_of_pose

    rng = np.random.default_rng(5)
    info = FrameInfo.make(752, 480, 400.0, 400.0, 376.0, 240.0)
    npts, nkf = 40, 3
    kps, desc, slots = [], [], []
    for _ in range(nkf):
        k = np.zeros(npts + 5, KEYPOINT_DTYPE)
        k["x"], k["y"] = rng.uniform(0, 752, npts + 5), rng.uniform(0, 480, npts + 5)
        kps.append(k), desc.append(rng.integers(0, 256, (npts + 5, 32), dtype=np.uint8))
        s = np.full(npts + 5, -1, np.int32)
        s[rng.permutation(npts + 5)[:npts]] = np.arange(npts)
        slots.append(s)
    mps = np.zeros(npts + 1, MAP_POINT_DTYPE)
    mps["pos"][:, 2], mps["normal"][:, 2], mps["min_dist"], mps["max_dist"] = 4, 1, 1, 20
    bad = np.zeros(npts + 1, bool)
    bad[npts] = True  # a bad loop point that is in no keyframe
    lm = LoopMap(info, kps, desc, slots, mps, rng.integers(0, 256, (npts + 1, 32), dtype=np.uint8), bad,
                 distinctive=cpu_distinctive)
    before = [s.copy() for s in lm.slots]
    cor = {k: sim3_of_pose(np.eye(4, dtype=np.float32)) for k in range(nkf)}
    out = search_and_fuse(lm, cor, np.arange(npts + 1, dtype=np.int32))
    assert out["nFused"] == {0: 0, 1: 0, 2: 0} and all(not a for a in out["actions"].values())
    assert all(np.array_equal(a, b) for a, b in zip(before, lm.slots))
    assert search_and_fuse(lm, cor, np.zeros(0, np.int32))["nFused"] == {0: 0, 1: 0, 2: 0}
    with pytest.raises(ValueError):
        search_and_fuse(lm, cor, np.array([npts + 7], np.int32))
