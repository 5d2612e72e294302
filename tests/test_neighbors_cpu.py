"""SearchInNeighbors without a GPU: the tests' restatement
(tests/helpers/neighbors_ref.cpp) against the CPU oracle's Fuse and against the
loop-closing restatement's Replace / UpdateNormalAndDepth / UpdateConnections,
the conditions the synthetic scene must meet to be worth testing on, and the
marker assumption (docs/ORACLE_ASSUMPTIONS.md A28)."""
import numpy as np
import pytest

import neighbors_ref as NR
import neighbors_scenes as S
from gf_orb_slam_amd.matcher import FUSE_ADD, FUSE_KEEP, FUSE_NONE, FUSE_REPLACE, camera_center

A_NONE, A_ADD, A_REPLACE, A_KEEP = range(4)


@pytest.fixture(scope="module")
def run():
    """The restatement's SearchInNeighbors on the scene: (scene, world after, report)."""
    sc = S.small()
    w = S.ref_world(sc)
    return sc, w, w.search_in_neighbors(sc["cur"])


def test_fuse_agrees_with_the_oracle():
    """Single Fuse calls: the new keyframe's points into three targets, each on
    a fresh world. The oracle decides from the tables as they are when the
    call begins; inside one call that is what the live map gives."""
    import oracle_lib as O

    sc = S.small()
    pts = sc["kf_mp"][sc["cur"]]
    safe = np.maximum(pts, 0)
    for k in (0, 3, 5):
        w = S.ref_world(sc)
        r = w.fuse(k, pts, 3.0, apply=True)
        in_kf = np.array([p < 0 or sc["mp_bad"][p] or k in sc["observations"][p] for p in pts])
        slots = sc["kf_mp"][k]
        slot_bad = np.where(slots >= 0, sc["mp_bad"][np.maximum(slots, 0)], False).astype(np.uint8)
        T = sc["kf_Tcw"][k]
        nf, res = O.fuse(sc["info"], T, camera_center(T), sc["kf_kps"][k], sc["kf_desc"][k], slots, slot_bad,
                         sc["mps"][safe], sc["mp_desc"][safe], in_kf.astype(np.uint8), pts, 3.0)
        assert nf == r["nFused"] > 20
        assert np.array_equal(res["kp"], r["kp"])
        want = {FUSE_NONE: A_NONE, FUSE_ADD: A_ADD, FUSE_REPLACE: A_REPLACE, FUSE_KEEP: A_KEEP}
        assert np.array_equal([want[int(a)] for a in res["action"]], r["action"])
        rep = r["action"] == A_REPLACE
        assert np.array_equal(res["target"][rep], r["other"][rep])
        assert {A_ADD, A_REPLACE, A_KEEP} <= set(int(a) for a in r["action"])


def test_map_calls_agree_with_the_loop_restatement():
    """Replace, UpdateNormalAndDepth and UpdateConnections against
    loopfuse_ref.RefMap on the same world."""
    from loopfuse_ref import RefMap

    sc = S.small()
    # both graphs start empty, the bad flag set from the start
    a = NR.RefWorld(*[sc[k] for k in S._KEYS], kf_Tcw=sc["kf_Tcw"], ref_kf=sc["ref_kf"], kf_id=sc["kf_id"])
    b = RefMap(*[sc[k] for k in S._KEYS])
    b.set_scale_factor(sc["info"].scale_factor)
    for k, T in enumerate(sc["kf_Tcw"]):
        b.set_pose(k, T)
    for p, r in enumerate(sc["ref_kf"]):
        b.set_ref(p, r)
    # pairs of instances of one world point, the second already in a keyframe of the first where there is one
    world, bad = sc["world"], sc["mp_bad"]
    pairs = []
    for wi in np.unique(world):
        ids = [int(p) for p in np.nonzero((world == wi) & ~bad)[0] if sc["observations"][p]]
        if len(ids) >= 2:
            pairs.append((ids[0], ids[1]))
    assert len(pairs) > 50
    for x, y in pairs[:60]:
        a.replace(x, y), b.replace(x, y)
    assert a.counter("erase_branch") == b.counter("erase_branch") > 0
    ids = range(len(sc["mps"]))
    a.update_normal_and_depth(ids), b.update_normal_and_depth(ids)
    for k in range(len(sc["kf_kps"])):
        a.update_connections(k), b.update_connections(k)
    assert all(np.array_equal(x, y) for x, y in zip(a.slots(), b.slots()))
    assert all(np.array_equal(x, y) for x, y in zip(a.points(), b.points()))
    assert np.array_equal(a.observation_rows(), b.observation_rows())
    assert a.geometry().tobytes() == b.geometry().tobytes()
    # ordered covisibles, their weights, the weight map and the parent of every keyframe
    for k in range(len(sc["kf_kps"])):
        assert a.connections(k) == b.connections(k), k
    assert len(a.connections(sc["cur"])[0]) >= 6


def _forward_rows(r):
    """(target index, candidate index) of every fused forward candidate, by action."""
    out = {A_ADD: [], A_REPLACE: [], A_KEEP: []}
    for j in range(len(r["targets"])):
        for i in np.nonzero(r["f_exit"][j] == NR.X["fused"])[0]:
            out[int(r["f_action"][j, i])].append((j, int(i)))
    return out


def test_scene_forward_actions(run):
    sc, w, r = run
    pts = sc["kf_mp"][sc["cur"]]
    rows = _forward_rows(r)
    assert len(rows[A_ADD]) > 100 and len(rows[A_KEEP]) >= 2
    # replaced by the slot's occupant at the start, or by a candidate this call added before
    by_occ = by_cand = 0
    for j, i in rows[A_REPLACE]:
        k, kp, other = int(r["targets"][j]), int(r["f_kp"][j, i]), int(r["f_other"][j, i])
        added_before = [(int(pts[i2]), int(r["f_kp"][j, i2])) for j2, i2 in rows[A_ADD] if j2 == j and i2 < i]
        if (other, kp) in added_before:
            by_cand += 1
        else:
            by_occ += 1
        assert k != sc["cur"]
    assert by_occ >= 10 and by_cand >= 3
    assert np.array_equal(r["nfused"], (r["f_exit"] == NR.X["fused"]).sum(1))


def test_scene_backward_actions(run):
    sc, w, r = run
    act, fused = r["b_action"], r["b_exit"] == NR.X["fused"]
    assert r["b_nfused"] == fused.sum()
    assert (act == A_ADD).sum() > 50 and (act == A_KEEP).sum() >= 2
    added = {}
    by_occ = by_cand = 0
    for i in np.nonzero(fused)[0]:
        kp = int(r["b_kp"][i])
        if act[i] == A_ADD:
            added[kp] = int(r["cand"][i])
        elif act[i] == A_REPLACE:
            if added.get(kp) == int(r["b_other"][i]):
                by_cand += 1
            else:
                by_occ += 1
    assert by_occ >= 5 and by_cand >= 20
    # the candidates: each once, none bad when listed, from the targets' tables
    assert len(set(r["cand"].tolist())) == len(r["cand"]) > 300


def test_scene_serial_effects(run):
    sc, w, r = run
    assert w.counter("erase_branch") >= 5
    # a descriptor changed under a candidate that is searched later: the stale search differs
    live = ~np.isin(r["f_exit"], [NR.X["null"], NR.X["bad"], NR.X["inkf"]])
    differs = live & (r["f_stale"] != r["f_kp"])
    assert differs.sum() >= 3
    assert (differs & (r["f_exit"] == NR.X["fused"])).sum() >= 1
    # a target listed twice, and what it fused the second time
    t = r["targets"].tolist()
    twice = [k for k in set(t) if t.count(k) > 1]
    assert twice
    second = [j for j, k in enumerate(t) if k in t[:j]]
    assert all(r["nfused"][j] <= r["nfused"][t.index(t[j])] for j in second)
    assert any(r["nfused"][j] > 0 for j in second)
    # the bad neighbour is skipped, as a first and as a second neighbour
    assert r["skipped_bad_kf"] >= 1 and S.BAD_KF not in t
    # a candidate an earlier target's walk turned bad
    pts = sc["kf_mp"][sc["cur"]]
    was_good = (pts >= 0) & ~sc["mp_bad"][np.maximum(pts, 0)]
    assert ((r["f_exit"][1:] == NR.X["bad"]) & was_good[None, :]).any()


def test_scene_bad_neighbour_is_a_first_neighbour():
    sc = S.small()
    w = S.ref_world(sc)
    assert S.BAD_KF in w.connections(sc["cur"])[0][:20]


def test_scene_early_exits(run):
    """No more than half the candidates of any search problem (every list
    entry, NULL slots included) leave before the descriptor loop, on the map as
    it stands when the problem is launched."""
    sc, w, r = run
    for j in range(len(r["targets"])):
        early = np.isin(r["f_exit0"][j], NR.BEFORE_DESCRIPTORS)
        assert early.mean() <= 0.5, (j, early.mean())
    assert np.isin(r["b_exit0"], NR.BEFORE_DESCRIPTORS).mean() <= 0.5


def test_markers_never_stamped_is_the_initial_value(run):
    """A28: the markers start at -1, the first call stamps first neighbours and
    candidates with the new keyframe's mnId, and a second call for the same
    keyframe finds every first neighbour stamped: no targets, no candidates."""
    sc, w, r = run
    cur_id = int(sc["kf_id"][sc["cur"]])
    fresh = S.ref_world(sc)
    kf0, mp0 = fresh.markers()
    assert (kf0 == -1).all() and (mp0 == -1).all()
    kf1, mp1 = w.markers()
    first = w.connections(sc["cur"])  # after the call; the first neighbours are read before it
    assert set(np.nonzero(kf1 == cur_id)[0]) == set(r["targets"].tolist())
    assert set(np.unique(kf1)) == {-1, cur_id} and first
    assert set(np.nonzero(mp1 == cur_id)[0]) == set(r["cand"].tolist())
    again = w.search_in_neighbors(sc["cur"])
    assert len(again["targets"]) == 0 and len(again["cand"]) == 0


def test_fuse_targets_matches_the_restatement(run):
    """localmapping.fuse_targets on the LoopMap: the same list, duplicates
    included, the same stamps, and nothing the second time."""
    from gf_orb_slam_amd.localmapping import fuse_targets

    sc, w, r = run
    m = S.loop_map(sc)
    fresh = S.ref_world(sc)
    assert m.ordered[sc["cur"]] == fresh.connections(sc["cur"])[0]
    assert (m.fuse_target_for == -1).all() and (m.fuse_candidate_for == -1).all()
    assert fuse_targets(m, sc["cur"]) == r["targets"].tolist()
    assert np.array_equal(m.fuse_target_for, w.markers()[0])
    assert fuse_targets(m, sc["cur"]) == []
    p = m.new_map_point([0, 0, 1], sc["cur"])
    assert len(m.fuse_candidate_for) == p + 1 and m.fuse_candidate_for[p] == -1
