"""KeyFrameCulling without a GPU: the planted outcomes of tests/kfcull_scenes.py
in the serial restatement (tests/helpers/kfcull_ref.cpp), LoopMap's
set_bad_keyframe / erase_observation / set_erase / children against it field by
field, and the host walk of localmapping.keyframe_culling with the
restatement's counter in the device's place."""
import kfcull_ref as R
import kfcull_scenes as S
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd.loopmap import LoopMap


def _world():
    sc = S.scene()
    m = S.loop_map(sc)
    return sc, m, R.RefWorld.from_loopmap(m)


def test_scene_planted_outcomes_in_the_restatement():
    sc, m, w = _world()
    n, pts, cur = sc["names"], sc["pts"], sc["cur"]
    R.assert_same_state(m, w)  # from_loopmap copies every field
    sizes = [len(k) for k in sc["kf_kps"]]
    assert len(sizes) >= 15 and min(sizes) >= 40 and max(sizes) <= 300
    assert m.ordered[cur] == [n[r] for r in S.ORDER] + [n["S1"]]
    first = {r: w.count(n[r]) for r in S.ROLES}  # what a single launch on the initial map sees
    r = w.keyframe_culling(cur)
    at = {k: j for j, k in enumerate(r["candidates"])}
    turn = lambda role: (r["nmps"][at[n[role]]], r["nredundant"][at[n[role]]])  # noqa: E731
    culled = lambda role: r["culled_at"][at[n[role]]]  # noqa: E731
    # protected: mnId 0 is listed, above 90 % and skipped
    assert n["K0"] in m.ordered[cur] and n["K0"] not in r["candidates"] and first["K0"][:2] == (10, 10)
    assert r["candidates"] == [n[x] for x in S.ORDER[1:]] + [n["S1"]]
    # row gates, octave boundary and A26 in M's flags at its turn
    fl, sl = r["flags"][at[n["M"]]], m.obs
    M = n["M"]
    assert [fl[sl[pts[x]][M]] for x in ("gate3", "gate4", "gate5")] == [1, 2, 2]
    assert [fl[sl[pts[x]][M]] for x in ("oct_pass", "oct_fail", "oct_fail5")] == [2, 1, 1]
    assert [fl[i] for i in sc["slots_of"]["twice"]] == [2, 1]
    assert fl[sc["slots_of"]["unlisted"]] == 2 and M not in sl[pts["unlisted"]]
    assert fl[sc["slots_of"]["phantom"]] == 0 and M in sl[pts["phantom"]]
    fq = r["flags"][at[n["Q"]]]
    assert fq[sl[pts["phantom"]][n["Q"]]] == 2  # redundant only through the observation without a table entry
    assert turn("M") == (int((fl > 0).sum()), int((fl == 2).sum())) == (21, 5) and not culled("M")
    # a bad point with an empty row
    assert m.mp_bad[pts["empty_row"]] and not sl[pts["empty_row"]] and pts["empty_row"] in sc["kf_mp"][n["D0"]]
    # decision boundary
    assert turn("D9") == (10, 9) and not culled("D9")
    assert turn("D10") == (10, 10) and culled("D10")
    assert turn("D11") == (11, 10) and culled("D11")
    assert turn("D0") == (0, 0) and not culled("D0")
    # order dependence
    assert first["A"][:2] == (22, 20) and turn("A") == (22, 20) and culled("A")
    assert first["B"][:2] == (10, 10) and turn("B") == (10, 0) and not culled("B")
    assert first["C"][:2] == (12, 10) and turn("C") == (10, 10) and culled("C")
    assert r["points_bad"] == [pts["ref_stays"]] + pts["ac"]
    # protected: deferred, to_be_erased
    st = w.state()
    for role in ("N", "L"):
        assert turn(role) == (10, 10) and r["deferred_at"][at[n[role]]] and not culled(role)
        assert st["to_be_erased"][n[role]] and not st["kf_bad"][n[role]]
    assert r["culled"] == [n[x] for x in ("D10", "D11", "A", "C", "T")]
    assert not r["culled_at"][at[n["S1"]]]
    # spanning tree
    assert r["reparented"] == [(n["c1"], n["S1"]), (n["c2"], n["c1"]), (n["c3"], n["S1"]), (n["c4"], n["c3"]),
                               (n["c5"], n["S1"])]
    assert [st["parent"][n[c]] for c in ("c1", "c2", "c3", "c4", "c5")] == [n[x] for x in
                                                                          ("S1", "c1", "S1", "c3", "S1")]
    # reference keyframe
    assert sc["ref_kf"][pts["ref_moves"]] == n["D10"] and st["ref_kf"][pts["ref_moves"]] == n["S1"]
    assert st["ref_kf"][pts["ref_stays"]] == n["D11"] and st["mp_bad"][pts["ref_stays"]]
    # a later SetErase: N goes, L keeps its flag (loop edge)
    assert w.set_erase(n["N"]) == 1 and w.set_erase(n["L"]) == 2
    st = w.state()
    assert st["kf_bad"][n["N"]] and not st["kf_bad"][n["L"]] and st["not_erase"][n["L"]] and not st["not_erase"][n["N"]]


def test_map_primitives_equal_the_restatement():
    sc, m, w = _world()
    n, pts = sc["names"], sc["pts"]
    assert m.children(n["T"]) == w.children(n["T"]) == {n[c] for c in ("c1", "c2", "c3", "c4", "c5")}
    for k in range(m.nkf):
        assert m.children(k) == w.children(k), k
    # erase_observation: absent keyframe, the reference keyframe, down to two observations
    p = pts["gate5"]
    for kf in (n["CUR"], min(m.obs[p]), n["S2"], n["M"]):
        bad = m.erase_observation(p, kf)
        w.erase_observation(p, kf)
        R.assert_same_state(m, w)
    assert bad and m.mp_bad[p] and m.ref_kf[p] == n["S3"]  # S1 -> S2 -> S3 as each reference keyframe left
    # erase_map_point_match has no counterpart call in the restatement's interface: the world is rebuilt
    assert m.slots[n["M"]][0] >= 0
    m.erase_map_point_match(n["M"], 0)
    assert m.slots[n["M"]][0] == -1
    w = R.RefWorld.from_loopmap(m)
    # set_bad_keyframe one by one: mnId 0, deferred, a plain one, the tree, the order-dependent pair
    for role, want in (("K0", 0), ("N", 2), ("L", 2), ("D11", 1), ("T", 1), ("A", 1), ("C", 1), ("S1", 1)):
        w.clear_log()
        log = m.set_bad_keyframe(n[role])
        assert w.set_bad_keyframe(n[role]) == want == (1 if log["erased"] else 2 if log["deferred"] else 0)
        wl = w.log()
        assert log["points_bad"] == wl["points_bad"] and log["reparented"] == wl["reparented"], role
        R.assert_same_state(m, w)
        for k in range(m.nkf):
            if not m.kf_bad[k]:
                assert m.children(k) == w.children(k), (role, k)
    assert not m.weights[n["S1"]] and not m.ordered[n["S1"]]
    # set_erase: N is culled now, L keeps its protection
    for role, want in (("N", 1), ("L", 2), ("D9", 0)):
        log = m.set_erase(n[role])
        assert w.set_erase(n[role]) == want
        assert (log is None) == (want == 0)
        R.assert_same_state(m, w)
    assert m.kf_bad[n["N"]] and not m.kf_bad[n["L"]] and m.not_erase[n["L"]]
    m.set_not_erase(n["D9"])
    assert m.not_erase[n["D9"]]


class _Db:
    def __init__(self):
        self.erased = []

    def erase(self, slot):
        self.erased.append(slot)


def _assert_report(rep, r):
    assert rep["candidates"] == r["candidates"]
    per = rep["per_candidate"]
    assert [q["kf"] for q in per] == r["candidates"]
    assert [q["nmps"] for q in per] == r["nmps"] and [q["nredundant"] for q in per] == r["nredundant"]
    assert [q["culled"] for q in per] == r["culled_at"] and [q["deferred"] for q in per] == r["deferred_at"]
    assert rep["culled"] == r["culled"] and rep["points_bad"] == r["points_bad"]
    assert rep["reparented"] == r["reparented"]


def test_keyframe_culling_walk_equals_the_restatement():
    sc, m, w = _world()
    n, cur = sc["names"], sc["cur"]
    db = _Db()
    rep = LM.keyframe_culling(m, cur, db=db, counter=R.counts)
    r = w.keyframe_culling(cur)
    _assert_report(rep, r)
    R.assert_same_state(m, w)
    assert db.erased == rep["culled"] and len(rep["culled"]) == 5
    assert rep["launches"] == 1 + len(rep["culled"])  # the last culled candidate is not the last of the list
    # only later candidates are counted again, once per cull before their turn
    at = {q["kf"]: q for q in rep["per_candidate"]}
    assert at[n["M"]]["recounted"] == 0 and at[n["D10"]]["recounted"] == 0 and at[n["D11"]]["recounted"] == 1
    assert at[n["S1"]]["recounted"] == 5
    # the order dependence, explicitly: B survives and C goes, against what the first launch alone says
    first = R.counts(*LM.culling_tables(S.loop_map(sc))[:6], [n["B"], n["C"]])
    assert first.tolist() == [[10, 10], [12, 10]]
    assert (at[n["B"]]["nmps"], at[n["B"]]["nredundant"], at[n["B"]]["culled"]) == (10, 0, False)
    assert (at[n["C"]]["nmps"], at[n["C"]]["nredundant"], at[n["C"]]["culled"]) == (10, 10, True)
    assert not m.kf_bad[n["B"]] and m.kf_bad[n["C"]]
    # a second walk finds nothing more to cull
    rep2 = LM.keyframe_culling(m, cur, counter=R.counts)
    _assert_report(rep2, w.keyframe_culling(cur))
    assert rep2["culled"] == [] and rep2["launches"] == 1
    R.assert_same_state(m, w)


def test_nothing_to_cull_is_one_launch():
    sc = S.scene(cull=False)
    m = S.loop_map(sc)
    w = R.RefWorld.from_loopmap(m)
    rep = LM.keyframe_culling(m, sc["cur"], counter=R.counts)
    _assert_report(rep, w.keyframe_culling(sc["cur"]))
    assert rep["culled"] == [] and rep["launches"] == 1 and not any(q["deferred"] for q in rep["per_candidate"])
    assert not m.to_be_erased.any() and not m.kf_bad.any()
    R.assert_same_state(m, w)


def test_realistic_map_after_search_in_neighbors():
    """neighbors_scenes.small() after SearchInNeighbors (run by that stage's
    own restatement, so no device is needed): the walk equals the restatement
    on a map built by the stages before it."""
    import neighbors_scenes as NS

    sc = NS.small()
    cur = sc["cur"]
    nw = NS.ref_world(sc)
    nw.search_in_neighbors(cur)
    rows = nw.observation_rows()
    obs = [dict() for _ in range(len(sc["mps"]))]
    for p, kf, idx in rows:
        obs[p][int(kf)] = int(idx)
    bad, desc = nw.points()
    m = LoopMap(sc["info"], sc["kf_kps"], sc["kf_desc"], nw.slots(), sc["mps"], desc, mp_bad=bad, observations=obs,
                kf_Tcw=sc["kf_Tcw"], ref_kf=sc["ref_kf"], kf_id=sc["kf_id"])
    for k in range(m.nkf):
        m.update_connections(k)
    m.kf_bad[:] = sc["kf_bad"]
    assert len(m.ordered[cur]) >= 4
    w = R.RefWorld.from_loopmap(m)
    rep = LM.keyframe_culling(m, cur, counter=R.counts)
    r = w.keyframe_culling(cur)
    _assert_report(rep, r)
    R.assert_same_state(m, w)
    # every keyframe of this scene sees most of one small world, so some are redundant; culling them ends it
    assert sum(r["nmps"]) > 1000 and 0 < len(rep["culled"]) < len(rep["candidates"])
