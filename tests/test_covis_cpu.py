"""UpdateConnections / ProcessNewKeyFrame without a GPU: the planted outcomes of
tests/covis_scenes.py in the serial restatement (tests/helpers/covis_ref.cpp),
LoopMap's add_keyframe / apply_connections / update_connections_batch against
the serial host walk and the restatement field by field, process_new_keyframe
and LocalMapper.step with the restatement's counter in the device's place."""
import numpy as np
import pytest

import covis_ref as R
import covis_scenes as S
import oracle_lib as O
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd import synth
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.loopmap import LoopMap
from test_loopfuse_cpu import cpu_distinctive

VOC = synth.synth_vocabulary(7, k=10, L=3)


def oracle_transform(desc, levelsup):
    return O.bow_transform(VOC, desc, levelsup)


def tables_of(m):
    t = LM.culling_tables(m)
    return t[0], t[2], t[3], t[4], t[5]


def rows_of(out, i):
    """(weight map, ordered keyframes, ordered weights) of query i of a counts result."""
    w, n, ok, ow = out
    return ({int(k): int(w[i, k]) for k in np.nonzero(w[i])[0]}, ok[i, :n[i]].tolist(), ow[i, :n[i]].tolist())


def order_of(weights: dict):
    """The ordering rule restated once more in Python, for the raw rows."""
    pairs = sorted(((w, k) for k, w in weights.items() if w >= 15), reverse=True)
    if not pairs and weights:
        top = max(weights.values())
        pairs = [(top, min(k for k, w in weights.items() if w == top))]
    return [k for _, k in pairs], [w for w, _ in pairs]


def assert_padding(out):
    w, n, ok, ow = out
    for i in range(len(n)):
        assert np.all(ok[i, n[i]:] == -1) and np.all(ow[i, n[i]:] == 0), i


def test_planted_outcomes_in_the_restatement():
    sc = S.scene()
    m = S.loop_map(sc)
    n, expect = sc["names"], sc["expect"]
    roles = list(S.ROLES)
    out = R.counts(*tables_of(m), [n[r] for r in roles])
    assert_padding(out)
    got = {r: rows_of(out, i) for i, r in enumerate(roles)}
    for r, want in expect.items():
        assert got[r] == want, r
    # threshold: exactly 14 stays out of the list, 15 and 16 are in it
    assert got["TH"][1] == [n["T16"], n["T15"]] and got["TH"][0][n["T14"]] == 14
    # fallback: the lower index wins the tie at the maximum; a single shared point is enough
    assert n["F1"] < n["F2"] and got["FB"][1:] == ([n["F1"]], [9]) and got["ONE"][1:] == ([n["ONE_N"]], [1])
    # order: the tie at 20 comes highest index first, between the distinct weights
    assert n["Oa"] < n["Ob"] < n["Oc"] and got["ORD"][2] == [30, 25, 20, 20, 20, 17]
    assert got["ORD"][1][2:5] == [n["Oc"], n["Ob"], n["Oa"]]
    # empty: no slots, points of its own only, bad points only
    for r in ("EMPTY0", "LONE", "BADONLY"):
        assert got[r] == ({}, [], []), r
    assert len(sc["kf_mp"][n["EMPTY0"]]) == 0 and all(m.mp_bad[p] and m.obs[p] for p in sc["pts"]["badonly"])
    # A26
    so, pts, AQ = sc["slots_of"], sc["pts"], n["AQ"]
    assert [m.slots[AQ][i] for i in so["twice"]] == [pts["twice"]] * 2 and got["AQ"][0][n["A1"]] == 3
    assert m.slots[AQ][so["unlisted"]] == pts["unlisted"] and AQ not in m.obs[pts["unlisted"]]
    assert m.slots[AQ][so["phantom"]] == -1 and m.obs[pts["phantom"]][AQ] == so["phantom"]
    assert n["A4"] not in got["AQ"][0] and got["A4"][0] == {AQ: 1}
    # own observation: the query is in its own points' rows and never in its counter
    for r in roles:
        k = n[r]
        assert k not in got[r][0]
    assert all(n["TH"] in m.obs[p] for p in m.slots[n["TH"]] if p >= 0)
    # a query outside [0, nkf) and a repeated one
    out = R.counts(*tables_of(m), [n["TH"], -1, m.nkf, n["TH"]])
    assert rows_of(out, 0) == rows_of(out, 3) == expect["TH"] and rows_of(out, 1) == rows_of(out, 2) == ({}, [], [])


def test_raw_tables_in_the_restatement():
    sc = S.scene(edges=True)
    m = S.loop_map(sc)
    n = sc["names"]
    *t, info = S.raw_tables(m, sc)
    out = R.counts(*t, [n["AQ"], n["RAWQ"]])
    assert_padding(out)
    aq, rawq = rows_of(out, 0), rows_of(out, 1)
    assert aq[0] == info["aq"] and aq[0][n["A2"]] == 2 and aq[0][n["A3"]] == 2 and aq[1:] == ([n["A1"]], [3])
    assert rawq[0] == info["rawq"] and rawq[1:] == order_of(info["rawq"])
    assert sum(info["rawq"].values()) > 400 and len(rawq[1]) >= 1


@pytest.mark.parametrize("nkf", [1, 2, 65, 1100])
def test_thin_tables_in_the_restatement(nkf):
    *t, query, listed = S.thin_tables(nkf)
    out = R.counts(*t, query)
    assert_padding(out)
    for i, want in enumerate(listed):
        wmap, ok, ow = rows_of(out, i)
        assert (ok, ow) == order_of(wmap), i
        if nkf == 1:
            assert (wmap, ok) == ({}, [])
        elif want:
            assert len(ok) == want and min(ow) >= 15
        else:
            assert len(ok) == 1 and ow[0] < 15  # the fallback
    if nkf == 1100:
        assert listed == list(S.LIST_SIZES)


def test_second_witness_on_a_realistic_map():
    """neighbors_ref.RefWorld.update_connections (another restatement, on
    its own world) agrees with the flat-table one on neighbors_scenes.small()."""
    import neighbors_scenes as NS

    sc = NS.small()
    m = NS.loop_map(sc)
    w = NS.ref_world(sc)
    out = R.counts(*tables_of(m), np.arange(m.nkf))
    for k in range(m.nkf):
        w.update_connections(k)
        o, ow, wm, _ = w.connections(k)
        assert rows_of(out, k) == (wm, o, ow), k
    assert max(out[1]) >= 6


def _graph_maps(which):
    if which == "planted":
        sc = S.scene()
        return S.loop_map(sc), S.loop_map(sc)
    if which == "neighbors":
        import neighbors_scenes as NS

        return NS.loop_map(NS.small()), NS.loop_map(NS.small())
    import kfcull_scenes as KS

    return KS.loop_map(KS.scene()), KS.loop_map(KS.scene())


@pytest.mark.parametrize("which", ["planted", "neighbors", "kfcull"])
def test_batch_equals_the_serial_walk(which):
    a, b = _graph_maps(which)
    rng = np.random.default_rng(3)
    order = [int(k) for k in rng.permutation(a.nkf)] * 2 + [0, 0]  # every keyframe twice over, repeats included
    for k in order:
        a.update_connections(k)
    b.update_connections_batch(order, counter=R.counts)
    R.assert_same_maps(a, b)
    assert sum(len(o) for o in a.ordered) > a.nkf / 2
    if which == "planted":  # mnId = index there: the restatement's world walks the same way
        sc = S.scene()
        w = R.RefWorld.from_loopmap(S.loop_map(sc))
        for k in order:
            w.update_connections(k)
        R.assert_same_state(b, w)
        n = sc["names"]
        assert b.parent[n["K0"]] == -1 and b.first_connection[n["K0"]] and b.weights[n["K0"]] == {n["S"]: 3}
        assert b.parent[n["TH"]] == n["T16"] and not b.first_connection[n["TH"]]


def test_apply_connections_first_connection_and_empty_counts():
    sc = S.scene()
    m = S.loop_map(sc)
    n = sc["names"]
    # empty counts change nothing, a pre-set non-empty weight map included
    for r in ("EMPTY0", "LONE", "BADONLY"):
        k = n[r]
        m.weights[k], m.ordered[k], m.ordered_w[k] = {n["S"]: 40}, [n["S"]], [40]
    before = R.loopmap_state(m)
    m.update_connections_batch([n[r] for r in ("EMPTY0", "LONE", "BADONLY")], counter=R.counts)
    after = R.loopmap_state(m)
    assert all(np.array_equal(before[f], after[f]) for f in R.STATE)
    assert m.weights[n["LONE"]] == {n["S"]: 40} and m.first_connection[n["LONE"]]
    # the parent is set once: a second apply with another head keeps it
    TH = n["TH"]
    w, ordered = m.connections_counts([TH], counter=R.counts)
    m.apply_connections(TH, w[0], *ordered[0])
    assert m.parent[TH] == n["T16"] and not m.first_connection[TH]
    row = w[0].copy()
    row[n["T15"]] = 50
    m.apply_connections(TH, row, [n["T15"], n["T16"]], [50, 16])
    assert m.ordered[TH] == [n["T15"], n["T16"]] and m.parent[TH] == n["T16"]
    assert m.weights[n["T15"]][TH] == 50 and m.weights[TH] == {n["T14"]: 14, n["T15"]: 50, n["T16"]: 16}
    # mnId 0 never gets a parent
    K0 = n["K0"]
    assert m.kf_id[K0] == 0
    m.update_connections_batch([K0, K0], counter=R.counts)
    assert m.ordered[K0] == [n["S"]] and m.parent[K0] == -1 and m.first_connection[K0]
    assert m.weights[n["S"]][K0] == 3 and m.ordered[n["S"]] == [K0]


def test_add_keyframe_grows_every_field():
    m, (kps, desc, slots, Tcw, kf_id), _ = S.small_without_cur()
    nkf = m.nkf
    per_kf = [name for name, v in vars(m).items()
              if name != "mps" and hasattr(v, "__len__") and not isinstance(v, (str, dict)) and len(v) == nkf
              and name not in ("mp_desc", "mp_bad", "obs")]
    assert set(per_kf) >= {"kf_kps", "kf_desc", "slots", "kf_bad", "Tcw", "kf_id", "fuse_target_for", "weights",
                           "ordered", "ordered_w", "parent", "first_connection", "loop_edges", "not_erase",
                           "to_be_erased", "kf_bow", "kf_fv"}
    rows = m.observation_rows().copy()
    k = m.add_keyframe(kps, desc, slots, Tcw, kf_id)
    assert k == nkf and m.nkf == nkf + 1
    for name in per_kf:
        assert len(getattr(m, name)) == nkf + 1, name
    assert np.array_equal(m.slots[k], slots) and m.slots[k] is not slots and m.kf_id[k] == kf_id
    assert m.Tcw.shape == (nkf + 1, 4, 4) and m.Tcw[k].tobytes() == np.asarray(Tcw, np.float32).tobytes()
    assert not m.kf_bad[k] and m.parent[k] == -1 and m.first_connection[k] and m.weights[k] == {} and m.ordered[k] == []
    assert m.fuse_target_for[k] == -1 and m.kf_bow[k] is None and m.kf_fv[k] is None and m.loop_edges[k] == []
    assert np.array_equal(m.observation_rows(), rows)  # no observation is added
    assert m.add_keyframe(kps[:0], desc[:0], slots[:0], Tcw) == k + 1 and m.kf_id[k + 1] == kf_id + 1
    for bad_id in (kf_id + 1, kf_id, 0):
        with pytest.raises(GFError):
            m.add_keyframe(kps, desc, slots, Tcw, bad_id)
    with pytest.raises(GFError):
        m.add_keyframe(kps, desc, np.full(len(slots), len(m.mps), np.int32), Tcw)
    assert m.nkf == nkf + 2


def _serial_association(m, cur):
    """The per-point host methods in slot order, as LocalMapping.cc:179-191 calls them."""
    for i, p in enumerate(m.slots[cur].copy()):
        p = int(p)
        if p < 0 or m.mp_bad[p]:
            continue
        m.add_observation(p, cur, i)
        m.update_normal_and_depth([p])
        m.compute_distinctive_descriptors([p])


def test_process_new_keyframe_mnid_above_one():
    m, kf, planted = S.small_without_cur(distinctive=cpu_distinctive)
    ser, _, _ = S.small_without_cur(distinctive=cpu_distinctive)
    cur = m.add_keyframe(*kf)
    assert ser.add_keyframe(*kf) == cur and m.kf_id[cur] > 1
    sl = m.slots[cur]
    assert sl[planted["first"]] == sl[planted["second"]] == planted["point"] and planted["first"] < planted["second"]
    assert m.mp_bad[sl[planted["bad"]]] and sl[planted["null"]] == -1
    w = R.RefWorld.from_loopmap(m, recent=[5, 6])
    recent = [5, 6]
    calls = []

    def transform(desc, levelsup):
        calls.append(levelsup)
        return oracle_transform(desc, levelsup)

    rep = LM.process_new_keyframe(m, cur, transform, recent, levelsup=2, counter=R.counts)
    want = w.process_new_keyframe(cur)
    assert rep["associated"] == want["associated"] and recent == want["recent"] == [5, 6] and rep["recent_added"] == []
    assert want["bow_computed"][cur] == 1 and calls == [2]
    R.assert_same_state(m, w)
    assert rep["associated"].count(planted["point"]) == 2 and m.obs[planted["point"]][cur] == planted["second"]
    assert int(sl[planted["bad"]]) not in rep["associated"] and cur not in m.obs[int(sl[planted["bad"]])]
    assert rep["n_ordered"] == len(m.ordered[cur]) >= 4 and rep["parent"] == m.parent[cur] == m.ordered[cur][0]
    assert set(rep["times"]) == {"bow", "association", "tables", "launch", "apply"}
    # BoW: both stored, equal to the oracle's
    wo, vo, (nodes, start, feats) = oracle_transform(m.kf_desc[cur], 2)
    assert np.array_equal(m.kf_bow[cur][0], wo) and np.array_equal(m.kf_bow[cur][1], vo)
    fv = m.kf_fv[cur]
    assert np.array_equal(fv.nodes, nodes) and np.array_equal(fv.start, start) and np.array_equal(fv.feats, feats)
    # descriptors, normals and distance bounds: the per-point host methods, serially in slot order
    _serial_association(ser, cur)
    ser.update_connections(cur)
    assert m.mps.tobytes() == ser.mps.tobytes() and m.mp_desc.tobytes() == ser.mp_desc.tobytes()
    assert np.array_equal(m.observation_rows(), ser.observation_rows())
    x, y = R.loopmap_state(m), R.loopmap_state(ser)
    assert all(np.array_equal(x[f], y[f]) for f in R.STATE)
    ids = list(dict.fromkeys(rep["associated"]))
    assert len(ids) > 200 and np.any(m.mps["normal"][ids] != S.small_without_cur()[0].mps["normal"][ids])
    # ComputeBoW is not run again when both fields are set
    def never(desc, levelsup):
        raise AssertionError("ComputeBoW ran twice")

    rep2 = LM.process_new_keyframe(m, cur, never, recent, counter=R.counts)
    assert w.process_new_keyframe(cur)["bow_computed"][cur] == 1
    R.assert_same_state(m, w)
    assert rep2["associated"] == rep["associated"] and rep2["parent"] == rep["parent"]
    m.kf_fv[cur] = None  # one of the two missing is enough to compute both again
    LM.process_new_keyframe(m, cur, transform, recent, levelsup=2, counter=R.counts)
    assert calls == [2, 2] and m.kf_fv[cur] is not None


def _first_two_map():
    """A map of one keyframe (mnId 0) with 30 points, four of them bad, and the
    arrays of a second keyframe that matched some of them."""
    import neighbors_scenes as NS

    sc = NS.small()
    kps, desc = sc["kf_kps"][0][:40], sc["kf_desc"][0][:40]
    slots0 = np.full(40, -1, np.int32)
    slots0[:30] = np.arange(30)
    bad = np.zeros(30, bool)
    bad[[3, 7, 11, 20]] = True
    obs = [{} if bad[p] else {0: p} for p in range(30)]
    m = LoopMap(sc["info"], [kps], [desc], [slots0], sc["mps"][:30], sc["mp_desc"][:30], mp_bad=bad, observations=obs,
                kf_Tcw=sc["kf_Tcw"][:1], ref_kf=np.zeros(30, np.int32), distinctive=cpu_distinctive)
    slots1 = np.full(40, -1, np.int32)
    slots1[5:25] = np.arange(2, 22)  # bad 3, 7, 11 and 20 among them, NULL slots around
    return m, (sc["kf_kps"][1][:40], sc["kf_desc"][1][:40], slots1, sc["kf_Tcw"][1])


def test_process_new_keyframe_first_two_keyframes():
    # mnId 0: BoW only
    m, kf1 = _first_two_map()
    empty = LoopMap(m.info, [], [], [], m.mps, m.mp_desc, mp_bad=m.mp_bad, observations=[{} for _ in m.obs],
                    ref_kf=np.full(len(m.mps), -1, np.int32), first_kf=np.full(len(m.mps), -1, np.int64))
    k0 = empty.add_keyframe(m.kf_kps[0], m.kf_desc[0], m.slots[0], m.Tcw[0])
    assert k0 == 0 and empty.kf_id[0] == 0
    w = R.RefWorld.from_loopmap(empty)
    recent = []
    before = R.loopmap_state(empty)
    rep = LM.process_new_keyframe(empty, k0, oracle_transform, recent, counter=R.counts)
    want = w.process_new_keyframe(k0)
    assert rep["associated"] == want["associated"] == [] and recent == want["recent"] == [] and rep["n_ordered"] == 0
    assert empty.kf_bow[0] is not None and empty.kf_fv[0] is not None and want["bow_computed"] == [1]
    after = R.loopmap_state(empty)
    assert all(np.array_equal(before[f], after[f]) for f in R.STATE)
    R.assert_same_state(empty, w)
    # mnId 1: every non-NULL point enters the recent list, bad ones included; nothing is associated
    k1 = m.add_keyframe(*kf1)
    assert m.kf_id[k1] == 1
    w = R.RefWorld.from_loopmap(m, recent=[29])
    recent = [29]
    rows = m.observation_rows().copy()
    geo, desc = m.mps.copy(), m.mp_desc.copy()
    rep = LM.process_new_keyframe(m, k1, oracle_transform, recent, counter=R.counts)
    want = w.process_new_keyframe(k1)
    assert rep["associated"] == want["associated"] == []
    assert rep["recent_added"] == list(range(2, 22)) and recent == want["recent"] == [29] + list(range(2, 22))
    assert all(p in recent for p in (3, 7, 11, 20)) and m.mp_bad[[3, 7, 11, 20]].all()
    assert np.array_equal(m.observation_rows(), rows) and m.mps.tobytes() == geo.tobytes()
    assert m.mp_desc.tobytes() == desc.tobytes()
    R.assert_same_state(m, w)
    assert m.weights[k1] == {0: 16} and m.ordered[k1] == [0] and m.parent[k1] == 0 and rep["parent"] == 0
    assert m.weights[0] == {k1: 16} and m.parent[0] == -1


def test_local_mapper_runs_the_stages_in_order():
    import kfcull_ref
    import lbamap_ref
    from test_lbamap_cpu import oracle_solver

    def mapper(log):
        m, kf, _ = S.small_without_cur(distinctive=cpu_distinctive)

        def create(map, cur, kf_fv, ctx=None):
            assert kf_fv is map.kf_fv and kf_fv[cur] is not None
            log.append("create_new_map_points")
            return [], dict(points=[])

        def search(map, cur, ctx=None):
            log.append("search_in_neighbors")
            map.update_connections(cur)
            return dict(targets=[])

        def spy(name, fn):
            def run(*a, **kw):
                log.append(name)
                return fn(*a, **kw)
            return run

        stages = dict(create_new_map_points=create, search_in_neighbors=search)
        for name in ("process_new_keyframe", "map_point_culling", "local_bundle_adjustment", "keyframe_culling"):
            stages[name] = spy(name, getattr(LM, name))
        lm = LM.LocalMapper(m, oracle_transform, levelsup=2, counter=R.counts, cull_counter=kfcull_ref.counts,
                            assembler=lambda t, local: lbamap_ref.assembler(m)[0](t, local), solver=oracle_solver,
                            stages=stages)
        return lm, lm.insert_keyframe(*kf)

    log = []
    lm, cur = mapper(log)
    assert cur == lm.map.nkf - 1
    lm.recent.extend(int(p) for p in lm.map.slots[cur][lm.map.slots[cur] >= 0][:40])
    rep = lm.step(cur)
    assert log == list(LM.LocalMapper.STAGES) == rep["order"]
    assert rep["to_loop_closer"] == cur
    for name in LM.LocalMapper.STAGES:
        assert rep[name]["seconds"] >= 0.0 and "report" in rep[name]
    assert rep["process_new_keyframe"]["report"]["n_ordered"] >= 4
    assert rep["local_bundle_adjustment"]["report"]["nedges"] > 100
    assert rep["keyframe_culling"]["report"]["candidates"]
    assert lm.recent == rep["map_point_culling"]["report"]
    # mbAbortBA / stopRequested: no adjustment, no culling
    log2 = []
    lm2, cur2 = mapper(log2)
    rep2 = lm2.step(cur2, abort_ba=True)
    assert log2 == list(LM.LocalMapper.STAGES[:4]) == rep2["order"] and rep2["to_loop_closer"] == cur2
    assert "local_bundle_adjustment" not in rep2 and "keyframe_culling" not in rep2
