"""LocalBundleAdjustment on a LoopMap on the device: gf_lba_graph / _dev byte for
byte against the serial restatement (tests/helpers/lbamap_ref.cpp) on the
structural cases of tests/lbamap_scenes.py, tombstones against a rebuilt map,
the refusals, and localmapping.local_bundle_adjustment end to end against the
oracle solving the restatement's graph, with a set stop flag, and chained
between search_in_neighbors and keyframe_culling."""
import ctypes

import numpy as np
import pytest

import lbamap_ref as R
import lbamap_scenes as S
import oracle_lib as O
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd._lib import GFError, lib, ptr
from gf_orb_slam_amd.loopmap import LoopMap
from gf_orb_slam_amd.orb import default_context
from test_lbamap_cpu import CASES, assert_same_graph, case_map

pytestmark = pytest.mark.gpu
RTOL = 1e-5  # the project's LBA tolerance (tests/test_lba_gpu.py)
SENTINEL = 0xEE


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b)))


def graph_dev(m, local):
    t = LM._LBATables(m, default_context())
    t.launch(local)
    return t.download()


def graph_host(m, local):
    return LM.lba_graph_arrays(LM.lba_tables(m), local)


def assert_counts(g, want):
    assert (g["nkf"], g["npts"], g["nedges"]) == (want["nkf"], want["npts"], want["nedges"])


@pytest.mark.parametrize("entry", [graph_dev, graph_host])
@pytest.mark.parametrize("case", CASES)
def test_graph_equals_the_restatement(case, entry):
    m, cur = case_map(case)
    want = R.RefWorld.from_loopmap(m).graph(cur, m.ordered[cur])
    g = entry(m, LM.lba_local_keyframes(m, cur))
    assert_counts(g, want)
    assert_same_graph(g, want)
    assert want["nedges"] > 100


def test_tombstones_equal_a_rebuilt_map():
    """-1 over observation entries of the tables against the map with those
    observations deleted and its tables built again."""
    m, cur = case_map("structural")
    local = LM.lba_local_keyframes(m, cur)
    t = LM.lba_tables(m)
    rng = np.random.default_rng(1)
    want0 = R.RefWorld.from_loopmap(m).graph(cur, m.ordered[cur])
    pairs = sorted(t["where"])
    gone = [pairs[j] for j in rng.choice(len(pairs), 150, replace=False)]
    obs_gkp = t["obs_gkp"].copy()
    for pk in gone:
        obs_gkp[t["where"][pk]] = -1
        del m.obs[pk[0]][pk[1]]
    want = R.RefWorld.from_loopmap(m).graph(cur, m.ordered[cur])
    assert want["nedges"] < want0["nedges"]
    edited = dict(t, obs_gkp=obs_gkp)
    g = LM.lba_graph_arrays(edited, local)
    assert_counts(g, want)
    assert_same_graph(g, want)
    assert_same_graph(graph_host(m, local), want)  # the rebuilt tables


def _call_host(t, local):
    """gf_lba_graph on sentinel-filled outputs -> (return code, outputs)."""
    host = {name: np.ascontiguousarray(t[name], dt).reshape(-1) for name, dt, _, _ in LM._LBA_TABLES}
    q = LM._lba_struct(t, host)
    bound = (q.nkf, q.nmp, q.nobs)
    bufs = {name: np.full(max(bound[which], 1) * per * np.dtype(dt).itemsize, SENTINEL, np.uint8)
            for name, dt, per, which in LM._LBA_OUT}
    counts = np.full(3, -7, np.int32)
    out = LM.LBAGraphOut(ptr(counts), *[ptr(bufs[name]) for name, *_ in LM._LBA_OUT])
    local = np.ascontiguousarray(local, np.int32)
    rc = lib().gf_lba_graph(default_context().handle, ctypes.byref(q), len(local), ptr(local), ctypes.byref(out))
    return rc, counts, bufs


def test_refusals_write_nothing():
    sc = S.structural()
    m = S.structural_map(sc, first_local=True)
    cur, n = sc["cur"], sc["names"]
    t = LM.lba_tables(m)
    local = LM.lba_local_keyframes(m, cur)
    assert len(local) == 33
    rc, counts, _ = _call_host(t, local)  # 32 of kind 0 and keyframe 0: accepted
    assert rc == 0 and counts[0] >= 33
    spare = next(k for k in sc["far"][6:] if k not in local)
    big = dict(t, kf_off=t["kf_off"].copy())
    big["kf_off"][n["E4096"] + 1:] += 1  # 4097 keypoints
    for name, per in (("octave", 1), ("slots", 1), ("kp_xy", 2)):
        big[name] = np.concatenate([t[name].reshape(-1, per), np.zeros((1, per), t[name].dtype)])
    bad_lists = dict(outside=local[:5] + [m.nkf], negative=local[:5] + [-1], repeat=local[:5] + [local[2]],
                     too_many=local + [spare], empty=[])
    calls = [(t, l) for l in bad_lists.values()] + [(big, local), (dict(t, kf0=m.nkf), local),
                                                    (dict(t, obs_gkp=np.where(t["obs_gkp"] == t["obs_gkp"][0],
                                                                              len(t["octave"]), t["obs_gkp"])), local)]
    for tt, l in calls:
        rc, counts, bufs = _call_host(tt, l)
        assert rc == -1 and lib().gf_last_error()
        assert np.all(counts == -7) and all(np.all(b == SENTINEL) for b in bufs.values())
    with pytest.raises(GFError) as e:  # inconsistent table lengths
        LM.lba_graph_arrays(dict(t, octave=t["octave"][:-1]), local)
    assert e.value.code == -1
    with pytest.raises(GFError) as e:  # the device entry checks the list too
        graph_dev(m, local + [spare])
    assert e.value.code == -1
    with pytest.raises(GFError) as e:
        LM.local_bundle_adjustment(_too_wide(m, cur, spare), cur)
    assert e.value.code == -1


def _too_wide(m, cur, spare):
    m.add_connection(cur, spare, 1)
    return m


def test_end_to_end_against_the_oracle():
    sc = S.parity()
    m = S.parity_map(sc)
    w = R.RefWorld.from_loopmap(m)
    want = w.graph(sc["cur"], m.ordered[sc["cur"]])
    To, Xo, fo, io = O.local_ba(want)
    rep = LM.local_bundle_adjustment(m, sc["cur"])
    assert_counts(rep["graph"], want)
    assert_same_graph(rep["graph"], want)
    assert rep["iterations"] == tuple(io) and np.array_equal(rep["flags"], fo)
    assert _close(rep["kf_Tcw"], To), np.abs(rep["kf_Tcw"] - To).max()
    assert _close(rep["pt_pos"], Xo), np.abs(rep["pt_pos"] - Xo).max()
    log = w.apply(rep["flags"], rep["kf_Tcw"], rep["pt_pos"])  # the device's own result
    for name in ("erased", "points_bad", "bad_round2", "stale_outliers"):
        assert rep[name] == log[name], name
    assert rep["stale_outliers"] == 0 and sorted(rep["points_bad"]) == sorted(sc["pts"]["turn_bad"])
    R.assert_same_state(m, w, skip_depth=rep["bad_round2"])
    assert rep["fixed_kfs"] and 0 in rep["fixed_kfs"] and set(rep["times"]) == {
        "tables", "assembly", "download", "solve", "writeback", "update"}


def test_solver_leaves_a_point_without_edges():
    """docs/ORACLE_ASSUMPTIONS.md A32: ``dead`` has no live observer; the solver
    accepts the vertex and returns its position bit for bit."""
    from gf_orb_slam_amd.optimizer import local_bundle_adjustment
    from test_lbamap_cpu import dead_point_problem

    g, q = dead_point_problem()
    _, X, _, its = local_bundle_adjustment(g)
    assert its[0] > 0 and np.asarray(X[q], np.float32).tobytes() == g["pt_pos"][q].tobytes()
    assert np.all(np.isfinite(X))


def test_set_stop_flag_matches_the_oracle_without_iterations():
    sc = S.parity()
    m = S.parity_map(sc)
    w = R.RefWorld.from_loopmap(m)
    want = w.graph(sc["cur"], m.ordered[sc["cur"]])
    To, Xo, fo, io = O.local_ba(want, its=(0, 0))
    rep = LM.local_bundle_adjustment(m, sc["cur"], stop_flag=ctypes.c_uint8(1))
    assert rep["iterations"] == (0, 0) == tuple(io) and np.array_equal(rep["flags"], fo)
    assert _close(rep["kf_Tcw"], To) and _close(rep["pt_pos"], Xo)
    w.apply(rep["flags"], rep["kf_Tcw"], rep["pt_pos"])
    R.assert_same_state(m, w, skip_depth=rep["bad_round2"])


def test_chained_between_search_in_neighbors_and_keyframe_culling():
    """CreateNewMapPoints -> SearchInNeighbors -> LocalBundleAdjustment ->
    KeyFrameCulling on the localmap_scenes scene, each step followed by its own
    restatement: the first two as in test_neighbors_gpu.py, the adjustment's
    graph against this restatement's and its write-back from the device's own
    result, the culling by kfcull_ref from the world the adjustment left."""
    import kfcull_ref
    import localmap_scenes
    from neighbors_ref import RefWorld as NeighborsWorld

    sc = localmap_scenes.scene()
    cur = sc["cur"]
    m = LoopMap(sc["info"], sc["kps"], sc["desc"], sc["slots"], sc["mps"], sc["mp_desc"], observations=sc["obs"],
                kf_Tcw=sc["Tcw"], ref_kf=sc["ref_kf"])
    m.ordered[cur] = list(sc["neighbours"])
    LM.create_new_map_points(m, cur, sc["fv"])
    nw = NeighborsWorld.from_loopmap(m)
    for k in range(m.nkf):
        m.update_connections(k), nw.update_connections(k)
    LM.search_in_neighbors(m, cur)
    nw.search_in_neighbors(cur)
    assert all(np.array_equal(a, b) for a, b in zip(m.slots, nw.slots()))
    assert np.array_equal(m.observation_rows(), nw.observation_rows())
    w = R.RefWorld.from_loopmap(m)
    want = w.graph(cur, m.ordered[cur])
    rep = LM.local_bundle_adjustment(m, cur)
    assert_counts(rep["graph"], want)
    assert_same_graph(rep["graph"], want)
    assert rep["nedges"] > 100 and rep["iterations"][0] >= 0
    log = w.apply(rep["flags"], rep["kf_Tcw"], rep["pt_pos"])
    for name in ("erased", "points_bad", "bad_round2", "stale_outliers"):
        assert rep[name] == log[name], name
    R.assert_same_state(m, w, skip_depth=rep["bad_round2"])
    kw = kfcull_ref.RefWorld.from_loopmap(m)
    cull = LM.keyframe_culling(m, cur)
    r = kw.keyframe_culling(cur)
    assert cull["candidates"] == r["candidates"] and cull["culled"] == r["culled"]
    assert [q["nmps"] for q in cull["per_candidate"]] == r["nmps"]
    assert [q["nredundant"] for q in cull["per_candidate"]] == r["nredundant"]
    kfcull_ref.assert_same_state(m, kw)
