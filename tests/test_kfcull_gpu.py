"""KeyFrameCulling on the device: gf_keyframe_culling_counts / _dev bit for bit
against the serial restatement (tests/helpers/kfcull_ref.cpp) on the planted
scene of tests/kfcull_scenes.py, the slot-count edges, tombstones against a
rebuilt CSR, and localmapping.keyframe_culling end to end and chained after
create_new_map_points and search_in_neighbors."""
import numpy as np
import pytest
import torch

import kfcull_ref as R
import kfcull_scenes as S
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd._lib import check, lib, ptr
from gf_orb_slam_amd.loopmap import LoopMap
from gf_orb_slam_amd.orb import default_context

pytestmark = pytest.mark.gpu
SENTINEL = 0xEE


def counts_dev(tables, cand, want_flags=True):
    """gf_keyframe_culling_counts_dev on torch buffers -> (counts, flags plane
    pre-filled with SENTINEL)."""
    ctx = default_context()
    kf_off, octave, slots, mp_bad, obs_off, obs_gkp = tables
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
    d = [up(kf_off, np.int32), up(octave, np.uint8), up(slots, np.int32), up(mp_bad, np.uint8), up(obs_off, np.int32),
         up(obs_gkp, np.int32), up(cand, np.int32)]
    d_counts = torch.full((len(cand) * 2,), -7, dtype=torch.int32, device="cuda")
    d_flags = torch.full((len(slots),), SENTINEL, dtype=torch.uint8, device="cuda") if want_flags else None
    torch.cuda.current_stream().synchronize()
    check(lib().gf_keyframe_culling_counts_dev(ctx.handle, len(kf_off) - 1, len(slots), ptr(d[0]), ptr(d[1]), ptr(d[2]),
                                               len(mp_bad), ptr(d[3]), ptr(d[4]), ptr(d[5]), len(obs_gkp), len(cand),
                                               ptr(d[6]), ptr(d_counts), ptr(d_flags), ctx.stream))
    ctx.sync()
    return d_counts.cpu().numpy().reshape(-1, 2), (d_flags.cpu().numpy() if want_flags else None)


def counts_ref(tables, cand):
    flags = np.full(len(tables[2]), SENTINEL, np.uint8)
    return R.counts(*tables, cand, flags=flags), flags


def counts_host(tables, cand):
    flags = np.full(len(tables[2]), SENTINEL, np.uint8)
    return LM.keyframe_culling_counts(*tables, cand, flags=flags), flags


def test_counts_and_flags_equal_the_restatement():
    sc = S.scene()
    m = S.loop_map(sc)
    n = sc["names"]
    w = R.RefWorld.from_loopmap(m)
    *tables, planted = S.raw_tables(m, sc)
    kf_off, slots = tables[0], tables[2]
    cand = [k for k in m.ordered[sc["cur"]] if k != n["K0"]] + [n["S2"], n["S4"], n["c3"], n["M"]]  # M twice
    want, want_fl = counts_ref(tables, cand)
    got, got_fl = counts_dev(tables, cand)
    assert got.tobytes() == want.tobytes() and got_fl.tobytes() == want_fl.tobytes()
    assert np.array_equal(got[cand.index(n["M"])], got[-1])
    # untouched outside the candidates' ranges, written everywhere inside
    inside = np.zeros(len(slots), bool)
    for k in cand:
        inside[kf_off[k]:kf_off[k + 1]] = True
    assert (got_fl[~inside] == SENTINEL).all() and (got_fl[inside] <= 2).all() and (~inside).sum() > 100
    # the host entry: the same bytes (the out-of-map id is the device entry's case: NULL here)
    host_tables = list(tables)
    host_tables[2] = slots.copy()
    host_tables[2][planted["out"]] = -1
    hc, hf = counts_host(host_tables, cand)
    assert hc.tobytes() == got.tobytes() and hf.tobytes() == got_fl.tobytes()
    assert got_fl[planted["long"]] == 2 and got_fl[planted["out"]] == 0
    # and the restatement's world (std::map observation maps) at every candidate's first turn, where the tables
    # are the map's own: everything but the two planted slots
    plain = LM.culling_tables(m)[:6]
    pc, pf = counts_dev(plain, cand)
    for j, k in enumerate(cand):
        nmps, nred, fl = w.count(k)
        assert (int(pc[j, 0]), int(pc[j, 1])) == (nmps, nred), k
        assert np.array_equal(pf[kf_off[k]:kf_off[k + 1]], fl), k
    assert pc[cand.index(n["B"])].tolist() == [10, 10] and pc[cand.index(n["D9"])].tolist() == [10, 9]
    # no flags plane asked for
    assert counts_dev(tables, cand, want_flags=False)[0].tobytes() == want.tobytes()


def test_slot_count_edges_in_one_launch():
    sc = S.scene(edges=True)
    m = S.loop_map(sc)
    n = sc["names"]
    *tables, planted = S.raw_tables(m, sc)
    cand = [n[f"E{s}"] for s in S.EDGE_SIZES] + [n["M"], n["Q"]]
    sizes = [int(tables[0][k + 1] - tables[0][k]) for k in cand[:6]]
    assert sizes == list(S.EDGE_SIZES)
    want, want_fl = counts_ref(tables, cand)
    got, got_fl = counts_dev(tables, cand)
    assert got.tobytes() == want.tobytes() and got_fl.tobytes() == want_fl.tobytes()
    assert got[0].tolist() == [0, 0] and got[5, 0] > 2000 and got[5, 1] > 100 and got[3, 1] > 0
    assert got_fl[planted["long"]] == 2 and got_fl[planted["out"]] == 0
    host_tables = list(tables)
    host_tables[2] = tables[2].copy()
    host_tables[2][planted["out"]] = -1
    hc, hf = counts_host(host_tables, cand)
    assert hc.tobytes() == got.tobytes() and hf.tobytes() == got_fl.tobytes()


def test_tombstones_equal_a_rebuilt_csr():
    sc = S.scene(edges=True)
    m = S.loop_map(sc)
    n = sc["names"]
    kf_off, octave, slots, mp_bad, obs_off, obs_gkp = LM.culling_tables(m)[:6]
    rng = np.random.default_rng(5)
    a0, a1 = kf_off[n["A"]], kf_off[n["A"] + 1]
    gone = ((obs_gkp >= a0) & (obs_gkp < a1)) | (rng.random(len(obs_gkp)) < 0.15)  # all of A's, and a sixth at random
    assert gone.sum() > 100
    point = np.repeat(np.arange(len(mp_bad)), np.diff(obs_off))
    off2 = np.zeros_like(obs_off)
    off2[1:] = np.cumsum(np.bincount(point[~gone], minlength=len(mp_bad)))
    rebuilt = (kf_off, octave, slots, mp_bad, off2, obs_gkp[~gone])
    marked = (kf_off, octave, slots, mp_bad, obs_off, np.where(gone, -1, obs_gkp).astype(np.int32))
    cand = [k for k in range(m.nkf) if k != n["A"]]
    a, af = counts_dev(rebuilt, cand)
    b, bf = counts_dev(marked, cand)
    assert a.tobytes() == b.tobytes() and af.tobytes() == bf.tobytes()
    want, want_fl = counts_ref(marked, cand)
    assert b.tobytes() == want.tobytes() and bf.tobytes() == want_fl.tobytes()
    before = counts_dev((kf_off, octave, slots, mp_bad, obs_off, obs_gkp), cand)[0]
    assert (before[:, 1] > b[:, 1]).sum() >= 5 and (before[:, 0] == b[:, 0]).all()  # the erasures cost redundancy only


def _database(nkf):
    from gf_orb_slam_amd.loopdetect import KeyFrameDatabase

    db = KeyFrameDatabase()
    rng = np.random.default_rng(9)
    for k in range(nkf):
        words = np.sort(rng.choice(500, 12, replace=False)).astype(np.int32)
        v = rng.random(12)
        assert db.insert(words, v / v.sum()) == k
        db.add(k)
    return db


def _assert_report(rep, r):
    per = rep["per_candidate"]
    assert rep["candidates"] == r["candidates"] == [q["kf"] for q in per]
    assert [q["nmps"] for q in per] == r["nmps"] and [q["nredundant"] for q in per] == r["nredundant"]
    assert [q["culled"] for q in per] == r["culled_at"] and [q["deferred"] for q in per] == r["deferred_at"]
    assert rep["culled"] == r["culled"] and rep["points_bad"] == r["points_bad"]
    assert rep["reparented"] == r["reparented"]


def test_keyframe_culling_end_to_end():
    sc = S.scene()
    m = S.loop_map(sc)
    n, cur = sc["names"], sc["cur"]
    w = R.RefWorld.from_loopmap(m)
    db = _database(m.nkf)
    assert db.nlisted == m.nkf
    rep = LM.keyframe_culling(m, cur, db=db)
    r = w.keyframe_culling(cur)
    _assert_report(rep, r)
    R.assert_same_state(m, w)
    assert rep["culled"] == [n[x] for x in ("D10", "D11", "A", "C", "T")] and rep["launches"] == 6
    assert db.nlisted == m.nkf - 5
    assert not m.kf_bad[n["B"]] and m.to_be_erased[n["N"]] and m.to_be_erased[n["L"]]
    # the deferred ones when their protection ends
    assert m.set_erase(n["N"], db)["erased"] and not m.set_erase(n["L"], db)["erased"]
    assert (w.set_erase(n["N"]), w.set_erase(n["L"])) == (1, 2)
    R.assert_same_state(m, w)
    assert db.nlisted == m.nkf - 6
    # nothing to cull: one launch is all the device work
    sc0 = S.scene(cull=False)
    m0 = S.loop_map(sc0)
    w0 = R.RefWorld.from_loopmap(m0)
    rep0 = LM.keyframe_culling(m0, sc0["cur"])
    _assert_report(rep0, w0.keyframe_culling(sc0["cur"]))
    assert rep0["launches"] == 1 and rep0["culled"] == [] and not m0.kf_bad.any()
    R.assert_same_state(m0, w0)


def test_chained_after_create_new_map_points_and_search_in_neighbors():
    """CreateNewMapPoints -> SearchInNeighbors -> KeyFrameCulling on the
    localmap_scenes scene (the one with FeatureVectors), the first two followed
    by their own restatement as in test_neighbors_gpu.py, the culling by this
    one's from the world they left; then SearchInNeighbors -> KeyFrameCulling
    on neighbors_scenes.small()."""
    import localmap_scenes
    import neighbors_scenes as NS
    from neighbors_ref import RefWorld as NeighborsWorld

    sc = localmap_scenes.scene()
    cur = sc["cur"]
    m = LoopMap(sc["info"], sc["kps"], sc["desc"], sc["slots"], sc["mps"], sc["mp_desc"], observations=sc["obs"],
                kf_Tcw=sc["Tcw"], ref_kf=sc["ref_kf"])
    m.ordered[cur] = list(sc["neighbours"])
    ids, _ = LM.create_new_map_points(m, cur, sc["fv"])
    nw = NeighborsWorld.from_loopmap(m)
    for k in range(m.nkf):
        m.update_connections(k), nw.update_connections(k)
    LM.search_in_neighbors(m, cur)
    nw.search_in_neighbors(cur)
    assert all(np.array_equal(a, b) for a, b in zip(m.slots, nw.slots()))
    assert np.array_equal(m.observation_rows(), nw.observation_rows()) and np.array_equal(m.mp_bad, nw.points()[0])
    w = R.RefWorld.from_loopmap(m)
    rep = LM.keyframe_culling(m, cur)
    r = w.keyframe_culling(cur)
    _assert_report(rep, r)
    R.assert_same_state(m, w)
    assert len(rep["candidates"]) >= 2 and sum(r["nmps"]) > 100

    sc = NS.small()
    m = NS.loop_map(sc)
    LM.search_in_neighbors(m, sc["cur"])
    w = R.RefWorld.from_loopmap(m)
    rep = LM.keyframe_culling(m, sc["cur"])
    r = w.keyframe_culling(sc["cur"])
    _assert_report(rep, r)
    R.assert_same_state(m, w)
    assert 0 < len(rep["culled"]) < len(rep["candidates"]) and rep["launches"] >= 2
