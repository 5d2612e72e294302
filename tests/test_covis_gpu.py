"""UpdateConnections / ProcessNewKeyFrame on the device: gf_update_connections
and gf_update_connections_dev against the serial restatement
(tests/helpers/covis_ref.cpp) on the planted scene, the raw tables and every
size of tests/covis_scenes.py, LoopMap.update_connections_batch against the
serial host walk, process_new_keyframe through the device and the device
vocabulary against the CPU path, and LocalMapper.step end to end against the
stage functions called by hand."""
import numpy as np
import pytest

import covis_ref as R
import covis_scenes as S
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd._lib import GFError, check, lib, ptr
from gf_orb_slam_amd.orb import default_context
from test_covis_cpu import VOC, oracle_transform, tables_of
from test_loopfuse_cpu import cpu_distinctive

pytestmark = pytest.mark.gpu
SENTINEL = -77


def counts_host(kf_off, slots, mp_bad, obs_off, obs_gkp, query):
    return LM.update_connections_counts(kf_off, slots, mp_bad, obs_off, obs_gkp, query)


def counts_dev(kf_off, slots, mp_bad, obs_off, obs_gkp, query):
    """gf_update_connections_dev on sentinel-filled outputs: every entry must be written."""
    import torch

    ctx = default_context()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(dev)  # noqa: E731
    d = [t(kf_off, np.int32), t(slots, np.int32), t(mp_bad, np.uint8), t(obs_off, np.int32), t(obs_gkp, np.int32),
         t(query, np.int32)]
    nkf, nq = len(kf_off) - 1, len(query)
    out = [torch.full((max(nq * nkf, 1),), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]
    n = torch.full((max(nq, 1),), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.current_stream().synchronize()
    check(lib().gf_update_connections_dev(ctx.handle, nkf, len(slots), ptr(d[0]), ptr(d[1]), len(mp_bad), ptr(d[2]),
                                          ptr(d[3]), ptr(d[4]), len(obs_gkp), nq, ptr(d[5]), ptr(out[0]), ptr(n),
                                          ptr(out[1]), ptr(out[2]), ctx.stream))
    ctx.sync()
    w, ok, ow = (o.cpu().numpy()[:nq * nkf].reshape(nq, nkf) for o in out)
    return w, n.cpu().numpy()[:nq], ok, ow


def assert_equal_counts(got, want, what):
    for name, a, b in zip(("weights", "n_ordered", "ordered_kf", "ordered_w"), got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (what, name)


def check_tables(entry, tables, queries, what):
    """All queries in one launch, then one by one, against the restatement."""
    queries = np.asarray(queries, np.int32)
    want = R.counts(*tables, queries)
    assert_equal_counts(entry(*tables, queries), want, what)
    for i, q in enumerate(queries):
        one = entry(*tables, [q])
        assert_equal_counts(one, [a[i:i + 1] for a in want], (what, int(q)))


@pytest.mark.parametrize("entry", [counts_dev, counts_host])
def test_planted_scene_and_raw_tables_equal_the_restatement(entry):
    sc = S.scene(edges=True)
    m = S.loop_map(sc)
    n = sc["names"]
    assert [len(m.slots[n[f"E{s}"]]) for s in S.EDGE_SIZES] == list(S.EDGE_SIZES)
    queries = list(range(m.nkf)) + [-1, m.nkf, n["TH"]]  # outside [0, nkf) and a repeat
    check_tables(entry, tables_of(m), queries, "planted")
    *raw, info = S.raw_tables(m, sc)
    check_tables(entry, raw, queries, "raw")
    got = entry(*raw, [n["AQ"], n["RAWQ"]])
    assert {int(k): int(got[0][0, k]) for k in np.nonzero(got[0][0])[0]} == info["aq"]
    assert {int(k): int(got[0][1, k]) for k in np.nonzero(got[0][1])[0]} == info["rawq"]
    want = sc["expect"]["ORD"]
    one = entry(*tables_of(m), [n["ORD"]])
    assert one[2][0, :one[1][0]].tolist() == want[1] and one[3][0, :one[1][0]].tolist() == want[2]


@pytest.mark.parametrize("entry", [counts_dev, counts_host])
@pytest.mark.parametrize("nkf", [1, 2, 65, 1100])
def test_thin_tables_equal_the_restatement(nkf, entry):
    *t, query, listed = S.thin_tables(nkf)
    check_tables(entry, t, list(query) + [nkf - 1, nkf], f"thin{nkf}")
    n = entry(*t, query)[1]
    assert [int(x) for x in n] == [c if c else min(1, nkf - 1) for c in listed]


def test_host_entry_limits():
    kf_off = np.array([0, 4097], np.int32)
    slots = np.full(4097, -1, np.int32)
    none = np.zeros(0, np.int32)
    with pytest.raises(GFError) as e:
        counts_host(kf_off, slots, np.zeros(0, np.uint8), np.zeros(1, np.int32), none, [0])
    assert e.value.code == -3
    kf_off[1] = 4096  # the limit itself is accepted, by the device entry too
    for entry in (counts_host, counts_dev):
        w, n, ok, ow = entry(kf_off, slots[:4096], np.zeros(0, np.uint8), np.zeros(1, np.int32), none, [0])
        assert w.tolist() == [[0]] and n.tolist() == [0] and ok.tolist() == [[-1]] and ow.tolist() == [[0]]
    with pytest.raises(GFError) as e:  # kf_off must not decrease
        counts_host(np.array([0, 3, 2], np.int32), slots[:2], np.zeros(0, np.uint8), np.zeros(1, np.int32), none, [0])
    assert e.value.code == -1


def test_batch_on_the_device_equals_the_serial_walk():
    import kfcull_scenes as KS

    sc = KS.scene(edges=True)
    a, b = KS.loop_map(sc), KS.loop_map(sc)
    order = [int(k) for k in np.random.default_rng(5).permutation(a.nkf)] * 2
    for k in order:
        a.update_connections(k)
    b.update_connections_batch(order)
    R.assert_same_maps(a, b)
    # not an empty comparison: the 4096 random points of E4096 have observers, M lists its supports
    n = sc["names"]
    assert a.ordered[n["E4096"]] and len(a.weights[n["E4096"]]) >= 10 and n["S1"] in a.weights[n["M"]]


def test_process_new_keyframe_on_the_device_equals_the_cpu_path():
    from gf_orb_slam_amd.bow import ORBVocabulary

    dev, kf, _ = S.small_without_cur()
    cpu, _, _ = S.small_without_cur(distinctive=cpu_distinctive)
    cur = dev.add_keyframe(*kf)
    assert cpu.add_keyframe(*kf) == cur
    voc = ORBVocabulary(VOC)
    rd, rc = [1, 2], [1, 2]
    a = LM.process_new_keyframe(dev, cur, voc, rd, levelsup=2)
    b = LM.process_new_keyframe(cpu, cur, oracle_transform, rc, levelsup=2, counter=R.counts)
    for name in ("associated", "recent_added", "n_ordered", "parent"):
        assert a[name] == b[name], name
    assert rd == rc and a["n_ordered"] >= 4 and len(a["associated"]) > 200
    R.assert_same_maps(dev, cpu)
    for x, y in zip(dev.kf_bow[cur], cpu.kf_bow[cur]):
        assert np.array_equal(x, y)
    for name in ("nodes", "start", "feats"):
        assert np.array_equal(getattr(dev.kf_fv[cur], name), getattr(cpu.kf_fv[cur], name)), name


def test_local_mapper_step_equals_the_stages_by_hand():
    from gf_orb_slam_amd.bow import ORBVocabulary

    voc = ORBVocabulary(VOC)
    a, kf, _ = S.small_without_cur()
    b, _, _ = S.small_without_cur()
    for m in (a, b):
        for k in range(m.nkf):
            words, values, fv = voc.transform(m.kf_desc[k], 2)
            m.kf_bow[k], m.kf_fv[k] = (words, values), fv
    seed = [int(p) for p in kf[2][kf[2] >= 0][:30]]  # points tracking added lately
    mapper = LM.LocalMapper(a, voc, levelsup=2)
    mapper.recent.extend(seed)
    cur = mapper.insert_keyframe(*kf)
    rep = mapper.step(cur)
    assert rep["order"] == list(LM.LocalMapper.STAGES) and rep["to_loop_closer"] == cur
    # the same stages by hand on the second copy
    assert b.add_keyframe(*kf) == cur
    recent = list(seed)
    LM.process_new_keyframe(b, cur, voc, recent, 2)
    recent = LM.map_point_culling(b, recent, cur)
    ids, made = LM.create_new_map_points(b, cur, b.kf_fv)
    recent += ids
    LM.search_in_neighbors(b, cur)
    ba = LM.local_bundle_adjustment(b, cur)
    cull = LM.keyframe_culling(b, cur)
    R.assert_same_maps(a, b)
    assert mapper.recent == recent
    assert rep["create_new_map_points"]["report"][0] == ids
    assert rep["local_bundle_adjustment"]["report"]["iterations"] == ba["iterations"] and ba["nedges"] > 100
    assert rep["keyframe_culling"]["report"]["culled"] == cull["culled"]
    assert rep["process_new_keyframe"]["report"]["n_ordered"] >= 4
    # the stages left their mark: observations of the new keyframe, its connections, a solved window
    assert sum(cur in o for o in a.obs) > 200 and a.ordered[cur] and a.parent[cur] >= 0
    assert ba["iterations"][0] >= 0
