"""Resident map tables on the device: gf_map_tables_apply / _dev and
gf_map_tables_move / _dev byte for byte against the serial restatement
(tests/helpers/maptables_ref.cpp) on the planted journals of
tests/maptables_scenes.py, the random walk with ``check()`` at every flush, and
every stage and LocalMapper.step with tables attached against the same without."""
import numpy as np
import pytest
import torch

import covis_ref
import covis_scenes
import kfcull_scenes
import maptables_ref as R
import maptables_scenes as S
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd import maptables as MT
from gf_orb_slam_amd._lib import GFError, check, lib, ptr
from gf_orb_slam_amd.orb import default_context
from test_covis_cpu import VOC
from test_maptables_cpu import apply_ref, live_rows

pytestmark = pytest.mark.gpu
SENTINEL = -7
OUT = ("slots", "mp_bad", "obs_gkp")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def apply_dev(t, j):
    """gf_map_tables_apply_dev on torch buffers -> (tables, status)."""
    ctx = default_context()
    d = {k: _up(v) for k, v in t.items()}
    q = {k: _up(np.ascontiguousarray(v, np.int32).reshape(-1)) for k, v in j.items()}
    d_status = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    check(lib().gf_map_tables_apply_dev(ctx.handle, len(t["kf_off"]) - 1, len(t["slots"]), ptr(d["kf_off"]),
                                        ptr(d["slots"]), len(t["mp_bad"]), ptr(d["mp_bad"]), ptr(d["obs_off"]),
                                        ptr(d["obs_gkp"]), len(t["obs_gkp"]), len(j["slot_g"]), ptr(q["slot_g"]),
                                        ptr(q["slot_v"]), len(j["bad_p"]), ptr(q["bad_p"]), len(j["row_ids"]),
                                        ptr(q["row_ids"]), ptr(q["row_op_off"]), len(j["ops"]), ptr(q["ops"]),
                                        ptr(d_status), ctx.stream))
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in d.items()}, d_status.cpu().numpy()


def apply_host(t, j):
    t = {k: v.copy() for k, v in t.items()}
    st = MT.tables_apply(t["kf_off"], t["slots"], t["mp_bad"], t["obs_off"], t["obs_gkp"], j["slot_g"], j["slot_v"],
                         j["bad_p"], j["row_ids"], j["row_op_off"], j["ops"])
    return t, st


def assert_apply(t, j, what):
    """Both entries against the restatement, every table byte for byte -> (tables, status)."""
    want, st = apply_ref(t, j)
    for name, fn in (("dev", apply_dev), ("host", apply_host)):
        got, gst = fn(t, j)
        assert gst.tolist() == st.tolist(), (what, name, gst, st)
        for k in t:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, name, k)
    return want, st


def move_dev(old_off, old_gkp, new_off):
    ctx = default_context()
    d = [_up(old_off), _up(old_gkp), _up(new_off)]
    d_new = torch.full((int(new_off[-1]) if len(new_off) else 0,), SENTINEL, dtype=torch.int32, device="cuda")
    d_status = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    check(lib().gf_map_tables_move_dev(ctx.handle, max(len(old_off) - 1, 0), ptr(d[0]), ptr(d[1]), len(old_gkp), ptr(d[2]),
                                       ptr(d_new), len(d_new), ptr(d_status), ctx.stream))
    ctx.sync()
    return d_new.cpu().numpy(), d_status.cpu().numpy()


def test_planted_journal_equals_the_restatement():
    t, j, names, expect = S.planted()
    out, st = assert_apply(t, j, "planted")
    assert st.tolist() == [1, 10]
    after, off = live_rows(out), t["obs_off"]
    for name, p in names.items():
        assert [g // S.KP for g in after[p]] == expect[name], name
        assert np.all(out["obs_gkp"][off[p] + len(after[p]):off[p + 1]] == -1), name
    touched = set(int(p) for p in j["row_ids"]) - {names["nofit"]}
    same = [p for p in range(len(after)) if p not in touched]
    assert len(same) > 15
    for p in same:
        assert out["obs_gkp"][off[p]:off[p + 1]].tobytes() == t["obs_gkp"][off[p]:off[p + 1]].tobytes(), p


def test_row_longer_than_the_buffer_is_left_alone():
    nkf = MT.MT_ROW + 10
    t = S._tables(nkf, [list(range(MT.MT_ROW)), list(range(MT.MT_ROW + 1)), [1, 2]], [MT.MT_ROW + 4, MT.MT_ROW + 4, 2])
    j = S._journal(3, {0: [(MT.OBS_SET, MT.MT_ROW + 5, 0), (MT.OBS_ERASE, 3, 0)], 1: [(MT.OBS_ERASE, 0, 0)],
                       2: [(MT.OBS_ERASE, 1, 0)]})
    out, st = assert_apply(t, j, "long rows")
    assert st.tolist() == [2, 0] and out["obs_gkp"][:t["obs_off"][2]].tobytes() == t["obs_gkp"][:t["obs_off"][2]].tobytes()
    # a row of exactly MT_ROW entries takes an overwrite and an erase
    j = S._journal(3, {0: [(MT.OBS_SET, 5, 7), (MT.OBS_ERASE, 0, 0), (MT.OBS_SET, MT.MT_ROW + 5, 1)]})
    out, st = assert_apply(t, j, "full buffer")
    assert st.tolist() == [0, 0] and len(live_rows(out)[0]) == MT.MT_ROW


@pytest.mark.parametrize("nrows", [0, 1, 65, 5000])
def test_touched_row_counts(nrows):
    t = S.wide_tables(6000)
    j = S.random_journal(t, nrows)
    assert len(j["row_ids"]) == nrows
    out, st = assert_apply(t, j, nrows)
    assert st[1] == 0 and (nrows < 65 or len(live_rows(out)) and out["obs_gkp"].tobytes() != t["obs_gkp"].tobytes())
    # nothing in the journal at all
    out, st = assert_apply(t, dict(S.EMPTY), "empty")
    assert st.tolist() == [0, 0] and all(out[k].tobytes() == t[k].tobytes() for k in t)


@pytest.mark.parametrize("nkf", [1, 2, 65, 1100])
def test_map_sizes(nkf):
    t = S.slack_tables(covis_scenes.thin_tables(nkf))
    j = S.random_journal(t, 60, seed=nkf)
    out, st = assert_apply(t, j, nkf)
    assert st.tolist() == [0, 0]  # three ops at most per row, three entries of slack
    for row in live_rows(out):
        assert row == sorted(row)


def test_host_entry_refusals():
    t, j, _, _ = S.planted()
    for change in (dict(row_ids=j["row_ids"][::-1].copy()), dict(slot_g=np.r_[j["slot_g"], j["slot_g"][1]].astype(np.int32),
                                                                 slot_v=np.r_[j["slot_v"], 0].astype(np.int32)),
                   dict(row_op_off=j["row_op_off"][:-1].copy())):
        before = {k: v.copy() for k, v in t.items()}
        with pytest.raises(GFError):
            apply_host(t, dict(j, **change))
        assert all(before[k].tobytes() == t[k].tobytes() for k in t)
    off = t["obs_off"].copy()
    off[3] = off[2] - 1
    with pytest.raises(GFError):
        MT.tables_move(off, t["obs_gkp"], t["obs_off"], np.zeros(len(t["obs_gkp"]), np.int32))


def test_move_equals_the_restatement():
    old_off, old_gkp, new_off, live, short = S.move_case()
    want = np.full(new_off[-1], SENTINEL, np.int32)
    st = R.move(old_off, old_gkp, new_off, want)
    got, gst = move_dev(old_off, old_gkp, new_off)
    host = np.full(new_off[-1], SENTINEL, np.int32)
    hst = MT.tables_move(old_off, old_gkp, new_off, host)
    assert gst.tolist() == hst.tolist() == st.tolist() == [1]
    assert got.tobytes() == host.tobytes() == want.tobytes() and not np.any(got == SENTINEL)
    p = short
    assert np.all(got[new_off[p]:new_off[p + 1]] == -1) and live[p] > new_off[p + 1] - new_off[p]
    # an empty table, and a table of empty rows
    z = np.zeros(1, np.int32)
    assert move_dev(z[:0], z[:0], z[:0])[1].tolist() == [0]
    assert move_dev(np.zeros(5, np.int32), z[:0], np.zeros(5, np.int32))[1].tolist() == [0]
    assert MT.tables_move(z, z[:0], z, np.zeros(0, np.int32)).tolist() == [0]
    # a whole slack table to tight capacities and back to roomy ones
    t = S.wide_tables(3000)
    cnt = np.asarray([len(r) for r in live_rows(t)])
    for cap in (cnt, cnt + 5):
        off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int32)
        want = np.full(off[-1], SENTINEL, np.int32)
        assert R.move(t["obs_off"], t["obs_gkp"], off, want).tolist() == [0]
        got, gst = move_dev(t["obs_off"], t["obs_gkp"], off)
        assert gst.tolist() == [0] and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("policy", [dict(), dict(min_cap=0, growth=0)], ids=["default", "tight"])
def test_random_walk_on_the_device(policy):
    m = S.thin_map(65, distinctive=S.keep_descriptors)
    assert m.nkf == 65
    t = m.attach_tables(**policy)
    t.check()
    n = []

    def flush():
        t.flush()
        t.check()
        n.append(t.pending)

    done = S.random_walk(m, 300, seed=6, flush=flush)
    assert len(done) == 9 and len(n) > 8 and not any(n) and t.rebuilds == 0 and t.launches >= len(n) // 2
    if policy:
        assert t.regrows > 8


def _pair(make, **policy):
    a, b = make(), make()
    b.attach_tables(**policy)
    return a, b


def _touch(maps):
    """An observation erased and put back through the map's methods: the map
    is as before, the attached one has a journal to flush and a row rewritten."""
    for m in maps:
        p = next(p for p, o in enumerate(m.obs) if len(o) >= 4 and not m.mp_bad[p])
        kf = min(m.obs[p])
        idx = m.obs[p][kf]
        assert not m.erase_observation(p, kf)
        m.add_observation(p, kf, idx)


def test_process_new_keyframe_attached_equals_unattached():
    from gf_orb_slam_amd.bow import ORBVocabulary

    voc = ORBVocabulary(VOC)
    a, kf, _ = covis_scenes.small_without_cur()
    b, _, _ = covis_scenes.small_without_cur()
    t = b.attach_tables()
    reps = []
    for m in (a, b):
        cur = m.add_keyframe(*kf)
        recent = [1, 2]
        reps.append((LM.process_new_keyframe(m, cur, voc, recent, levelsup=2), recent))
    S.assert_same_report(reps[0], reps[1])
    covis_ref.assert_same_maps(a, b)
    assert reps[0][0]["n_ordered"] >= 4 and len(reps[0][0]["associated"]) > 200 and t.flushes == 1
    t.check()


@pytest.mark.parametrize("cull", [False, True], ids=["none", "several"])
def test_keyframe_culling_attached_equals_unattached(cull):
    sc = kfcull_scenes.scene(cull=cull)
    a, b = _pair(lambda: kfcull_scenes.loop_map(sc))
    _touch((a, b))
    ra, rb = LM.keyframe_culling(a, sc["cur"]), LM.keyframe_culling(b, sc["cur"])
    S.assert_same_report(ra, rb)
    covis_ref.assert_same_maps(a, b)
    assert len(ra["culled"]) == (5 if cull else 0) and ra["launches"] == (6 if cull else 1)
    b.tables.check()


def test_update_connections_batch_attached_equals_unattached():
    sc = kfcull_scenes.scene(edges=True)
    a, b = _pair(lambda: kfcull_scenes.loop_map(sc), min_cap=0, growth=0)
    _touch((a, b))
    for m in (a, b):  # one more observer for a point: its row is full, the table regrows
        p = next(p for p, o in enumerate(m.obs) if len(o) >= 4 and not m.mp_bad[p])
        kf = next(k for k in range(m.nkf) if k not in m.obs[p] and len(m.kf_kps[k]))
        m.add_observation(p, kf, 0)
        m.add_map_point(kf, p, 0)
    order = [int(k) for k in np.random.default_rng(5).permutation(a.nkf)] * 2
    wa, oa = a.connections_counts(order)
    wb, ob = b.connections_counts(order)
    assert wa.tobytes() == wb.tobytes() and oa == ob and b.tables.regrows == 1
    a.update_connections_batch(order)
    b.update_connections_batch(order)
    covis_ref.assert_same_maps(a, b)
    assert len(a.weights[sc["names"]["E4096"]]) >= 10


def test_local_bundle_adjustment_attached_equals_unattached():
    import lbamap_scenes

    sc = lbamap_scenes.parity()
    a, b = _pair(lambda: lbamap_scenes.parity_map(sc))
    _touch((a, b))
    ra, rb = LM.local_bundle_adjustment(a, sc["cur"]), LM.local_bundle_adjustment(b, sc["cur"])
    # the assembled graph bit for bit (the row order is the map's), hence the same solve, poses and positions
    S.assert_same_report(ra, rb)
    covis_ref.assert_same_maps(a, b)
    assert ra["nedges"] > 100 and ra["iterations"][0] >= 0 and ra["points_bad"]
    assert b.tables.slack() > 1.2  # the assembly read padded rows
    assert b.tables.pending  # the write-back's erasures wait for the next stage
    b.tables.flush()
    b.tables.check()


def test_local_mapper_step_resident_equals_unattached():
    from gf_orb_slam_amd.bow import ORBVocabulary

    voc = ORBVocabulary(VOC)
    reps, maps, recents = [], [], []
    for resident in (False, True):
        m, kf, _ = covis_scenes.small_without_cur()
        for k in range(m.nkf):
            words, values, fv = voc.transform(m.kf_desc[k], 2)
            m.kf_bow[k], m.kf_fv[k] = (words, values), fv
        mapper = LM.LocalMapper(m, voc, levelsup=2, resident=resident)
        mapper.recent.extend(int(p) for p in kf[2][kf[2] >= 0][:30])
        cur = mapper.insert_keyframe(*kf)
        reps.append(mapper.step(cur))
        maps.append(m)
        recents.append(list(mapper.recent))
    S.assert_same_report(reps[0], reps[1])
    covis_ref.assert_same_maps(maps[0], maps[1])
    assert recents[0] == recents[1] and reps[0]["order"] == list(LM.LocalMapper.STAGES)
    assert reps[0]["local_bundle_adjustment"]["report"]["nedges"] > 100
    t = maps[1].tables
    assert maps[0].tables is None and t.flushes >= 3 and t.rebuilds == 0
    t.flush()
    t.check()
