"""Resident map tables without a GPU: the planted journal of
tests/maptables_scenes.py in the serial restatement
(tests/helpers/maptables_ref.cpp), random walks over the LoopMap mutators with
the restatement injected as ``applier`` and ``check()`` after every flush, the
stages on host-resident tables against the stages on rebuilt tables, and
LocalMapper.step with ``resident=True`` against the unattached step."""
import numpy as np
import pytest

import covis_ref
import covis_scenes
import kfcull_scenes
import maptables_ref as R
import maptables_scenes as S
import neighbors_scenes
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd import maptables as MT
from gf_orb_slam_amd._lib import GFError


def fresh_map(which):
    kw = dict(distinctive=S.keep_descriptors)
    if which == "covis":
        return covis_scenes.loop_map(covis_scenes.scene(), **kw)
    if which == "kfcull":
        return kfcull_scenes.loop_map(kfcull_scenes.scene(), **kw)
    return neighbors_scenes.loop_map(neighbors_scenes.small(), **kw)


def live_rows(t):
    """The observation rows of flat tables with the -1 entries dropped."""
    off, g = t["obs_off"], t["obs_gkp"]
    return [g[off[p]:off[p + 1]][g[off[p]:off[p + 1]] >= 0].tolist() for p in range(len(off) - 1)]


def apply_ref(t, j):
    t = {k: v.copy() for k, v in t.items()}
    st = R.apply(t["kf_off"], t["slots"], t["mp_bad"], t["obs_off"], t["obs_gkp"], j["slot_g"], j["slot_v"], j["bad_p"],
                 j["row_ids"], j["row_op_off"], j["ops"])
    return t, st


def test_planted_journal_in_the_restatement():
    t, j, names, expect = S.planted()
    out, st = apply_ref(t, j)
    assert st.tolist() == [1, 10]
    before, after = live_rows(t), live_rows(out)
    off = t["obs_off"]
    for name, p in names.items():
        assert [g // S.KP for g in after[p]] == expect[name], name
        cap = off[p + 1] - off[p]
        row = out["obs_gkp"][off[p]:off[p + 1]]
        assert np.all(row[len(after[p]):] == -1) and len(after[p]) <= cap, name  # live first, then -1
    # the overwrite changed the value, not the place; the row that does not fit kept its bytes
    p = names["len64"]
    assert [a != b for a, b in zip(after[p], before[p])].count(True) == 1 and after[p] == sorted(after[p])
    p = names["nofit"]
    assert out["obs_gkp"][off[p]:off[p + 1]].tobytes() == t["obs_gkp"][off[p]:off[p + 1]].tobytes()
    assert len(after[names["len63"]]) == 64 == off[names["len63"] + 1] - off[names["len63"]]
    # every entry is its keyframe's: kp * k + idx with idx < kp, ascending
    for p, row in enumerate(after):
        assert row == sorted(row) and len({g // S.KP for g in row}) == len(row), p
    touched = set(int(p) for p in j["row_ids"])
    for p in range(len(before)):
        if p not in touched:
            assert out["obs_gkp"][off[p]:off[p + 1]].tobytes() == t["obs_gkp"][off[p]:off[p + 1]].tobytes(), p
    # slots and flags: the in-range targets written, nothing else
    g, v = j["slot_g"], j["slot_v"]
    ok = (g >= 0) & (g < len(t["slots"]))
    want = t["slots"].copy()
    want[g[ok]] = v[ok]
    assert np.array_equal(out["slots"], want) and ok.sum() == len(g) - 2
    bad = np.zeros(len(t["mp_bad"]), np.uint8)
    bad[[names["len300"], names["nofit"], 1]] = 1
    assert np.array_equal(out["mp_bad"], bad)


def test_row_longer_than_the_kernel_buffer_is_left_alone():
    nkf = MT.MT_ROW + 10
    t = S._tables(nkf, [list(range(MT.MT_ROW)), list(range(MT.MT_ROW + 1)), [1, 2]], [MT.MT_ROW + 4, MT.MT_ROW + 4, 2])
    j = S._journal(3, {0: [(MT.OBS_SET, MT.MT_ROW + 5, 0), (MT.OBS_ERASE, 3, 0)], 1: [(MT.OBS_ERASE, 0, 0)],
                       2: [(MT.OBS_ERASE, 1, 0)]})
    out, st = apply_ref(t, j)
    assert st.tolist() == [2, 0]  # 1024 + 1 on the way; 1025 to begin with
    off = t["obs_off"]
    assert out["obs_gkp"][:off[2]].tobytes() == t["obs_gkp"][:off[2]].tobytes()
    assert out["obs_gkp"][off[2]:].tolist() == [S.KP * 2 + (2 + 2) % S.KP, -1]


def test_move_in_the_restatement():
    old_off, old_gkp, new_off, live, short = S.move_case()
    new = np.full(new_off[-1], -7, np.int32)
    st = R.move(old_off, old_gkp, new_off, new)
    assert st.tolist() == [1] and not np.any(new == -7)
    for p in range(len(live)):
        row = new[new_off[p]:new_off[p + 1]]
        old = old_gkp[old_off[p]:old_off[p + 1]]
        want = [] if p == short else old[old >= 0].tolist()
        assert row[:len(want)].tolist() == want and np.all(row[len(want):] == -1), p
    # an empty table
    z = np.zeros(1, np.int32)
    assert R.move(z, z[:0], z, np.zeros(0, np.int32)).tolist() == [0]
    assert R.move(z[:0], z[:0], z[:0], np.zeros(0, np.int32)).tolist() == [0]


@pytest.mark.parametrize("which", ["covis", "kfcull", "neighbors"])
@pytest.mark.parametrize("policy", [dict(), dict(min_cap=0, growth=0)], ids=["default", "tight"])
def test_random_walk_keeps_the_invariant(which, policy):
    m = fresh_map(which)
    t = m.attach_tables(applier=R.APPLIER, **policy)
    t.check()
    flushes = []

    def flush():
        t.flush()
        t.check()
        flushes.append(t.pending)

    done = S.random_walk(m, 400, seed=len(which), flush=flush)
    assert set(done) == {"add_observation", "add_map_point", "erase_map_point_match", "erase_observation",
                         "set_bad_point", "replace", "set_bad_keyframe", "new_map_point", "add_keyframe"}
    assert len(flushes) > 10 and not any(flushes) and t.rebuilds == 0
    if policy:
        assert t.regrows > 10  # every insertion into a full row goes through the move
        assert t.slack() < 1.5
    # the resident host arrays, -1 dropped, are culling_tables(map)
    kf_off, octave, slots, mp_bad, obs_off, obs_gkp, _ = LM.culling_tables(m)
    a = t.download()
    assert np.array_equal(a["kf_off"], kf_off) and np.array_equal(a["octave"], octave)
    assert np.array_equal(a["slots"], slots) and np.array_equal(a["mp_bad"], mp_bad)
    assert np.array_equal(a["obs_gkp"][a["obs_gkp"] >= 0], obs_gkp) and len(a["obs_gkp"]) >= len(obs_gkp)


def test_check_names_the_row_that_differs():
    m = fresh_map("covis")
    t = m.attach_tables(applier=R.APPLIER)
    p = next(p for p, o in enumerate(m.obs) if len(o) >= 2)
    m.obs[p].pop(min(m.obs[p]))  # behind the journal's back
    with pytest.raises(GFError, match=f"row {p} "):
        t.check()
    m.add_observation(0, 0, 0)
    with pytest.raises(GFError, match="flushed"):
        t.check()


def test_stages_on_resident_tables_equal_the_rebuilt_ones():
    """connections_counts / update_connections_batch and keyframe_culling with
    the restatements' counters: the same numbers from the padded resident
    tables as from culling_tables, also after a walk has left -1 padding and
    regrown rows."""
    import kfcull_ref

    for policy in (dict(), dict(min_cap=0, growth=0)):
        a, b = fresh_map("kfcull"), fresh_map("kfcull")
        t = b.attach_tables(applier=R.APPLIER, **policy)
        for m in (a, b):
            S.random_walk(m, 150, seed=1)  # a walk after which the current keyframe still has candidates
        covis_ref.assert_same_maps(a, b)
        assert t.pending > 100
        kfs = list(range(a.nkf))
        wa, oa = a.connections_counts(kfs, counter=covis_ref.counts)
        wb, ob = b.connections_counts(kfs, counter=covis_ref.counts)
        assert np.array_equal(wa, wb) and oa == ob and t.pending == 0
        t.check()
        cur = kfcull_scenes.scene()["cur"]
        ra = LM.keyframe_culling(a, cur, counter=kfcull_ref.counts)
        rb = LM.keyframe_culling(b, cur, counter=kfcull_ref.counts)
        ra.pop("times"), rb.pop("times")
        assert ra == rb and len(ra["candidates"]) >= 10 and ra["culled"]
        covis_ref.assert_same_maps(a, b)
        t.check()
    # the planted cull: several keyframes go, every refresh is a flush
    a, b = fresh_map("kfcull"), fresh_map("kfcull")
    t = b.attach_tables(applier=R.APPLIER)
    ra = LM.keyframe_culling(a, cur, counter=kfcull_ref.counts)
    rb = LM.keyframe_culling(b, cur, counter=kfcull_ref.counts)
    ra.pop("times"), rb.pop("times")
    assert ra == rb and len(ra["culled"]) >= 5 and t.flushes == len(ra["culled"])
    covis_ref.assert_same_maps(a, b)
    t.check()
    # device stages refuse tables that live on the host
    with pytest.raises(GFError):
        LM._resident(t, False)


def test_local_mapper_step_resident_equals_unattached(monkeypatch):
    import kfcull_ref
    import lbamap_ref
    from test_covis_cpu import oracle_transform
    from test_lbamap_cpu import oracle_solver
    from test_loopfuse_cpu import cpu_distinctive

    seen, checking = [], []

    def mapper(resident):
        m, kf, _ = covis_scenes.small_without_cur(distinctive=cpu_distinctive)

        def create(map, cur, kf_fv, ctx=None):
            # the bookkeeping of CreateNewMapPoints (:393-406) for three made-up points
            ids = []
            for j, k2 in enumerate(map.ordered[cur][:3]):
                i1 = int(np.nonzero(map.slots[cur] < 0)[0][0])
                i2 = int(np.nonzero(map.slots[k2] < 0)[0][0])
                p = map.new_map_point(map.mps["pos"][j], cur)
                map.add_observation(p, k2, i2), map.add_observation(p, cur, i1)
                map.add_map_point(cur, p, i1), map.add_map_point(k2, p, i2)
                ids.append(p)
            return ids, dict(points=ids)

        def search(map, cur, ctx=None):
            # a fusion each way: a point of the first neighbour replaced by one of cur's, a point of cur's added
            k = map.ordered[cur][0]
            mine = [int(p) for p in map.slots[cur] if p >= 0 and not map.mp_bad[p] and not map.is_in_keyframe(p, k)]
            theirs = [int(p) for p in map.slots[k] if p >= 0 and not map.mp_bad[p] and not map.is_in_keyframe(p, cur)]
            map.replace(mine[0], theirs[0])
            free = int(np.nonzero(map.slots[k] < 0)[0][0])
            map.add_observation(mine[1], k, free), map.add_map_point(k, mine[1], free)
            map.update_connections(cur)
            return dict(targets=[k])

        def assembler(t, local):
            if resident:  # what the device assembly would read: the padded rows hold the map's, in order
                checking.append(1)  # the comparison's own rebuild is not the step's
                want = LM.lba_tables(m)
                checking.pop()
                g = np.asarray(t["obs_gkp"])
                assert np.array_equal(g[g >= 0], want["obs_gkp"]) and len(g) > len(want["obs_gkp"])
                for name in ("kf_off", "octave", "slots", "mp_bad", "kp_xy", "kf_bad", "kf_Tcw", "mp_pos"):
                    assert np.array_equal(np.asarray(t[name]), want[name]), name
                seen.append(len(g))
            return lbamap_ref.assembler(m)[0](t, local)

        lm = LM.LocalMapper(m, oracle_transform, levelsup=2, counter=covis_ref.counts, cull_counter=kfcull_ref.counts,
                            assembler=assembler, solver=oracle_solver,
                            stages=dict(create_new_map_points=create, search_in_neighbors=search), resident=resident,
                            applier=R.APPLIER)
        cur = lm.insert_keyframe(*kf)
        lm.recent.extend(int(p) for p in m.slots[cur][m.slots[cur] >= 0][:40])
        return lm, cur

    a, cur = mapper(False)
    b, cur_b = mapper(True)
    assert a.map.tables is None and isinstance(b.map.tables, MT.ResidentTables) and cur == cur_b
    calls = []
    real = LM.culling_tables
    monkeypatch.setattr(LM, "culling_tables", lambda m: (checking or calls.append(m)) and None or real(m))
    ra = a.step(cur)
    built = len(calls)
    assert built >= 3 and all(m is a.map for m in calls)  # one rebuild per stage without the tables
    rb = b.step(cur)
    assert len(calls) == built, "the resident step rebuilt the tables"
    monkeypatch.undo()
    assert ra["order"] == rb["order"] == list(LM.LocalMapper.STAGES)

    S.assert_same_report(ra, rb)
    covis_ref.assert_same_maps(a.map, b.map)
    assert a.recent == b.recent and seen and rb["local_bundle_adjustment"]["report"]["nedges"] > 100
    b.map.tables.check()
    assert b.map.tables.flushes >= 3 and b.map.tables.rebuilds == 0
