"""The relocalisation keyframe database that grows on the device
(csrc/kfdbgrow.hip: gf_kfdb_create_growable, gf_kfdb_append,
gf_frontend_update_maps_kfdb) against the serial restatement
(tests/helpers/kfdb_ref.cpp) and against a fixed database built from scratch
with all keyframes, bit for bit through gf_kfdb_read: the append tables over the
shapes at which the kernels can go wrong, the refusals, the pinned LOST /
relocalise run of kfdb_grow_scenes.py against the oracle chain (eager and
through a captured graph), and the closed loop tracker -> keyframe -> mapper ->
map + database -> tracker."""
import numpy as np
import pytest

import kfdb_grow_scenes as GS
import kfdb_ref as R
import mapupdate_ref as MR
import mapupdate_scenes as S
import oracle_chain as C
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.localmap import MapDelta
from gf_orb_slam_amd.orb import default_context
from gf_orb_slam_amd.pipeline import STATS, TR, FrontEnd

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. append tables
def _grow(kfs0, groups, max_kf, max_rows):
    """A growable database over ``kfs0``, then one append per group of
    keyframes; after every call the device equals the restatement, at the end
    also a fixed database built from scratch and the host arrays."""
    ctx = default_context()
    db = R.db_of(kfs0, max_kf=max_kf, max_rows=max_rows)
    ref = R.RefDB(R.db_of(kfs0), max_kf, max_rows)
    assert R.same(db.read(ctx), ref.packed()) == [], "after creation"
    for i, g in enumerate(groups):
        rows = R.db_of(g)
        assert ref.append(rows) == 0, i
        db.append(rows)
        assert R.same(db.read(ctx), ref.packed()) == [], f"after append {i}"
    everything = list(kfs0) + [k for g in groups for k in g]
    whole = R.db_of(everything)
    assert R.same(db.read(ctx), whole.read(ctx)) == [], "against the fixed database"
    assert R.same(db.read(ctx), R.build(whole)) == [], "against KeyFrameDatabase::add"
    assert all(getattr(db, k).tobytes() == getattr(whole, k).tobytes() for k in R.ROW_KEYS), "host arrays"
    return db, ref


def _kf(nkp, words, seed=0):
    return R.keyframe(np.random.default_rng(seed), nkp, words)


def test_words_present_absent_and_at_the_ends():
    """A database of one keyframe of 3 keypoints; new keyframes whose words are
    all listed, none listed, mixed, below the first and above the last listed
    word; a keyframe without keypoints; one word per keypoint."""
    _grow([_kf(3, [10, 20, 30])],
          [[_kf(3, [10, 20, 30], 1)], [_kf(4, [11, 12, 25], 2)], [_kf(5, [10, 15, 30, 31], 3)], [_kf(2, [1, 2], 4)],
           [_kf(2, [98, 99], 5)], [_kf(0, [], 6)], [_kf(6, [0, 10, 40, 50, 99, 100], 7)], [_kf(1, [20], 8)]], 16, 64)


def test_from_an_empty_database_and_several_keyframes_in_one_call():
    """Two and three keyframes in one call equal one at a time (the device
    against the restatement that adds them in index order)."""
    kfs = R.random_keyframes(5, 8, nkp=(0, 12), vocab=25)
    a, _ = _grow([], [kfs[:2], kfs[2:5], kfs[5:]], 8, 100)
    b, _ = _grow([], [[k] for k in kfs], 8, 100)
    ctx = default_context()
    assert R.same(a.read(ctx), b.read(ctx)) == []


def test_exactly_the_capacities_and_64_keyframes():
    kfs = R.random_keyframes(6, 64, nkp=(1, 6), vocab=40)
    rows = sum(len(k[0]) for k in kfs)
    db, ref = _grow(kfs[:61], [kfs[61:63], [kfs[63]]], 64, rows)  # 63 -> 64 keyframes, exactly max_kf and max_rows
    ctx = default_context()
    before = db.read(ctx)
    for rows_, code in ((R.db_of([_kf(0, [], 1)]), -3), (R.db_of([_kf(1, [3], 2)]), -3)):
        with pytest.raises(GFError) as e:
            db.append(rows_)
        assert e.value.code == code
        assert R.same(db.read(ctx), before) == [] and db.nkf == 64
    small, _ = _grow(kfs[:2], [], 3, len(kfs[0][0]) + len(kfs[1][0]) + 4)
    before = small.read(ctx)
    for rows_, code in ((R.db_of([_kf(1, [1], 1), _kf(1, [2], 2)]), -3), (R.db_of([_kf(5, [1], 3)]), -3)):
        with pytest.raises(GFError) as e:  # max_kf + 1, max_rows + 1
            small.append(rows_)
        assert e.value.code == code and R.same(small.read(ctx), before) == []
    small.append(R.db_of([_kf(4, [1, 2], 4)]))  # exactly max_kf and max_rows
    assert small.read(ctx)["nkf"] == 3


def test_wide_keyframes_wrap_every_scan_and_grid_loop():
    """Keyframes of more than 256 and more than 1024 words (the scan's rounds),
    into an inverted file of more than 1024 words, and one call of more than
    4096 keypoints (the merge grid's loops wrap)."""
    rng = np.random.default_rng(8)
    w = lambda n, hi: np.sort(rng.choice(hi, n, replace=False))  # noqa: E731
    first = [R.keyframe(rng, 1500, w(1500, 6000)), R.keyframe(rng, 300, w(300, 6000))]
    groups = [[R.keyframe(rng, 300, w(300, 9000))], [R.keyframe(rng, 1100, w(1100, 9000))],
              [R.keyframe(rng, 1100, w(1100, 20000)) for _ in range(5)], [R.keyframe(rng, 7, w(7, 50))]]
    _grow(first, groups, 16, 12000)


def test_refused_appends_leave_the_database_untouched():
    ctx = default_context()
    db, _ = _grow([_kf(3, [10, 20, 30]), _kf(2, [7, 8], 1)], [], 8, 64)
    before = db.read(ctx)
    bad_words = R.db_of([_kf(3, [5, 6, 7], 2)])
    bad_words.bow_words[:] = [5, 5, 7]
    bad_feat = R.db_of([_kf(3, [5, 6, 7], 2)])
    bad_feat.fv_feats[0] = 3
    bad_off = R.db_of([_kf(3, [5, 6, 7], 2)])
    bad_off.kp_off[:] += 1
    for name, rows in (("words not ascending", bad_words), ("feature index out of range", bad_feat),
                       ("offsets not from 0", bad_off)):
        with pytest.raises(GFError) as e:
            db.append(rows)
        assert e.value.code == -1, name
        assert R.same(db.read(ctx), before) == [] and db.nkf == 2, name
    fixed = R.db_of([_kf(3, [10, 20, 30])])
    fixed.device(ctx)
    with pytest.raises(GFError) as e:
        fixed.append(R.db_of([_kf(1, [1], 1)]))
    assert e.value.code == -1 and fixed.nkf == 1
    assert R.same(fixed.read(ctx), R.build(R.db_of([_kf(3, [10, 20, 30])]))) == []


# ---------------------------------------------------------------- 2. refusals of the map feedback
def _db_for(graph, seed):
    """Keyframes with as many keypoints as the graph's keyframes have slots."""
    rng = np.random.default_rng(seed)
    n = np.diff(graph["kf_mp_off"])
    return [R.keyframe(rng, int(k), np.sort(rng.choice(60, min(int(k), 5), replace=False))) for k in n]


def test_feedback_refusals_leave_every_stream_and_database_untouched():
    import test_mapupdate_gpu as MU

    M = 48
    maps = [S.random_map(30, 40, 6, odd_offsets=True), S.random_map(31, 40, 5, slots=(3, 9)),
            S.random_map(32, 40, 3, slots=(5, 9))]
    fe = MU._frontend(maps, M)
    kfs1, kfs2 = _db_for(maps[1]["graph"], 1), _db_for(maps[2]["graph"], 2)
    rows1 = sum(len(k[0]) for k in kfs1)
    db1 = R.db_of(kfs1, max_kf=6, max_rows=rows1 + 12)  # room for one keyframe of up to 12 keypoints
    db2 = R.db_of(kfs2)
    fe.set_kfdb(1, db1)
    fe.set_kfdb(2, db2)
    ref1 = R.RefDB(R.db_of(kfs1), 6, rows1 + 12)
    with pytest.raises(GFError) as e:  # a growable database belongs to one stream
        fe.set_kfdb(0, db1)
    assert e.value.code == -1
    states, st0 = MU._states(fe)
    m = [S.map_of_state(s) for s in states]
    good0 = S.diff(0, m[0], S.evolve(40, m[0], new_mp=2, rewrite=3, slot_writes=4))
    good2 = S.diff(2, m[2], S.evolve(41, m[2], new_mp=1, rewrite=2))
    new = _kf(7, [3, 9, 70], 5)
    slots = lambda n: np.arange(n, dtype=np.int32) - 1  # noqa: E731
    bad = {
        "keypoints differ from the slots": (MapDelta(1, new_kf=[slots(6)], kf_rows=[new]), -1),
        "rows without a database": (MapDelta(0, new_kf=[slots(7)], kf_rows=[new]), -1),
        "rows without an appended keyframe": (MapDelta(1, bad_mp=[1], kf_rows=[new]), -1),
        "two keyframes, rows of one": (MapDelta(1, new_kf=[slots(7), slots(7)], kf_rows=[new]), -1),
        "words not ascending": (MapDelta(1, new_kf=[slots(7)], kf_rows=[_kf(7, [9, 3, 70], 5)]), -1),
        "a keyframe without rows on a growable stream": (MapDelta(1, new_kf=[slots(7)]), -4),
        "rows on a fixed database": (MapDelta(2, new_kf=[slots(7)], kf_rows=[new]), -4),
        "max_kf + 1": (MapDelta(1, new_kf=[slots(1), slots(1)], kf_rows=[_kf(1, [1], 6), _kf(1, [2], 7)]), -3),
        "max_rows + 1": (MapDelta(1, new_kf=[slots(13)], kf_rows=[_kf(13, [1], 8)]), -3),
    }
    ctx = fe.ctx
    for name, (d, code) in bad.items():
        others = [g for g in (good0, good2) if g.stream != d.stream]
        for call in ([d] + others, others + [d]):
            with pytest.raises(GFError) as e:
                fe.update_maps(call)
            assert e.value.code == code, (name, str(e.value))
            MU._assert_device_equals(fe, states, st0, set(), name)
            assert R.same(db1.read(ctx), ref1.packed()) == [] and db1.nkf == 5, name
            assert R.same(db2.read(ctx), R.build(R.db_of(kfs2))) == [], name
    # the valid deltas pass, the one that grows the database among them (exactly max_rows)
    wide = _kf(12, [3, 9, 70], 9)
    good1 = MapDelta(1, new_kf=[slots(12)], kf_rows=[wide], new_mp=m[1]["mp"][:1], new_mp_desc=m[1]["desc"][:1])
    for st, d in ((states[0], good0), (states[1], good1), (states[2], good2)):
        assert st.apply(d) == 0
    assert ref1.append(R.db_of([wide])) == 0
    fe.update_maps([good2, good1, good0])
    MU._assert_device_equals(fe, states, st0, {0, 1, 2}, "after the refusals")
    assert R.same(db1.read(ctx), ref1.packed()) == [] and db1.nkf == 6
    assert R.same(db1.read(ctx), R.build(R.db_of(kfs1 + [wide]))) == []
    assert all(getattr(db1, k).tobytes() == getattr(R.db_of(kfs1 + [wide]), k).tobytes() for k in R.ROW_KEYS)
    assert not fe.read("reloc")[1].view(np.uint8).any()  # no query has touched a keyframe, the appended one included
    fe.close()


# ---------------------------------------------------------------- 3. / 4. the pinned run
_RUNS = {}


def _scene():
    if "scene" in _RUNS:
        return _RUNS["scene"]
    import torch

    import oracle_lib as O
    from gf_orb_slam_amd.bow import ORBVocabulary

    voc = GS.vocabulary()
    W = GS.workload()
    frames = W.render_all("cuda").contiguous()
    for s, i in GS.blank_frames(W):
        frames[s, i] = 100
    gmaps = W.build_global_maps(lambda im: O.extract(im), GS.G)
    dvoc = ORBVocabulary(voc)
    m0, m1, rows = GS.maps_of(W, gmaps, dvoc.transform)
    gm1 = gmaps[W.scene_of[1]]
    rows1 = [(k, d) + tuple(dvoc.transform(d)) for k, d in zip(gm1["kf_kps"], gm1["kf_desc"])]
    T, V = W.boot_state()
    torch.cuda.synchronize()
    sc = dict(W=W, frames=frames, fr=frames.cpu().numpy(), voc=voc, dvoc=dvoc, m0=m0, m1=m1, rows=rows, gm1=gm1,
              rows1=rows1, T=T, V=V)
    _RUNS["scene"] = sc
    return sc


def _run(captured):
    """Steps 1 .. K_BEFORE on K - 1 keyframes, the update that appends keyframe
    K - 1 with its database rows, the steps up to LAST_STEP."""
    sc = _scene()
    W, rows = sc["W"], sc["rows"]
    K = len(rows)
    fe = FrontEnd("euroc", 1000, 2, GS.G, GS.BUDGET)
    fe.set_vocab(sc["dvoc"])
    fe.set_map(0, sc["m0"]["mp"], sc["m0"]["desc"])
    fe.set_covis(0, sc["m0"]["graph"])
    db = GS.database(rows[:-1], max_kf=K + 2, max_rows=sum(len(r[0]) for r in rows) + 100)
    fe.set_kfdb(0, db)
    fe.set_map(1, sc["gm1"]["mp"], sc["gm1"]["desc"])
    fe.set_covis(1, sc["gm1"]["graph"])
    db1 = GS.database(sc["rows1"])
    fe.set_kfdb(1, db1)
    for b in range(2):
        fe.set_rng(b, 7 + b)
    fe.set_source(sc["frames"], W.scene_of, W.phase)
    fe.bootstrap(sc["T"], sc["V"], 0.0)
    out = dict(steps=[])
    for k in range(1, GS.K_BEFORE + 1):
        if captured and k == 2:  # the first step ran eagerly (it sizes the context's scratch)
            fe.capture_graph()
        fe.step()
        out["steps"].append(C.read_state(fe))
    delta = S.diff(0, sc["m0"], sc["m1"])
    assert len(delta.new_kf_off) == 2 and delta.has_cov and len(delta.obs_mp) > 0
    delta.kf_rows = GS.database([rows[-1]])  # the appended keyframe's database rows
    fe.update_maps(delta)
    out["updated"] = C.read_state(fe)
    out["graph"] = fe.covis(0)
    out["db"], out["db1"] = db.read(fe.ctx), db1.read(fe.ctx)
    out["host_db"] = db
    for k in range(GS.K_BEFORE + 1, GS.LAST_STEP + 1):
        fe.step()
        out["steps"].append(C.read_state(fe))
    out["db_end"] = db.read(fe.ctx)
    fe.close()
    return out


def test_the_stream_relocalises_against_the_appended_keyframe():
    import test_track_loss_gpu as TL

    sc = _scene()
    run = _RUNS["eager"] = _run(False)
    W, rows, m1 = sc["W"], sc["rows"], sc["m1"]
    K = len(rows)
    before, upd = run["steps"][GS.K_BEFORE - 1], run["updated"]
    assert int(before["track"][0][TR["state"]]) == 1, "stream 0 is not LOST when the keyframe arrives"
    # the update: nothing it does not own moves, stream 1 not at all
    for k in C.FIELDS:
        if k not in ("map", "map_desc", "nmp", "last_pos", "mp_upd", "views"):
            assert upd[k].tobytes() == before[k].tobytes(), k
        assert upd[k][1].tobytes() == before[k][1].tobytes(), k
    assert MR.same_graph(run["graph"], m1["graph"]) == []
    full = GS.database(rows)
    assert R.same(run["db"], R.build(full)) == [], "the database against KeyFrameDatabase::add"
    assert R.same(run["db"], full.read(default_context())) == [], "the database against a fixed one from scratch"
    assert R.same(run["db_end"], run["db"]) == [] and R.same(run["db1"], R.build(GS.database(sc["rows1"]))) == []
    assert all(getattr(run["host_db"], k).tobytes() == getattr(full, k).tobytes() for k in R.ROW_KEYS)
    # every later step equals the oracle chain on the full graph and the full database
    db_of = {0: full, 1: GS.database(sc["rows1"])}
    map_of = {0: m1, 1: dict(mp=sc["gm1"]["mp"], desc=sc["gm1"]["desc"], graph=sc["gm1"]["graph"])}
    prev = upd
    for k in range(GS.K_BEFORE + 1, GS.LAST_STEP + 1):
        after = run["steps"][k - 1]
        for b in range(2):
            ch = GS.chain(map_of[b], db_of[b], sc["voc"])
            ch.load_from(prev, b)
            ch.write("reloc", prev["reloc"][b])
            ch.step(sc["fr"][W.scene_of[b], (W.phase[b] + k) % W.period])
            TL._compare(after, ch, b, f"step {k}: ")
            if b == 0 and k == GS.RELOC_STEP:
                cands, state, q = GS.candidates(ch, prev["reloc"][0], full, m1["graph"], sc["voc"])
                st = {n: int(after["stats"][i, 0]) for i, n in enumerate(STATS)}
                print(f"step {k}: candidates {cands.tolist()}, flags {st['flags']:#x}, ncand {st['ncand']}")
                assert K - 1 in cands.tolist() and st["ncand"] == len(cands)
                assert int(after["reloc"][0][K - 1]["query"]) == q and after["reloc"][0].tobytes() == state.tobytes()
                assert st["flags"] & 32768 and int(after["track"][0][TR["state"]]) == 0, "stream 0 did not relocalise"
        prev = after


def test_the_same_run_through_a_captured_graph():
    eager = _RUNS.get("eager") or _run(False)
    cap = _run(True)
    assert MR.same_graph(cap["graph"], eager["graph"]) == []
    assert R.same(cap["db"], eager["db"]) == [] and R.same(cap["db_end"], eager["db_end"]) == []
    pairs = list(zip(cap["steps"], eager["steps"])) + [(cap["updated"], eager["updated"])]
    for i, (a, b) in enumerate(pairs):
        for k in C.FIELDS:
            if k != "clock":
                assert a[k].tobytes() == b[k].tobytes(), (i, k)


# ---------------------------------------------------------------- 5. the closed loop
def test_closed_loop_with_a_database_that_grows():
    import torch

    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import tracking
    from gf_orb_slam_amd.localmapping import LocalMapper

    voc = GS.vocabulary()
    W, fr, gmaps, dbs, fe0, T, V, dvoc = TL._scene_setup(1, GS.G, 4, voc)
    fe0.close()
    gm = gmaps[0]
    M = len(gm["mp"]) + 1400  # room for what CreateNewMapPoints appends
    fe = FrontEnd("euroc", 1000, 1, M, 100)
    fe.set_vocab(dvoc)
    fe.set_map(0, gm["mp"], gm["desc"])
    fe.set_covis(0, gm["graph"])
    m = tracking.loopmap_from_global_map(TL.INFO, gm, voc=dvoc)
    nkf0 = m.nkf
    rows = lambda: [(m.kf_kps[k], m.kf_desc[k], m.kf_bow[k][0], m.kf_bow[k][1], m.kf_fv[k]) for k in range(m.nkf)]  # noqa: E731,E501
    db = GS.database(rows(), max_kf=64, max_rows=sum(len(k) for k in m.kf_kps) + 4 * fe.cap)
    fe.set_kfdb(0, db)  # attached from the start: it grows with the graph
    fe.set_rng(0, 7)
    fe.set_source(torch.from_numpy(fr).cuda().contiguous(), W.scene_of, W.phase)
    fe.bootstrap(T, V, 0.0)
    fb = tracking.MapFeedback(fe, 0, m)
    ins = tracking.KeyFrameInserter(fe, [LocalMapper(m, dvoc)], feedback=[fb])
    fe.enable_keyframes()
    k = 0
    while not fe.keyframe_state()["pending"][0]:
        k += 1
        assert k <= 4, "no keyframe within four steps"
        fe.step()
    assert ins.pump() == [(0, nkf0)]
    ins.run_mapper(0)
    sent = ins.feed_back()
    assert len(sent) == 1 and sent[0].kf_rows is not None and sent[0].kf_rows.nkf == 1
    want = tracking.covis_graph_from_loopmap(m)
    assert MR.same_graph(fe.covis(0), want) == []
    full = GS.database(rows())
    assert full.nkf == nkf0 + 1
    got = db.read(fe.ctx)
    assert R.same(got, R.build(full)) == [] and R.same(got, full.read(fe.ctx)) == []
    assert all(getattr(db, k_).tobytes() == getattr(full, k_).tobytes() for k_ in R.ROW_KEYS)
    # the next step tracks the mapper's map with the grown database
    n = len(m.mps)
    st = C.read_state(fe)
    ch = C.Chain("euroc", 1000, M, 100)
    ch.set_map(m.mps, m.mp_desc)
    ch.set_covis(want)
    ch.set_kfdb(full)
    ch.set_vocab(voc)
    ch.load_from(st, 0)
    ch.write("reloc", st["reloc"][0])
    fe.step()
    ch.step(fr[0, (W.phase[0] + k + 1) % W.period])
    TL._compare(C.read_state(fe), ch, 0, "the step after the feedback: ")
    assert int(st["nmp"][0]) == n
    fe.close()
