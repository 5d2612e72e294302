"""The relocalisation keyframe database that grows, without a GPU: the serial
restatement (tests/helpers/kfdb_ref.cpp: KeyFrameDatabase::add into the packed
inverted file, the append of database rows, the verdicts), the host arrays of
``KeyframeDB.extend`` and ``MapFeedback``'s rows, and the scene pin of the GPU
step test with the oracle chain alone (kfdb_grow_scenes.py)."""
import numpy as np
import pytest

import kfdb_grow_scenes as GS
import kfdb_ref as R
import oracle_lib as O
from gf_orb_slam_amd.pipeline import TR


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_append_equals_build_for_every_split(seed):
    """append(build(first k), rows k .. K - 1) is byte-identical to build(all
    K), for every k, in one call and one keyframe at a time."""
    K = 7
    kfs = R.random_keyframes(seed, K, nkp=(0, 12), vocab=20 if seed % 2 else 300)
    full = R.build(R.db_of(kfs))
    rows_all = sum(len(k[0]) for k in kfs)
    for k in range(K + 1):
        for one_by_one in (False, True):
            ref = R.RefDB(R.db_of(kfs[:k]), K, rows_all, fill=0xA5)
            groups = [[x] for x in kfs[k:]] if one_by_one else ([kfs[k:]] if k < K else [])
            for g in groups:
                assert ref.append(R.db_of(g)) == 0
            assert R.same(ref.packed(), full) == [], (k, one_by_one)
    # the host arrays of a KeyframeDB that was extended are those of the one built whole
    # (a growable one extends in place inside arrays held at the capacities, a fixed one by concatenation)
    whole = R.db_of(kfs)
    for db in (R.db_of(kfs[:3]), R.db_of(kfs[:3], max_kf=K, max_rows=rows_all), R.db_of([], max_kf=K, max_rows=rows_all)):
        first = db.nkf
        db.extend(R.db_of(kfs[first:5]))
        db.extend(R.db_of(kfs[5:]))
        assert db.nkf == K and all(getattr(db, k).tobytes() == getattr(whole, k).tobytes() for k in R.ROW_KEYS)
        assert R.same(R.build(db), full) == []


def _kf(nkp, words, seed=0):
    return R.keyframe(np.random.default_rng(seed), nkp, words)


def test_hand_written_inverted_files():
    # words present, absent and mixed; below the first and above the last listed word
    ref = R.RefDB(R.db_of([_kf(3, [10, 20, 30])]), 8, 64)
    p = ref.packed()
    assert p["inv_words"].tolist() == [10, 20, 30] and p["inv_off"].tolist() == [0, 1, 2, 3]
    assert p["inv_kf"].tolist() == [0, 0, 0]
    assert ref.append(R.db_of([_kf(4, [5, 20, 25, 40], 1)])) == 0
    p = ref.packed()
    assert p["inv_words"].tolist() == [5, 10, 20, 25, 30, 40]
    assert p["inv_off"].tolist() == [0, 1, 2, 4, 5, 6, 7]
    assert p["inv_kf"].tolist() == [1, 0, 0, 1, 1, 0, 1]
    # a keyframe without keypoints, then two in one call: all present, none present
    assert ref.append(R.db_of([_kf(0, [], 2)])) == 0
    assert ref.packed()["inv_kf"].tolist() == [1, 0, 0, 1, 1, 0, 1] and ref.packed()["nkf"] == 3
    assert ref.append(R.db_of([_kf(3, [10, 20, 30], 3), _kf(2, [1, 99], 4)])) == 0
    p = ref.packed()
    assert p["inv_words"].tolist() == [1, 5, 10, 20, 25, 30, 40, 99]
    assert p["inv_off"].tolist() == [0, 1, 2, 4, 7, 8, 10, 11, 12]
    assert p["inv_kf"].tolist() == [4, 1, 0, 3, 0, 1, 3, 1, 0, 3, 1, 4]
    assert p["kp_off"].tolist() == [0, 3, 7, 7, 10, 12] and p["bow_off"].tolist() == [0, 3, 7, 7, 10, 12]
    assert R.same(p, R.build(R.db_of([_kf(3, [10, 20, 30]), _kf(4, [5, 20, 25, 40], 1), _kf(0, [], 2),
                                      _kf(3, [10, 20, 30], 3), _kf(2, [1, 99], 4)]))) == []


def test_verdicts():
    base = [_kf(3, [10, 20, 30]), _kf(2, [7, 8], 1)]
    ref = R.RefDB(R.db_of(base), 3, 9)
    before = ref.packed()

    def refused(rows, code):
        assert ref.append(rows) == code
        assert R.same(ref.packed(), before) == []

    refused(R.db_of([_kf(1, [1], 2), _kf(1, [2], 3)]), -3)  # max_kf + 1
    refused(R.db_of([_kf(5, [1], 2)]), -3)  # max_rows + 1
    bad = R.db_of([_kf(3, [5, 6, 7], 2)])
    bad.bow_words[:] = [5, 5, 7]
    refused(bad, -1)  # words not ascending
    bad = R.db_of([_kf(3, [5, 6, 7], 2)])
    bad.fv_feats[0] = 3
    refused(bad, -1)  # a feature index out of range
    bad = R.db_of([_kf(3, [5, 6, 7], 2)])
    bad.kp_off[:] += 1
    refused(bad, -1)  # offsets that do not start at 0
    assert R.check(R.db_of(base)) == 0
    # exactly max_kf and exactly max_rows pass
    assert ref.append(R.db_of([_kf(4, [1, 2, 3, 4], 5)])) == 0
    assert ref.packed()["nkf"] == 3 and len(ref.packed()["kps"]) == 9


def test_map_feedback_fills_the_rows_of_a_growable_stream():
    """MapFeedback.delta() carries the new keyframes' rows when the stream's
    database grows, none when it is fixed or absent, and refuses a keyframe
    without BoW before anything is sent."""
    from types import SimpleNamespace

    from gf_orb_slam_amd import tracking

    kfs = R.random_keyframes(9, 3, nkp=(4, 9))
    slots = [np.full(len(k[0]), -1, np.int32) for k in kfs]
    g = lambda n: dict(kf_bad=np.zeros(n, np.uint8), kf_mp_off=np.concatenate([[0], np.cumsum([len(s) for s in slots[:n]])]).astype(np.int32),  # noqa: E731,E501
                       kf_mp=np.concatenate(slots[:n]), kf_cov_off=np.zeros(n + 1, np.int32), kf_cov=np.zeros(0, np.int32),
                       mp_bad=np.zeros(1, np.uint8), mp_obs_off=np.zeros(2, np.int32), mp_obs=np.zeros(0, np.int32))
    m = SimpleNamespace(nkf=3, mps=np.zeros(1, tracking.MAP_POINT_DTYPE), mp_desc=np.zeros((1, 32), np.uint8), slots=slots,
                        kf_kps=[k[0] for k in kfs], kf_desc=[k[1] for k in kfs],
                        kf_bow=[(k[2], k[3]) for k in kfs], kf_fv=[k[4] for k in kfs])
    real = tracking.covis_graph_from_loopmap
    tracking.covis_graph_from_loopmap = lambda mm: g(mm.nkf)
    try:
        shadow = dict(mp=m.mps, desc=m.mp_desc, graph=g(2))
        for db, want in ((R.db_of(kfs[:2], max_kf=4, max_rows=64), True), (R.db_of(kfs[:2]), False), (None, False)):
            fe = SimpleNamespace(_kfdbs={0: db})
            d = tracking.MapFeedback(fe, 0, m, shadow=shadow).delta()
            assert (d.kf_rows is not None) == want
            if want:
                assert d.kf_rows.nkf == 1 and R.same(R.build(d.kf_rows), R.build(R.db_of(kfs[2:]))) == []
        m.kf_bow[2] = None
        with pytest.raises(ValueError):
            tracking.MapFeedback(SimpleNamespace(_kfdbs={0: R.db_of(kfs[:2], max_kf=4, max_rows=64)}), 0, m, shadow=shadow)
    finally:
        tracking.covis_graph_from_loopmap = real


# ---------------------------------------------------------------- the scene pin
def test_scene_pin_relocalises_only_with_the_appended_keyframe():
    """PHASE_OFFSET 12, keyframe 11 moved last, blank steps 2 and 3: with the
    graph and database of all K keyframes from step 3 on, the oracle chain
    relocalises at step 4 and the last keyframe is among that step's
    candidates; with the keyframe withheld from both it stays LOST."""
    voc = GS.vocabulary()
    W = GS.workload()
    fr = W.render_all("cpu").numpy()
    gmaps = W.build_global_maps(lambda im: O.extract(im), GS.G, device="cpu")
    m0, m1, rows = GS.maps_of(W, gmaps, GS.oracle_transform(voc))
    K = len(rows)
    db0, db1 = GS.database(rows[:-1]), GS.database(rows)
    T, V = W.boot_state()
    ch = GS.chain(m0, db0, voc)
    ch.set_rng(7)
    ch.bootstrap(fr[W.scene_of[0], W.phase[0] % W.period], T[0], V[0])
    for k in range(1, GS.K_BEFORE + 1):
        ch.step(GS.frame_of(W, fr, k))
    assert int(ch.read("track")[TR["state"]]) == 1, "the stream is not LOST when the keyframe arrives"
    st = GS.chain_state(ch)
    out = {}
    for name, (m, db) in dict(full=(m1, db1), withheld=(m0, db0)).items():
        c = GS.chain(m, db, voc)
        c.load_from(st, 0)
        c.write("reloc", st["reloc"][0])
        for k in range(GS.K_BEFORE + 1, GS.RELOC_STEP):
            c.step(GS.frame_of(W, fr, k))
        before = c.read("reloc")
        c.step(GS.frame_of(W, fr, GS.RELOC_STEP))
        cands, after, q = GS.candidates(c, before, db, m["graph"], voc)
        assert after[:db.nkf].tobytes() == c.read("reloc")[:db.nkf].tobytes(), name
        out[name] = (c, cands, q)
        print(name, "candidates", cands.tolist(), "state", int(c.read("track")[TR["state"]]), "flags",
              c.stats()["flags"] & 32768)
    full, cands, q = out["full"]
    assert full.stats()["flags"] & 32768 and int(full.read("track")[TR["state"]]) == 0, "the full chain stays LOST"
    assert K - 1 in cands.tolist() and int(full.read("reloc")[K - 1]["query"]) == q
    held = out["withheld"][0]
    assert int(held.read("track")[TR["state"]]) == 1 and not held.stats()["flags"] & 32768
    assert not np.array_equal(full.read("kp2mp"), held.read("kp2mp"))
    assert not np.array_equal(full.read("track"), held.read("track"))
