"""Loop detection on the device (csrc/loopdetect.hip through
gf_orb_slam_amd.loopdetect) against the serial restatement
(tests/helpers/loopdetect_ref.cpp). Every comparison is exact: candidate
lists, mnLoopWords, minCommonWords and the float bit patterns of the scores
(zero for every slot that is not scored). The conditions each scene is built for are asserted on
the restatement in tests/test_loopdetect_cpu.py."""
import numpy as np
import pytest

import loopdetect_ref as R
import loopdetect_scenes as S
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.loopdetect import KeyFrameDatabase, LoopDetector, covisibles_csr

pytestmark = pytest.mark.gpu


def build_device(sc, ops=None):
    db = KeyFrameDatabase()
    for v in sc["vectors"]:
        db.insert(*v)
    for op, k in (sc["ops"] if ops is None else ops):
        getattr(db, op)(k)
    return db


def device_result(db, sc, query=None, min_score=None):
    q = sc["query"] if query is None else query
    off, cov = covisibles_csr(sc["ordered"])
    n = db.nslots
    return db.detect_loop_candidates(q, sc["connected"][q], off[:n + 1], cov[:off[n]],
                                     sc["min_score"] if min_score is None else min_score, full=True)


def assert_same(g, r):
    assert g["min_common"] == r["min_common"]
    assert np.array_equal(g["words"], r["words"])
    # mLoopScore where words > minCommonWords, zero for every slot that is not scored
    assert np.array_equal(g["score"].view(np.uint32), r["score"].view(np.uint32))
    assert g["cands"].tolist() == r["cands"].tolist()


def check(sc):
    db = build_device(sc)
    r = S.reference_result(sc)
    assert_same(device_result(db, sc), r)
    db.close()
    return r


@pytest.mark.parametrize("nslots", [1, 63, 64, 65, 300])
def test_random_scenes_equal_restatement(nslots):
    r = check(S.random_scene(100 + nslots, nslots))
    assert len(r["cands"]) >= 1


@pytest.mark.parametrize("kind,seed", [("empty", 7), ("disjoint", 8)])
def test_query_without_common_words(kind, seed):
    r = check(S.random_scene(seed, 65, query_kind=kind))
    assert len(r["cands"]) == 0 and not r["words"].any()


def test_tie_scene_orders_by_add_sequence():
    assert check(S.tie_scene())["cands"].tolist()[-1] == 3


def test_exclusion_of_connected_erased_and_unlisted():
    sc = S.exclusion_scene()
    check(sc)
    db = build_device(sc)
    # the slot that was inserted but never added is scored, as are the erased ones
    slots = list(range(len(sc["vectors"])))
    want = np.array([np.float32(R.score_vectors(sc["vectors"][sc["query"]], sc["vectors"][k])) for k in slots])
    got = db.score_against(sc["query"], slots)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got[1] > 0.9
    db.close()


def test_thresholds():
    r = check(S.threshold_scene())
    assert sorted(r["cands"].tolist()) == [0, 2, 4]  # 4: si == minScore is kept; 1: exactly minCommonWords


@pytest.mark.parametrize("seed,kept", [(12, True), (9, False)])
def test_neighbour_sums_are_float(seed, kept):
    sc, _ = S.float_sum_scene(seed)
    assert (11 in check(sc)["cands"].tolist()) == kept


def test_selection():
    assert check(S.selection_scene())["cands"].tolist().count(0) == 1


def test_every_slot_survives():
    sc = S.same_vector_scene()
    r = check(sc)
    assert r["trace"]["passed"] == len(sc["vectors"]) - 1


def test_scores_equal_restatement():
    sc = S.random_scene(21, 300)
    db = build_device(sc)
    slots = list(range(300))
    for q in (299, 1, 50):  # 1 holds the empty vector
        want = np.array([np.float32(R.score_vectors(sc["vectors"][q], sc["vectors"][k])) for k in slots])
        assert np.array_equal(db.score_against(q, slots).view(np.uint32), want.view(np.uint32))
    assert len(db.score_against(0, [])) == 0
    db.close()


def test_larger_case():
    check(S.random_scene(31, 3000, mean_words=200, special=False))


def test_sixteen_thousand_slots():
    """No keyframe cap: 16,384 slots of a few words each, all but the query
    listed. Six of eight base words each, so about half of them share more than
    minCommonWords = 4 with the query and thousands reach pass 3."""
    rng = np.random.default_rng(5)
    n = 16384
    vectors = [S.vec(rng, np.arange(8), 6, 0) for _ in range(n)]
    # no covisibles: the accumulated score is the keyframe's own, so hundreds stay above 0.75 * best and
    # pass 3 orders a long list
    ordered = [[] for _ in range(n)]
    sc = S.scene(vectors, ordered, [set(o) for o in ordered], [("add", k) for k in range(n - 1)], n - 1, 0.02)
    r = check(sc)
    assert r["trace"]["passed"] > 1000 and len(r["cands"]) > 300


def test_every_slot_of_sixteen_thousand_is_a_candidate():
    """All 16,383 listed slots hold the query's vector and have no covisibles:
    every one survives, is retained and names itself, so pass 3 orders the
    longest list the database allows (in global memory, not in LDS)."""
    n = 16384
    w, v = np.array([3, 9, 11, 40], np.int32), np.array([.25, .25, .25, .25])
    sc = S.scene([(w, v)] * n, [[] for _ in range(n)], [set() for _ in range(n)],
                 [("add", k) for k in range(n - 1, 0, -1)], 0, 0.5)
    r = check(sc)
    assert r["cands"].tolist() == list(range(n - 1, 0, -1))  # add order


def test_growth_equals_one_go():
    """200 queries, each followed by add, on a growing database: every result
    equals the restatement's, and at four sizes a database built in one go."""
    sc = S.random_scene(41, 201, mean_words=60, special=False)
    sc["ops"] = []
    off, cov = covisibles_csr(sc["ordered"])
    db, ref = KeyFrameDatabase(), R.RefWorld()
    nfound = 0
    for k in range(200):
        # the graph as it stands when keyframe k arrives: earlier keyframes only
        sub = dict(sc, ordered=[[j for j in o if j <= k] for o in sc["ordered"][:k + 1]],
                   connected=[{j for j in c if j <= k} for c in sc["connected"][:k + 1]])
        assert db.insert(*sc["vectors"][k]) == k == ref.insert(*sc["vectors"][k])
        for j in range(k + 1):
            ref.set_graph(j, sub["ordered"][j], sub["connected"][j])
        g = device_result(db, sub, query=k, min_score=0.02)
        assert_same(g, ref.detect_candidates(k, 0.02))
        nfound += len(g["cands"])
        if k in (49, 99, 149, 199):
            sub["vectors"] = sc["vectors"][:k + 1]
            once = build_device(sub, [("add", j) for j in range(k)])
            assert_same(device_result(once, sub, query=k, min_score=0.02), g)
            once.close()
        db.add(k)
        ref.add(k)
    assert nfound > 100 and db.nlisted == 200
    db.close()


def test_vocabulary_score_uses_its_scoring_type():
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary

    tree = synth.synth_vocabulary(7, k=10, L=3)
    a = (np.array([1, 4, 7], np.int32), np.array([.25, .5, .25]))
    b = (np.array([4, 7, 9], np.int32), np.array([.25, .5, .25]))
    voc = ORBVocabulary(dict(tree, scoring=0))
    assert voc.scoring() == 0 and voc.score(a, b) == 0.5 == R.score_vectors(a, b)
    voc.close()
    voc = ORBVocabulary(dict(tree, scoring=1))  # L2_NORM: not implemented, and not silently L1
    with pytest.raises(GFError) as e:
        voc.score(a, b)
    assert e.value.code == -4
    voc.close()


def test_add_erase_clear_rules():
    db = KeyFrameDatabase()
    a = db.insert([1, 2], [.5, .5])
    b = db.insert([2, 3], [.5, .5])
    db.add(a)
    with pytest.raises(GFError):
        db.add(a)  # already listed
    with pytest.raises(GFError):
        db.add(7)
    with pytest.raises(GFError):
        db.insert([3, 2], [.5, .5])  # words must ascend
    db.erase(b)  # not listed: nothing happens
    db.add(b)
    assert (db.nslots, db.nlisted) == (2, 2)
    q = db.insert([2], [1.0])
    off = np.zeros(4, np.int32)
    assert db.detect_loop_candidates(q, [], off, [], 0.1).tolist() == [a, b]
    db.erase(a)
    db.add(a)
    assert db.detect_loop_candidates(q, [], off, [], 0.1).tolist() == [b, a]
    db.clear()
    assert db.nlisted == 0 and db.detect_loop_candidates(q, [], off, [], 0.1).tolist() == []
    db.add(a)
    assert db.detect_loop_candidates(q, [], off, [], 0.1).tolist() == [a]
    db.close()


def test_insert_dev_equals_host_insert():
    import torch

    sc = S.random_scene(51, 40, special=False)
    cap = 256
    n = len(sc["vectors"])
    words, values, nw = np.zeros((n, cap), np.int32), np.zeros((n, cap)), np.zeros(n, np.int32)
    for i, (w, v) in enumerate(sc["vectors"]):
        words[i, :len(w)], values[i, :len(w)], nw[i] = w, v, len(w)
    dw, dv, dn = (torch.from_numpy(x).cuda() for x in (words, values, nw))
    torch.cuda.synchronize()
    db = KeyFrameDatabase()
    for i in range(n):
        assert db.insert_dev(dw, dv, dn, cap, i, stream=db.ctx.stream) == i
    for op, k in sc["ops"]:
        getattr(db, op)(k)
    assert_same(device_result(db, sc), S.reference_result(sc))
    db.close()


def test_loop_detector_on_device_equals_restatement():
    from test_loopdetect_cpu import check_sequence

    db = KeyFrameDatabase()
    steps = check_sequence(db)
    assert sum(1 for s in steps if s[0] == "detected") >= 1
    db.close()
