"""Loop detection without a GPU: the serial restatement
(tests/helpers/loopdetect_ref.cpp) on hand-computed cases, gf_bow_score against
it, LoopDetector's host logic against the restatement's DetectLoop, and the
conditions the GPU tests' scenes must meet, asserted on the restatement's
trace. Every comparison is exact."""
import numpy as np
import pytest

import loopdetect_ref as R
import loopdetect_scenes as S
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.loopdetect import LoopDetector, bow_score

F32 = np.float32


def _bv(d):
    w = np.array(sorted(d), np.int32)
    return w, np.array([d[k] for k in w.tolist()], np.float64)


def test_restatement_lists_and_erase_by_hand():
    w = R.RefWorld()
    a = w.insert(*_bv({1: .5, 4: .5}))
    b = w.insert(*_bv({4: .25, 7: .75}))
    c = w.insert(*_bv({1: .5, 7: .5}))
    for k in (a, b, c):
        w.add(k)
    assert w.word_list(1) == [a, c] and w.word_list(4) == [a, b] and w.word_list(7) == [b, c]
    w.erase(a)
    assert w.word_list(1) == [c] and w.word_list(4) == [b]
    w.add(a)  # back of every list
    assert w.word_list(1) == [c, a] and w.word_list(4) == [b, a] and w.word_list(9) == []
    w.clear()
    assert w.word_list(1) == []


def test_restatement_score_by_hand():
    # common words 4 and 7: (|.5-.25| - .5 - .25) + (|.25-.5| - .25 - .5) = -1.0 -> 0.5
    v1, v2 = _bv({1: .25, 4: .5, 7: .25}), _bv({4: .25, 7: .5, 9: .25})
    assert R.score_vectors(v1, v2) == 0.5
    assert R.score_vectors(v1, _bv({2: 1.0})) == 0.0
    assert R.score_vectors(v1, v1) == 1.0  # .25, .5, .25 add exactly


def test_restatement_candidates_by_hand():
    """Four database keyframes and a query {1, 2, 3, 4} of quarters.
    Words: kf0 {1,2,3,4}, kf1 {2,3,4,9}, kf2 {3,9}, kf3 {1,2,3,4} connected.
    Lists walked by word: 1 -> kf0 (kf3 connected); 2 -> kf1; 3 -> kf2. Common
    words 4, 3, 1; max 4, min (int)(3.2f) = 3: kf0 is scored (1.0), kf1 has
    exactly 3 and is not, kf2 neither. kf0's covisible kf1 is not summed."""
    q4 = {1: .25, 2: .25, 3: .25, 4: .25}
    w = R.RefWorld()
    for d in (q4, {2: .25, 3: .25, 4: .25, 9: .25}, {3: .5, 9: .5}, q4, q4):
        w.insert(*_bv(d))
    for k in range(4):
        w.add(k)
    w.set_graph(0, [1], [1])
    w.set_graph(4, [3], [3])
    r = w.detect_candidates(4, 0.5)
    assert r["words"].tolist() == [4, 3, 1, 0, 0] and r["min_common"] == 3
    assert r["cands"].tolist() == [0] and r["score"][0] == F32(1.0) and r["score"][1] == 0
    t = r["trace"]
    assert (t["sharing"], t["scored"], t["passed"], t["at_min_common"], t["neigh_skipped"]) == (3, 1, 1, 1, 1)
    # with the floor above every score nothing is returned
    assert len(w.detect_candidates(4, float(np.nextafter(F32(1), F32(2))))["cands"]) == 0


def test_restatement_order_and_best_by_hand():
    """kf0 and kf1 both meet the query at word 1; kf1 was added first, so it
    leads. kf2 (word 2 only... and 3) names its better covisible kf1."""
    q = {1: .5, 2: .25, 3: .25}
    w = R.RefWorld()
    w.insert(*_bv({1: .25, 2: .25, 3: .25, 8: .25}))  # 0.75
    w.insert(*_bv(q))                                   # 1.0
    w.insert(*_bv({1: .125, 2: .25, 3: .125, 9: .5}))  # 0.5
    w.insert(*_bv(q))
    for k in (1, 0, 2):
        w.add(k)
    w.set_graph(2, [0, 1], [0, 1])
    r = w.detect_candidates(3, 0.25)
    assert r["score"][:3].tolist() == [0.75, 1.0, 0.5]
    # accumulated: kf1 1.0, kf0 0.75, kf2 0.5 + 0.75 + 1.0 = 2.25 -> retain > 1.6875: only kf2's entry, naming kf1
    assert r["cands"].tolist() == [1]
    assert r["trace"]["best_differs"] == 1 and r["trace"]["dropped"] == 2
    w.set_graph(2, [], [])
    assert w.detect_candidates(3, 0.25)["cands"].tolist() == [1]  # kf0's 0.75 is not above 0.75 * 1.0
    w.erase(1)
    assert w.detect_candidates(3, 0.25)["cands"].tolist() == [0]  # now best 0.75: kf2's 0.5 is not above 0.5625



@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bow_score_equals_restatement(seed):
    rng = np.random.default_rng(seed)
    base = rng.choice(S.NWORDS, 300, replace=False)
    for n1, n2 in ((0, 0), (0, 5), (1, 1), (64, 65), (200, 180), (400, 30)):
        v1, v2 = S.vec(rng, base, n1, n1 // 4), S.vec(rng, base, n2, n2 // 4)
        assert bow_score(v1, v2) == R.score_vectors(v1, v2)
        assert bow_score(v2, v1) == R.score_vectors(v2, v1)
        # score(v, v) is the sequential sum of the values, which numpy normalised to 1: n roundings of each
        assert abs(bow_score(v1, v1) - (1.0 if len(v1[0]) else 0.0)) <= (len(v1[0]) + 2) * 2.0 ** -52
    assert bow_score(_bv({3: .5, 4: .5}), _bv({3: .5, 4: .5})) == 1.0


def test_bow_score_other_scoring_unsupported():
    v = _bv({3: 1.0})
    with pytest.raises(GFError) as e:
        bow_score(v, v, scoring=1)
    assert e.value.code == -4


def _run_sequence(db, graph, ref, vectors):
    det = LoopDetector(db, graph, 3)
    steps = []
    for kf in range(1, len(vectors)):  # keyframe 0 never enters the queue (LoopClosing.cc:101)
        before = len(det.consistent_groups)
        ok, enough = det.detect_loop(kf)
        path, min_score, ref_enough = ref.detect_loop(kf)
        assert ok == (path == "detected") and enough == ref_enough, (kf, path)
        assert det.consistent_groups == ref.groups(), kf
        if path != "early":
            assert F32(det.min_score) == F32(min_score), kf
        steps.append((path, before, len(enough)))
    return steps


def _sequence_reference(vectors, graph):
    ref = R.RefWorld(3)
    for v in vectors:
        ref.insert(*v)
    for k in range(len(vectors)):
        ref.set_graph(k, graph.ordered[k], graph.connected[k])
        ref.set_bad(k, graph.kf_bad[k])
    return ref


def check_sequence(db):
    """LoopDetector over `db` against the restatement's DetectLoop on the
    40-keyframe sequence: outputs, groups and counters at every step."""
    vectors, graph = S.sequence_scene()
    for v in vectors:
        db.insert(*v)
    steps = _run_sequence(db, graph, _sequence_reference(vectors, graph), vectors)
    paths = [s[0] for s in steps]
    assert "detected" in paths and "early" in paths
    assert any(p == "no_candidate" and before > 0 for p, before, _ in steps), "no step cleared live groups"
    return steps


def test_loop_detector_equals_restatement_on_sequence():
    steps = check_sequence(R.RefDatabase())
    assert [s[0] for s in steps[:9]] == ["early"] * 9  # mnId < 0 + 10


def test_loop_detector_last_loop_id_moves_the_early_return():
    vectors, graph = S.sequence_scene()
    db, ref = R.RefDatabase(), _sequence_reference(vectors, graph)
    for v in vectors:
        db.insert(*v)
    det = LoopDetector(db, graph, 3)
    det.last_loop_kf_id = 20
    ref.set_last_loop(20)
    for kf in range(1, 35):
        ok, enough = det.detect_loop(kf)
        path, _, ref_enough = ref.detect_loop(kf)
        assert (path == "early") == (kf < 30) and ok == (path == "detected") and enough == ref_enough
        assert det.consistent_groups == ref.groups()


# ---- the GPU scenes' conditions, on the restatement alone

def test_tie_scene_conditions():
    sc = S.tie_scene()
    r = S.reference_result(sc)
    assert r["trace"]["same_first_word"] >= 20
    c = r["cands"].tolist()
    assert len(c) == 25 and c[-1] == 3 and c[:3] == [0, 1, 2]  # the re-added slot went to the back


def test_exclusion_scene_conditions():
    sc = S.exclusion_scene()
    w = S.build_reference(sc)
    r = w.detect_candidates(sc["query"], sc["min_score"])
    assert r["words"][[0, 1, 2, 3, 4, 5]].tolist() == [0] * 6  # connected, never added, erased
    assert not set(r["cands"].tolist()) & {0, 1, 2, 3, 4, 5} and len(r["cands"]) > 0
    assert r["trace"]["max_common"] == 100 and r["trace"]["neigh_skipped"] >= 8 * 5
    # without the exclusion the copies would have held the maximum too and entered the sums
    for k in (0, 2, 3):
        sc["connected"][sc["query"]].discard(k)
    r2 = S.reference_result(sc)
    assert r2["words"][0] == 100 and r2["cands"].tolist() != r["cands"].tolist()
    assert w.score(sc["query"], 1) > 0.9  # the never-added slot still scores


def test_threshold_scene_conditions():
    sc = S.threshold_scene()
    r = S.reference_result(sc)
    t = r["trace"]
    assert t["max_common"] == 64 and t["min_common"] == 51 and float(F32(64) * F32(0.8)) != 51
    # exactly minCommonWords: not scored, not a candidate; one more word: scored and a candidate
    assert r["words"][1] == 51 and r["score"][1] == 0 and r["words"][2] == 52 and r["score"][2] > 0
    assert t["at_min_common"] == 1 and t["just_above"] >= 1
    # the copy of the covisible that sets minScore scores minScore and is kept: it is in the result
    assert t["at_min_score"] == 1 and r["score"][4] == F32(sc["min_score"]) and r["words"][3] == 0
    assert sorted(r["cands"].tolist()) == [0, 2, 4] and t["dropped"] == 0
    above = float(np.nextafter(F32(sc["min_score"]), F32(2)))
    assert sorted(S.build_reference(sc).detect_candidates(sc["query"], above)["cands"].tolist()) == [0, 2]
    # the eleventh covisible is scored but not summed: as the tenth it would drop every other entry
    assert t["eleventh"] >= 1 and sc["ordered"][0][10] == 2 and r["score"][2] > 0.7
    sc["ordered"][0][9], sc["ordered"][0][10] = sc["ordered"][0][10], sc["ordered"][0][9]
    assert S.reference_result(sc)["cands"].tolist() == [2]


@pytest.mark.parametrize("seed,kept", [(12, True), (9, False)])
def test_float_sum_scene_conditions(seed, kept):
    """Slot 11's score equals the larger of the two 0.75f bars that float and
    double neighbour sums give, so it is kept or dropped by the sum's type."""
    sc, k = S.float_sum_scene(seed)
    assert k == kept
    r = S.reference_result(sc)
    assert (11 in r["cands"].tolist()) == kept and r["trace"]["neigh_summed"] == 10


def test_selection_scene_conditions():
    r = S.reference_result(S.selection_scene())
    t = r["trace"]
    assert t["best_differs"] >= 2 and t["duplicates"] >= 1 and t["dropped"] >= 1 and t["passed"] == 6
    assert r["cands"].tolist().count(0) == 1


def test_same_vector_scene_conditions():
    sc = S.same_vector_scene()
    r = S.reference_result(sc)
    assert r["trace"]["passed"] == len(sc["vectors"]) - 1 == r["trace"]["sharing"]
    assert r["trace"]["retained"] > 1 and r["trace"]["dropped"] >= 1


@pytest.mark.parametrize("nslots", [1, 63, 64, 65, 300])
def test_random_scene_conditions(nslots):
    sc = S.random_scene(100 + nslots, nslots)
    r = S.reference_result(sc)
    assert r["trace"]["sharing"] >= 1 and len(r["cands"]) >= 1
    if nslots > 8:
        lens = {len(v[0]) for v in sc["vectors"]}
        assert {0, 1, 64, 65, 400} <= lens
        assert r["trace"]["scored"] < r["trace"]["sharing"]
    assert S.reference_result(S.random_scene(7, 65, query_kind="empty"))["trace"]["sharing"] == 0
    assert S.reference_result(S.random_scene(8, 65, query_kind="disjoint"))["trace"]["sharing"] == 0
