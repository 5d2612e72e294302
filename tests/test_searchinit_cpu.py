"""The CPU restatement of ORBmatcher::SearchForInitialization
(tests/helpers/searchinit_ref.cpp) on cases small enough to work out by hand,
and the conditions on the scenes that the GPU parity tests rely on: every
branch counter is > 0 on each contended seed, and each two-view seed used end
to end gives at least 100 matches. No GPU."""
import numpy as np
import pytest

import searchinit_ref as R
import searchinit_scenes as S

CONTENDED_SEEDS = (1, 2, 3)
TWO_VIEW_SEEDS = (1, 2, 3)


def D(k):
    """256 bits, the first k set: dist(D(a), D(b)) = |a - b|."""
    bits = np.zeros(256, np.uint8)
    bits[:k] = 1
    return np.packbits(bits)


def run(q, c, prev=None, **kw):
    """q, c: lists of (x, y, angle, descriptor) of level-0 keypoints."""
    k1 = S.kparr([(x, y) for x, y, _, _ in q], 0, [a for _, _, a, _ in q])
    k2 = S.kparr([(x, y) for x, y, _, _ in c], 0, [a for _, _, a, _ in c])
    d1, d2 = np.stack([d for *_, d in q]), np.stack([d for *_, d in c])
    return R.search(S.INFO, k1, d1, k2, d2, S.prev_of(k1) if prev is None else prev, **kw)


def test_steal():
    # q0: c0 at 3, c1 at 30 -> accepts c0. q1: c0 at 0 (3 <= 0 is false: not filtered), c1 at 27 -> accepts c0 and
    # robs q0. Both accepts fall into bin 0; q0's entry is stale.
    nm, m12, prev, cnt = run([(100, 100, 0, D(10)), (105, 100, 0, D(13))], [(110, 100, 0, D(13)), (120, 100, 0, D(40))])
    assert nm == 1 and m12.tolist() == [-1, 0]
    assert prev.tolist() == [[100, 100], [110, 100]]
    assert cnt == dict(steals=1, filtered=0, ratio_equal=0, hist_removed=0, stale=1)


def test_filter_skip_changes_the_outcome():
    # q0: c0 at 1, c1 at 20 -> c0, vMatchedDistance[c0] = 1. q1: c0 at 9 is hidden (1 <= 9), c1 at 10 is alone:
    # accepted. Unfiltered, q1 would see 9 and 10 and fail the ratio test (9 < 10 * 0.9f is false).
    nm, m12, prev, cnt = run([(100, 100, 0, D(10)), (105, 100, 0, D(20))], [(110, 100, 0, D(11)), (120, 100, 0, D(30))])
    assert nm == 2 and m12.tolist() == [0, 1]
    assert prev.tolist() == [[110, 100], [120, 100]]
    assert cnt == dict(steals=0, filtered=1, ratio_equal=0, hist_removed=0, stale=0)


@pytest.mark.parametrize("a,b", [(12, 8), (10, 10)])
def test_equal_distances_fail_the_ratio_test(a, b):
    # two candidates at the same distance (2 and 2, then 0 and 0), in different cells: the first in walk order is
    # the best, the second becomes bestDist2 = bestDist, and best < best2 * 0.9f is false.
    nm, m12, prev, cnt = run([(100, 100, 0, D(10))], [(140, 100, 0, D(a)), (90, 100, 0, D(b))])
    assert nm == 0 and m12.tolist() == [-1] and prev.tolist() == [[100, 100]]
    assert cnt["ratio_equal"] == 1


def test_thresholds_50_51_and_the_ratio():
    # alone at 50: accepted (best2 = INT_MAX); alone at 51: not. 8 against 10: 8 < 9; 9 against 10: 9 < 9 is false.
    far = 300
    q = [(100 + far * (i % 2), 100 + far * (i // 2) * 0.5, 0, D(100)) for i in range(4)]
    c = [(q[0][0] + 5, q[0][1], 0, D(150)), (q[1][0] + 5, q[1][1], 0, D(151)),
         (q[2][0] + 5, q[2][1], 0, D(108)), (q[2][0] - 5, q[2][1], 0, D(90)),
         (q[3][0] + 5, q[3][1], 0, D(109)), (q[3][0] - 5, q[3][1], 0, D(90))]
    nm, m12, _, cnt = run(q, c)
    assert m12.tolist() == [0, -1, 2, -1] and nm == 2


def test_stale_entry_decides_the_three_maxima():
    """Bins: 0 <- three pairs and the robber, 2 <- two pairs, 4 <- one pair and
    the robbed query's stale entry, 6 <- two pairs. ComputeThreeMaxima sees
    4, 2, 2, 2: bins 0, 2 and 4 (the first to reach 2 as third) are kept and
    bin 6's two matches are removed. Without the stale entry bin 4 would hold
    1 and lose to bin 6."""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, size=(9, 32), dtype=np.uint8)
    dist = np.unpackbits(base[:, None] ^ base[None], axis=2).sum(2)
    assert dist[~np.eye(9, dtype=bool)].min() > 60  # the families never meet below TH_LOW

    def near(d, k):
        bits = np.unpackbits(d)
        bits[:k] ^= 1
        return np.packbits(bits)

    q, c = [], []
    for p, rot in enumerate([0, 0, 0, 60, 60, 120, 180, 180]):  # eight plain pairs, each at distance 2
        x, y = 40 + 80 * p, 100
        q.append((x, y, 200 + rot, base[p]))
        c.append((x + 10, y, 200, near(base[p], 2)))
    # the robbed pair: q8 takes c8 at distance 3 with rot 120 (bin 4), q9 = c8's descriptor takes it at 0 with rot 0
    q.append((300, 350, 120, base[8]))
    c.append((310, 350, 0, near(base[8], 3)))
    q.append((305, 350, 0, near(base[8], 3)))
    nm, m12, prev, cnt = run(q, c)
    assert m12.tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1, 8]
    # (neighbouring families see each other's matched candidates at ~128 and skip them: the filter count is not 0)
    assert nm == 7 and (cnt["steals"], cnt["ratio_equal"], cnt["hist_removed"], cnt["stale"]) == (1, 0, 2, 1)
    assert prev[6].tolist() == [40 + 80 * 6, 100] and prev[9].tolist() == [310, 350]
    # the same scene without the robbed query and the robber: bin 4 holds one entry, bin 6 is third, bin 4's match goes
    nm, m12, _, cnt = run(q[:8], c)
    assert m12.tolist() == [0, 1, 2, 3, 4, -1, 6, 7] and nm == 7 and cnt["hist_removed"] == 1
    # and with the orientation check off nothing is removed
    nm, m12, _, _ = run(q, c, check_ori=False)
    assert m12.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, 8] and nm == 9


def test_prev_matched_is_the_window_centre():
    # the candidate is 150 px from the keypoint and 10 px from vbPrevMatched
    prev = np.array([[250, 100]], np.float32)
    nm, m12, out, _ = run([(100, 100, 0, D(10))], [(260, 100, 0, D(12))], prev=prev)
    assert nm == 1 and m12.tolist() == [0] and out.tolist() == [[260, 100]]
    nm, m12, out, _ = run([(100, 100, 0, D(10))], [(260, 100, 0, D(12))])
    assert nm == 0 and out.tolist() == [[100, 100]]


def test_gate_and_first_initialization():
    s = S.two_view(1)
    assert R.first_initialization(s["kps1"][:100]) is None and R.first_initialization(s["kps1"][:101]) is not None
    ini = np.full(len(s["kps1"]), 7, np.int32)
    st, nm, m, prev = R.gate(S.INFO, s["kps1"], s["desc1"], s["kps2"][:100], s["desc2"][:100], s["prev"], ini)
    assert st == R.FEW_KEYPOINTS and (m == -1).all() and np.array_equal(prev, s["prev"])
    st, nm, m, prev = R.gate(S.INFO, s["kps1"], s["desc1"], s["kps2"][:150], s["desc2"][:150], s["prev"], ini)
    assert st == R.FEW_MATCHES and 0 < nm < 100 and (m >= 0).sum() == nm and not np.array_equal(prev, s["prev"])
    st, nm, m, prev = R.gate(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"], ini)
    assert st == R.OK and nm >= 100


@pytest.mark.parametrize("seed", CONTENDED_SEEDS)
def test_contended_scenes_take_every_branch(seed):
    s = S.contended(seed)
    assert 150 <= len(s["kps1"]) <= 400 and 150 <= len(s["kps2"]) <= 400
    nm, m12, prev, cnt = R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"])
    print(seed, nm, cnt)
    assert all(cnt[k] > 0 for k in R.COUNTERS), cnt
    assert (m12 >= 0).sum() == nm


@pytest.mark.parametrize("seed", TWO_VIEW_SEEDS)
def test_two_view_scenes_reach_the_initialiser(seed):
    s = S.two_view(seed)
    nm, m12, _, _ = R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"])
    assert nm >= 100 and np.array_equal(m12[m12 >= 0], s["gt"][m12 >= 0])


def test_crowded_scene_exceeds_any_list():
    s = S.crowded(1)
    c = np.array([S.W / 2, S.H / 2], np.float32)
    k2 = s["kps2"]
    inside = (k2["octave"] == 0) & (np.abs(k2["x"] - c[0]) <= 100) & (np.abs(k2["y"] - c[1]) <= 100)
    assert inside.sum() >= 600
    nm, *_ = R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"])
    assert nm > 0
