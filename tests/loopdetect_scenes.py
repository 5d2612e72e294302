"""Scenes for the loop-detection tests: BowVectors made directly with numpy
(sorted words from a space of ~20,000 ids, positive doubles normalised to sum
1), a covisibility graph and the add / erase history of the database. A scene
is a dict: ``vectors`` [(words, values)], ``ordered`` (list of lists),
``connected`` (list of sets), ``ops`` [("add" | "erase", slot)], ``query``,
``min_score``."""
from __future__ import annotations

import numpy as np

import loopdetect_ref as R

NWORDS = 20000


class Graph:
    """The part of a keyframe map a LoopDetector reads."""

    def __init__(self, ordered, connected, kf_bad=None, kf_id=None):
        self.ordered = [list(o) for o in ordered]
        self.connected = [set(c) for c in connected]
        n = len(self.ordered)
        self.kf_bad = np.zeros(n, bool) if kf_bad is None else np.asarray(kf_bad, bool)
        self.kf_id = np.arange(n) if kf_id is None else np.asarray(kf_id)

    def get_connected_keyframes(self, kf):
        return set(self.connected[kf])


def normalised(rng, n):
    v = rng.random(n) + 0.05
    return v / v.sum()


def vec(rng, base, n_base, n_rand, lo=0, hi=NWORDS):
    """n_base words drawn from `base` plus n_rand random ones of [lo, hi)."""
    w = set(rng.choice(base, min(n_base, len(base)), replace=False).tolist()) if n_base else set()
    w |= set(rng.integers(lo, hi, n_rand).tolist())
    w = np.array(sorted(w), np.int32)
    return w, normalised(rng, len(w))


def scaled(rng, q, a, n_other, lo):
    """Every word of q with a times its value, and n_other words of [lo, ...)
    sharing the rest of the mass: scores about `a` against q."""
    ow = np.array(sorted(set(rng.integers(lo, lo + 5000, n_other).tolist())), np.int32)
    ov = normalised(rng, len(ow)) * (1.0 - a)
    w = np.concatenate([q[0], ow])
    v = np.concatenate([q[1] * a, ov])
    o = np.argsort(w, kind="stable")
    return w[o].astype(np.int32), v[o]


def scene(vectors, ordered, connected, ops, query, min_score):
    return dict(vectors=vectors, ordered=[list(o) for o in ordered], connected=[set(c) for c in connected], ops=ops,
                query=query, min_score=float(np.float32(min_score)))


def reference_min_score(sc):
    """minScore as DetectLoop takes it: the lowest float score of the query to
    its ordered covisibles, from 1."""
    q = sc["vectors"][sc["query"]]
    m = np.float32(1)
    for k in sc["ordered"][sc["query"]]:
        s = np.float32(R.score_vectors(q, sc["vectors"][k]))
        if s < m:
            m = s
    return float(m)


def random_scene(seed, nslots, mean_words=120, special=True, query_kind="normal"):
    """Places of shared base words; most slots added in a shuffled order, some
    erased, some re-added, some never added; the query is the last slot."""
    rng = np.random.default_rng(seed)
    nplaces = max(1, nslots // 12)
    bases = [rng.choice(NWORDS, int(mean_words * 1.3), replace=False) for _ in range(nplaces)]
    place = rng.integers(0, nplaces, nslots)
    vectors = [vec(rng, bases[place[i]], int(mean_words * 0.8), int(mean_words * 0.25)) for i in range(nslots)]
    if special:  # lengths at and around the wave width, and the extremes
        for i, n in zip(range(1, nslots - 1, max(1, (nslots - 2) // 5)), (0, 1, 64, 65, 400)):
            b = bases[place[i]]
            w = np.array(sorted(rng.choice(np.union1d(b, rng.integers(0, NWORDS, 600)), n, replace=False).tolist()),
                         np.int32) if n else np.zeros(0, np.int32)
            vectors[i] = (w, normalised(rng, n) if n else np.zeros(0))
    q = nslots - 1
    place[q] = place[0]
    vectors[q] = vec(rng, bases[place[q]], int(mean_words * 0.8), int(mean_words * 0.25))
    if query_kind == "empty":
        vectors[q] = (np.zeros(0, np.int32), np.zeros(0))
    elif query_kind == "disjoint":
        w = np.arange(NWORDS + 10, NWORDS + 90, dtype=np.int32)
        vectors[q] = (w, normalised(rng, len(w)))
    ordered, connected = [], []
    for i in range(nslots):
        near = [j for j in range(i - 7, i + 8) if 0 <= j < nslots and j != i]
        rng.shuffle(near)
        o = near[:int(rng.integers(0, 13))]
        ordered.append(o)
        connected.append(set(o) | set(near[:2]))
    order = rng.permutation(nslots).tolist()
    ops = [("add", k) for k in order if k != q or nslots == 1]
    if nslots > 8:
        never = set(rng.choice(nslots - 1, max(1, nslots // 20), replace=False).tolist())
        ops = [o for o in ops if o[1] not in never]
        listed = [o[1] for o in ops]
        for k in rng.choice(listed, max(2, nslots // 15), replace=False).tolist():
            ops.append(("erase", k))
            if rng.random() < 0.5:
                ops.append(("add", k))
    sc = scene(vectors, ordered, connected, ops, q, 0)
    sc["min_score"] = min(reference_min_score(sc), 0.05) if query_kind == "normal" else 0.0
    return sc


def tie_scene(seed=3):
    """25 database keyframes that all hold the query's smallest word, so the
    order of lKFsSharingWords falls to the add order; slot 3 is erased and
    added again, which moves it behind its neighbours."""
    rng = np.random.default_rng(seed)
    qw = np.array(sorted(rng.choice(np.arange(100, NWORDS), 80, replace=False).tolist()), np.int32)
    qw[0] = 5
    q = (qw, normalised(rng, 80))
    vectors = [scaled(rng, q, 0.8 + 0.1 * rng.random(), 20, NWORDS) for _ in range(25)] + [q]
    ops = [("add", k) for k in range(25)] + [("erase", 3), ("add", 3)]
    n = len(vectors)
    return scene(vectors, [[] for _ in range(n)], [set() for _ in range(n)], ops, n - 1, 0.01)


def exclusion_scene(seed=4):
    """Copies of the query (the highest common counts) are connected to it or
    erased; the survivors list them as covisibles. Slot 1 was never added."""
    rng = np.random.default_rng(seed)
    qw = np.array(sorted(rng.choice(NWORDS, 100, replace=False).tolist()), np.int32)
    q = (qw, normalised(rng, 100))
    vectors = [(q[0].copy(), q[1].copy()) for _ in range(6)]            # 0-3 connected, 4-5 erased
    vectors[1] = scaled(rng, q, 0.95, 5, NWORDS)                       # never added
    vectors += [scaled(rng, q, 0.4 + 0.05 * i, 30, NWORDS) for i in range(8)]  # 6-13 survivors
    vectors.append(q)                                                   # 14 the query
    n = len(vectors)
    ordered = [[] for _ in range(n)]
    for i in range(6, 14):
        ordered[i] = [0, 4, 1, (i - 6 + 1) % 8 + 6, 2, 5]
    ordered[14] = [0, 2, 3]
    connected = [set(o) for o in ordered]
    connected[14] = {0, 1, 2, 3}
    ops = [("add", k) for k in range(14) if k != 1] + [("erase", 4), ("erase", 5)]
    return scene(vectors, ordered, connected, ops, 14, 0.05)


def shaped(rng, q, k, a, n_other, lo, fixed=None):
    """k of q's words, each with a times q's value, and n_other words of
    [lo, ...) outside q's sharing the rest of the mass: exactly k common words
    and a score of a times the mass q has on them. fixed = (idx, ow, ov): the
    random choices of an earlier call, so that only `a` varies."""
    if fixed is None:
        idx = np.sort(rng.choice(len(q[0]), k, replace=False))
        ow = np.array(sorted(set(rng.integers(lo, lo + 5000, n_other).tolist())), np.int32)
        fixed = (idx, ow, normalised(rng, len(ow)))
    idx, ow, ov = fixed
    v = q[1][idx] * a
    w = np.concatenate([q[0][idx], ow])
    x = np.concatenate([v, ov * (1.0 - v.sum())])
    o = np.argsort(w, kind="stable")
    return (w[o].astype(np.int32), x[o]), fixed


def threshold_scene(seed=5):
    """max = 64 common words, so max * 0.8f = 51.2 and minCommonWords = 51.
    Slot 0 (score about 0.6) has twelve ordered covisibles: nine low-scoring
    ones, slot 1, then slot 2 as the eleventh. Slot 1 has exactly 51 common
    words and would score about 0.8, enough to be a candidate: it is neither scored, nor summed, nor a
    candidate. Slot 2 has 52 and scores about 0.77: a candidate of its own, but
    as the eleventh covisible not part of slot 0's sum (which would otherwise
    drop every other entry). Slot 3 is the query's covisible that sets minScore
    (connected, so excluded); slot 4 holds a copy of its vector, scores
    minScore exactly, is kept and, with ten low covisibles, stays above 0.75 of
    the best sum as its own best keyframe. Slots 5-14 score about 0.04: above
    minCommonWords, below minScore."""
    rng = np.random.default_rng(seed)
    qw = np.array(sorted(rng.choice(10000, 64, replace=False).tolist()), np.int32)
    q = (qw, normalised(rng, 64))
    mk = lambda k, a: shaped(rng, q, k, a, 25, 10000)[0]  # noqa: E731
    v3 = mk(56, 0.5)
    vectors = [mk(64, 0.6), mk(51, 0.99), mk(52, 0.95), v3, (v3[0].copy(), v3[1].copy())]
    vectors += [mk(53 + i % 8, 0.05) for i in range(10)]  # slots 5-14
    vectors.append(q)
    n = len(vectors)
    qs = n - 1
    ordered = [[] for _ in range(n)]
    ordered[0] = [5, 6, 7, 8, 9, 10, 11, 12, 13, 1, 2, 14]
    ordered[4] = list(range(5, 15))
    ordered[qs] = [3]
    connected = [set(o) for o in ordered]
    ops = [("add", k) for k in range(qs)]
    sc = scene(vectors, ordered, connected, ops, qs, 0)
    sc["min_score"] = reference_min_score(sc)
    return sc


def float_sum_scene(seed=9):
    """The neighbour sums are float additions in neighbour order. Slot 0 has ten
    scored covisibles whose float sum differs from the rounded double sum, so
    0.75f times it differs too; slot 11's score is tuned (by bisection on its
    vector's scale) to the larger of the two bars, which keeps or drops it.
    -> (scene, kept under float sums: bool)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    qw = np.array(sorted(rng.choice(10000, 60, replace=False).tolist()), np.int32)
    q = (qw, normalised(rng, 60))
    while True:
        vectors = [shaped(rng, q, 60, 0.04 + 0.08 * rng.random(), 20, 10000)[0] for _ in range(11)]
        s = [f32(R.score_vectors(q, v)) for v in vectors]
        fsum = s[0]
        for x in s[1:]:
            fsum = f32(fsum + x)
        dsum = f32(sum(float(x) for x in s))
        if f32(0.75) * fsum != f32(0.75) * dsum:
            break
    bar_f, bar_d = f32(0.75) * fsum, f32(0.75) * dsum
    target = max(bar_f, bar_d)  # above the smaller bar, not above the larger
    _, fixed = shaped(rng, q, 60, 0.5, 20, 10000)
    lo, hi = 0.0, 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        got = f32(R.score_vectors(q, shaped(rng, q, 60, mid, 20, 10000, fixed)[0]))
        if got == target:
            break
        lo, hi = (mid, hi) if got < target else (lo, mid)
    assert got == target
    vectors.append(shaped(rng, q, 60, mid, 20, 10000, fixed)[0])  # slot 11
    vectors.append(q)
    n = len(vectors)
    ordered = [[] for _ in range(n)]
    ordered[0] = list(range(1, 11))
    ops = [("add", k) for k in range(n - 1)]
    return scene(vectors, ordered, [set(o) for o in ordered], ops, n - 1, 0.01), bool(target > bar_f)


def selection_scene(seed=6):
    """Scores of about 0.9 (Y, slot 0), 0.5 and 0.55 (X1, X2: slots 1, 2, both
    with Y as covisible, so both name Y), 0.3 (Z, slot 3, alone: at or below
    0.75 * best)."""
    rng = np.random.default_rng(seed)
    qw = np.array(sorted(rng.choice(10000, 60, replace=False).tolist()), np.int32)
    q = (qw, normalised(rng, 60))
    vectors = [scaled(rng, q, a, 25, 10000) for a in (0.9, 0.5, 0.55, 0.3, 0.6, 0.45)] + [q]
    n = len(vectors)
    ordered = [[] for _ in range(n)]
    ordered[0] = [2]
    ordered[1] = [5, 0]
    ordered[2] = [0, 4]
    ordered[4] = [5]
    connected = [set(o) for o in ordered]
    ops = [("add", k) for k in (2, 1, 0, 3, 5, 4)]
    return scene(vectors, ordered, connected, ops, n - 1, 0.2)


def same_vector_scene(seed=7, nslots=130):
    """Every slot holds the same vector, the query too: every listed slot
    passes the common-word and the score test."""
    rng = np.random.default_rng(seed)
    q = vec(rng, np.arange(NWORDS), 90, 0)
    vectors = [(q[0].copy(), q[1].copy()) for _ in range(nslots)]
    ordered = []
    for i in range(nslots):
        near = [j for j in range(i - 6, i + 7) if 0 <= j < nslots - 1 and j != i]
        rng.shuffle(near)
        ordered.append(near[:int(rng.integers(0, 12))])
    ordered[-1] = []
    connected = [set(o) for o in ordered]
    ops = [("add", k) for k in rng.permutation(nslots - 1).tolist()]
    return scene(vectors, ordered, connected, ops, nslots - 1, 0.5)


def sequence_scene(seed=13):
    """40 keyframes along a path that leaves place 0, glimpses it again at
    keyframe 14 and returns to it from keyframe 23 on. -> (vectors, Graph)."""
    rng = np.random.default_rng(seed)
    place = [0] * 8 + [1] * 6 + [0] + [2] * 8 + [0] * 17
    bases = [rng.choice(NWORDS, 150, replace=False) for _ in range(3)]
    vectors = [vec(rng, bases[p], 120, 30) for p in place]
    run = np.cumsum([0] + [int(place[i] != place[i - 1]) for i in range(1, 40)])
    ordered, connected = [], []
    for i in range(40):
        o = [j for j in (i - 1, i + 1, i - 2, i + 2, i - 3) if 0 <= j < 40 and run[j] == run[i]]
        ordered.append(o)
        connected.append(set(o) | {j for j in (i - 4, i + 3) if 0 <= j < 40 and run[j] == run[i]})
    bad = np.zeros(40, bool)
    bad[26] = True
    return vectors, Graph(ordered, connected, bad)


def build_reference(sc, upto=None):
    w = R.RefWorld()
    for v in sc["vectors"]:
        w.insert(*v)
    for k in range(len(sc["vectors"])):
        w.set_graph(k, sc["ordered"][k], sc["connected"][k])
    for op, k in sc["ops"]:
        getattr(w, op)(k)
    return w


def reference_result(sc):
    return build_reference(sc).detect_candidates(sc["query"], sc["min_score"])
