"""The CPU restatement of LocalMapping::CreateNewMapPoints
(tests/helpers/localmap_ref.cpp) on its own: that the synthetic scene reaches
the exits, that the neighbours really depend on each other, that what it
accepts is geometrically right, and LoopMap's new methods and
map_point_culling against it. No GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import localmap_ref as R
import localmap_scenes as S
import oracle_lib as O
from gf_orb_slam_amd.loopmap import LoopMap
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE


@functools.lru_cache(maxsize=None)
def world():
    sc = S.scene(3)
    return sc, R.create_new_map_points(sc, chain=1), R.create_new_map_points(sc, chain=0)


def test_scene_reaches_every_exit():
    """Every exit but w0 and dist0 at least 3 times; the skipped neighbours
    are reported, the others matched."""
    sc, ref, _ = world()
    assert [R.STATUS[s] for s in ref["status"]] == ["ok", "ok", "baseline", "nodepth", "ok"]
    counts = {n: int((ref["exits"] == i).sum()) for i, n in enumerate(R.EXITS)}
    print(counts)
    for n in R.EXITS:
        if n not in ("w0", "dist0"):
            assert counts[n] >= 3, (n, counts)
    ok = ref["status"] == 0
    assert np.all(ref["nmatches"][ok] > 0) and np.all(ref["nmatches"][~ok] == 0)
    assert np.all((ref["exits"] >= 0).sum(1) == ref["nmatches"])
    assert np.all((ref["exits"] == R.X["accepted"]).sum(1) == ref["naccepted"])
    assert ref["naccepted"][4] > 0  # the chain goes on after the skipped neighbours
    # skipped: no F12; the short baseline still reports its median depth
    assert not ref["F12"][2].any() and not ref["F12"][3].any()
    assert ref["median"][2] > 0 and ref["median"][3] == 0
    # the median-depth ratio of the short-baseline neighbour is what skipped it
    C = lambda T: -T[:3, :3].T.astype(np.float64) @ T[:3, 3].astype(np.float64)  # noqa: E731
    base = np.linalg.norm(C(sc["Tcw"][2]) - C(sc["Tcw"][sc["cur"]]))
    assert base / ref["median"][2] < 0.01 < np.linalg.norm(C(sc["Tcw"][0]) - C(sc["Tcw"][sc["cur"]])) / ref["median"][0]


def test_w0_and_dist0_are_shadowed():
    """The two exact-zero exits cannot be reached by a hand-made input, and
    why. w0 (x3D(3) == 0) is a point at infinity: both rays parallel, which
    the parallax test (:322) rejects first. dist0 (x3D == a camera centre) is
    a point at depth 0 in that camera, which the depth tests (:346, :350)
    reject first. The two inputs below are those cases made exact."""
    info = FrameInfo.make(1024, 512, 512.0, 512.0, 256.0, 256.0, 8, 1.2)
    T1 = np.eye(4, dtype=np.float32)
    k1, k2 = np.zeros(1, KEYPOINT_DTYPE), np.zeros(1, KEYPOINT_DTYPE)
    # dist0: kp2 at the epipole (the image of camera 1's centre). The last column of A is exactly zero,
    # the SVD returns exactly (0, 0, 0, 1), x3D == Ow1 — and z1 == 0 leaves first.
    T2 = np.eye(4, dtype=np.float32)
    T2[:3, 3] = (-0.5, 0.0, -0.25)
    k1["x"], k1["y"] = 512.0, 384.0
    k2["x"], k2["y"] = 2.0 * 512 + 256, 256.0
    e, x = R.match_body(info, T1, T2, k1[0], k2[0])
    assert R.EXITS[e] == "z1" and not x.any()
    # w0: the same pixel in two cameras of equal orientation, a sideways baseline: parallel rays
    T2[:3, 3] = (-0.5, 0.0, 0.0)
    k2["x"], k2["y"] = k1["x"], k1["y"]
    e, _ = R.match_body(info, T1, T2, k1[0], k2[0])
    assert R.EXITS[e] == "parallax"
    xn = np.array([(512.0 - 256) / 512, (384.0 - 256) / 512], np.float32)
    A = np.stack([xn[0] * T1[2] - T1[0], xn[1] * T1[2] - T1[1], xn[0] * T2[2] - T2[0], xn[1] * T2[2] - T2[1]])
    _, vt = R.svd4(A)
    assert abs(vt[3, 3]) < 1e-6 and abs(np.linalg.norm(vt[3, :3]) - 1) < 1e-6


def test_chain_matters():
    """chain=1 (the reference) and chain=0 (every neighbour matched against
    the starting slot table) differ in at least 5 new points: the scene
    exercises the dependency between neighbours."""
    _, ref, ind = world()
    key = lambda r: set(map(tuple, r["points"][["neighbour", "idx1", "idx2"]].tolist()))  # noqa: E731
    assert len(key(ref) ^ key(ind)) >= 5
    # in the reference a keypoint of the new keyframe is triangulated once
    assert len(np.unique(ref["points"]["idx1"])) == len(ref["points"])
    assert len(np.unique(ind["points"]["idx1"])) < len(ind["points"])


def test_accepted_points_reproject_and_lie_in_front():
    """Accepted points, projected in float64 with the same poses, lie within
    the reference's own gate 5.991 sigma2 (plus rounding slack 1e-3) in both
    keyframes, at positive depth."""
    sc, ref, _ = world()
    info, cur = sc["info"], sc["cur"]
    s2 = info.scale_factors().astype(np.float64) ** 2
    pts = ref["points"]
    assert len(pts) > 50
    for kf_of, idx in ((lambda r: cur, "idx1"), (lambda r: sc["neighbours"][r["neighbour"]], "idx2")):
        for r in pts:
            k = kf_of(r)
            uv, z = S.project(info, sc["Tcw"][k], r["pos"].astype(np.float64))
            kp = sc["kps"][k][r[idx]]
            err = (uv[0] - np.float64(kp["x"])) ** 2 + (uv[1] - np.float64(kp["y"])) ** 2
            assert z > 0
            assert err <= 5.991 * s2[kp["octave"]] * (1 + 1e-3), (r, err)
    # and the slot tables hold exactly the new ids at those places
    nmp = len(sc["mps"])
    for j, r in enumerate(pts):
        assert ref["slots"][cur][r["idx1"]] == nmp + j == ref["slots"][sc["neighbours"][r["neighbour"]]][r["idx2"]]


def test_median_depth_with_ties():
    """ComputeSceneMedianDepth(2) is np.sort(depths)[(n-1)//2] of the
    restatement's own depth list, on lists with ties, of even and odd length
    and of length 1."""
    rng = np.random.default_rng(5)
    T = S.pose((0.1, -0.2, 0.3), (0.02, 0.01, -0.03))
    for n in (1, 2, 7, 64, 257, 1000):
        pos = np.stack([rng.uniform(-3, 3, 20), rng.uniform(-2, 2, 20), rng.uniform(3, 9, 20)], 1).astype(np.float32)
        slots = rng.integers(0, 20, 2 * n).astype(np.int32)  # many slots share a point: ties
        slots[rng.permutation(2 * n)[:n]] = -1
        d, med = R.median_depth(T, slots, pos)
        assert len(d) == n and len(np.unique(d)) <= 20  # 20 distinct points: ties as soon as n > 20
        assert med == np.sort(d)[(n - 1) // 2] == R.median_of(d)
        z = pos[slots[slots >= 0]].astype(np.float64) @ T[2, :3].astype(np.float64) + np.float64(T[2, 3])
        assert np.array_equal(d, z.astype(np.float32))
    d, med = R.median_depth(T, np.full(5, -1, np.int32), pos)
    assert len(d) == 0 and med is None


def test_compute_f12_is_the_fundamental_matrix():
    """x1' F12 x2 = 0 for projections of the same point (to float accuracy)."""
    sc, _, _ = world()
    info, cur = sc["info"], sc["cur"]
    rng = np.random.default_rng(1)
    X = np.stack([rng.uniform(-2, 2, 50), rng.uniform(-1, 1, 50), rng.uniform(3, 9, 50)], 1)
    for k in (0, 1, 4):
        F = R.compute_f12(info, sc["Tcw"][cur], sc["Tcw"][k]).astype(np.float64)
        u1, _ = S.project(info, sc["Tcw"][cur], X)
        u2, _ = S.project(info, sc["Tcw"][k], X)
        h = lambda u: np.concatenate([u, np.ones((len(u), 1))], 1)  # noqa: E731
        line = h(u1) @ F
        dist = np.abs(np.sum(line * h(u2), 1)) / np.hypot(line[:, 0], line[:, 1])
        assert dist.max() < 0.05  # pixels


def test_svd4_against_numpy():
    """The helper's float Jacobi SVD: singular values and the null direction
    agree with LAPACK's to float accuracy."""
    rng = np.random.default_rng(2)
    for _ in range(100):
        A = rng.normal(size=(4, 4)).astype(np.float32)
        w, vt = R.svd4(A)
        u2, w2, vt2 = np.linalg.svd(A.astype(np.float64))
        assert np.allclose(w, w2, rtol=1e-5, atol=1e-6)
        assert np.all(np.diff(w) <= 0)
        assert abs(abs(vt[3].astype(np.float64) @ vt2[3]) - 1) < 1e-3 * max(1.0, w2[2] / max(w2[2] - w2[3], 1e-3))


def test_svd4_against_the_oracle_triangulate():
    """The helper's SVD against oracle/initializer.cpp's Triangulate, bit for
    bit — if the oracle library exposes it; it does not (Triangulate is
    internal to orc_initialize), so this case is skipped."""
    if not hasattr(O.orc(), "orc_triangulate"):
        pytest.skip("oracle/initializer.cpp's Triangulate is not exported by the oracle library")
    rng = np.random.default_rng(3)  # pragma: no cover
    fn = O.orc().orc_triangulate
    for _ in range(100):
        P1, P2 = rng.normal(size=(3, 4)).astype(np.float32), rng.normal(size=(3, 4)).astype(np.float32)
        x1, x2 = rng.uniform(0, 700, 2).astype(np.float32), rng.uniform(0, 700, 2).astype(np.float32)
        A = np.stack([x1[0] * P1[2] - P1[0], x1[1] * P1[2] - P1[1], x2[0] * P2[2] - P2[0], x2[1] * P2[2] - P2[1]])
        out = np.zeros(3, np.float32)
        fn(O._p(x1), O._p(x2), O._p(P1), O._p(P2), O._p(out))
        _, vt = R.svd4(A)
        assert (vt[3, :3] * np.float32(1.0 / np.float64(vt[3, 3]))).tobytes() == out.tobytes()


def small_map():
    """5 keyframes (ids 10, 11, 13, 14, 15) of 6 keypoints, 7 points."""
    info = FrameInfo.make(752, 480, 457.3, 457.3, 367.2, 248.4, 8, 1.2)
    kps = [np.zeros(6, KEYPOINT_DTYPE) for _ in range(5)]
    desc = [np.zeros((6, 32), np.uint8) for _ in range(5)]
    slots = [np.full(6, -1, np.int32) for _ in range(5)]
    #        point: observed at (kf, slot)
    layout = {0: [(0, 0), (1, 0), (2, 0)], 1: [(0, 1), (1, 1)], 2: [(0, 2), (1, 2), (3, 2)], 3: [(1, 3), (2, 3)],
              4: [(0, 4), (2, 4), (3, 4)], 5: [(3, 5), (4, 5)], 6: [(2, 5), (4, 4), (3, 3)]}
    for p, o in layout.items():
        for k, s in o:
            slots[k][s] = p
    mps = np.zeros(7, MAP_POINT_DTYPE)
    return LoopMap(info, kps, desc, slots, mps, np.zeros((7, 32), np.uint8), kf_id=[10, 11, 13, 14, 15],
                   ref_kf=[0, 0, 0, 1, 0, 3, 2], found=[1, 1, 1, 5, 30, 1, 1], visible=[1, 1, 30, 5, 40, 1, 1],
                   mp_bad=[1, 0, 0, 0, 0, 0, 0])


def test_map_point_culling_and_loopmap_methods():
    """LoopMap.new_map_point / set_bad_point / get_found_ratio and
    localmapping.map_point_culling against the restatement, on a recent list
    that takes each of the four branches of LocalMapping.cc:221-237 and the
    fall-through."""
    from gf_orb_slam_amd import localmapping as LM

    m = small_map()
    assert list(m.first_kf) == [10, 10, 10, 11, 10, 14, 13]  # the reference keyframe's mnId
    cur = 4  # mnId 15
    p = m.new_map_point((1.0, 2.0, 3.0), cur)
    assert p == 7 and len(m.mps) == len(m.mp_desc) == len(m.mp_bad) == len(m.obs) == len(m.ref_kf) == 8
    assert m.first_kf[p] == 15 and m.found[p] == m.visible[p] == 1 and not m.mp_bad[p] and m.obs[p] == {}
    assert m.mps["pos"][p].tolist() == [1.0, 2.0, 3.0] and not m.mps["normal"][p].any()
    assert m.mps["min_dist"][p] == 0 == m.mps["max_dist"][p] and m.ref_kf[p] == cur
    m.add_observation(p, 3, 0)
    m.add_observation(p, cur, 0)
    m.add_map_point(cur, p, 0)
    m.add_map_point(3, p, 0)
    recent = [0, 1, 2, 3, 4, 5, 6, 7]
    act = R.map_point_culling(m.mp_bad[recent], m.found[recent], m.visible[recent], m.first_kf[recent],
                              [len(m.obs[q]) for q in recent], m.kf_id[cur])
    names = [R.CULL[a] for a in act]
    #   0 bad; 1 old with 2 observations; 2 found 1 of 30; 3 old with 2 obs; 4 old, 3 obs; 5 young; 6 young-ish; 7 new
    assert names == ["erased_bad", "bad_obs", "bad_ratio", "bad_obs", "erased_old", "kept", "kept", "kept"]
    assert set(names) == set(R.CULL)
    assert m.get_found_ratio(2) == np.float32(1) / np.float32(30) and m.get_found_ratio(4) == np.float32(0.75)
    before = [s.copy() for s in m.slots]
    obs2 = dict(m.obs[2])
    out = LM.map_point_culling(m, recent, cur)
    assert out == [q for q, a in zip(recent, act) if a == 0]
    want_bad = [a in (1, 2, 3) for a in act]
    assert m.mp_bad[recent].tolist() == want_bad
    # SetBadFlag: the observations are gone and the observing keyframes' slots erased; nothing else moved
    for q, a in zip(recent, act):
        if a in (2, 3):
            assert m.obs[q] == {}
    for k, s in obs2.items():
        assert before[k][s] == 2 and m.slots[k][s] == -1
    for k in range(5):
        keep = ~np.isin(before[k], [q for q, a in zip(recent, act) if a in (2, 3)])
        assert np.array_equal(m.slots[k][keep], before[k][keep])
    # point 0 was bad before the call: its observations are not SetBadFlag's business
    assert m.obs[0] and m.slots[0][0] == 0
