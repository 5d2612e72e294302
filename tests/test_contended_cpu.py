"""The contended scenes (contended_scenes.py) on the CPU oracle alone: proof
that they exercise what the device tests of test_contended_gpu.py rely on.
On every ladder scene the query order, the ratio test, the <= TH_HIGH boundary
and the rotation histogram each decide assignments (the floors below are
conditions on the scenes, met by the choice of seeds and ladders); the cluster
scenes give the result derived by hand from the reference loop.

The case lists and the oracle runs are shared with the device tests."""
import functools

import numpy as np
import pytest

import contended_scenes as CS
import oracle_lib as O
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, FrameInfo
from gf_orb_slam_amd.observability import ObsCamera

TH_HIGH = 100
RELOC_INFO = FrameInfo.make(*CS.RELOC_CAMERA)


def _c(a):
    return np.ascontiguousarray(a)


def changed(a, b, among=None):
    d = np.asarray(a) != np.asarray(b)
    return int((d if among is None else d & among).sum())


@pytest.mark.parametrize("rungs,step,flips", CS.LADDERS)
def test_ladder_distances(rungs, step, flips):
    """Without flips two rows are a whole number of rungs apart; with them the
    pairwise distances reach both sides of TH_HIGH."""
    d = CS.ladder_descriptors(np.random.default_rng(3), 200, rungs, step, 0)
    D = CS.hamming(d[:, None], d[None])
    assert set(np.unique(D).tolist()) == {j * step for j in range(rungs)}
    d = CS.ladder_descriptors(np.random.default_rng(3), 400, rungs, step, flips)
    D = CS.hamming(d[:, None], d[None])
    assert D.max() <= (rungs - 1) * step + 2 * flips
    assert (D == TH_HIGH).any() and (D == TH_HIGH + 1).any() and (D == 0).any()


# ------------------------------------------------- SearchByProjection(F, map)
# camera, map points, keypoints, seed, ladder, th, nnratio
PROJECT_CASES = [
    ("euroc", 800, 600, 1, 0, 1.0, 0.8),   # the narrow-window scene
    ("tum", 800, 600, 2, 1, 3.0, 0.6),
    ("euroc", 800, 600, 3, 2, 5.0, 0.8),
    ("euroc", 500, 600, 4, 3, 10.0, 0.9),
    ("tum", 700, 500, 5, 0, 3.0, 0.8),
    ("euroc", 777, 555, 6, 3, 5.0, 0.6),
]


@functools.lru_cache(maxsize=None)
def project_scene(cam, nmp, nkp, seed, ladder):
    """(scene, frame info, views, starting kp2mp / score with pre-claimed keypoints)."""
    sc = CS.ladder_scene(cam, nmp, nkp, seed, CS.LADDERS[ladder])
    info = FrameInfo.make(*sc["camera"])
    views, _ = O.frustum(info, sc["Tcw"], sc["map"])
    rng = np.random.default_rng(seed)
    pre = rng.choice(nkp, nkp // 20, replace=False)  # matches of an earlier stage
    kp2mp, score = np.full(nkp, -1, np.int32), np.full(nkp, 999, np.int32)
    kp2mp[pre], score[pre] = 100000 + pre, 7
    return sc, info, views, kp2mp, score


def oracle_project(scene, th, ratio, reverse=False):
    """-> (nmatches, kp2mp, score); reverse: the map points in reverse list
    order, their ids mapped back."""
    sc, info, views, kp2mp, score = scene
    km, s = kp2mp.copy(), score.copy()
    v, d = (_c(views[::-1]), _c(sc["mp_desc"][::-1])) if reverse else (views, sc["mp_desc"])
    n = O.match_project(info, sc["keypoints"], sc["descriptors"], v, d, th, ratio, km, s)
    if reverse:
        new = (km >= 0) & (kp2mp < 0)
        km[new] = len(views) - 1 - km[new]
    return n, km, s


@pytest.mark.parametrize("cam,nmp,nkp,seed,ladder,th,ratio", PROJECT_CASES)
def test_projection_scene_is_contended(cam, nmp, nkp, seed, ladder, th, ratio):
    scene = project_scene(cam, nmp, nkp, seed, ladder)
    n, km, s = oracle_project(scene, th, ratio)
    new = (km >= 0) & (scene[3] < 0)
    assert n == new.sum() and n >= 50
    _, km_r, _ = oracle_project(scene, th, ratio, reverse=True)
    order = changed(km, km_r, new)
    _, km_1, _ = oracle_project(scene, th, 1.0)
    nratio = changed(km, km_1)
    at = int((s[new] == TH_HIGH).sum())
    print(f"projection seed {seed} th {th} ratio {ratio}: {n} matches, reversed order changes {order}, "
          f"ratio off changes {nratio}, {at} at TH_HIGH")
    assert order >= (0.1 * n if th >= 3 else 1)
    assert nratio >= 5
    assert at >= 1 and s[new].max() == TH_HIGH


# ------------------------------------------- SearchByProjection(Cur, Last, th)
# seed, ladder, th
LAST_CASES = [(1, 0, 15.0), (2, 1, 15.0), (7, 2, 45.0), (4, 3, 7.0)]


@functools.lru_cache(maxsize=None)
def lastframe_scene(seed, ladder):
    """contended_scenes.lastframe_pair (800 map points, 600 keypoints) with
    ladder descriptors and quantised angles -> (last, cur, info)."""
    last, cur, info = CS.lastframe_pair(seed)
    rng = np.random.default_rng(seed + 7200)
    d = CS.ladder_descriptors(rng, last.N + cur.N, *CS.LADDERS[ladder])
    last.mDescriptors, cur.mDescriptors = _c(d[:last.N]), _c(d[last.N:])
    last.mvKeysUn["angle"] = CS.quantise_angles(rng, last.mvKeysUn["angle"])
    cur.mvKeysUn["angle"] = CS.quantise_angles(rng, cur.mvKeysUn["angle"])
    return last, cur, info


def oracle_lastframe(scene, th, ori, reverse=False):
    last, cur, info = scene
    km, s = cur.mvpMapPoints.copy(), cur.mvpMatchScore.copy()
    o = slice(None, None, -1) if reverse else slice(None)
    n = O.match_lastframe(info, cur.mvKeysUn, cur.mDescriptors, cur.mTcw, _c(last.mvKeysUn[o]),
                          _c(last.mDescriptors[o]), _c(last.mvpMapPoints[o]), _c(last.mvbOutlier[o]),
                          _c(last.mp_pos[o]), th, ori, km, s)
    return n, km, s


@pytest.mark.parametrize("seed,ladder,th", LAST_CASES)
def test_lastframe_scene_is_contended(seed, ladder, th):
    scene = lastframe_scene(seed, ladder)
    n, km, s = oracle_lastframe(scene, th, False)
    new = km >= 0
    assert n == new.sum() and n >= 50
    _, km_r, _ = oracle_lastframe(scene, th, False, reverse=True)
    order = changed(km, km_r, new)
    at = int((s[new] == TH_HIGH).sum())
    print(f"last frame seed {seed} th {th}: {n} matches, reversed order changes {order}, {at} at TH_HIGH")
    assert order >= 0.1 * n
    assert at >= 1 and s[new].max() == TH_HIGH


def test_lastframe_orientation_check_decides():
    hit = 0
    for seed, ladder, th in LAST_CASES:
        scene = lastframe_scene(seed, ladder)
        n0, km0, _ = oracle_lastframe(scene, th, False)
        n1, km1, _ = oracle_lastframe(scene, th, True)
        print(f"last frame seed {seed} th {th}: orientation check changes {changed(km0, km1)} ({n0} -> {n1})")
        assert n1 >= 50
        hit += changed(km0, km1) >= 5
    assert hit >= 2


# ------------------------------------------------------ runActiveMapMatching
# seed, ladder, num_to_match, th
ACTIVE_CASES = [(2, 0, 40, 1.0), (1, 3, 100, 1.0), (10, 1, 100, 1.0), (1, 3, 40, 3.0), (2, 2, 100, 3.0), (4, 1, 100, 3.0)]


@functools.lru_cache(maxsize=None)
def active_scene(seed, ladder, nmp=800, nkp=600, frac_updated=0.9):
    """test_gf_gpu._active_case on a ladder scene, its inputs from the oracle
    (views, Jacobians and information blocks are bit-equal to the device's:
    test_frustum_bit_exact, test_build_info_bit_exact)."""
    sc = CS.ladder_scene("euroc", nmp, nkp, seed, CS.LADDERS[ladder])
    fi = FrameInfo.make(*sc["camera"])
    views, _ = O.frustum(fi, sc["Tcw"], sc["map"])
    cam = ObsCamera.from_intrinsics(*sc["camera"][2:], sc["camera"][0], sc["camera"][1])
    T = sc["Tcw"]
    Xv = O.obs_update(0.0, T, 0.05, np.linalg.inv(T.astype(np.float64)).astype(np.float32))
    kine = O.obs_predict(Xv, 0.05, 1)
    H, info, uv, _ = O.obs_build_info(cam, np.array(kine[0].Xv[:]), sc["map"]["pos"], None, False)
    rng = np.random.default_rng(seed)
    updated = (rng.uniform(size=nmp) < frac_updated).astype(np.uint8)
    pre = rng.choice(nkp, nkp // 10, replace=False)
    kp2mp, score = np.full(nkp, -1, np.int32), np.full(nkp, 999, np.int32)
    kp2mp[pre], score[pre] = 100000 + pre, 11
    base = np.eye(7).reshape(-1) * 1e-5
    return dict(sc=sc, fi=fi, cam=cam, views=views, H=H, info=info, uv=uv, updated=updated, base=base, kp2mp=kp2mp,
                score=score)


def oracle_active(A, ntm, th, ratio, seed):
    """-> (nmatched, kp2mp, score, left-over map points, std::rand calls)."""
    km, s = A["kp2mp"].copy(), A["score"].copy()
    sig2 = (A["fi"].scale_factors() ** 2).astype(np.float32)
    sc = A["sc"]
    n, left = O.active_match(A["fi"], sc["keypoints"], sc["descriptors"], A["views"], sc["mp_desc"], A["updated"],
                             A["info"], A["H"], A["uv"], A["base"], sig2, ntm, th, ratio, seed, km, s)
    return n, km, s, left, O.last_rand_calls()


@pytest.mark.parametrize("seed,ladder,ntm,th", ACTIVE_CASES)
def test_active_scene_is_contended(seed, ladder, ntm, th):
    A = active_scene(seed, ladder)
    n, km, s, _, calls = oracle_active(A, ntm, th, 0.8, seed)
    new = (km >= 0) & (A["kp2mp"] < 0)
    _, km_1, _, _, _ = oracle_active(A, ntm, th, 1.0, seed)
    nratio = changed(km, km_1)
    print(f"active seed {seed} ntm {ntm} th {th}: {n} matched, ratio off changes {nratio}, "
          f"{int((s[new] == TH_HIGH).sum())} at TH_HIGH, {calls} rand calls")
    at = int((s[new] == TH_HIGH).sum())
    # one match a round: num_to_match bounds the count, so the 40-round cases
    # cannot reach 50 matches and must match in every round instead
    assert n == new.sum() == ntm and (n >= 50 or ntm < 50) and calls > 0
    if th >= 3:
        assert nratio >= 5
    assert at >= 1 and s[new].max() == TH_HIGH


# ------------------------------------------------- the track-loss matchers
# The floors of the projection matcher carry over to every scene here: a
# reversed query order moves at least 10% of the matches, the ratio test at
# least 5.
# seed, ladder, window, min_level
WINDOW_CASES = [(1, 0, 200, 4), (2, 1, 50, 0), (3, 0, 15, 0)]
# seed, ladder, window
FRAMES_CASES = [(3, 2, 20), (5, 3, 50)]
# seed, ladder, th, orb_dist
KF_CASES = [(9, 3, 10.0, 100), (4, 1, 3.0, 64)]


@functools.lru_cache(maxsize=None)
def reloc_scene(seed, ladder):
    """contended_scenes.reloc_pair (at most 540 + 594 keypoints) with ladder
    descriptors and quantised angles."""
    return CS.relabel_two_frames(CS.reloc_pair(seed), seed, CS.LADDERS[ladder])


def _rev(F):
    """The same problem with F1's keypoints (the queries) in reverse order."""
    F = dict(F)
    for k in ("X", "K1", "D1", "mp1"):
        F[k] = _c(F[k][::-1])
    return F


def window_args(F, window, min_level):
    return (F["K2"], F["D2"], F["K1"], F["D1"], F["mp1"], window, min_level)


def frames_args(F, seed, window):
    """test_search_frames_matches_oracle's problem."""
    rng = np.random.default_rng(seed)
    n2 = len(F["K2"])
    kp2mp = np.full(n2, -1, np.int32)  # some matches already set (spMapPointsAlreadyFound)
    pre = rng.choice(n2, n2 // 8, replace=False)
    ids = np.sort(F["mp1"][F["mp1"] >= 0])
    kp2mp[pre] = rng.choice(ids, len(pre), replace=False)
    score = np.full(n2, 999, np.int32)
    return (F["K2"], F["D2"], F["T2"], F["K1"], F["D1"], F["mp1"], F["X"][:len(F["K1"])], window, kp2mp, score)


def kf_args(F, seed, th, orb_dist):
    """test_search_kf_projection_matches_oracle's problem."""
    rng = np.random.default_rng(seed)
    mps = np.zeros(4000, MAP_POINT_DTYPE)
    mp_desc = rng.integers(0, 256, (4000, 32), dtype=np.uint8)
    ids = F["mp1"]
    ok = ids >= 0
    mps["pos"][ids[ok]] = F["X"][ok]
    d = np.linalg.norm(F["X"][ok].astype(np.float64), axis=1).astype(np.float32)
    scale = np.empty(len(ids), np.float32)  # drawn per point id, so that a reordered F1 gives the same map
    scale[np.argsort(ids, kind="stable")] = rng.uniform(1.0, 3.0, len(ids)).astype(np.float32)
    mps["min_dist"][ids[ok]] = d / scale[ok]
    mps["max_dist"][ids[ok]] = d * 4
    mp_desc[ids[ok]] = F["D1"][ok]
    found = (rng.uniform(size=4000) < 0.2).astype(np.uint8)
    n2 = len(F["K2"])
    kp2mp = np.full(n2, -1, np.int32)
    kp2mp[rng.choice(n2, n2 // 10, replace=False)] = np.flatnonzero(found)[:n2 // 10]
    score = np.full(n2, 999, np.int32)
    return (F["K2"], F["D2"], F["T2"], F["K1"], ids, mps, mp_desc, found, th, orb_dist, kp2mp, score)


@pytest.mark.parametrize("seed,ladder,window,min_level", WINDOW_CASES)
def test_window_search_scene_is_contended(seed, ladder, window, min_level):
    F = reloc_scene(seed, ladder)
    n, out = O.window_search(RELOC_INFO, *window_args(F, window, min_level), check_ori=False)
    _, out_r = O.window_search(RELOC_INFO, *window_args(_rev(F), window, min_level), check_ori=False)
    _, out_1 = O.window_search(RELOC_INFO, *window_args(F, window, min_level), nnratio=1.0, check_ori=False)
    order, nratio = changed(out, out_r, out >= 0), changed(out, out_1)
    print(f"window search seed {seed} window {window}: {n} matches, reversed order changes {order}, "
          f"ratio off changes {nratio}")
    assert n >= 50 and order >= 0.1 * n and nratio >= 5


@pytest.mark.parametrize("seed,ladder,window", FRAMES_CASES)
def test_search_frames_scene_is_contended(seed, ladder, window):
    F = reloc_scene(seed, ladder)
    a = frames_args(F, seed, window)
    n, km, s = O.search_frames(RELOC_INFO, *a)
    new = (km >= 0) & (a[8] < 0)
    _, km_r, _ = O.search_frames(RELOC_INFO, *frames_args(_rev(F), seed, window))
    _, km_1, _ = O.search_frames(RELOC_INFO, *a, nnratio=1.0)
    order, nratio = changed(km, km_r, new), changed(km, km_1)
    at = int((s[new] == TH_HIGH).sum())
    print(f"search frames seed {seed} window {window}: {n} matches, reversed order changes {order}, "
          f"ratio off changes {nratio}, {at} at TH_HIGH")
    assert n == new.sum() and n >= 50 and order >= 0.1 * n and nratio >= 5
    assert at >= 1 and s[new].max() == TH_HIGH


@pytest.mark.parametrize("seed,ladder,th,orb_dist", KF_CASES)
def test_search_kf_projection_scene_is_contended(seed, ladder, th, orb_dist):
    F = reloc_scene(seed, ladder)
    a = kf_args(F, seed, th, orb_dist)
    n, km, s = O.search_kf_projection(RELOC_INFO, *a, check_ori=False)
    new = (km >= 0) & (a[10] < 0)
    _, km_r, _ = O.search_kf_projection(RELOC_INFO, *kf_args(_rev(F), seed, th, orb_dist), check_ori=False)
    order = changed(km, km_r, new)
    at = int((s[new] == orb_dist).sum())
    print(f"keyframe projection seed {seed} th {th}: {n} matches, reversed order changes {order}, "
          f"{at} at ORBdist {orb_dist}")
    assert n == new.sum() and n >= 50 and order >= 0.1 * n
    assert at >= 1 and s[new].max() == orb_dist


def test_track_loss_orientation_check_decides():
    """WindowSearch and SearchByProjection(F, KF) bin rotations (the
    SearchByProjection(F1, F2, window) of TrackPreviousFrame has no orientation
    check: ORBmatcher.cc:1089-1168)."""
    hit = 0
    for seed, ladder, window, min_level in WINDOW_CASES:
        a = window_args(reloc_scene(seed, ladder), window, min_level)
        n0, o0 = O.window_search(RELOC_INFO, *a, check_ori=False)
        n1, o1 = O.window_search(RELOC_INFO, *a, check_ori=True)
        print(f"window search seed {seed}: orientation check changes {changed(o0, o1)} ({n0} -> {n1})")
        hit += changed(o0, o1) >= 5
    for seed, ladder, th, orb_dist in KF_CASES:
        a = kf_args(reloc_scene(seed, ladder), seed, th, orb_dist)
        n0, k0, _ = O.search_kf_projection(RELOC_INFO, *a, check_ori=False)
        n1, k1, _ = O.search_kf_projection(RELOC_INFO, *a, check_ori=True)
        print(f"keyframe projection seed {seed}: orientation check changes {changed(k0, k1)} ({n0} -> {n1})")
        hit += changed(k0, k1) >= 5
    assert hit >= 2


# ------------------------------------------------------------------ clusters
def oracle_cluster_lastframe(S, ori=True):
    info = FrameInfo.make(*S["camera"])
    km, s = S["kp2mp"].copy(), S["score"].copy()
    n = O.match_lastframe(info, S["kps"], S["desc"], S["Tcw"], S["last_kps"], S["last_desc"], S["last_kp2mp"],
                          S["last_outlier"], S["last_pos"], S["th"], ori, km, s)
    return n, km, s


def oracle_cluster_project(S, ratio=0.8):
    info = FrameInfo.make(*S["camera"])
    km, s = S["kp2mp"].copy(), S["score"].copy()
    n = O.match_project(info, S["kps"], S["desc"], S["views"], S["mp_desc"], S["th"], ratio, km, s)
    return n, km, s


@pytest.mark.parametrize("variant,preclaimed", CS.CLUSTER_VARIANTS)
@pytest.mark.parametrize("c", CS.CLUSTER_SIZES)
def test_cluster_matches_in_candidate_order(c, variant, preclaimed):
    """Query k takes the k-th unclaimed keypoint in candidate order, the extra
    keypoints stay unmatched: the oracle agrees with the derivation from
    ORBmatcher.cc:384-465 and :2081-2202."""
    for build, run in ((CS.cluster_lastframe, oracle_cluster_lastframe), (CS.cluster_project, oracle_cluster_project)):
        S = build(c, 2, variant, preclaimed)
        n, km, s = run(S)
        assert n == S["expect_n"] == c
        np.testing.assert_array_equal(km, S["expect_kp2mp"])
        np.testing.assert_array_equal(s, S["expect_score"])
        assert (km < 0).sum() == 2


ROTATION_CASES = [(p, v, n) for p in CS.ROTATION_PLANS for v, n in (("one", 0), ("columns", 3))]


@pytest.mark.parametrize("plan,variant,preclaimed", ROTATION_CASES)
def test_cluster_rotation_histogram(plan, variant, preclaimed):
    """Known matches with planned rotations: the bins ComputeThreeMaxima keeps
    (ties, the 0.1 rule at and below its boundary) as derived by hand."""
    S = CS.cluster_rotation(plan, variant, preclaimed)
    n0, km0, _ = oracle_cluster_lastframe(S, ori=False)
    assert n0 == len(S["last_kps"]) and (km0 >= 0).sum() == n0 + preclaimed
    n, km, s = oracle_cluster_lastframe(S, ori=True)
    hist, keep = CS.ROTATION_PLANS[plan]
    assert n == S["expect_n"] == sum(hist[b] for b in keep) < n0
    np.testing.assert_array_equal(km, S["expect_kp2mp"])
    np.testing.assert_array_equal(s, S["expect_score"])


def window_cluster_args(S):
    """The cluster as a WindowSearch problem: the last frame's keypoints as F1
    (window 15 px around their own positions, level 0), the cluster's keypoints as F2."""
    return (S["kps"], S["desc"], S["last_kps"], S["last_desc"], S["last_kp2mp"], 15, 0)


@pytest.mark.parametrize("variant", ["one", "columns"])
@pytest.mark.parametrize("plan", list(CS.ROTATION_PLANS))
def test_window_search_cluster_rotation(plan, variant):
    """WindowSearch on the same clusters (0 <= 0.9 x 0 passes its ratio test):
    the same claims in candidate order and the same surviving bins."""
    S = CS.cluster_rotation(plan, variant)
    info = FrameInfo.make(*S["camera"])
    n0, out0 = O.window_search(info, *window_cluster_args(S), check_ori=False)
    assert n0 == len(S["last_kps"]) == (out0 >= 0).sum()
    n, out = O.window_search(info, *window_cluster_args(S), check_ori=True)
    assert n == S["expect_n"]
    np.testing.assert_array_equal(out, S["expect_kp2mp"])
