"""SearchInNeighbors on the device: gf_fuse_search / gf_fuse_search_dev against
the CPU oracle, gf_fuse and the tests' restatement (tests/helpers/
neighbors_ref.cpp); gf_update_normal_and_depth bit for bit against
LoopMap.update_normal_and_depth and the restatement;
localmapping.search_in_neighbors against the restatement's world, alone and
chained after create_new_map_points."""
import ctypes

import numpy as np
import pytest

import neighbors_scenes as S
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd import synth
from gf_orb_slam_amd._lib import check, lib, ptr
from gf_orb_slam_amd.loopmap import LoopMap
from gf_orb_slam_amd.matcher import (FUSE_SEARCH_CHUNK_DEFAULT, FUSE_SEARCH_RESULT_DTYPE, MAP_POINT_DTYPE, FrameInfo,
                                     FuseSearchProblem, ORBmatcher, camera_center, fuse_search,
                                     update_normal_and_depth)
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE, default_context
from neighbors_ref import X, RefWorld

pytestmark = pytest.mark.gpu

CHUNK = FUSE_SEARCH_CHUNK_DEFAULT
SENTINEL = 0x7B7B7B7B


# ------------------------------------------------------------------ gf_fuse_search

def test_fuse_search_equals_oracle_and_gf_fuse():
    """On the lmap_scenes.fuse_scene inputs (the gathered rows are the map, the
    candidates its ids in order): the oracle's kp for every candidate, and the
    kp of the existing gf_fuse."""
    import lmap_scenes
    import oracle_lib as O

    for seed in (1, 2):
        sc = lmap_scenes.fuse_scene(seed)
        kf, m = sc["kf"], len(sc["mps"])
        _, want = O.fuse(sc["info"], sc["Tcw"], sc["Ow"], kf.mvKeysUn, kf.mDescriptors, sc["kf_mp"], sc["kf_bad"],
                         sc["mps"], sc["mp_desc"], sc["skip"], sc["ids"], 3.0)
        kp, dist = fuse_search(sc["info"], kf.mvKeysUn, kf.mDescriptors, sc["Tcw"], np.arange(m), sc["mps"],
                               sc["mp_desc"], None, sc["skip"], 3.0, Ow=sc["Ow"])
        assert np.array_equal(kp, want["kp"]) and (kp >= 0).sum() > 100
        assert np.array_equal(dist >= 0, kp >= 0) and dist.max() <= 50
        _, got = ORBmatcher().Fuse(kf, sc["Ow"], sc["mps"], sc["mp_desc"], 3.0, sc["kf_bad"], sc["skip"], sc["ids"])
        assert np.array_equal(kp, got["kp"])
        # the flags as map state instead of the caller's skip bytes
        kp2, _ = fuse_search(sc["info"], kf.mvKeysUn, kf.mDescriptors, sc["Tcw"], np.arange(m), sc["mps"],
                             sc["mp_desc"], sc["skip"], None, 3.0, Ow=sc["Ow"])
        assert np.array_equal(kp2, kp)


@pytest.fixture(scope="module")
def big_world():
    """The scene plus a ninth keyframe at the 4096-keypoint limit (keyframe 0's
    keypoints and pose, filled up with clutter) and a tenth without keypoints."""
    sc = S.small()
    rng = np.random.default_rng(17)
    n0 = len(sc["kf_kps"][0])
    kps = np.zeros(4096, KEYPOINT_DTYPE)
    kps[:n0] = sc["kf_kps"][0]
    kps["x"][n0:], kps["y"][n0:] = rng.uniform(0, 751, 4096 - n0), rng.uniform(0, 479, 4096 - n0)
    kps["octave"][n0:] = rng.integers(0, S.NLEVELS, 4096 - n0)
    desc = np.concatenate([sc["kf_desc"][0], rng.integers(0, 256, (4096 - n0, 32), dtype=np.uint8)])
    # clutter that competes: copies of map descriptors at random places
    desc[n0:n0 + 400] = synth.flip_bits(rng, sc["mp_desc"][rng.integers(0, len(sc["mps"]), 400)], 8)
    order = rng.permutation(4096)
    ext = dict(sc)
    ext["kf_kps"] = sc["kf_kps"] + [kps[order], np.zeros(0, KEYPOINT_DTYPE)]
    ext["kf_desc"] = sc["kf_desc"] + [desc[order], np.zeros((0, 32), np.uint8)]
    ext["kf_mp"] = sc["kf_mp"] + [np.full(4096, -1, np.int32), np.zeros(0, np.int32)]
    ext["kf_bad"] = np.concatenate([sc["kf_bad"], [False, False]])
    ext["kf_Tcw"] = np.concatenate([sc["kf_Tcw"], sc["kf_Tcw"][:1], sc["kf_Tcw"][1:2]])
    ext["kf_id"] = np.concatenate([sc["kf_id"], [20, 21]])
    w = RefWorld(*[ext[k] for k in S._KEYS], kf_Tcw=ext["kf_Tcw"], ref_kf=ext["ref_kf"], kf_id=ext["kf_id"])
    return ext, w


def _expected(w, k, pts, nmp):
    """The restatement's search of candidates pts in keyframe k; ids outside the map are NULL."""
    r = w.fuse(k, np.where((pts < 0) | (pts >= nmp), -1, pts), 3.0, apply=False)
    assert np.array_equal(r["kp"] >= 0, r["exit"] == X["fused"])
    return r["kp"], r["dist"]


def _launch(sc, problems, tail=7):
    """gf_fuse_search_dev over (keyframe, candidate ids, skip or None) problems,
    result buffers `tail` entries longer than the lists and sentinel-filled.
    -> per problem the whole buffer [npoints + tail, 2]."""
    import torch

    ctx = default_context()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_mps, d_md, d_bad = t(sc["mps"].view(np.uint8)), t(sc["mp_desc"]), t(sc["mp_bad"].astype(np.uint8))
    keep, probs, d_res = [], [], []
    for k, pts, skip in problems:
        n = len(sc["kf_kps"][k])
        kb = (t(sc["kf_kps"][k].view(np.uint8)), t(sc["kf_desc"][k])) if n else (None, None)
        d_pts = t(np.asarray(pts, np.int32))
        d_skip = None if skip is None else t(np.asarray(skip, np.uint8))
        r = torch.full(((len(pts) + tail) * 2,), SENTINEL, dtype=torch.int32, device=dev)
        keep += [kb, d_pts, d_skip]
        d_res.append(r)
        T = sc["kf_Tcw"][k]
        probs.append(FuseSearchProblem.make(T, camera_center(T), kb[0], kb[1], n, d_pts, d_skip, len(pts), 3.0, r))
    arr = (FuseSearchProblem * len(probs))(*probs)
    check(lib().gf_fuse_search_dev(ctx.handle, ctypes.byref(sc["info"]), len(probs), arr, ptr(d_mps), ptr(d_md),
                                   ptr(d_bad), len(sc["mps"]), ctx.stream))
    ctx.sync()
    return [r.cpu().numpy().reshape(-1, 2) for r in d_res]


def test_fuse_search_dev_block_table_and_edges(big_world):
    """Several problems in one launch: candidate counts around the chunk size,
    NULL and out-of-map ids, a keyframe without keypoints, one at 4096
    keypoints; result tails untouched; the host entry gives the same bytes."""
    sc, w = big_world
    nmp = len(sc["mps"])
    rng = np.random.default_rng(3)
    obs = sc["observations"]

    def cands(m):
        p = rng.integers(0, nmp, m).astype(np.int32)
        p[rng.uniform(size=m) < 0.05] = -1
        p[rng.uniform(size=m) < 0.03] = nmp + int(rng.integers(0, 5))
        p[rng.uniform(size=m) < 0.01] = -7
        return p

    def in_kf(k, pts):
        return np.asarray([0 <= p < nmp and k in obs[p] for p in pts], np.uint8)

    problems = []
    for k, m in zip((0, 1, 2, 3, 4), (1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)):
        pts = cands(m)
        if m == 1:
            pts[0] = next(p for p in sc["kf_mp"][S.CUR] if p >= 0 and 0 not in obs[p] and not sc["mp_bad"][p])
        problems.append((k, pts, in_kf(k, pts)))
    problems.append((5, np.asarray([-1, nmp, nmp + 100, -5], np.int32), None))  # nothing to search
    problems.append((9, cands(CHUNK + 3), None))                               # n = 0
    problems.append((8, np.arange(nmp, dtype=np.int32), None))                 # n = 4096, nobody observes it
    problems.append((S.CUR, np.zeros(0, np.int32), None))                      # an empty list
    out = _launch(sc, problems)
    nfused = 0
    for (k, pts, skip), res in zip(problems, out):
        m = len(pts)
        kp, dist = _expected(w, k, pts, nmp)
        assert np.array_equal(res[:m, 0], kp) and np.array_equal(res[:m, 1], dist), k
        assert (res[m:] == SENTINEL).all(), k
        nfused += int((kp >= 0).sum())
        h_kp, h_dist = fuse_search(sc["info"], sc["kf_kps"][k], sc["kf_desc"][k], sc["kf_Tcw"][k], pts, sc["mps"],
                                   sc["mp_desc"], sc["mp_bad"], skip, 3.0)
        assert np.stack([h_kp, h_dist], 1).astype(np.int32).tobytes() == res[:m].tobytes(), k
    assert (out[5][:4] == -1).all() and (out[6][:CHUNK + 3] == -1).all()
    assert (out[7][:nmp, 0] >= 0).sum() > 100 and nfused > 300
    assert FUSE_SEARCH_RESULT_DTYPE.itemsize == 8


# ------------------------------------------------------- gf_update_normal_and_depth

def _und_map(seed=2, nkf=320, npts=257):
    """320 keyframes of 4 keypoints; point 0 without observations, point 1 with
    one, point 2 seen by 300 keyframes, the others by 2-10; some reference
    keyframes that do not observe their point, some points without one."""
    rng = np.random.default_rng(seed)
    info = FrameInfo.make(*synth.CAMERAS["euroc"], nlevels=8, scale_factor=1.2)
    kf_kps = []
    for _ in range(nkf):
        k = np.zeros(4, KEYPOINT_DTYPE)
        k["octave"] = rng.integers(0, 8, 4)
        kf_kps.append(k)
    used = np.zeros(nkf, int)
    obs = [dict() for _ in range(npts)]
    obs[1][int(rng.integers(300, nkf))] = 0
    for kf in range(300):
        obs[2][kf] = 0
    used[:] = 1
    for p in range(3, npts):
        for kf in rng.choice(nkf, int(rng.integers(2, 11)), replace=False):
            if used[kf] < 4:
                obs[p][int(kf)] = int(used[kf])
                used[kf] += 1
    slots = [np.full(4, -1, np.int32) for _ in range(nkf)]
    for p, o in enumerate(obs):
        for kf, s in o.items():
            slots[kf][s] = p
    ref = np.asarray([min(o) if o else -1 for o in obs], np.int32)
    ref[0] = 5
    for p in range(10, npts, 9):
        ref[p] = next(k for k in range(nkf) if k not in obs[p])  # observations[pRefKF] reads slot 0
    ref[20:npts:37] = -1
    mps = np.zeros(npts, MAP_POINT_DTYPE)
    mps["pos"] = np.stack([rng.uniform(-3, 3, npts), rng.uniform(-2, 2, npts), rng.uniform(3, 9, npts)], 1)
    mps["normal"], mps["min_dist"], mps["max_dist"] = 7.5, 7.25, 7.125  # sentinels
    T = np.stack([synth.look_pose(rng, 0.5, 3.0) for _ in range(nkf)])
    args = (info, kf_kps, [np.zeros((4, 32), np.uint8)] * nkf, slots, mps, np.zeros((npts, 32), np.uint8))
    return args, dict(observations=obs, kf_Tcw=T, ref_kf=ref)


@pytest.mark.parametrize("ids", [[2], list(range(255)), list(range(257))], ids=["1", "255", "257"])
def test_update_normal_and_depth_bit_exact(ids):
    args, kw = _und_map()
    a, b = LoopMap(*args, **kw), LoopMap(*args, **kw)
    w = RefWorld(*args, **kw)
    a.update_normal_and_depth(ids)
    b.update_normal_and_depth_batch(ids)
    w.update_normal_and_depth(ids)
    assert a.mps.tobytes() == b.mps.tobytes()
    geo = np.concatenate([b.mps["pos"], b.mps["normal"], b.mps["min_dist"][:, None], b.mps["max_dist"][:, None]], 1)
    assert geo.astype(np.float32).tobytes() == w.geometry().tobytes()
    changed = b.mps["min_dist"] != np.float32(7.25)
    want = np.zeros(len(b.mps), bool)
    want[ids] = True
    want[np.asarray([p for p in ids if not kw["observations"][p] or kw["ref_kf"][p] < 0], int)] = False
    assert np.array_equal(changed, want)
    if len(ids) > 1:  # no observations, no reference keyframe: the sentinels stay
        for p in (0, 20):
            assert (b.mps["normal"][p] == 7.5).all() and b.mps["max_dist"][p] == np.float32(7.125)
        assert len(kw["observations"][1]) == 1 and len(kw["observations"][2]) == 300
        assert kw["ref_kf"][10] not in kw["observations"][10]


def test_update_normal_and_depth_arrays_leave_the_rest():
    """The array entry: an empty row and ref_kf < 0 keep their in / out values,
    whatever their ref_level says."""
    rng = np.random.default_rng(0)
    info = S.small()["info"]
    pos = rng.uniform(1, 5, (3, 3)).astype(np.float32)
    Ow = rng.uniform(-1, 1, (4, 3)).astype(np.float32)
    nr, mn, mx = update_normal_and_depth(info, pos, [0, 0, 2, 5], [0, 1, 1, 2, 3], Ow, [0, -1, 3], [1, 99, 2],
                                         np.full((3, 3), 9.0, np.float32), np.full(3, 8.0, np.float32),
                                         np.full(3, 6.0, np.float32))
    assert (nr[:2] == 9).all() and (mn[:2] == 8).all() and (mx[:2] == 6).all()
    assert (nr[2] != 9).all() and 0 < mn[2] < mx[2]
    assert 0.3 < np.linalg.norm(nr[2]) <= 1.0001  # the mean of three unit vectors


# ------------------------------------------------------------- search_in_neighbors

def _rows(pts, exit_, kp, action, other):
    names = ("none", "add", "replace", "keep")
    return [(int(pts[i]), int(kp[i]), names[action[i]], int(other[i])) for i in np.nonzero(exit_ == X["fused"])[0]]


def assert_same_world(m, w, rep, r, cur, pts):
    """The LoopMap after search_in_neighbors and its report against the
    restatement's world and report."""
    assert rep["targets"] == r["targets"].tolist()
    assert len(rep["forward"]) == len(r["targets"])
    for j, f in enumerate(rep["forward"]):
        assert f["kf"] == r["targets"][j]
        assert f["rows"] == _rows(pts, r["f_exit"][j], r["f_kp"][j], r["f_action"][j], r["f_other"][j]), j
        assert f["nFused"] == r["nfused"][j]
    assert rep["candidates"] == r["cand"].tolist()
    assert rep["backward"]["rows"] == _rows(r["cand"], r["b_exit"], r["b_kp"], r["b_action"], r["b_other"])
    assert rep["backward"]["nFused"] == r["b_nfused"]
    assert rep["updated"] == list(dict.fromkeys(r["updated"].tolist()))
    for a, b in zip(m.slots, w.slots()):
        assert np.array_equal(a, b)
    assert np.array_equal(m.observation_rows(), w.observation_rows())
    bad, desc = w.points()
    assert np.array_equal(m.mp_bad, bad) and np.array_equal(m.mp_desc, desc)
    geo = np.concatenate([m.mps["pos"], m.mps["normal"], m.mps["min_dist"][:, None], m.mps["max_dist"][:, None]], 1)
    assert geo.astype(np.float32).tobytes() == w.geometry().tobytes()
    o, ow, wm, parent = w.connections(cur)
    assert (m.ordered[cur], m.ordered_w[cur], m.weights[cur], m.parent[cur]) == (o, ow, wm, parent)
    kf_marker, mp_marker = w.markers()
    assert np.array_equal(m.fuse_target_for, kf_marker) and np.array_equal(m.fuse_candidate_for, mp_marker)


def test_search_in_neighbors_against_the_restatement():
    sc = S.small()
    cur = sc["cur"]
    m, w = S.loop_map(sc), S.ref_world(sc)
    pts = sc["kf_mp"][cur].copy()
    rep = LM.search_in_neighbors(m, cur)
    r = w.search_in_neighbors(cur)
    assert_same_world(m, w, rep, r, cur, pts)
    # the scene makes the walk matter: searches redone after a descriptor change, some with another result
    assert rep["researched"] >= 3 and rep["research_changed"] >= 1 and rep["researched_in_call"] == 0
    assert len(rep["targets"]) > len(set(rep["targets"])) and S.BAD_KF not in rep["targets"]
    assert sum(f["nFused"] for f in rep["forward"]) > 300 and rep["backward"]["nFused"] > 100
    # a second call: no first neighbour is left unstamped, so nothing but the update pass runs
    before = ([s.copy() for s in m.slots], m.observation_rows(), m.mp_bad.copy(), m.fuse_candidate_for.copy())
    pts2 = m.slots[cur].copy()
    rep2 = LM.search_in_neighbors(m, cur)
    r2 = w.search_in_neighbors(cur)
    assert rep2["targets"] == [] and rep2["candidates"] == [] and rep2["forward"] == []
    assert rep2["backward"] == dict(rows=[], nFused=0) and rep2["researched"] == 0
    assert rep2["updated"] == rep["updated"]
    assert_same_world(m, w, rep2, r2, cur, pts2)
    assert all(np.array_equal(a, b) for a, b in zip(before[0], m.slots))
    assert np.array_equal(before[1], m.observation_rows()) and np.array_equal(before[2], m.mp_bad)
    assert np.array_equal(before[3], m.fuse_candidate_for)


def test_search_in_neighbors_where_tables_and_observations_disagree():
    """A slot table that holds a point whose observation map does not name the
    keyframe (docs/ORACLE_ASSUMPTIONS.md A26 does not promise they agree): the
    ``stale`` points lose the observation of one of the two neighbours that hold
    them. At that neighbour the fresh instance is replaced by the tracked one,
    whose descriptor changes inside the call, and the tracked one, listed later
    and not in the keyframe by its observations, is then searched with the new
    descriptor and meets itself in the slot (Replace of a point by itself)."""
    sc = dict(S.small())
    obs = [dict(o) for o in sc["observations"]]
    stale = [wi for wi, r in sc["roles"].items() if r == "stale"]
    cut = 0
    for p in np.nonzero(np.isin(sc["world"], stale))[0]:
        ks = [k for k in obs[p] if k != sc["cur"]]
        if len(ks) == 2:  # the tracked instance
            del obs[p][min(ks)]
            cut += 1
    assert cut == len(stale)
    sc["observations"] = obs
    cur = sc["cur"]
    m, w = S.loop_map(sc), S.ref_world(sc)
    pts = sc["kf_mp"][cur].copy()
    rep = LM.search_in_neighbors(m, cur)
    r = w.search_in_neighbors(cur)
    assert w.counter("same_id") >= 1  # the restatement met the case
    assert rep["researched_in_call"] >= 1
    assert_same_world(m, w, rep, r, cur, pts)


def test_fuse_search_chunk_setting():
    """gf_fuse_search_set_chunk: the result does not depend on it; a value
    outside [64, 65536] is refused and changes nothing."""
    sc = S.small()
    ctx = default_context()
    k, pts = 2, sc["kf_mp"][S.CUR]
    args = (sc["info"], sc["kf_kps"][k], sc["kf_desc"][k], sc["kf_Tcw"][k], pts, sc["mps"], sc["mp_desc"], sc["mp_bad"])
    want = fuse_search(*args)
    try:
        check(lib().gf_fuse_search_set_chunk(ctx.handle, 64))
        got = fuse_search(*args)
        assert lib().gf_fuse_search_set_chunk(ctx.handle, 63) != 0
        assert lib().gf_fuse_search_set_chunk(ctx.handle, (1 << 16) + 1) != 0
    finally:
        check(lib().gf_fuse_search_set_chunk(ctx.handle, FUSE_SEARCH_CHUNK_DEFAULT))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[0] >= 0).sum() > 50


def test_search_in_neighbors_after_create_new_map_points():
    """The two stages in a row on the localmap_scenes scene: the restatement
    starts from the world create_new_map_points left."""
    import localmap_scenes

    sc = localmap_scenes.scene()
    cur = sc["cur"]
    m = LoopMap(sc["info"], sc["kps"], sc["desc"], sc["slots"], sc["mps"], sc["mp_desc"], observations=sc["obs"],
                kf_Tcw=sc["Tcw"], ref_kf=sc["ref_kf"])
    m.ordered[cur] = list(sc["neighbours"])
    ids, _ = LM.create_new_map_points(m, cur, sc["fv"])
    assert len(ids) > 50
    w = RefWorld.from_loopmap(m)
    for k in range(m.nkf):  # the graph the new points imply, on both sides
        m.update_connections(k), w.update_connections(k)
    assert m.ordered[cur] == w.connections(cur)[0] and len(m.ordered[cur]) >= 2
    pts = m.slots[cur].copy()
    rep = LM.search_in_neighbors(m, cur)
    r = w.search_in_neighbors(cur)
    assert_same_world(m, w, rep, r, cur, pts)
    assert sum(f["nFused"] for f in rep["forward"]) + rep["backward"]["nFused"] > 20
    # the new points are no longer two-view points only
    assert max(len(m.obs[p]) for p in ids if not m.mp_bad[p]) > 2
