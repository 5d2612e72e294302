"""The Hamming matchers on contended, tie-heavy scenes against the sequential
CPU oracle, bit for bit: kp -> map-point claims, scores and counts.

The scenes (contended_scenes.py) are those test_contended_cpu.py proves
sensitive to the query order, distance ties, the ratio rule, the <= TH_HIGH
boundary and the rotation histogram; the cluster scenes also carry a result
derived by hand. They drive k_match's claim-resolution rounds, k_match_seq's
in-batch collisions and window rescans, k_active_match's holder invalidation
and the track-loss matchers of reloc.hip, which the random-descriptor scenes
of test_match_gpu / test_gf_gpu / test_track_loss_gpu leave almost idle."""
import ctypes

import numpy as np
import pytest

import contended_scenes as CS
import oracle_lib as O
import test_contended_cpu as T
from gf_orb_slam_amd import reloc, synth
from gf_orb_slam_amd._lib import check, lib, ptr
from gf_orb_slam_amd.matcher import MP_VIEW_DTYPE, Frame, FrameInfo, ORBmatcher
from gf_orb_slam_amd.observability import Observability, Rng
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE, default_context

pytestmark = pytest.mark.gpu


def _frame(kps, desc, info, Tcw, kp2mp, score):
    F = Frame(kps, desc, info, Tcw)
    F.mvpMapPoints[:], F.mvpMatchScore[:] = kp2mp, score
    return F


# ------------------------------------------------- SearchByProjection(F, map)
@pytest.mark.parametrize("cam,nmp,nkp,seed,ladder,th,ratio", T.PROJECT_CASES)
def test_projection_ladder_bit_exact(cam, nmp, nkp, seed, ladder, th, ratio):
    scene = T.project_scene(cam, nmp, nkp, seed, ladder)
    sc, info, views, kp2mp, score = scene
    F = _frame(sc["keypoints"], sc["descriptors"], info, sc["Tcw"], kp2mp, score)
    assert F.isInFrustum(sc["map"], 0.5).tobytes() == views.tobytes()
    ng = ORBmatcher(ratio).SearchByProjection(F, views, sc["mp_desc"], th)
    no, km, s = T.oracle_project(scene, th, ratio)
    assert ng == no and ng >= 50
    np.testing.assert_array_equal(F.mvpMapPoints, km)
    np.testing.assert_array_equal(F.mvpMatchScore, s)


@pytest.mark.parametrize("case", [T.PROJECT_CASES[0], T.PROJECT_CASES[2]])
def test_projection_budget_ladder(case):
    """SearchByProjection_Budget on ladder scenes: the claims of the full list
    and an IncreaseFound per new match."""
    *key, th, ratio = case
    scene = T.project_scene(*key)
    sc, info, views, kp2mp, score = scene
    F = _frame(sc["keypoints"], sc["descriptors"], info, sc["Tcw"], kp2mp, score)
    assert ORBmatcher(ratio).SearchByProjection_Budget(F, views, sc["mp_desc"], th, 0.0) == 0
    assert np.array_equal(F.mvpMapPoints, kp2mp)
    found = np.zeros(len(views), np.int32)
    ng = ORBmatcher(ratio).SearchByProjection_Budget(F, views, sc["mp_desc"], th, 5.0, found)
    no, km, s = T.oracle_project(scene, th, ratio)
    assert ng == no and np.array_equal(F.mvpMapPoints, km) and np.array_equal(F.mvpMatchScore, s)
    expect = np.zeros(len(views), np.int32)
    np.add.at(expect, km[(km >= 0) & (kp2mp < 0)], 1)
    assert np.array_equal(found, expect) and found.sum() == ng


# ------------------------------------------- SearchByProjection(Cur, Last, th)
def _device_lastframe(scene, th, ori):
    last, cur, info = scene
    F = _frame(cur.mvKeysUn, cur.mDescriptors, info, cur.mTcw, cur.mvpMapPoints, cur.mvpMatchScore)
    n = ORBmatcher(0.9, ori).SearchByProjectionLast(F, last, th)
    return n, F.mvpMapPoints, F.mvpMatchScore


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("seed,ladder,th", T.LAST_CASES)
def test_lastframe_ladder_bit_exact(seed, ladder, th, ori):
    scene = T.lastframe_scene(seed, ladder)
    ng, km_g, s_g = _device_lastframe(scene, th, ori)
    no, km, s = T.oracle_lastframe(scene, th, ori)
    assert ng == no and ng >= 50
    np.testing.assert_array_equal(km_g, km)
    np.testing.assert_array_equal(s_g, s)


# ------------------------------------------------------ runActiveMapMatching
@pytest.mark.parametrize("seed,ladder,ntm,th", T.ACTIVE_CASES)
def test_active_matching_ladder_bit_exact(seed, ladder, ntm, th):
    """test_gf_gpu._check_active with the window factor th on both sides:
    claims, scores, left-overs and the RNG position."""
    A = T.active_scene(seed, ladder)
    sc = A["sc"]
    F = _frame(sc["keypoints"], sc["descriptors"], A["fi"], sc["Tcw"], A["kp2mp"], A["score"])
    ob = Observability(A["cam"])
    ob.rng = Rng.seeded(seed)
    ng = ob.runActiveMapMatching(F, A["views"], sc["mp_desc"], A["updated"], A["info"], A["H"], A["uv"], A["base"],
                                 ntm, th, 0.8)
    no, km, s, left, calls = T.oracle_active(A, ntm, th, 0.8, seed)
    assert ng == no and ng > 0 and calls > 0
    np.testing.assert_array_equal(F.mvpMapPoints, km)
    np.testing.assert_array_equal(F.mvpMatchScore, s)
    np.testing.assert_array_equal(ob.mLeftMapPoints, left)
    ref = Rng.seeded(seed)  # the RNG advanced exactly as std::rand would have
    ref.next(calls)
    assert bytes(ob.rng) == bytes(ref)


# ------------------------------------------------- the track-loss matchers
@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("seed,ladder,window,min_level", T.WINDOW_CASES)
def test_window_search_ladder(seed, ladder, window, min_level, ori):
    a = T.window_args(T.reloc_scene(seed, ladder), window, min_level)
    n_d, out_d = reloc.window_search(T.RELOC_INFO, *a, check_ori=ori)
    n_o, out_o = O.window_search(T.RELOC_INFO, *a, check_ori=ori)
    assert n_d == n_o and (n_d >= 50 or ori)  # the orientation check leaves 40 of the 200 px scene's 111
    np.testing.assert_array_equal(out_d, out_o)


@pytest.mark.parametrize("seed,ladder,window", T.FRAMES_CASES)
def test_search_frames_ladder(seed, ladder, window):
    a = T.frames_args(T.reloc_scene(seed, ladder), seed, window)
    n_d, km_d, sc_d = reloc.search_frames(T.RELOC_INFO, *a)
    n_o, km_o, sc_o = O.search_frames(T.RELOC_INFO, *a)
    assert n_d == n_o and n_d >= 50
    np.testing.assert_array_equal(km_d, km_o)
    np.testing.assert_array_equal(sc_d, sc_o)


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("seed,ladder,th,orb_dist", T.KF_CASES)
def test_search_kf_projection_ladder(seed, ladder, th, orb_dist, ori):
    a = T.kf_args(T.reloc_scene(seed, ladder), seed, th, orb_dist)
    n_d, km_d, sc_d = reloc.search_kf_projection(T.RELOC_INFO, *a, check_ori=ori)
    n_o, km_o, sc_o = O.search_kf_projection(T.RELOC_INFO, *a, check_ori=ori)
    assert n_d == n_o and n_d >= 50
    np.testing.assert_array_equal(km_d, km_o)
    np.testing.assert_array_equal(sc_d, sc_o)


# ------------------------------------------------------------------ clusters
def _device_cluster_lastframe(S):
    info = FrameInfo.make(*S["camera"])
    cur = _frame(S["kps"], S["desc"], info, S["Tcw"], S["kp2mp"], S["score"])
    last = Frame(S["last_kps"], S["last_desc"], info)
    last.mvpMapPoints[:], last.mp_pos[:] = S["last_kp2mp"], S["last_pos"]
    n = ORBmatcher(0.9, True).SearchByProjectionLast(cur, last, S["th"])
    return n, cur.mvpMapPoints, cur.mvpMatchScore


def _device_cluster_project(S):
    info = FrameInfo.make(*S["camera"])
    F = _frame(S["kps"], S["desc"], info, np.eye(4, dtype=np.float32), S["kp2mp"], S["score"])
    n = ORBmatcher(0.8).SearchByProjection(F, S["views"], S["mp_desc"], S["th"])
    return n, F.mvpMapPoints, F.mvpMatchScore


@pytest.mark.parametrize("variant,preclaimed", CS.CLUSTER_VARIANTS)
@pytest.mark.parametrize("c", CS.CLUSTER_SIZES)
def test_cluster_in_candidate_order(c, variant, preclaimed):
    """c queries on one spot, every distance 0: query k takes the k-th
    unclaimed keypoint in candidate order. c >= 5 makes k_match_seq rescan (its
    four precomputed candidates are gone), 64 / 65 / 70 cross its 64-lane
    batch, 130 is a chain of 130 rounds in k_match."""
    for build, dev, orc in ((CS.cluster_lastframe, _device_cluster_lastframe, T.oracle_cluster_lastframe),
                            (CS.cluster_project, _device_cluster_project, T.oracle_cluster_project)):
        S = build(c, 2, variant, preclaimed)
        ng, km_g, s_g = dev(S)
        no, km, s = orc(S)
        assert ng == no == c, build.__name__
        np.testing.assert_array_equal(km_g, km, err_msg=build.__name__)
        np.testing.assert_array_equal(s_g, s, err_msg=build.__name__)
        np.testing.assert_array_equal(km_g, S["expect_kp2mp"], err_msg=build.__name__)
        np.testing.assert_array_equal(s_g, S["expect_score"], err_msg=build.__name__)


@pytest.mark.parametrize("plan,variant,preclaimed", T.ROTATION_CASES)
def test_cluster_rotation_histogram(plan, variant, preclaimed):
    """Known matches with planned rotations: ties between bins and the 0.1 rule
    of ComputeThreeMaxima at and below its boundary, against the oracle and
    the bins derived by hand."""
    S = CS.cluster_rotation(plan, variant, preclaimed)
    ng, km_g, s_g = _device_cluster_lastframe(S)
    no, km, s = T.oracle_cluster_lastframe(S, ori=True)
    assert ng == no == S["expect_n"]
    np.testing.assert_array_equal(km_g, km)
    np.testing.assert_array_equal(s_g, s)
    np.testing.assert_array_equal(km_g, S["expect_kp2mp"])
    np.testing.assert_array_equal(s_g, S["expect_score"])


@pytest.mark.parametrize("variant", ["one", "columns"])
@pytest.mark.parametrize("plan", list(CS.ROTATION_PLANS))
def test_window_search_cluster_rotation(plan, variant):
    """WindowSearch (reloc.hip) on the same clusters: claims in candidate
    order, then its own rotation histogram."""
    S = CS.cluster_rotation(plan, variant)
    info = FrameInfo.make(*S["camera"])
    a = T.window_cluster_args(S)
    n_d, out_d = reloc.window_search(info, *a, check_ori=True)
    n_o, out_o = O.window_search(info, *a, check_ori=True)
    assert n_d == n_o == S["expect_n"]
    np.testing.assert_array_equal(out_d, out_o)
    np.testing.assert_array_equal(out_d, S["expect_kp2mp"])


# ------------------------------------------------------------ batched launch
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")


def _back(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def test_project_dev_four_frames():
    """One gf_match_project_dev launch over a ladder scene, an empty frame, a
    cluster and a random-descriptor scene: every frame equals its single-frame
    result (no round state leaks between the frames' workgroups, no frame's
    early exit ends another's rounds), the padding stays untouched."""
    th, ratio = 5.0, 0.8
    ls = T.project_scene(*T.PROJECT_CASES[2][:5])
    cl = CS.cluster_project(70, 2, "columns", 5)
    pl = synth.synth_scene("euroc", 800, 600, 31)
    info = ls[1]
    plv, _ = O.frustum(info, pl["Tcw"], pl["map"])
    none_k, none_v = np.zeros(0, KEYPOINT_DTYPE), np.zeros(0, MP_VIEW_DTYPE)
    e32, ei = np.zeros((0, 32), np.uint8), np.zeros(0, np.int32)
    # keypoints, descriptors, views, map descriptors, kp2mp, score
    frames = [(ls[0]["keypoints"], ls[0]["descriptors"], ls[2], ls[0]["mp_desc"], ls[3], ls[4]),
              (none_k, e32, none_v, e32, ei, ei),
              (cl["kps"], cl["desc"], cl["views"], cl["mp_desc"], cl["kp2mp"], cl["score"]),
              (pl["keypoints"], pl["descriptors"], plv, pl["mp_desc"], np.full(600, -1, np.int32),
               np.full(600, 999, np.int32))]
    nf, kp_cap, mp_cap = len(frames), 608, 801
    K, D = np.zeros((nf, kp_cap), KEYPOINT_DTYPE), np.zeros((nf, kp_cap, 32), np.uint8)
    V, Q = np.zeros((nf, mp_cap), MP_VIEW_DTYPE), np.zeros((nf, mp_cap, 32), np.uint8)
    C, S = np.full((nf, kp_cap), -7, np.int32), np.full((nf, kp_cap), -7, np.int32)
    N, M = np.zeros(nf, np.int32), np.zeros(nf, np.int32)
    V["in_view"] = 1  # padding that would match if a kernel read past a frame's count
    for f, (k, d, v, q, c, s) in enumerate(frames):
        n, m = len(k), len(v)
        K[f, :n], D[f, :n], V[f, :m], Q[f, :m], C[f, :n], S[f, :n], N[f], M[f] = k, d, v, q, c, s, n, m
    dK, dD, dV, dQ, dC, dS, dN, dM = (_dev(a) for a in (K, D, V, Q, C, S, N, M))
    dO = _dev(np.full(nf, -1, np.int32))
    ctx = default_context()
    check(lib().gf_match_project_dev(ctx.handle, ctypes.byref(info), nf, ptr(dK), ptr(dD), ptr(dN), kp_cap, ptr(dV),
                                     ptr(dQ), ptr(dM), mp_cap, ctypes.c_float(th), ctypes.c_float(ratio), ptr(dC),
                                     ptr(dS), ptr(dO), ctx.stream))
    check(lib().gf_ctx_sync(ctx.handle))
    Cg, Sg, Og = _back(dC, np.int32, (nf, kp_cap)), _back(dS, np.int32, (nf, kp_cap)), _back(dO, np.int32, nf)
    for f, (k, d, v, q, c, s) in enumerate(frames):
        n = len(k)
        km, sc = c.copy(), s.copy()
        no = O.match_project(info, k, d, v, q, th, ratio, km, sc) if n else 0
        assert Og[f] == no, f
        np.testing.assert_array_equal(Cg[f, :n], km, err_msg=f"frame {f}")
        np.testing.assert_array_equal(Sg[f, :n], sc, err_msg=f"frame {f}")
        assert (Cg[f, n:] == -7).all() and (Sg[f, n:] == -7).all(), f
        if n:  # and the single-frame launch on the device
            F = _frame(k, d, info, np.eye(4, dtype=np.float32), c, s)
            assert ORBmatcher(ratio).SearchByProjection(F, v, q, th) == Og[f]
            np.testing.assert_array_equal(F.mvpMapPoints, Cg[f, :n])
            np.testing.assert_array_equal(F.mvpMatchScore, Sg[f, :n])
    np.testing.assert_array_equal(Cg[2, :len(cl["kps"])], cl["expect_kp2mp"])
    assert Og[0] >= 50 and Og[3] >= 50


def test_lastframe_dev_four_frames():
    """The same for gf_match_lastframe_dev (k_match_seq_pre + k_match_seq)."""
    th, ori = 15.0, 1
    last, cur, info = T.lastframe_scene(*T.LAST_CASES[0][:2])
    cl = CS.cluster_lastframe(70, 2, "columns", 5)
    pl_last, pl_cur, _ = CS.lastframe_pair(33)
    none_k, e32, ei = np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32)
    eye = np.eye(4, dtype=np.float32)

    def of(la, cu):
        return (cu.mvKeysUn, cu.mDescriptors, cu.mTcw, la.mvKeysUn, la.mDescriptors, la.mvpMapPoints, la.mvbOutlier,
                la.mp_pos, cu.mvpMapPoints, cu.mvpMatchScore)

    # keypoints, descriptors, Tcw, last: keypoints, descriptors, map points, outliers, positions; kp2mp, score
    frames = [of(last, cur),
              (none_k, e32, eye, none_k, e32, ei, np.zeros(0, np.uint8), np.zeros((0, 3), np.float32), ei, ei),
              (cl["kps"], cl["desc"], cl["Tcw"], cl["last_kps"], cl["last_desc"], cl["last_kp2mp"],
               cl["last_outlier"], cl["last_pos"], cl["kp2mp"], cl["score"]),
              of(pl_last, pl_cur)]
    nf, kp_cap, l_cap = len(frames), 608, 601
    K, D = np.zeros((nf, kp_cap), KEYPOINT_DTYPE), np.zeros((nf, kp_cap, 32), np.uint8)
    LK, LD = np.zeros((nf, l_cap), KEYPOINT_DTYPE), np.zeros((nf, l_cap, 32), np.uint8)
    LM, LO = np.full((nf, l_cap), 77, np.int32), np.zeros((nf, l_cap), np.uint8)
    LP = np.zeros((nf, l_cap, 3), np.float32)
    LP[:, :, 2] = 4.0  # padding that would match if a kernel read past a frame's count
    Tc = np.zeros((nf, 4, 4), np.float32)
    C, S = np.full((nf, kp_cap), -7, np.int32), np.full((nf, kp_cap), -7, np.int32)
    N, NL = np.zeros(nf, np.int32), np.zeros(nf, np.int32)
    for f, (k, d, t, lk, ld, lm, lo, lp, c, s) in enumerate(frames):
        n, m = len(k), len(lk)
        K[f, :n], D[f, :n], Tc[f], C[f, :n], S[f, :n], N[f] = k, d, t, c, s, n
        LK[f, :m], LD[f, :m], LM[f, :m], LO[f, :m], LP[f, :m], NL[f] = lk, ld, lm, lo, lp, m
    dK, dD, dT, dLK, dLD, dLM, dLO, dLP, dC, dS, dN, dNL = (_dev(a) for a in (K, D, Tc, LK, LD, LM, LO, LP, C, S, N,
                                                                              NL))
    dO = _dev(np.full(nf, -1, np.int32))
    dScr = _dev(np.zeros(nf * l_cap, np.int32))
    ctx = default_context()
    check(lib().gf_match_lastframe_dev(ctx.handle, ctypes.byref(info), nf, ptr(dK), ptr(dD), ptr(dN), kp_cap, ptr(dT),
                                       ptr(dLK), ptr(dLD), ptr(dLM), ptr(dLO), ptr(dLP), ptr(dNL), l_cap,
                                       ctypes.c_float(th), ori, ptr(dC), ptr(dS), ptr(dO), ptr(dScr), ctx.stream))
    check(lib().gf_ctx_sync(ctx.handle))
    Cg, Sg, Og = _back(dC, np.int32, (nf, kp_cap)), _back(dS, np.int32, (nf, kp_cap)), _back(dO, np.int32, nf)
    for f, (k, d, t, lk, ld, lm, lo, lp, c, s) in enumerate(frames):
        n = len(k)
        km, sc = c.copy(), s.copy()
        no = O.match_lastframe(info, k, d, t, lk, ld, lm, lo, lp, th, ori, km, sc) if n else 0
        assert Og[f] == no, f
        np.testing.assert_array_equal(Cg[f, :n], km, err_msg=f"frame {f}")
        np.testing.assert_array_equal(Sg[f, :n], sc, err_msg=f"frame {f}")
        assert (Cg[f, n:] == -7).all() and (Sg[f, n:] == -7).all(), f
        if n:  # and the single-frame launch on the device
            F = _frame(k, d, info, t, c, s)
            L = Frame(lk, ld, info)
            L.mvpMapPoints[:], L.mvbOutlier[:], L.mp_pos[:] = lm, lo, lp
            assert ORBmatcher(0.9, bool(ori)).SearchByProjectionLast(F, L, th) == Og[f]
            np.testing.assert_array_equal(F.mvpMapPoints, Cg[f, :n])
            np.testing.assert_array_equal(F.mvpMatchScore, Sg[f, :n])
    np.testing.assert_array_equal(Cg[2, :len(cl["kps"])], cl["expect_kp2mp"])
    assert Og[0] >= 50 and Og[3] >= 50
