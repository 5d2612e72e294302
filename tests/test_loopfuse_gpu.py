"""SearchAndFuse on the device against the serial restatement
(tests/helpers/loopfuse_ref.cpp): the searches of gf_fuse_sim3 /
gf_fuse_sim3_dev candidate by candidate, and search_and_fuse's map afterwards.
Every compared value is an integer or a byte: no tolerance."""
import ctypes

import numpy as np
import pytest

import loopfuse_ref as R
import loopfuse_scenes as S
from gf_orb_slam_amd import sim3
from gf_orb_slam_amd._lib import check, lib, ptr
from gf_orb_slam_amd.loopmap import LoopMap
from gf_orb_slam_amd.orb import default_context
from gf_orb_slam_amd.sim3 import FUSE_SIM3_RESULT_DTYPE, FuseSim3Problem, fuse_sim3, search_and_fuse

pytestmark = pytest.mark.gpu


def _single(sc, kf, pts, th=4.0, mp_bad="scene"):
    bad = sc["mp_bad"] if isinstance(mp_bad, str) else mp_bad
    return fuse_sim3(sc["info"], sc["kf_kps"][kf], sc["kf_desc"][kf], sc["corrected"][kf], pts, sc["kf_mp"][kf],
                     sc["mps"], sc["mp_desc"], bad, th)


@pytest.mark.parametrize("kf", [0, 1, 2])
@pytest.mark.parametrize("th", [4.0, 2.5])
def test_fuse_sim3_equals_restatement_small(kf, th):
    sc = S.small()
    kp, dist = _single(sc, kf, sc["loop_points"], th)
    o = R.RefMap(*S.map_args(sc)).fuse(kf, sc["corrected"][kf], sc["loop_points"], th)
    assert np.array_equal(kp, o["kp"]) and np.array_equal(dist, o["dist"])
    assert (kp >= 0).sum() > 50


def test_fuse_sim3_edge_shapes():
    """n = 1000 against 1500 candidates (six workgroups, the last one partly
    filled), a list of one, an empty list, a keyframe without keypoints, no
    bad array."""
    sc = S.edges()
    ref = R.RefMap(*S.map_args(sc))
    pts = sc["loop_points"]
    kp, dist = _single(sc, 0, pts)
    o = ref.fuse(0, sc["corrected"][0], pts, 4.0)
    assert np.array_equal(kp, o["kp"]) and np.array_equal(dist, o["dist"]) and (kp >= 0).sum() > 300
    hit = int(np.nonzero(kp >= 0)[0][-1])
    for sub in (pts[hit:hit + 1], pts[:1], pts[:257], pts[:0]):
        k1, d1 = _single(sc, 0, sub)
        o1 = ref.fuse(0, sc["corrected"][0], sub, 4.0)
        assert np.array_equal(k1, o1["kp"]) and np.array_equal(d1, o1["dist"]) and len(k1) == len(sub)
    k0, d0 = _single(sc, 1, pts)
    assert (k0 == -1).all() and (d0 == -1).all() and len(k0) == 1500
    assert sc["mp_bad"].sum() == 0
    kn, dn = _single(sc, 0, pts, mp_bad=None)
    assert np.array_equal(kn, kp) and np.array_equal(dn, dist)


def test_fuse_sim3_rejects_bad_arguments():
    from gf_orb_slam_amd._lib import GFError

    sc = S.small()
    with pytest.raises(GFError):
        _single(sc, 0, np.array([len(sc["mps"])], np.int32))
    with pytest.raises(GFError):
        fuse_sim3(sc["info"], sc["kf_kps"][0], sc["kf_desc"][0], sc["corrected"][0], sc["loop_points"],
                  np.full(len(sc["kf_kps"][0]), len(sc["mps"]), np.int32), sc["mps"], sc["mp_desc"], sc["mp_bad"])


def test_fuse_sim3_dev_ragged_batch_equals_single_calls():
    import torch

    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sc = S.small()
    pts = sc["loop_points"]
    lists = [pts, pts[:300][::-1].copy(), pts[:0], pts[100:101], pts[:257]]
    kfs = [0, 1, 2, 2, 5]  # different n; 5 is a loop-side keyframe: any keyframe can be searched
    scw = [sc["corrected"][k] if k in sc["corrected"] else sc["corrected"][0] for k in kfs]
    d_mps, d_md, d_bad = t(sc["mps"].view(np.uint8)), t(sc["mp_desc"]), t(sc["mp_bad"].astype(np.uint8))
    keep, probs, outs = [], [], []
    for k, lst, S_ in zip(kfs, lists, scw):
        bufs = [t(sc["kf_kps"][k].view(np.uint8)), t(sc["kf_desc"][k]), t(sc["kf_mp"][k]),
                t(lst) if len(lst) else None,
                torch.full((max(len(lst), 1) * 2,), 7, dtype=torch.int32, device=dev)]
        keep += bufs
        outs.append(bufs[4])
        probs.append(FuseSim3Problem.make(S_, bufs[0], bufs[1], len(sc["kf_kps"][k]), bufs[2], bufs[3], len(lst), 4.0,
                                          bufs[4]))
    arr = (FuseSim3Problem * len(probs))(*probs)
    ctx = default_context()
    check(lib().gf_fuse_sim3_dev(ctx.handle, ctypes.byref(sc["info"]), len(probs), arr, ptr(d_mps), ptr(d_md),
                                 ptr(d_bad), len(sc["mps"]), ctx.stream))
    ctx.sync()
    for k, lst, S_, r in zip(kfs, lists, scw, outs):
        got = r.cpu().numpy()[:2 * len(lst)].view(FUSE_SIM3_RESULT_DTYPE)
        kp, dist = fuse_sim3(sc["info"], sc["kf_kps"][k], sc["kf_desc"][k], S_, lst, sc["kf_mp"][k], sc["mps"],
                             sc["mp_desc"], sc["mp_bad"], 4.0)
        want = np.zeros(len(lst), FUSE_SIM3_RESULT_DTYPE)
        want["kp"], want["dist"] = kp, dist
        assert got.tobytes() == want.tobytes()
    assert (outs[2].cpu().numpy() == 7).all()  # the empty problem wrote nothing


def _ref_run(sc):
    ref = R.RefMap(*S.map_args(sc))
    kfs = sc["cur"]
    return ref, ref.search_and_fuse(kfs, np.stack([sc["corrected"][k] for k in kfs]), sc["loop_points"], 4.0)


def _ref_actions(sc, o):
    out = {}
    for j, k in enumerate(sc["cur"]):
        idx = np.nonzero(o["action"][j] != 0)[0]
        out[k] = [(int(sc["loop_points"][i]), int(o["kp"][j][i]), R.ACTIONS[o["action"][j][i]], int(o["replaced"][j][i]))
                  for i in idx]
    return out


def _same_map(lm, ref):
    for a, b in zip(lm.slots, ref.slots()):
        assert np.array_equal(a, b)
    bad, d = ref.points()
    assert np.array_equal(lm.mp_bad, bad)
    assert np.array_equal(lm.mp_desc, d)
    assert np.array_equal(lm.observation_rows(), ref.observation_rows())


def test_search_and_fuse_equals_restatement():
    sc = S.small()
    lm = LoopMap(*S.map_args(sc))
    got = search_and_fuse(lm, sc["corrected"], sc["loop_points"], 4.0)
    ref, o = _ref_run(sc)
    assert [got["nFused"][k] for k in sc["cur"]] == list(o["nFused"])
    assert got["actions"] == _ref_actions(sc, o)
    _same_map(lm, ref)
    kinds = {a[2] for acts in got["actions"].values() for a in acts}
    assert kinds == {"add", "replace", "keep"}


def _sequential(lm, corrected, pts, th):
    """SearchAndFuse the slow way: one fuse_sim3 call per keyframe at its turn,
    against the map the previous keyframes left."""
    out = dict(nFused={}, actions={})
    for k in sorted(corrected):
        kp, _ = fuse_sim3(lm.info, lm.kf_kps[k], lm.kf_desc[k], corrected[k], pts, lm.slots[k], lm.mps, lm.mp_desc,
                          lm.mp_bad, th)
        acts = []
        for i, p in enumerate(int(x) for x in pts):
            # the call's skip set is in kp already; a point turned bad inside the call is caught here
            if kp[i] < 0 or lm.mp_bad[p]:
                continue
            idx = int(kp[i])
            occ = int(lm.slots[k][idx])
            if occ >= 0:
                if not lm.mp_bad[occ]:
                    lm.replace(occ, p)
                    acts.append((p, idx, "replace", occ))
                else:
                    acts.append((p, idx, "keep", occ))
            else:
                lm.add_observation(p, k, idx)
                lm.add_map_point(k, p, idx)
                acts.append((p, idx, "add", -1))
        out["nFused"][k], out["actions"][k] = len(acts), acts
    return out


def test_search_and_fuse_equals_sequential_calls():
    sc = S.small()
    a, b = LoopMap(*S.map_args(sc)), LoopMap(*S.map_args(sc))
    got = search_and_fuse(a, sc["corrected"], sc["loop_points"], 4.0)
    want = _sequential(b, sc["corrected"], sc["loop_points"], 4.0)
    assert got == want
    for x, y in zip(a.slots, b.slots):
        assert np.array_equal(x, y)
    assert np.array_equal(a.mp_bad, b.mp_bad) and np.array_equal(a.mp_desc, b.mp_desc)
    assert np.array_equal(a.observation_rows(), b.observation_rows())


def test_stale_descriptors_change_the_result(monkeypatch):
    """Without the second search of the candidates whose descriptor changed,
    the planted case (g) takes the keypoint its launch-time descriptor likes."""
    sc = S.small()
    monkeypatch.setattr(sim3, "_dirty", lambda map, pts, used: np.zeros(len(pts), bool))
    lm = LoopMap(*S.map_args(sc))
    got = search_and_fuse(lm, sc["corrected"], sc["loop_points"], 4.0)
    ref, o = _ref_run(sc)
    assert got["actions"] != _ref_actions(sc, o)
    stale = {(k, a[0]): a[1] for k, acts in got["actions"].items() for a in acts}
    g = (o["exit"] == R.X["fused"]) & (o["stale_kp"] >= 0) & (o["stale_kp"] != o["kp"])
    planted = np.isin(sc["loop_points"], sc["roles"]["g"])
    j, i = next((int(j), int(i)) for j, i in zip(*np.nonzero(g & planted)) if j == 1)
    assert stale[(sc["cur"][j], int(sc["loop_points"][i]))] == o["stale_kp"][j, i] != o["kp"][j, i]


POSE_RTOL = 1e-5  # the project's pose tolerance (tests/test_essgraph_gpu.py): |d| <= 1e-5 * max(1, |x|) per entry


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def _sim_map(S, x):
    """g2o::Sim3::map in double: s * (q * x) + t, the quaternion product as uv = 2 (q x v), v + w uv + q x uv."""
    q, w = S[:3], S[3]
    uv = 2.0 * np.cross(q, x)
    return S[7] * (x + w * uv + np.cross(q, uv)) + S[4:7]


def _loop_case():
    """The small map with poses: the current side (keyframes 0-2) carries a
    scale drift of 1.3 in its translations, so that the propagated corrected
    similarities are the scene's s * [R | t]."""
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.optimizer import quat_from_R

    sc = S.small()
    rng = np.random.default_rng(9)
    T = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    for k in sc["cur"]:
        T[k, :3, :3] = (sc["corrected"][k][:3, :3].astype(np.float64) / 1.3).astype(np.float32)
        T[k, :3, 3] = sc["corrected"][k][:3, 3]
    for k in sc["loopkf"]:
        T[k] = synth.look_pose(rng, 0.3, 3.0)
    cur, matched_kf = 2, 5
    gScw = np.zeros(8)
    gScw[:4] = quat_from_R(T[cur][:3, :3])
    gScw[4:7], gScw[7] = T[cur][:3, 3].astype(np.float64), 1.3
    # mvpCurrentMatchedPoints: loop points the current keyframe would fuse with, one per keypoint
    o = R.RefMap(*S.map_args(sc)).fuse(cur, sc["corrected"][cur], sc["loop_points"], 4.0)
    matched = np.full(len(sc["kf_kps"][cur]), -1, np.int32)
    for i in np.nonzero(o["kp"] >= 0)[0][:80]:
        if matched[o["kp"][i]] < 0:
            matched[o["kp"][i]] = sc["loop_points"][i]
    return sc, T, cur, matched_kf, gScw, matched


def test_correct_loop_end_to_end(capsys):
    import essgraph_ref as E
    from gf_orb_slam_amd.optimizer import sim3_from_g2o
    from gf_orb_slam_amd.sim3 import correct_loop

    sc, T0, cur, matched_kf, gScw, matched = _loop_case()
    lm = LoopMap(*S.map_args(sc), kf_Tcw=T0)
    ref = R.RefMap(*S.map_args(sc))
    ref.set_scale_factor(sc["info"].scale_factor)
    n = len(sc["mps"])
    for k in range(6):
        lm.update_connections(k), ref.update_connections(k), ref.set_pose(k, T0[k])
    for p in range(n):
        ref.set_ref(p, lm.ref_kf[p])
    ref_kf, bad0 = lm.ref_kf.copy(), lm.mp_bad.copy()
    got = correct_loop(lm, cur, matched_kf, gScw, matched, sc["loop_points"])

    # ---- the restatement, chained by hand (LoopClosing.cc:426-560)
    T = T0.copy()
    ref.update_connections(cur)
    connected = ref.connections(cur)[0] + [cur]
    assert sorted(connected) == [0, 1, 2]
    Tc = T[cur]
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = Tc[:3, :3].T
    Twc[:3, 3] = -(Tc[:3, :3].T @ Tc[:3, 3])
    non, cor = {}, {cur: gScw.copy()}
    for i in connected:
        if i != cur:
            cor[i] = E.sim_mul(E.sim_from_pose((T[i] @ Twc).astype(np.float32)), gScw)
        non[i] = E.sim_from_pose(T[i])
    slots = ref.slots()
    geo = ref.geometry()
    corrected_ref = np.full(n, -1, np.int32)
    for k in sorted(cor):
        inv = E.sim_inverse(cor[k])
        mine = []
        for p in slots[k]:
            if p < 0 or bad0[p] or corrected_ref[p] >= 0:
                continue
            ref.set_pos(p, _sim_map(inv, _sim_map(non[k], geo[p, :3].astype(np.float64))).astype(np.float32))
            corrected_ref[p] = k
            mine.append(int(p))
        ref.update_normal_and_depth(mine)
        s, Rm, t = sim3_from_g2o(cor[k])
        T[k] = np.eye(4, dtype=np.float32)
        T[k, :3, :3] = Rm.astype(np.float32)
        T[k, :3, 3] = (t * (1.0 / s)).astype(np.float32)
        ref.set_pose(k, T[k])
        ref.update_connections(k)
    ref.loop_fusion(cur, matched)
    keys = sorted(cor)
    Scw = []
    for k in keys:
        s, Rm, t = sim3_from_g2o(cor[k])
        M = np.eye(4, dtype=np.float32)
        M[:3, :3], M[:3, 3] = (s * Rm).astype(np.float32), t.astype(np.float32)
        Scw.append(M)
    o = ref.search_and_fuse(keys, np.stack(Scw), sc["loop_points"], 4.0)
    LC = ref.loop_connections(connected)
    conn = [ref.connections(k) for k in range(6)]
    bad, _ = ref.points()
    emap = dict(kf_id=np.arange(6), Tcw=T, parent=[c[3] for c in conn], cov=[(c[0], c[1]) for c in conn],
                loop_edges=[[] for _ in range(6)], pos=ref.geometry()[:, :3], bad=bad, ref=ref_kf,
                corrected_ref=corrected_ref)
    want = E.solve((emap, matched_kf, cur, non, cor, LC))

    # ---- integers: equal
    assert got["LoopConnections"] == LC and any(LC.values())
    assert [got["fuse"]["nFused"][k] for k in keys] == list(o["nFused"]) and sum(o["nFused"]) > 100
    sc2 = dict(sc, cur=keys)
    assert got["fuse"]["actions"] == _ref_actions(sc2, o)
    _same_map(lm, ref)
    for k in range(6):
        assert (lm.ordered[k], lm.ordered_w[k], lm.weights[k], lm.parent[k]) == conn[k], k
    assert np.array_equal(lm.corrected_ref, corrected_ref)
    assert lm.loop_edges[cur] == [matched_kf] and lm.loop_edges[matched_kf] == [cur]
    # ---- poses and points: the project's 1e-5 relative
    e_T, e_X = _rel(got["Tcw"], want["Tcw"]), _rel(got["pos"][~bad], want["pos"][~bad])
    with capsys.disabled():
        print(f"\ncorrect_loop vs restatement: worst relative error poses {e_T:.3g}, points {e_X:.3g}; "
              f"{got['iterations']} iterations, {sum(o['nFused'])} fused")
    assert got["iterations"] == want["iterations"] and got["chi2_initial"] > 0
    assert not np.array_equal(got["Tcw"][keys], T[keys])  # the optimiser moved the corrected keyframes
    assert e_T <= POSE_RTOL and e_X <= POSE_RTOL
    assert np.array_equal(lm.Tcw, got["Tcw"]) and np.array_equal(lm.mps["pos"][~bad], got["pos"][~bad])
    # the final UpdateNormalAndDepth ran against the optimised poses: the restatement's, fed the device's result
    for k in range(6):
        ref.set_pose(k, got["Tcw"][k])
    for p in np.nonzero(~bad)[0]:
        ref.set_pos(p, got["pos"][p])
    ref.update_normal_and_depth(np.nonzero(~bad)[0])
    g = ref.geometry()
    obs_ok = ~bad & np.asarray([bool(o_) for o_ in lm.obs]) & (lm.ref_kf >= 0)
    assert np.array_equal(lm.mps["normal"][obs_ok], g[obs_ok, 3:6])
    assert np.array_equal(lm.mps["min_dist"][obs_ok], g[obs_ok, 6])
