"""The CPU restatement of Tracking::CreateInitialMap
(tests/helpers/initmap_ref.cpp) against brute-force numpy, line by line of the
reference (Tracking.cc:1126-1133, 1206-1249, 1268-1299; MapPoint.cc:285-324;
KeyFrame.cc:253-265, 659-689). No GPU: the restatement is what the device
stages are held to bit for bit in tests/test_initmap_gpu.py."""
import numpy as np
import pytest

import initmap_ref as R
import initmap_scenes as S
from gf_orb_slam_amd.matcher import camera_center
from gf_orb_slam_amd.optimizer import inv_level_sigma2

f32 = np.float32


def _norm(d):
    d = d.astype(np.float64)
    return f32(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def _normal_depth(X, T0, T1, level, info):
    """UpdateNormalAndDepth of one point seen by KFini and KFcur, mpRefKF = KFcur."""
    sf, scales = f32(info.scale_factor), info.scale_factors()
    nr = np.zeros(3, f32)
    for T in (T0, T1):
        d = X - camera_center(T)
        nr = nr + d * f32(1.0 / np.float64(_norm(d)))
    dist = _norm(X - camera_center(T1))
    return (nr * f32(0.5), ((f32(1.0) / sf) * dist) / scales[level], (sf * dist) * scales[info.nlevels - 1 - level])


def _expected_points(sc):
    """Stage 1 by numpy: (ids' keypoint pairs, slots1, slots2)."""
    m, tri = sc["matches12"], sc["tri"]
    keep = np.nonzero((m >= 0) & (tri != 0))[0]
    s1, s2 = np.full(len(sc["kps1"]), -1, np.int32), np.full(len(sc["kps2"]), -1, np.int32)
    for j, i in enumerate(keep):
        s1[i] = j
        s2[m[i]] = j
    return keep, s1, s2


@pytest.mark.parametrize("n1", [0, 1, 63, 64, 65, 130])
def test_points_ids_in_index_order(n1):
    sc = S.hand_made(10 + n1, n1)
    a = R.points(S.INFO, *S.args(sc))
    keep, s1, s2 = _expected_points(sc)
    assert a["status"] == R.OK and a["npts"] == len(keep)
    assert np.array_equal(a["pt_kp"][:, 0], keep) and np.array_equal(a["pt_kp"][:, 1], sc["matches12"][keep])
    assert np.array_equal(a["slots1"], s1) and np.array_equal(a["slots2"], s2)
    assert np.array_equal(a["mp_desc"], sc["desc1"][keep])  # the first observation's row: KFini's
    assert np.array_equal(a["mps"]["pos"], sc["p3d"][keep])
    T1 = np.eye(4, dtype=f32)
    T1[:3, :3], T1[:3, 3] = sc["init"]["R21"][0].reshape(3, 3), sc["init"]["t21"][0]
    assert a["ba"]["kf_Tcw"].tobytes() == np.stack([np.eye(4, dtype=f32), T1]).tobytes()
    assert a["ba"]["kf_kind"].tolist() == [1, 0]
    invs = inv_level_sigma2(S.INFO.nlevels, S.INFO.scale_factor)
    for j, i in enumerate(keep):
        i2 = sc["matches12"][i]
        nr, mn, mx = _normal_depth(sc["p3d"][i], np.eye(4, dtype=f32), T1, int(sc["kps2"]["octave"][i2]), S.INFO)
        assert a["mps"]["normal"][j].tobytes() == nr.tobytes()
        assert a["mps"]["min_dist"][j] == mn and a["mps"]["max_dist"][j] == mx
        assert a["ba"]["edge_pt"][2 * j:2 * j + 2].tolist() == [j, j]
        assert a["ba"]["edge_kf"][2 * j:2 * j + 2].tolist() == [0, 1]
        assert a["ba"]["edge_z"][2 * j].tolist() == [sc["kps1"]["x"][i], sc["kps1"]["y"][i]]
        assert a["ba"]["edge_z"][2 * j + 1].tolist() == [sc["kps2"]["x"][i2], sc["kps2"]["y"][i2]]
        assert a["ba"]["edge_inv_sigma2"][2 * j] == invs[sc["kps1"]["octave"][i]]
        assert a["ba"]["edge_inv_sigma2"][2 * j + 1] == invs[sc["kps2"]["octave"][i2]]


def test_slot_overwrite_with_a_duplicated_kfcur_index():
    """Two matches name one KFcur keypoint: the later point owns the slot, the
    tracked count drops by one per duplicate and both observations are kept."""
    sc = S.hand_made(5, 1000, nmatch=700, dup=3)
    a = R.points(S.INFO, *S.args(sc))
    keep, s1, s2 = _expected_points(sc)
    i2 = sc["matches12"][keep]
    dups = [v for v in np.unique(i2) if (i2 == v).sum() == 2]
    assert len(dups) == 3
    for v in dups:
        first, later = np.nonzero(i2 == v)[0]
        assert a["slots2"][v] == later
        assert a["pt_kp"][first, 1] == v and a["pt_kp"][later, 1] == v
    assert np.array_equal(a["slots2"], s2)
    T, X, _ = R.oracle_ba(a["ba"])
    b = R.finish(S.INFO, a, T, X)
    assert b["tracked"] == a["npts"] - 3 == int((a["slots2"] >= 0).sum())


@pytest.mark.parametrize("n", [7, 8])
def test_median_with_ties(n):
    """The element (n - 1) / 2 of the sorted depths, ties included, for odd and even n."""
    sc = S.hand_made(40 + n, n, nmatch=n, tri_frac=1.1, tie_depths=True)
    a = R.points(S.INFO, *S.args(sc))
    assert a["npts"] == n
    T, X = a["ba"]["kf_Tcw"].reshape(2, 4, 4), a["ba"]["pt_pos"].copy()
    z = np.sort(X[:, 2].copy())
    assert len(np.unique(z)) < n  # ties
    b = R.finish(S.INFO, a, T, X, thres=1)
    assert b["status"] == R.OK and b["median"] == z[(n - 1) // 2]
    inv = f32(1.0) / z[(n - 1) // 2]
    assert b["mps"]["pos"].tobytes() == (X * inv).astype(f32).tobytes()
    assert b["Tcw"][1][:3, 3].tobytes() == (T[1][:3, 3] * inv).astype(f32).tobytes()
    assert b["Tcw"][1][:3, :3].tobytes() == T[1][:3, :3].tobytes() and b["Tcw"][0].tobytes() == T[0].tobytes()


def test_statuses():
    sc = S.hand_made(3, 300, nmatch=250)
    a = R.points(S.INFO, *S.args(sc))
    T, X = a["ba"]["kf_Tcw"].reshape(2, 4, 4), a["ba"]["pt_pos"]
    assert a["npts"] >= 100
    assert R.finish(S.INFO, a, T, X)["status"] == R.OK
    assert R.finish(S.INFO, a, T, X, thres=a["npts"])["status"] == R.OK          # tracked == threshold
    assert R.finish(S.INFO, a, T, X, thres=a["npts"] + 1)["status"] == R.RESET_FEW
    neg = R.finish(S.INFO, a, T, -X)
    assert neg["status"] == R.RESET_DEPTH and neg["median"] < 0
    assert neg["mps"]["pos"].tobytes() == (-X).tobytes() and neg["Tcw"].tobytes() == T.tobytes()  # nothing scaled
    failed = S.hand_made(3, 300, nmatch=250, ok=0)
    a0 = R.points(S.INFO, *S.args(failed))
    assert a0["status"] == R.NOT_INITIALIZED and a0["npts"] == 0 and (a0["slots1"] == -1).all() and (a0["slots2"] == -1).all()
    assert R.finish(S.INFO, a0, None, None)["status"] == R.NOT_INITIALIZED
    none = S.hand_made(4, 50, nmatch=30, tri_frac=0.0)  # every match untriangulated
    assert (none["matches12"] >= 0).sum() == 30 and not none["tri"][none["matches12"] >= 0].any()
    a1 = R.points(S.INFO, *S.args(none))
    assert a1["status"] == R.OK and a1["npts"] == 0
    assert R.finish(S.INFO, a1, a1["ba"]["kf_Tcw"], np.zeros((0, 3), f32))["status"] == R.RESET_FEW


def test_distances_stay_unscaled_after_the_scaling():
    """UpdateNormalAndDepth runs before the median-depth scaling and is not
    repeated: normals and min / max distances are those of the unscaled points."""
    sc = S.hand_made(6, 200, nmatch=160)
    a = R.points(S.INFO, *S.args(sc))
    T, X = a["ba"]["kf_Tcw"].reshape(2, 4, 4), (a["ba"]["pt_pos"] * f32(1.01)).astype(f32)
    b = R.finish(S.INFO, a, T, X)
    assert b["status"] == R.OK and b["median"] != 1
    for j in range(a["npts"]):
        lvl = int(sc["kps2"]["octave"][a["pt_kp"][j, 1]])
        nr, mn, mx = _normal_depth(X[j], T[0], T[1], lvl, S.INFO)
        assert b["mps"]["normal"][j].tobytes() == nr.tobytes()
        assert b["mps"]["min_dist"][j] == mn and b["mps"]["max_dist"][j] == mx
    assert b["mps"]["pos"].tobytes() == (X * (f32(1.0) / b["median"])).astype(f32).tobytes()


@pytest.mark.parametrize("seed", [1, 2, 3, 5])
def test_end_to_end_on_the_initialiser(seed):
    """Restatement + oracle BA on the oracle initialiser's output: a map of
    252-268 points whose KFini median depth is 1 after the scaling."""
    a, b = R.create(S.INFO, *S.args(S.two_view(seed)))
    assert 252 <= a["npts"] <= 268 and b["status"] == R.OK and 12 <= b["ba_iterations"] <= 14
    z = np.sort(b["mps"]["pos"][:, 2])
    assert abs(z[(len(z) - 1) // 2] - 1.0) <= 1e-6
