"""LocalBundleAdjustment on a LoopMap, host side: the restatement
(tests/helpers/lbamap_ref.cpp) against a brute-force construction, the
driver's write-back against the restatement's with the oracle's local_ba as
the solver, and the threshold margin of the parity scenes."""
from __future__ import annotations

import numpy as np
import pytest

import lbamap_ref as R
import lbamap_scenes as S
import oracle_lib as O
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd.optimizer import inv_level_sigma2

CHI2 = 5.991
CASES = ("structural", "first_local", "empty", "parity")


def case_map(case):
    """-> (a fresh LoopMap, the current keyframe)."""
    if case == "parity":
        sc = S.parity()
        return S.parity_map(sc), sc["cur"]
    sc = S.structural()
    m = S.structural_map(sc, first_local=case == "first_local")
    return m, sc["names"]["EMPTY"] if case == "empty" else sc["cur"]


def brute_force(m, cur):
    """Optimizer.cc:1517-1675 read off the LoopMap with sets and sorts."""
    local = [cur] + [k for k in m.ordered[cur] if not m.kf_bad[k]]
    nmp = len(m.mps)
    walk = [int(p) for k in local for p in m.slots[k]]
    local_pts = list(dict.fromkeys(p for p in walk if 0 <= p < nmp and not m.mp_bad[p]))
    fixed = {k for p in local_pts for k in m.obs[p] if k not in local and not m.kf_bad[k]}
    prob_kf = sorted(set(local) | fixed)
    prob_pt = sorted(local_pts)
    kind = [2 if k in fixed else int(m.kf_id[k] == 0) for k in prob_kf]
    off = np.concatenate([[0], np.cumsum([len(k) for k in m.kf_kps])])
    inv = inv_level_sigma2(m.info.nlevels, m.info.scale_factor)
    edges = [(p, k, m.obs[p][k]) for p in local_pts for k in sorted(m.obs[p]) if not m.kf_bad[k]]
    g = dict(prob_kf=np.asarray(prob_kf, np.int32), kf_kind=np.asarray(kind, np.uint8),
             kf_Tcw=m.Tcw[prob_kf].reshape(-1, 16),
             kf_cam=np.tile(np.asarray([m.info.fx, m.info.fy, m.info.cx, m.info.cy], np.float32), (len(prob_kf), 1)),
             prob_pt=np.asarray(prob_pt, np.int32), pt_pos=m.mps["pos"][prob_pt].reshape(-1, 3),
             edge_pt=np.asarray([prob_pt.index(p) for p, _, _ in edges], np.int32),
             edge_kf=np.asarray([prob_kf.index(k) for _, k, _ in edges], np.int32),
             edge_z=np.asarray([(m.kf_kps[k]["x"][i], m.kf_kps[k]["y"][i]) for _, k, i in edges],
                               np.float32).reshape(-1, 2),
             edge_inv_sigma2=np.asarray([inv[m.kf_kps[k]["octave"][i]] for _, k, i in edges], np.float32),
             edge_gkp=np.asarray([off[k] + i for _, k, i in edges], np.int32))
    return g, local, sorted(fixed), local_pts


def assert_same_graph(a, b):
    for name in R.PROBLEM:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_brute_force(case):
    m, cur = case_map(case)
    w = R.RefWorld.from_loopmap(m)
    g = w.graph(cur, m.ordered[cur])
    want, local, fixed, local_pts = brute_force(m, cur)
    assert_same_graph(g, want)
    assert g["local_kfs"].tolist() == local and sorted(g["fixed_kfs"].tolist()) == fixed
    assert g["local_pts"].tolist() == local_pts
    O.local_ba(g)  # the oracle's validation accepts the problem


def test_structural_cases_are_planted():
    sc = S.structural()
    n, pts = sc["names"], sc["pts"]
    m = S.structural_map(sc)
    cur = sc["cur"]
    g, local, fixed, local_pts = brute_force(m, cur)
    assert len(local) == 32 and n["BADCOV"] in m.ordered[cur] and n["BADCOV"] not in local
    assert [len(m.slots[n[f"E{s}"]]) for s in S.EDGE_SIZES] == list(S.EDGE_SIZES)
    assert n["K0"] in fixed and g["kf_kind"][g["prob_kf"].tolist().index(n["K0"])] == 2
    assert np.count_nonzero(m.slots[n["L1"]] == pts["twice"]) == 2
    assert pts["dead"] in local_pts and pts["dead"] not in g["prob_pt"][g["edge_pt"]]  # a vertex without edges
    assert pts["badpt"] in m.slots[n["L1"]] and pts["badpt"] not in local_pts
    assert m.slots[n["L2"]][sc["slots_of"]["past"]] >= len(m.mps)
    assert len(m.obs[pts["long"]]) == 70 and pts["long"] in local_pts
    assert n["BADOBS"] in m.obs[pts["badobs"]] and n["BADOBS"] not in g["prob_kf"]
    unlisted = [p for p in m.slots[n["E4096"]] if 0 <= p < len(m.mps) and n["E4096"] not in m.obs[p]]
    assert unlisted
    first = {p: next(k for k in local if p in m.slots[k]) for p in local_pts}
    assert any(k != min(q for q in local if p in m.slots[q]) for p, k in first.items())
    # keyframe 0 as a local keyframe: the 32nd neighbour, kind 1
    m = S.structural_map(sc, first_local=True)
    g, local, fixed, _ = brute_force(m, cur)
    assert len(local) == 33 and g["kf_kind"][g["prob_kf"].tolist().index(n["K0"])] == 1
    # a current keyframe without points: two local keyframes' points, its own vertex without edges
    g, local, _, _ = brute_force(m, n["EMPTY"])
    assert local == [n["EMPTY"], n["L1"], n["L2"]] and n["EMPTY"] not in g["prob_kf"][g["edge_kf"]]


def dead_point_problem():
    """The structural graph and the problem index of ``dead``, the vertex without edges."""
    sc = S.structural()
    m = S.structural_map(sc)
    g = R.RefWorld.from_loopmap(m).graph(sc["cur"], m.ordered[sc["cur"]])
    q = g["prob_pt"].tolist().index(sc["pts"]["dead"])
    assert q not in g["edge_pt"]
    return g, q


def test_oracle_leaves_a_point_without_edges():
    g, q = dead_point_problem()
    _, X, _, its = O.local_ba(g)
    assert its[0] > 0 and X[q].astype(np.float32).tobytes() == g["pt_pos"][q].tobytes()
    assert np.all(np.isfinite(X))


def chi2_and_depth(g, T, X):
    """Every edge's chi2 and depth in numpy double from poses [nkf, 4, 4] and points [npts, 3]."""
    T, X = np.asarray(T, np.float64), np.asarray(X, np.float64)
    Te = T[g["edge_kf"]]
    c = np.einsum("eij,ej->ei", Te[:, :3, :3], X[g["edge_pt"]]) + Te[:, :3, 3]
    cam = np.asarray(g["kf_cam"], np.float64)[g["edge_kf"]]
    u = cam[:, 0] * c[:, 0] / c[:, 2] + cam[:, 2]
    v = cam[:, 1] * c[:, 1] / c[:, 2] + cam[:, 3]
    z = np.asarray(g["edge_z"], np.float64)
    return ((z[:, 0] - u) ** 2 + (z[:, 1] - v) ** 2) * np.asarray(g["edge_inv_sigma2"], np.float64), c[:, 2]


def assert_margin(m, cur):
    """No edge within 5 % of the chi2 threshold and no depth within 5 % of zero
    (against the scene's median depth) at either outlier check of the oracle."""
    w = R.RefWorld.from_loopmap(m)
    g = w.graph(cur, m.ordered[cur])
    T1, X1, f1, _ = O.local_ba(g, its=(5, 0))
    T2, X2, f2, its = O.local_ba(g, its=(5, 10))
    c1, d1 = chi2_and_depth(g, T1, X1)
    c2, d2 = chi2_and_depth(g, T2, X2)
    scale = np.median(d1)
    for c, d, keep in ((c1, d1, np.ones(len(c1), bool)), (c2, d2, f2 != 1)):
        assert np.all(np.abs(c[keep] / CHI2 - 1.0) > 0.05)
        assert np.all(np.abs(d[keep]) > 0.05 * scale)
    assert np.array_equal(f2 == 1, (c1 > CHI2) | (d1 <= 0))
    assert np.array_equal(f2 == 2, (f2 != 1) & ((c2 > CHI2) | (d2 <= 0)))
    return g, f2, its


def oracle_solver(g):
    return O.local_ba(g)


def run_both(sc, m):
    """The driver on ``m`` with the restatement's graph and the oracle's solver,
    and the restatement's write-back of the same result on its own world."""
    run, w = R.assembler(m)
    rep = LM.local_bundle_adjustment(m, sc["cur"], assembler=run, solver=oracle_solver)
    T, X, flags, _ = O.local_ba(rep["graph"])
    log = w.apply(flags, T, X)
    return rep, log, w


def test_parity_scene_margin():
    sc = S.parity()
    g, flags, its = assert_margin(S.parity_map(sc), sc["cur"])
    planted = sc["pts"]["outlier"] + sc["pts"]["turn_bad"]
    assert sorted(set(g["prob_pt"][g["edge_pt"][flags == 1]].tolist())) == sorted(planted)
    assert np.count_nonzero(flags == 1) == len(planted) and its[0] > 0
    assert set(np.unique(g["kf_kind"])) == {0, 2}


def test_writeback_equals_restatement():
    sc = S.parity()
    m = S.parity_map(sc)
    before = m.mps.copy()
    rep, log, w = run_both(sc, m)
    assert rep["stale_outliers"] == 0 and log["stale_outliers"] == 0
    for name in ("erased", "points_bad", "bad_round2"):
        assert rep[name] == log[name], name
    assert rep["erased"][0] == len(sc["pts"]["outlier"]) + len(sc["pts"]["turn_bad"])
    assert sorted(rep["points_bad"]) == sorted(sc["pts"]["turn_bad"])
    R.assert_same_state(m, w, skip_depth=rep["bad_round2"])
    for p in sc["pts"]["turn_bad"]:  # SetBadFlag cleared the other slots; the position is written all the same
        assert m.mp_bad[p] and not m.obs[p] and not any(np.any(s == p) for s in m.slots)
        assert not np.array_equal(m.mps["pos"][p], before["pos"][p])
        assert np.array_equal(m.mps["normal"][p], before["normal"][p])
    live = [p for p in rep["graph"]["prob_pt"] if not m.mp_bad[p]]
    assert np.any(m.mps["normal"][live] != before["normal"][live])
    assert rep["nedges"] == len(rep["flags"]) and rep["iterations"][0] > 0 and rep["iterations"][1] > 0


def test_stale_outlier_departure():
    """docs/ORACLE_ASSUMPTIONS.md A31: three observations, two gross outliers.
    The point turns bad at the first; the second is counted, not erased."""
    sc = S.parity(stale=True)
    m = S.parity_map(sc)
    p = sc["pts"]["stale"][0]
    assert len(m.obs[p]) == 3
    rep, log, w = run_both(sc, m)
    g, flags = rep["graph"], rep["flags"]
    assert np.count_nonzero(flags[g["prob_pt"][g["edge_pt"]] == p] == 1) == 2
    assert rep["stale_outliers"] == 1 and log["stale_outliers"] == 1
    assert p in rep["points_bad"] and rep["erased"] == log["erased"] and rep["points_bad"] == log["points_bad"]
    R.assert_same_state(m, w, skip_depth=rep["bad_round2"])


def test_no_edges_no_solve():
    sc = S.structural()
    m = S.structural_map(sc)
    lonely = sc["names"]["E0"]  # no points, and nothing in its ordered list
    m.weights[lonely], m.ordered[lonely], m.ordered_w[lonely] = {}, [], []
    run, w = R.assembler(m)

    def never(g):
        raise AssertionError("solved a problem without edges")

    rep = LM.local_bundle_adjustment(m, lonely, assembler=run, solver=never)
    assert rep["nedges"] == 0 and rep["npts"] == 0 and rep["iterations"] == (-1, -1) and rep["local_kfs"] == [lonely]


def test_table_lengths_are_checked():
    from gf_orb_slam_amd._lib import GFError

    sc = S.parity()
    t = LM.lba_tables(S.parity_map(sc))
    for name in ("octave", "kp_xy", "kf_bad", "mp_pos", "obs_off"):
        bad = dict(t)
        bad[name] = t[name][:-1]
        with pytest.raises(GFError) as e:
            LM._lba_struct(bad, bad)
        assert e.value.code == -1
