"""The scenes of tests/ba_batch_scenes.py, held to their claims with the CPU
oracle alone (no GPU): tests/test_ba_batch_gpu.py compares the batched solver
with the oracle on them and asks for identical outlier flags, so no edge may
sit at the chi2 threshold, the schedule must really run, and every named
window must have the plan geometry it is named for.

Margin: the oracle returns float32 poses and points, so chi2 recomputed from
them in float64 carries about 1e-5 relative noise; the bound on the distance
from 5.991 is 1e-4 relative. A seed that falls under it is replaced on this
evidence only."""
import numpy as np

import ba_batch_scenes as S
import oracle_lib as O

CHI2 = 5.991
MARGIN = 1e-4
_cache = {}


def oracle(p, its):
    key = (p["name"], its)
    if key not in _cache:
        _cache[key] = O.local_ba(p, its=its)
    return _cache[key]


def windows():
    seen = {}
    for name in S.ALL:
        for p in S.batch(name):
            seen.setdefault(p["name"], p)
    return list(seen.values())


def chi2_of(p, T, X):
    """chi2 and depth of every edge at the estimate (T, X), in float64."""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    kf, pt = np.asarray(p["edge_kf"]), np.asarray(p["edge_pt"])
    pc = np.einsum("eij,ej->ei", T[kf, :3, :3], X[pt]) + T[kf, :3, 3]
    cam = np.asarray(p["kf_cam"], np.float64)[kf]
    z = np.asarray(p["edge_z"], np.float64)
    e0 = z[:, 0] - (pc[:, 0] / pc[:, 2] * cam[:, 0] + cam[:, 2])
    e1 = z[:, 1] - (pc[:, 1] / pc[:, 2] * cam[:, 1] + cam[:, 3])
    return np.asarray(p["edge_inv_sigma2"], np.float64) * (e0 * e0 + e1 * e1), pc[:, 2]


def test_margin_from_the_threshold_and_flags_recompute():
    worst = (np.inf, None)
    for p in windows():
        if not len(p["edge_pt"]):
            continue
        T5, X5, f5, _ = oracle(p, (5, 0))
        T, X, f, _ = oracle(p, (5, 10))
        removed = f5 != 0  # the first pass checks every edge at the optimize(5) state
        c5, z5 = chi2_of(p, T5, X5)
        c, z = chi2_of(p, T, X)
        assert np.array_equal((c5 > CHI2) | ~(z5 > 0), removed), p["name"]
        assert np.array_equal(((c > CHI2) | ~(z > 0))[~removed], (f != 0)[~removed]), p["name"]
        assert (f != 0)[removed].all(), p["name"]
        m = min(np.abs(c5 / CHI2 - 1).min(), np.abs(c[~removed] / CHI2 - 1).min() if (~removed).any() else np.inf)
        if m < worst[0]:
            worst = (m, p["name"])
        assert min(z5.min(), z[~removed].min() if (~removed).any() else np.inf) > 1e-3, p["name"]
    print("smallest chi2 margin", worst)
    assert worst[0] >= MARGIN, worst


def test_the_schedule_is_exercised():
    for name in S.ALL:
        nout = []
        for p in S.batch(name):
            if not len(p["edge_pt"]):
                assert oracle(p, (5, 10))[3] == (-1, -1), p["name"]
                continue
            f, its = oracle(p, (5, 10))[2:]
            assert its[0] == 5, (p["name"], its)  # the first round runs to its cap
            nout.append(int((f != 0).sum()))
        assert max(nout) > 0, name
        if name == "noisy":
            print("noisy outliers per window", nout)
            assert sum(nout) >= 10 * len(nout), nout


def test_no_window_is_an_exact_fit():
    """The stop rules compare chi2 differences with chi2 itself (1e-3 relative)
    and take the sign of rho. In a window with fewer residuals than unknowns
    chi2 falls to rounding noise and those decisions are noise; such a window
    cannot be held to equal iteration counts. Every window here has more
    residuals than unknowns and ends with a chi2 far above the 1e-10 that the
    float32 outputs leave of an exact fit."""
    for p in windows():
        if not len(p["edge_pt"]):
            continue
        col, _ = S.free_cols(p)
        nf = len({int(c) for c in col[p["edge_kf"]] if c >= 0})
        assert 2 * len(p["edge_pt"]) > 3 * np.unique(p["edge_pt"]).size + 6 * nf, p["name"]
        for its in ((5, 10), (20, 0)):
            T, X, _, _ = oracle(p, its)
            assert chi2_of(p, T, X)[0].sum() > 1e-3, (p["name"], its)


def test_batches_sit_on_both_sides_of_the_switch():
    want = {8: None, 9: 29, 16: 16, 64: 4, 255: 2, 256: 1, 300: 1}
    for n in S.SIZES:
        probs = S.batch(("size", n))
        assert len(probs) == n
        g = S.geometry(probs[0], n)
        assert g["sparse"] == (want[n] is None)
        if want[n]:
            assert g["nsplit"] == want[n]
    for name in S.GEOMETRY + ("placed_dense",):
        assert len(S.batch(name)) >= 9, name
    for name in S.ALL:  # a dropped last split must show: some window has a nonzero mask word in it
        probs = S.batch(name)
        gs = [S.geometry(p, len(probs)) for p in probs]
        assert gs[0]["sparse"] or any(g["mask"][(g["nsplit"] - 1) * g["sps"]:].any() for g in gs), name
    assert len(S.batch("placed_sparse")) == 8
    assert len(S.batch("pts_sps10")) == 64


def _find(name, win):
    """Geometry of window win inside batch name, and the batch size."""
    probs = S.batch(name)
    assert sum(p is win for p in probs) == 1  # the named window sits in that batch, once
    return S.geometry(win, len(probs)), len(probs)


def test_free_keyframe_counts():
    for nfree, name in ((0, "free_small"), (1, "free_small"), (2, "free_small"), (3, "free_small"),
                        (8, "free_mult16"), (16, "free_mult16"), (24, "free_mult16"), (32, "free_limit")):
        g, nb = _find(name, S.free_window(nfree))
        assert not g["sparse"] and g["nfree"] == nfree and g["n"] == 6 * nfree
        if nfree == 0:  # only the coefficient column
            assert g["npad"] == 16 and g["ntiles"] == 1 and not g["mask"].any()
        if nfree == 3:  # pose block 2 (columns 12-17) straddles tiles 0 and 1
            assert g["n"] == 18 and g["straddle"] and (g["mask"] == 3).any()
        if nfree in (8, 16, 24, 32):  # db alone in its tile column
            assert g["n"] % 16 == 0 and g["tdb"] == g["nt"] - 1 and g["npad"] == g["n"] + 16
            assert not (g["mask"] >> g["tdb"]).any()
        if nfree == 32:
            assert g["ntiles"] == 103 and g["lds"] == 107520
            assert max(S.geometry(p, nb)["npad"] for p in S.batch(name)) == 208
    assert all(len(p["pt_pos"]) <= 120 for p in windows() if p is not S.big_window())


def test_point_counts():
    g, _ = _find("pts_small", S.one_point_fixed())  # no free pose: every mask word 0, the product skips it
    assert not g["mask"].any() and g["steps"] == 1 and g["n"] == 0 and g["nsplit"] == 29 and g["sps"] == 1
    assert len(S.one_point_fixed()["pt_pos"]) == 1 and len(S.one_point_fixed()["edge_pt"]) >= 2
    # one point under a free pose: the smallest shape on which the dense product computes anything
    p = S.one_point_free()
    g, _ = _find("pts_small", p)
    assert len(p["pt_pos"]) == 1 and len(p["edge_pt"]) == 5 and g["nsplit"] == 29 and g["sps"] == 1
    assert g["steps"] == 1 and g["n"] == 6 and g["mask"][0] == 1 and not g["mask"][1:].any()
    g, _ = _find("pts_small", S.three_points())  # a pose tile over 3 k-steps
    assert g["steps"] == 3 and g["n"] == 6 and (g["mask"][:3] == 1).all() and not g["mask"][3:].any()
    g, _ = _find("pts_small", S.five_points())  # 4 k-steps for 29 splits: most splits see zero padding
    assert g["steps"] == 4 and g["nsplit"] == 29 and g["sps"] == 1 and g["mask"][:4].any() and not g["mask"][4:].any()
    for p in S.batch("pts_small")[3:6]:  # 5, 6, 7 points: a k-step holds rows of two points
        assert (3 * len(p["pt_pos"])) % 4 != 0
    for p in S.batch("pts_sps10"):
        g = S.geometry(p, 64)
        assert len(p["pt_pos"]) == 50 and g["steps"] == 38 and g["nsplit"] == 4 and g["sps"] == 10
        assert g["sps"] % S.BA_GCH == 2
    assert {S.geometry(p, 64)["nfree"] for p in S.batch("pts_sps10")} == {2, 3, 4, 5}
    g, _ = _find("pts_big", S.big_window())
    assert len(S.big_window()["pt_pos"]) == 320 and g["nsplit"] == 29 and g["sps"] == 9 > S.BA_GCH


def test_ragged_batch():
    probs = S.batch("ragged")
    gs = [S.geometry(p, len(probs)) for p in probs]
    assert not gs[0]["sparse"]
    assert sorted({g["npad"] for g in gs}) == [16, 32, 112, 208]
    assert gs[0]["nsplit"] == 22 and max(g["sps"] for g in gs) == 11 and min(g["sps"] for g in gs) == 1


def test_graph_shapes():
    probs = S.batch("graphs")
    nb = len(probs)
    assert nb >= 9
    # a free keyframe with no edge
    for p in (probs[1], probs[7]):
        col, nfree = S.free_cols(p)
        idle = [k for k in range(len(col)) if col[k] >= 0 and not (np.asarray(p["edge_kf"]) == k).any()]
        assert idle == [len(col) - 1] and S.geometry(p, nb)["n"] == 6 * nfree
    # a point with no edge
    p = probs[2]
    assert not (np.asarray(p["edge_pt"]) == 0).any() and np.unique(p["edge_pt"]).size == len(p["pt_pos"]) - 1
    # points seen by fixed keyframes only: k-steps with an all-zero mask before masked ones
    p = probs[3]
    g = S.geometry(p, nb)
    col, _ = S.free_cols(p)
    lone = [i for i in range(len(p["pt_pos"])) if (col[p["edge_kf"][p["edge_pt"] == i]] < 0).all()]
    assert len(lone) >= 3 and lone == list(range(len(lone)))
    assert not g["mask"][:(3 * len(lone)) // 4].any() and g["mask"][(3 * len(lone)) // 4:g["steps"]].all()
    assert np.all(np.diff(p["edge_pt"]) >= 0)
    # no keyframe and no point, in the middle; a window without an edge
    assert 0 < 4 < nb - 1 and len(probs[4]["kf_kind"]) == 0 and len(probs[4]["pt_pos"]) == 0
    assert len(probs[5]["edge_pt"]) == 0 and len(probs[5]["pt_pos"]) > 0 and S.geometry(probs[5], nb)["n"] > 0


def test_placement_batches():
    for name, pos in S.PLACEMENT:
        probs = S.batch(name)
        assert all(probs[i] is S.PLACED for i in pos) and pos[0] == 0 and pos[-1] == len(probs) - 1
        assert S.geometry(probs[0], len(probs))["sparse"] == (name == "placed_sparse")
        sizes = [(len(p["kf_kind"]), len(p["pt_pos"])) for p in probs]
        for a, b in zip(pos[:-1], pos[1:]):  # windows of other sizes in between
            assert any(s != sizes[0] for s in sizes[a + 1:b])
