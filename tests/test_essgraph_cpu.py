"""The CPU restatement of Optimizer::OptimizeEssentialGraph
(tests/helpers/essgraph_ref.cpp) pinned on its own: a closed form, the fixed
point, the edge rules against a literal reading of Optimizer.cc:1832-1957, the
numeric Jacobian against extended precision, Sim3::log, and the scenes the GPU
tests rely on."""
import numpy as np
import pytest

import essgraph_ref as R
import essgraph_scenes as S

LD = np.longdouble


# ------------------------------------------------------------------ closed form
# worst |log(|p'| / |p|) - expected| the restatement shows (float32 point output):
# 3.6e-8 at M = 7, 5.8e-8 at M = 40; the bound is 4 x the larger
CLOSED_FORM_WORST = 5.8e-8


@pytest.mark.parametrize("M", [7, 40])
def test_closed_form_scale_chain(M):
    D = 0.3
    sc = S.scale_chain(M, D)
    out = R.solve(sc)
    p0 = np.asarray(sc[0]["pos"], np.float64)
    got = np.log(np.linalg.norm(out["pos"].astype(np.float64), axis=1) / np.linalg.norm(p0, axis=1))
    after = np.arange(M + 1) * D / (M + 1)  # keyframe i ends at the log scale i D / (M + 1)
    before = np.zeros(M + 1)
    before[M] = D  # vScw of the corrected current keyframe
    err = np.abs(got - (before - after)).max()
    print(f"M={M}: worst log-scale error {err:.3e}, iterations {out['iterations']}, trials {out['trials']}, "
          f"chi2 {out['chi2_initial']!r} -> {out['chi2_final']!r}")
    assert err <= 4 * CLOSED_FORM_WORST
    # nothing else moves: identity poses (t / s with t = 0), point directions kept
    assert np.array_equal(out["Tcw"], np.asarray(sc[0]["Tcw"], np.float32))
    d0 = p0 / np.linalg.norm(p0, axis=1)[:, None]
    d1 = out["pos"] / np.linalg.norm(out["pos"], axis=1)[:, None]
    assert np.abs(d1 - d0).max() <= 2e-7
    assert out["chi2_final"] == pytest.approx(D * D / (M + 1), rel=1e-12)


# ------------------------------------------------------------------ fixed point
def _axis_scene():
    """Poses whose Sim3 arithmetic is exact: identity rotations and dyadic translations."""
    N = 12
    Tcw = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    for i in range(N):
        Tcw[i, :3, 3] = [0.5 * i, -0.25 * i, 0.125 * (i % 3)]
    cov = [([j for j in (i - 1, i + 1) if 0 <= j < N], [150] * len([j for j in (i - 1, i + 1) if 0 <= j < N]))
           for i in range(N)]
    pos = np.array([[0.5 * k, 1.0 + 0.25 * k, 2.0] for k in range(20)], np.float32)
    m = dict(kf_id=np.arange(N), Tcw=Tcw, parent=np.arange(-1, N - 1), cov=cov, loop_edges=[[] for _ in range(N)],
             pos=pos, bad=np.arange(20) % 7 == 0, ref=np.arange(20) % N, corrected_ref=np.full(20, -1))
    non = {i: R.sim_from_pose(Tcw[i]) for i in (N - 2, N - 1)}
    return (m, 1, N - 1, non, {k: v.copy() for k, v in non.items()}, {N - 1: [1]})


def test_fixed_point_exact():
    """CorrectedSim3 == NonCorrectedSim3 on poses with exact arithmetic: chi2 is
    0, the first iteration ends on rho == 0, everything comes back."""
    sc = _axis_scene()
    out = R.solve(sc)
    assert out["chi2_initial"] == 0.0 and out["chi2_final"] == 0.0
    assert (out["iterations"], out["trials"], out["stop"]) == (1, 1, 1)
    assert np.abs(out["Tcw"] - sc[0]["Tcw"]).max() <= 1e-6
    assert np.abs(out["pos"] - sc[0]["pos"]).max() <= 1e-6


def test_fixed_point_float_poses():
    """The same on a drifted map. The float poses give quaternions that are unit
    only to float rounding and g2o::Sim3 never normalises, so the residuals are
    of the order 1e-7 |t| (chi2 about 1e-12 over some sixty edges, not 0) and the
    Levenberg loop runs on rounding noise; poses and points still come back
    within float rounding of the input."""
    m, loop, cur, non, _, lc = S.make_scene(26, 5)
    out = R.solve((m, loop, cur, non, {k: v.copy() for k, v in non.items()}, lc))
    print(f"fixed point: chi2 {out['chi2_initial']:.3e} -> {out['chi2_final']:.3e}, "
          f"iterations {out['iterations']}, pose diff {np.abs(out['Tcw'] - m['Tcw']).max():.3e}")
    # 64 edges x 7 components x (6e-8 x |t| <= 6)^2
    assert out["chi2_initial"] <= 64 * 7 * (6e-8 * 6) ** 2
    assert np.abs(out["Tcw"] - m["Tcw"]).max() <= 4e-6
    live = ~np.asarray(m["bad"], bool)
    assert np.abs(out["pos"] - m["pos"])[live].max() <= 4e-6


# ------------------------------------------------------------------ edge rules
def literal_edges(map_, loop_kf, cur_kf, LoopConnections):
    """Optimizer.cc:1832-1957 read literally, sets and maps in id order."""
    ids = [int(v) for v in map_["kf_id"]]
    N = len(ids)
    minFeat = 100
    weight = [{int(n): int(w) for n, w in zip(*map_["cov"][i])} for i in range(N)]
    rows, inserted = [], set()
    for i in sorted(LoopConnections, key=lambda k: ids[k]):
        for j in sorted(set(LoopConnections[i]), key=lambda k: ids[k]):
            if (ids[i] != ids[cur_kf] or ids[j] != ids[loop_kf]) and weight[i].get(j, 0) < minFeat:
                continue
            rows.append((i, j, 0))
            inserted.add((min(ids[i], ids[j]), max(ids[i], ids[j])))
    for i in range(N):
        parent = int(map_["parent"][i])
        if parent >= 0:
            rows.append((i, parent, 1))
        loop_edges = sorted(set(int(v) for v in map_["loop_edges"][i]), key=lambda k: ids[k])
        for l in loop_edges:
            if ids[l] < ids[i]:
                rows.append((i, l, 2))
        nbrs, ws = map_["cov"][i]
        for n, w in zip(nbrs, ws):
            if w < minFeat:  # GetCovisiblesByWeight(minFeat)
                break
            n = int(n)
            has_child = int(map_["parent"][n]) == i
            if n != parent and not has_child and n not in loop_edges:
                if ids[n] < ids[i]:
                    if (min(ids[i], ids[n]), max(ids[i], ids[n])) in inserted:
                        continue
                    rows.append((i, n, 3))
    return np.asarray(rows, np.int32).reshape(-1, 3)


def _hand_graph(gaps=False):
    """7 keyframes; loop keyframe 1, current keyframe 6."""
    N = 7
    W = {(0, 1): 180, (1, 2): 170, (2, 3): 160, (3, 4): 150, (4, 5): 140, (5, 6): 130,  # the chain: parents
         (0, 2): 120,   # plain covisibility edge 2 -> 0
         (0, 3): 90,    # below 100: nothing
         (2, 4): 110,   # 4's parent is 2 (a branch): skipped as parent / child
         (2, 5): 105,   # a past loop edge as well: emitted as kind 2 only
         (1, 6): 40,    # (current, loop): kept although below 100
         (2, 6): 60,    # loop connection below 100: dropped
         (0, 6): 130,   # loop connection kept, and its covisibility edge skipped (sInsertedEdges)
         (1, 5): 101,   # loop connection of a neighbour kept
         (3, 6): 115}   # not a loop connection: covisibility edge 6 -> 3
    cov = []
    for i in range(N):
        nb = sorted([(-w, (a if b == i else b)) for (a, b), w in W.items() if i in (a, b)])
        cov.append(([n for _, n in nb], [-w for w, _ in nb]))
    parent = np.array([-1, 0, 1, 2, 2, 4, 5])
    loop_edges = [[] for _ in range(N)]
    loop_edges[5].append(2)
    loop_edges[2].append(5)
    kf_id = np.array([0, 3, 4, 9, 10, 20, 31]) if gaps else np.arange(N)
    m = dict(kf_id=kf_id, Tcw=np.tile(np.eye(4, dtype=np.float32), (N, 1, 1)), parent=parent, cov=cov,
             loop_edges=loop_edges, pos=np.zeros((0, 3), np.float32), bad=np.zeros(0, bool),
             ref=np.zeros(0, np.int32), corrected_ref=np.zeros(0, np.int32))
    lc = {6: [2, 1, 0], 5: [1]}
    return (m, 1, 6, {}, {}, lc)


EXPECTED_HAND = [(5, 1, 0), (6, 0, 0), (6, 1, 0),
                 (1, 0, 1), (2, 1, 1), (2, 0, 3), (3, 2, 1), (4, 2, 1), (4, 3, 3), (5, 4, 1), (5, 2, 2),
                 (6, 5, 1), (6, 3, 3)]


@pytest.mark.parametrize("gaps", [False, True])
def test_edge_rules_hand_graph(gaps):
    sc = _hand_graph(gaps)
    rows = R.edges(sc)
    assert [tuple(r) for r in rows] == EXPECTED_HAND
    assert np.array_equal(rows, literal_edges(sc[0], sc[1], sc[2], sc[5]))
    got = {tuple(r) for r in rows}
    assert (6, 2, 0) not in got            # a loop connection below 100 is dropped
    assert (6, 1, 0) in got                # except the (current, loop) pair
    assert (6, 0, 3) not in got            # a pair in sInsertedEdges is not a covisibility edge again
    assert (4, 2, 3) not in got and (5, 2, 3) not in got   # parent / child / loop edge neighbours
    assert all(i > j for i, j, k in got if k in (2, 3))    # only lower ids


@pytest.mark.parametrize("N,seed,kw", [(10, 10, {}), (26, 26, {}), (70, 70, dict(past_loops=True, gaps=True)),
                                       (40, 1, dict(past_loops=True))])
def test_edge_rules_generated(N, seed, kw):
    sc = S.make_scene(N, seed, **kw)
    rows = R.edges(sc)
    assert np.array_equal(rows, literal_edges(sc[0], sc[1], sc[2], sc[5]))
    assert set(rows[:, 2]) >= {0, 1, 3}
    # gaps in kf_id change nothing
    sc2 = S.make_scene(N, seed, **dict(kw, gaps=not kw.get("gaps", False)))
    assert np.array_equal(R.edges(sc2), rows)


# ------------------------------------------------------------------ Sim3 in extended precision
def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)


def _coef(theta, sigma):
    s = np.exp(sigma)
    if abs(sigma) < 1e-12:
        C = LD(1) + sigma / 2
    else:
        C = (s - 1) / sigma
    if theta < 1e-6:
        if abs(sigma) < 1e-12:
            return LD(1) / 2, LD(1) / 6, C
        s2 = sigma * sigma
        return ((sigma - 1) * s + 1) / s2, ((s2 / 2 - sigma + 1) * s) / (s2 * sigma), C
    if abs(sigma) < 1e-12:
        t2 = theta * theta
        return (1 - np.cos(theta)) / t2, (theta - np.sin(theta)) / (t2 * theta), C
    a, b, c = s * np.sin(theta), s * np.cos(theta), theta * theta + sigma * sigma
    return (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) / (theta * theta), C


def _inv3(M):
    a, b, c, d, e, f, g, h, i = [M[r, k] for r in range(3) for k in range(3)]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return np.array([[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
                     [d * h - e * g, b * g - a * h, a * e - b * d]], LD) / det


def ld_exp(u):
    u = np.asarray(u, LD)
    w, ups, sigma = u[:3], u[3:6], u[6]
    theta = np.sqrt(w @ w)
    O = _skew(w)
    A, B, C = _coef(theta, sigma)
    if theta < 1e-6:
        Rm = np.eye(3, dtype=LD) + O + O @ O / 2
    else:
        Rm = np.eye(3, dtype=LD) + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * (O @ O)
    return Rm, (A * O + B * (O @ O) + C * np.eye(3, dtype=LD)) @ ups, np.exp(sigma)


def ld_log(Rm, t, s):
    sigma = np.log(s)
    d = (np.trace(Rm) - 1) / 2
    dR = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]], LD)
    sn = np.sqrt(dR @ dR) / 2  # sin(theta)
    theta = np.arctan2(sn, d)
    w = dR / 2 if theta < 1e-6 else theta / (2 * sn) * dR
    O = _skew(w)
    A, B, C = _coef(theta, sigma)
    W = A * O + B * (O @ O) + C * np.eye(3, dtype=LD)
    return np.concatenate([w, _inv3(W) @ t, [sigma]])


def _ld_sim(S8):
    x, y, z, w = [LD(v) for v in S8[:4]]
    n = x * x + y * y + z * z + w * w  # the 8 doubles hold a unit quaternion to rounding
    Rm = np.array([[1 - 2 * (y * y + z * z) / n, 2 * (x * y - z * w) / n, 2 * (x * z + y * w) / n],
                   [2 * (x * y + z * w) / n, 1 - 2 * (x * x + z * z) / n, 2 * (y * z - x * w) / n],
                   [2 * (x * z - y * w) / n, 2 * (y * z + x * w) / n, 1 - 2 * (x * x + y * y) / n]], LD)
    return Rm, np.asarray(S8[4:7], LD), LD(S8[7])


def _ld_mul(a, b):
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def _ld_inv(a):
    return a[0].T, -(a[0].T @ a[1]) / a[2], 1 / a[2]


def ld_edge_error(C, v1, v2):
    return ld_log(*_ld_mul(_ld_mul(C, v1), _ld_inv(v2)))


def _random_sim(rng, rot=0.6, tr=3.0, sc=0.3):
    return R.sim_exp(np.concatenate([rng.uniform(-rot, rot, 3), rng.uniform(-tr, tr, 3), rng.uniform(-sc, sc, 1)]))


# worst |J - J_ld| the restatement shows over the pairs below: delta = 1e-9 leaves
# rounding noise of about 1e-16 |e| / 2e-9, amplified by |t|. Measured: 9.4e-7.
JACOBIAN_WORST = 9.4e-7


def test_numeric_jacobian_against_extended_precision():
    rng = np.random.default_rng(11)
    h = LD(1e-5)
    worst = 0.0
    for _ in range(12):
        v1, v2 = _random_sim(rng), _random_sim(rng)
        # a measurement near v2 v1^-1: the error of a drifted edge, not a large one
        C = R.sim_mul(R.sim_mul(v2, R.sim_inverse(v1)), _random_sim(rng, 0.05, 0.1, 0.02))
        Ji, Jj = R.edge_jacobian(C, v1, v2)
        Cl, a, b = _ld_sim(C), _ld_sim(v1), _ld_sim(v2)
        e0 = ld_edge_error(Cl, a, b)
        assert np.abs(e0.astype(np.float64) - R.edge_error(C, v1, v2)).max() <= 1e-12
        for side, J in ((0, Ji), (1, Jj)):
            for d in range(7):
                u = np.zeros(7, LD)
                u[d] = h
                ep = ld_edge_error(Cl, _ld_mul(ld_exp(u), a), b) if side == 0 else ld_edge_error(
                    Cl, a, _ld_mul(ld_exp(u), b))
                em = ld_edge_error(Cl, _ld_mul(ld_exp(-u), a), b) if side == 0 else ld_edge_error(
                    Cl, a, _ld_mul(ld_exp(-u), b))
                col = ((ep - em) / (2 * h)).astype(np.float64)
                worst = max(worst, float(np.abs(J[:, d] - col).max()))
    print(f"numeric Jacobian: worst difference to extended precision {worst:.3e} (bound {4 * JACOBIAN_WORST:.3e})")
    assert worst <= 4 * JACOBIAN_WORST


# ------------------------------------------------------------------ Sim3 log
@pytest.mark.parametrize("theta,sigma", [(0.7, 0.3), (0.7, 3e-6), (4e-6, 0.3), (4e-6, 3e-6), (2e-3, -0.2),
                                         (2.5, 1e-7)])
def test_sim3_log_inverts_exp(theta, sigma):
    """The four eps branches of Sim3::log (|sigma| and the rotation on either
    side of 1e-5; d > 1 - 1e-5 is theta < 4.5e-3) and of the exponential. The
    small-angle branches drop terms of relative order theta^2 <= 2e-5 from A, B
    and R, which multiply theta-sized or translation-sized quantities: the
    round trip is exact to 1e-9 (|upsilon| <= 3) outside them and to
    theta^2 |upsilon| inside. With |sigma| >= 1e-5 the reference's small-angle
    B, (sigma^2/2 - sigma + 1) s / sigma^3, lacks the -1 of the limit of the
    general formula (sim3.h:199 against :211): W is off by Omega^2 / sigma^3
    there, which the restatement keeps and the bound allows for."""
    rng = np.random.default_rng(int(theta * 1e7) + 1)
    for _ in range(20):
        ax = rng.normal(0, 1, 3)
        ax /= np.linalg.norm(ax)
        u = np.concatenate([theta * ax, rng.uniform(-3, 3, 3), [sigma]])
        back = R.sim_log(R.sim_exp(u))
        small = theta < 4.5e-3
        tol = 1e-9
        if small:
            tol = max(1e-9, 2 * theta * theta * 3 * (1 + (abs(sigma) ** -3 if abs(sigma) >= 1e-5 else 0)))
        assert np.abs(back - u).max() <= tol, (u, back)
        assert abs(back[6] - sigma) <= 1e-15


# ------------------------------------------------------------------ the GPU tests' scenes
def test_decision_stable_scenes():
    """The scenes of tests/test_essgraph_gpu.py whose counts are compared: the
    restatement returns the same iterations, trials and accepted flags under
    LLt and LDLt, and its initial chi2 moves by at most CHI2_SPREAD between
    its two summation orders."""
    import test_essgraph_gpu as G

    spread = 0.0
    for name, counts in G.STABLE.items():
        sc = G.scene(name)
        a, b, c = R.solve(sc, R.LLT), R.solve(sc, R.LDLT), R.solve(sc, R.LLT, reverse=True)
        assert (a["iterations"], a["trials"]) == counts == (b["iterations"], b["trials"]), name
        assert np.array_equal(a["trace_accepted"], b["trace_accepted"]), name
        assert G.close(a["Tcw"], b["Tcw"]) and G.close(a["pos"], b["pos"])
        spread = max(spread, abs(a["chi2_initial"] - c["chi2_initial"]) / a["chi2_initial"])
        print(f"{name}: {counts}, accepted {a['trace_accepted'].astype(int)}")
    print(f"chi2 spread between the summation orders: {spread:.3e}")
    assert spread <= G.CHI2_SPREAD
