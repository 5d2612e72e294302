"""Optimizer::OptimizeEssentialGraph and CorrectLoop's Sim3 propagation on the
GPU (csrc/essgraph.hip) against the CPU restatement
(tests/helpers/essgraph_ref.cpp)."""
import ctypes
import functools

import numpy as np
import pytest

import essgraph_ref as R
import essgraph_scenes as S

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-5  # README / tests/test_pose_gpu.py: |d| <= 1e-5 * max(1, |x|) per entry

# name -> (N, seed, generator arguments): 3 one nearly empty tile; 9 exactly one
# full tile; 10 a second tile with one keyframe; 26 four tile rows, the envelope
# skips tiles and the loop rows are long; 70 nine tile rows, kf_id gaps, past
# loop edges; 26-low a low-drift map whose second iteration ends on an accepted
# tenth trial at a large lambda
SCENES = {"3": (3, 3, {}), "9": (9, 9, {}), "10": (10, 10, {}), "26": (26, 26, {}),
          "70": (70, 70, dict(past_loops=True, gaps=True)), "26-low": (26, 2, dict(drift=0.03))}
# Decision-stable scenes (tests/test_essgraph_cpu.py::test_decision_stable_scenes
# checks this list on the CPU): the restatement returns the same iterations,
# trials and accepted flags under its LLt and its LDLt solver. In all of them
# the first Gauss-Newton step is accepted and the trials of the second
# iteration raise chi2 severalfold, far from a rounding-level decision.
# (Low-drift maps that run many iterations, e.g. N = 26, seed 26, drift 0.03,
# are not stable: there the restatement's own two solvers end 2e-5 to 1e-4
# apart, above the pose tolerance, so they cannot serve as a pose comparison.)
STABLE = {"3": (2, 11), "9": (2, 11), "10": (2, 11), "26": (2, 11), "70": (2, 11), "26-low": (2, 11)}
# The restatement's own spread of the initial chi2 between its two summation
# orders (edges first to last / last to first), the largest over the scenes:
# 8.6e-16 relative, on 26-low (measured on the CPU by
# test_decision_stable_scenes, which prints it; at most 1.9e-16 on the others).
# The device may differ by 16 x that.
CHI2_SPREAD = 8.6e-16
CHI2_RTOL = 16 * CHI2_SPREAD


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= POSE_RTOL * np.maximum(1.0, np.abs(b))).all())


def worst(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def scene(name):
    N, seed, kw = SCENES[str(name)]
    return S.make_scene(N, seed, **kw)


@functools.lru_cache(maxsize=None)
def ref_result(N):
    return R.solve(scene(N))


@functools.lru_cache(maxsize=None)
def gpu_single(N):
    from gf_orb_slam_amd.optimizer import EssentialGraphPlan

    plan = EssentialGraphPlan([scene(N)])
    try:
        edges = plan.edges(0)
        plan.solve()
        return edges, plan.results()[0]
    finally:
        plan.close()


def same_bytes(a, b):
    keys = ("Tcw", "pos", "trace_lambda", "trace_chi2", "trace_accepted")
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and all(
        a[k] == b[k] for k in ("iterations", "trials", "stop", "chi2_initial", "chi2_final"))


@pytest.mark.parametrize("N", list(SCENES))
def test_against_restatement(N):
    sc = scene(N)
    edges, g = gpu_single(N)
    r = ref_result(N)
    assert np.array_equal(edges, R.edges(sc))
    rel = abs(g["chi2_initial"] - r["chi2_initial"]) / r["chi2_initial"]
    print(f"N={N}: {len(edges)} edges, chi2_initial rel diff {rel:.3e} (bound {CHI2_RTOL:.3e}), "
          f"pose worst {worst(g['Tcw'], r['Tcw']):.3e}, point worst {worst(g['pos'], r['pos']):.3e}, "
          f"iterations {g['iterations']}/{r['iterations']}, trials {g['trials']}/{r['trials']}, "
          f"stop {g['stop']}/{r['stop']}, chi2_final {g['chi2_final']!r}/{r['chi2_final']!r}")
    assert rel <= CHI2_RTOL
    assert close(g["Tcw"], r["Tcw"])
    assert close(g["pos"], r["pos"])
    if N in STABLE:
        assert (r["iterations"], r["trials"]) == STABLE[N]
        assert (g["iterations"], g["trials"]) == STABLE[N]
        assert np.array_equal(g["trace_accepted"], r["trace_accepted"])
    m = sc[0]
    untouched = np.asarray(m["bad"], bool) | ((np.asarray(m["ref"]) < 0) & (np.asarray(m["corrected_ref"]) < 0))
    assert untouched.any() and (~untouched).any()
    assert g["pos"][untouched].tobytes() == np.asarray(m["pos"], np.float32)[untouched].tobytes()


def test_ragged_batch():
    from gf_orb_slam_amd.optimizer import optimize_essential_graph_batch

    sizes = ("3", "10", "26")
    batch = optimize_essential_graph_batch([scene(N) for N in sizes])
    for N, b in zip(sizes, batch):
        assert same_bytes(b, gpu_single(N)[1]), N


def test_determinism():
    from gf_orb_slam_amd.optimizer import EssentialGraphPlan

    plan = EssentialGraphPlan([scene("26")])
    try:
        plan.solve()
        a = plan.results()[0]
        plan.solve()
        b = plan.results()[0]
    finally:
        plan.close()
    assert same_bytes(a, b)
    assert same_bytes(a, gpu_single("26")[1])


def test_convenience_call():
    from gf_orb_slam_amd.optimizer import Optimizer

    m, loop, cur, non, cor, lc = scene("10")
    out = Optimizer.OptimizeEssentialGraph(m, loop, cur, cor[cur], non, cor, lc)
    assert same_bytes(out, gpu_single("10")[1])


def _map64(Sim, p):
    """g2o::Sim3::map in float64 NumPy: s (R p) + t with R = toRotationMatrix()."""
    from gf_orb_slam_amd.optimizer import sim3_from_g2o

    s, Rm, t = sim3_from_g2o(Sim)
    return s * (Rm @ p) + t


def _propagation_reading(Tcw, cur, covisibles, Scw, observations, pos, bad):
    """LoopClosing.cc:428-506 read literally in float64 NumPy (the Sim3 products
    through the restatement's g2o::Sim3)."""
    from gf_orb_slam_amd.optimizer import sim3_from_g2o

    non, cor = S.propagate(Tcw, cur, covisibles, Scw)
    pos = np.asarray(pos, np.float32).copy()
    cref = np.full(len(pos), -1, np.int32)
    times = np.zeros(len(pos), np.int32)
    T = np.asarray(Tcw, np.float32).copy()
    for k in sorted(cor):
        Swi = R.sim_inverse(cor[k])
        for m in observations[k]:
            if m < 0 or bad[m] or cref[m] >= 0:
                continue
            pos[m] = _map64(Swi, _map64(non[k], pos[m].astype(np.float64))).astype(np.float32)
            cref[m] = k
            times[m] += 1
        s, Rm, t = sim3_from_g2o(cor[k])
        T[k, :3, :3] = Rm.astype(np.float32)
        T[k, :3, 3] = (t * (1.0 / s)).astype(np.float32)
    return non, cor, pos, cref, T, times


def test_propagation():
    from gf_orb_slam_amd.optimizer import Optimizer
    from gf_orb_slam_amd.sim3 import propagate_loop_correction

    m, loop, cur, _, cor0, lc = scene("26")
    covis = [k for k in sorted(cor0) if k != cur]
    Scw = cor0[cur]
    rng = np.random.default_rng(5)
    ref = np.asarray(m["ref"])
    obs = {}
    for k in sorted(cor0):
        own = np.nonzero(ref == k)[0]
        # seen from every corrected keyframe, and a few from some of them
        shared = np.concatenate([np.arange(0, 60, 5), rng.integers(0, len(ref), 6)])
        obs[k] = np.concatenate([own, shared, [-1, -1]])
    seen_twice = np.intersect1d(obs[covis[0]], obs[cur])
    seen_twice = seen_twice[seen_twice >= 0]
    assert len(seen_twice) > 0
    g = propagate_loop_correction(m["Tcw"], cur, covis, Scw, obs, m["pos"], m["bad"])
    non, cor, pos, cref, T, times = _propagation_reading(m["Tcw"], cur, covis, Scw, obs, m["pos"], m["bad"])
    assert times.max() == 1
    assert sorted(g["CorrectedSim3"]) == sorted(cor) and sorted(g["NonCorrectedSim3"]) == sorted(non)
    for k in cor:
        assert close(g["CorrectedSim3"][k], cor[k]) and close(g["NonCorrectedSim3"][k], non[k])
    print(f"propagation: pose worst {worst(g['Tcw'], T):.3e}, point worst {worst(g['pos'], pos):.3e}")
    assert np.array_equal(g["corrected_ref"], cref)
    assert close(g["Tcw"], T) and close(g["pos"], pos)
    # a point seen from two corrected keyframes moves once, by the first in id order
    first = min(covis[0], cur)
    for p in seen_twice:
        if not m["bad"][p]:
            assert g["corrected_ref"][p] <= first
    assert g["pos"][np.asarray(m["bad"], bool)].tobytes() == np.asarray(m["pos"], np.float32)[
        np.asarray(m["bad"], bool)].tobytes()
    # the propagation's outputs are the optimiser's inputs
    mg = dict(m, Tcw=g["Tcw"], pos=g["pos"], corrected_ref=g["corrected_ref"])
    mr = dict(m, Tcw=T, pos=pos, corrected_ref=cref)
    a = Optimizer.OptimizeEssentialGraph(mg, loop, cur, Scw, g["NonCorrectedSim3"], g["CorrectedSim3"], lc)
    b = Optimizer.OptimizeEssentialGraph(mr, loop, cur, Scw, non, cor, lc)
    print(f"propagation -> optimiser: pose worst {worst(a['Tcw'], b['Tcw']):.3e}, "
          f"point worst {worst(a['pos'], b['pos']):.3e}")
    assert close(a["Tcw"], b["Tcw"]) and close(a["pos"], b["pos"])
    assert (a["iterations"], a["trials"]) == (b["iterations"], b["trials"])


def test_argument_errors():
    from gf_orb_slam_amd import _lib
    from gf_orb_slam_amd.optimizer import EssGraphArrays
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    lib = _lib.lib()

    def create(args):
        arr = EssGraphArrays(*args)
        h = ctypes.c_void_p()
        rc = lib.gf_essgraph_plan_create(ctx.handle, 1, ctypes.byref(arr.problem), ctypes.byref(h))
        assert not h.value
        return rc, lib.gf_last_error().decode()

    m, loop, cur, non, cor, lc = scene("10")
    ids = np.asarray(m["kf_id"]).copy()
    ids[4], ids[5] = ids[5], ids[4]
    rc, msg = create((dict(m, kf_id=ids), loop, cur, non, cor, lc))
    assert rc == -1 and "kf_id" in msg
    par = np.asarray(m["parent"]).copy()
    par[3] = 10
    rc, msg = create((dict(m, parent=par), loop, cur, non, cor, lc))
    assert rc == -1 and "range" in msg
    rc, msg = create((m, loop, 10, non, cor, lc))
    assert rc == -1 and "range" in msg
    n = _lib.ESSGRAPH_MAX_KF + 1
    big = dict(kf_id=np.arange(n), Tcw=np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), parent=np.arange(-1, n - 1),
               cov=[([], [])] * n, loop_edges=[[]] * n, pos=np.zeros((0, 3), np.float32), bad=np.zeros(0, bool),
               ref=np.zeros(0, np.int32), corrected_ref=np.zeros(0, np.int32))
    rc, msg = create((big, 0, n - 1, {}, {}, {}))
    assert rc == -1 and "GF_ESSGRAPH_MAX_KF" in msg
    rc, msg = create((dict(big, kf_id=[0], Tcw=big["Tcw"][:1], parent=[-1], cov=[([], [])], loop_edges=[[]]), 0, 0,
                      {}, {}, {}))
    assert rc == -1 and "fewer than 2" in msg
