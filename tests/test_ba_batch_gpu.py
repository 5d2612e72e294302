"""GPU parity of the batched bundle adjustment (gf_ba_plan_*, csrc/ba.hip)
with the CPU oracle on both sides of the switch between its two Schur
products: k_ba_spgemm for plans of up to 8 windows, k_ba_gemm (dense split-K
through LDS, then the dense branch of k_ba_gemm_reduce) from 9 on. The scenes
are tests/ba_batch_scenes.py; tests/test_ba_batch_cpu.py holds them away from
the chi2 threshold and to the geometry they are named for.

Tolerance: the solver's existing bound (tests/test_lba_gpu.py): poses and
points within RTOL = 1e-5 relative (|d| <= 1e-5 * max(1, |v|)), iteration
counts equal, outlier flags identical. The short schedules follow
tests/test_ba_iters_gpu.py: first count equal, second -1, no flag. After one
iteration the result is a direct function of the Schur product."""
import ctypes

import numpy as np
import pytest

import ba_batch_scenes as S
import initmap_scenes as IS
import oracle_lib as O
from gf_orb_slam_amd import tracking
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
from gf_orb_slam_amd.optimizer import LocalBAPlan

pytestmark = pytest.mark.gpu
RTOL = 1e-5
_cache = {}


def oracle(p, its):
    key = (p["name"], its)
    if key not in _cache:
        _cache[key] = O.local_ba(p, its=its)
    return _cache[key]


def solve(probs, iterations=None, twice=False, stop_flag=None):
    plan = LocalBAPlan(probs, iterations=iterations)
    try:
        plan.solve(stop_flag=stop_flag)
        res = plan.results()
        if twice:
            plan.solve(stop_flag=stop_flag)
            res = (res, plan.results())
    finally:
        plan.close()
    return res


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b)))


def _err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


def _check_all(res, refs, probs, flags=True):
    """Every window of the batch; the failures are collected so that one report names them all."""
    assert len(res) == len(refs) == len(probs)
    bad, worst = [], 0.0
    for i, (g, o, p) in enumerate(zip(res, refs, probs)):
        Tg, Xg, og, ig = g
        To, Xo, oo, io = o
        e = max(_err(Tg, To), _err(Xg, Xo))
        worst = max(worst, e)
        its_ok = tuple(ig) == tuple(io) if flags else (ig[0] == io[0] and ig[1] == -1)
        flags_ok = np.array_equal(og, oo) if flags else not og.any()
        if not (its_ok and flags_ok and _close(Tg, To) and _close(Xg, Xo)):
            bad.append((i, p["name"], tuple(ig), tuple(io), int((og != oo).sum()) if flags else int(og.sum()), e))
    print(f"{len(probs)} windows, largest relative difference {worst:.3g}")
    assert not bad, bad


def _same_bits(a, b):
    return (a[3] == b[3] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and
            a[2].tobytes() == b[2].tobytes())


@pytest.mark.parametrize("name", S.LOCAL, ids=S.batch_id)
def test_local_schedule_matches_oracle(name):
    probs = S.batch(name)
    _check_all(solve(probs), [oracle(p, (5, 10)) for p in probs], probs)


@pytest.mark.parametrize("k", [1, 2, 20])
@pytest.mark.parametrize("name", S.SHORT, ids=S.batch_id)
def test_short_schedule_matches_oracle(name, k):
    probs = S.batch(name)
    _check_all(solve(probs, iterations=k), [oracle(p, (k, 0)) for p in probs], probs, flags=False)


@pytest.mark.parametrize("name,pos", S.PLACEMENT, ids=[n for n, _ in S.PLACEMENT])
@pytest.mark.parametrize("iterations", [None, 1], ids=["local", "one"])
def test_placement_and_second_solve(name, pos, iterations):
    """The same window at three places of one plan between windows of other
    sizes gives the same bits (tile0, ss0, mask0, panel0 and the task-list
    offsets), and a second solve() of the plan repeats the first bit for bit."""
    probs = S.batch(name)
    first, second = solve(probs, iterations=iterations, twice=True)
    its = (5, 10) if iterations is None else (iterations, 0)
    _check_all(first, [oracle(p, its) for p in probs], probs, flags=iterations is None)
    for i in pos[1:]:
        assert _same_bits(first[pos[0]], first[i]), i
    for i, (a, b) in enumerate(zip(first, second)):
        assert _same_bits(a, b), i


def test_both_paths_agree():
    """Windows 0-7 solved by the task list (a plan of 8) and by the dense
    product (a plan of 9)."""
    sparse, dense = solve(S.batch(("size", 8))), solve(S.batch(("size", 9)))
    for i, (a, b) in enumerate(zip(sparse, dense)):
        assert a[3] == b[3] and np.array_equal(a[2], b[2]), i
        assert _close(a[0], b[0]) and _close(a[1], b[1]), (i, _err(a[0], b[0]), _err(a[1], b[1]))


def test_stop_flag_raised_before_a_dense_solve():
    probs = S.batch(("size", 9))
    res = solve(probs, stop_flag=ctypes.c_uint8(1))
    assert all(list(g[3]) == [0, 0] for g in res), [g[3] for g in res]
    _check_all(res, [oracle(p, (0, 0)) for p in probs], probs)
    _check_all(solve(probs, stop_flag=ctypes.c_uint8(0)), [oracle(p, (5, 10)) for p in probs], probs)


# ---------------------------------------------------------------- CreateInitialMap, 12 streams
def test_twelve_initial_maps_equal_the_single_calls():
    """tests/test_initmap_gpu.py's batch of five, repeated to 12 problems: one
    LocalBAPlan(iterations=20) of 12 takes the dense path; the single calls
    take the task list. Integer fields equal, floats within the parity bound."""
    import torch

    B7 = dict(n_match=110, n_extra=30, outlier_frac=0.0)
    five = [IS.two_view(1), IS.hand_made(75, 65), IS.two_view(4), IS.two_view(7, mask=4, **B7), IS.two_view(5)]
    order = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    scs = [five[i] for i in order]
    res = tracking.create_initial_maps_device(IS.INFO, *IS.device_batch(scs))
    rep = res["report"].cpu().numpy().view(tracking.REPORT_DTYPE).reshape(-1)
    mps = res["mps"].cpu().numpy().reshape(len(scs), -1).view(MAP_POINT_DTYPE)
    singles = [tracking.create_initial_maps_device(IS.INFO, *IS.device_batch([sc])) for sc in five]
    for p, (sc, one) in enumerate(zip(scs, [singles[i] for i in order])):
        r1 = one["report"].cpu().numpy().view(tracking.REPORT_DTYPE).reshape(-1)[0]
        n, n1, n2 = int(r1["npts"]), len(sc["kps1"]), len(sc["kps2"])
        for k in ("status", "npts", "tracked", "ba_iterations"):
            assert rep[p][k] == r1[k], (p, k)
        assert int(res["npts"][p]) == n
        m1 = one["mps"].cpu().numpy().reshape(1, -1).view(MAP_POINT_DTYPE)[0, :n]
        assert _close(rep[p]["median_depth"], r1["median_depth"]) and _close(rep[p]["Tcw"], r1["Tcw"]), p
        for k in ("pos", "normal", "min_dist", "max_dist"):
            assert _close(mps[p, :n][k], m1[k]), (p, k)
        for k in ("pt_kp", "mp_desc"):
            assert torch.equal(res[k][p, :n], one[k][0, :n]), (p, k)
        assert torch.equal(res["slots1"][p, :n1], one["slots1"][0, :n1])
        assert torch.equal(res["slots2"][p, :n2], one["slots2"][0, :n2])
    assert [int(s) for s in rep["status"]] == [[0, 3, 1, 3, 0][i] for i in order]
