"""GPU parity of Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations,
pbStopFlag) (Optimizer.cc:36-142; gf_bundle_adjustment, gf_ba_plan_create_iters)
with the CPU oracle: ``O.local_ba(p, its=(n, 0))`` is optimize(n) followed by
optimize(0), whose outlier flags are ignored (BundleAdjustment has no outlier
pass).

Tolerance: poses and points within RTOL = 1e-5 relative (|d| <= 1e-5 *
max(1, |v|)), the bound tests/test_lba_gpu.py holds the solver to; iteration
counts equal; edge_outlier all zero."""
import ctypes

import numpy as np
import pytest

import initmap_ref as R
import initmap_scenes as S
import oracle_lib as O
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.optimizer import LocalBAPlan, bundle_adjustment, local_bundle_adjustment
from gf_orb_slam_amd.synth import synth_lba_problem

pytestmark = pytest.mark.gpu
RTOL = 1e-5
_cache = {}


def two_view_problem(seed):
    """The two-keyframe graph CreateInitialMap hands to GlobalBundleAdjustemnt,
    from synth_two_view(seed) + the oracle's initialiser."""
    if seed not in _cache:
        a = R.points(S.INFO, *S.args(S.two_view(seed)))
        assert a["status"] == R.OK and 252 <= a["npts"] <= 268
        _cache[seed] = a["ba"]
    return _cache[seed]


def oracle(p, n):
    key = (id(p), n)
    if key not in _cache:
        _cache[key] = O.local_ba(p, its=(n, 0))
    return _cache[key]


class _DevBytes:
    """Device memory at an address, for torch.as_tensor."""

    def __init__(self, addr, nbytes):
        self.__cuda_array_interface__ = dict(shape=(nbytes,), typestr="|u1", data=(int(addr), False), version=2)


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b)))


def _check(g, o):
    Tg, Xg, og, ig = g
    To, Xo, _, io = o
    print("iterations", ig, io, "max |dT|", np.abs(Tg - To).max() if Tg.size else 0.0, "max |dX|",
          np.abs(Xg - Xo).max() if Xg.size else 0.0)
    assert ig[0] == io[0] and ig[1] == -1, (ig, io)
    assert not og.any()
    assert _close(Tg, To), np.abs(Tg - To).max()
    assert _close(Xg, Xo), np.abs(Xg - Xo).max()


@pytest.mark.parametrize("seed", [1, 2, 3, 5])
def test_two_view_matches_oracle(seed):
    p = two_view_problem(seed)
    o = oracle(p, 20)
    assert 12 <= o[3][0] <= 14, o[3]
    _check(bundle_adjustment(p, 20), o)


def test_local_window_matches_oracle():
    p = synth_lba_problem(2, 6, 300)
    _check(bundle_adjustment(p, 20), O.local_ba(p, its=(20, 0)))


def test_schedule_differs_from_the_local_one():
    """One optimize(20) and the local optimize(5) + optimize(10) with outlier
    passes give different maps on seed 2: the entry really runs the new
    schedule."""
    p = two_view_problem(2)
    Tg, Xg, _, _ = bundle_adjustment(p, 20)
    Tl, Xl, _, il = local_bundle_adjustment(p)
    d = np.abs(np.asarray(Tg, np.float64)[1] - np.asarray(Tl, np.float64)[1]).max()
    print("max |dT| against the 5 + 10 schedule", d, il)
    assert d > 1e-4


def test_zero_iterations():
    """optimize(0): initialised, no iteration; the inputs come back (through
    the quaternion, as the oracle's do)."""
    p = two_view_problem(1)
    g = bundle_adjustment(p, 0)
    assert g[3] == (0, -1)
    _check(g, O.local_ba(p, its=(0, 0)))


def test_empty_graph_and_fixed_only():
    """No edge: initializeOptimization finds nothing to optimise, optimize()
    returns -1 and nothing changes."""
    p = two_view_problem(1)
    empty = dict(p, edge_pt=p["edge_pt"][:0], edge_kf=p["edge_kf"][:0], edge_z=p["edge_z"][:0],
                 edge_inv_sigma2=p["edge_inv_sigma2"][:0])
    g = bundle_adjustment(empty, 20)
    o = O.local_ba(empty, its=(20, 0))
    assert g[3] == (-1, -1) and o[3][0] == -1
    assert _close(g[0], o[0]) and _close(g[1], o[1])
    none = dict(kf_Tcw=p["kf_Tcw"][:0], kf_kind=p["kf_kind"][:0], kf_cam=p["kf_cam"][:0], pt_pos=p["pt_pos"][:0],
                edge_pt=p["edge_pt"][:0], edge_kf=p["edge_kf"][:0], edge_z=p["edge_z"][:0],
                edge_inv_sigma2=p["edge_inv_sigma2"][:0])
    assert bundle_adjustment(none, 20)[3] == (-1, -1)
    only_fixed = dict(none, kf_Tcw=p["kf_Tcw"][:1], kf_kind=p["kf_kind"][:1], kf_cam=p["kf_cam"][:1])
    assert int(only_fixed["kf_kind"][0]) == 1
    g = bundle_adjustment(only_fixed, 20)
    assert g[3] == (-1, -1) and np.array_equal(g[0].reshape(-1), np.asarray(p["kf_Tcw"][:1], np.float32).reshape(-1))
    # every keyframe fixed, edges present: the points are the free vertices, as in the oracle
    fixed = dict(p, kf_kind=np.full_like(p["kf_kind"], 2))
    _check(bundle_adjustment(fixed, 20), O.local_ba(fixed, its=(20, 0)))
    for kind in (0, 1, 2):  # all three kinds are accepted for the second keyframe
        q = dict(p, kf_kind=np.array([1, kind], np.uint8))
        _check(bundle_adjustment(q, 3), O.local_ba(q, its=(3, 0)))


def test_stop_flag_raised_before_the_call():
    p = two_view_problem(3)
    g = bundle_adjustment(p, 20, stop_flag=ctypes.c_uint8(1))
    assert g[3] == (0, -1), g[3]
    _check(g, O.local_ba(p, its=(0, 0)))
    _check(bundle_adjustment(p, 20, stop_flag=ctypes.c_uint8(0)), oracle(p, 20))


def test_iteration_count_limits():
    p = two_view_problem(1)
    for n in (65, -1):
        with pytest.raises(GFError) as e:
            bundle_adjustment(p, n)
        assert e.value.code == -1
    with pytest.raises(GFError) as e:
        bundle_adjustment(synth_lba_problem(4, 34, 200, nfixed=0), 20)  # 33 free keyframes
    assert e.value.code == -4
    # the cap holds: 64 is accepted, and 2 iterations stop at 2
    assert bundle_adjustment(p, 2)[3] == (2, -1)
    _check(bundle_adjustment(p, 64), oracle(p, 64))


def test_batch_plan_equals_the_single_calls_and_device_results():
    """Four problems of different sizes in one plan: every result equals the
    single call's bit for bit, and gf_ba_plan_results_dev points at the bytes
    gf_ba_plan_results copies out."""
    import torch

    probs = [two_view_problem(1), synth_lba_problem(2, 6, 300), two_view_problem(5), synth_lba_problem(9, 3, 40)]
    plan = LocalBAPlan(probs, iterations=20)
    steps = plan.solve()
    assert 0 < steps <= 204  # the guard: 10 trials an iteration and one step to end, checked every 4 steps
    res = plan.results()
    for g, p in zip(res, probs):
        s = bundle_adjustment(p, 20)
        assert g[3] == s[3] and g[0].tobytes() == s[0].tobytes() and g[1].tobytes() == s[1].tobytes()
        assert not g[2].any()
    for i, (g, p) in enumerate(zip(res, probs)):
        T, X, it = plan.results_dev(i)
        nkf, npts = len(p["kf_kind"]), len(p["pt_pos"])
        hT, hX, hI = np.zeros((nkf, 4, 4), np.float32), np.zeros((npts, 3), np.float32), np.zeros(2, np.int32)
        for dst, src in ((hT, T), (hX, X), (hI, it)):
            if dst.nbytes:
                dst.view(np.uint8).reshape(-1)[:] = torch.as_tensor(_DevBytes(src, dst.nbytes), device="cuda").cpu().numpy()
        assert hT.tobytes() == g[0].tobytes() and hX.tobytes() == g[1].tobytes() and tuple(hI) == g[3]
    plan.close()
