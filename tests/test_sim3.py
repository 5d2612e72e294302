"""Loop-closure Sim3 solver: Sim3Solver (src/Sim3Solver.cc) — Horn's closed
form on random three-point sets in RANSAC, CheckInliers with the truncated
size_t bounds, iterate()/bNoMore bookkeeping and the std::rand() draws. The
OpenCV calls are restated (tests/helpers/sim3_ref.cpp, assumption A22), so
parity is unpinned against OpenCV itself; the CPU tests pin the restatement to
ground-truth similarity transforms and to the reference's control flow, the GPU
tests hold the device path to the restatement bit for bit (transforms, inlier
masks, counts, flags, every state field and the caller's rand() state)."""
import ctypes

import numpy as np
import pytest

import sim3_ref as R
from gf_orb_slam_amd._lib import check, lib, ptr
from gf_orb_slam_amd.pnp import RNG_DTYPE
from gf_orb_slam_amd.sim3 import (GF_SIM3_FOUND, GF_SIM3_NOMORE, SIM3_STATE_DTYPE, Sim3KeyFrame, Sim3Solver,
                                  sim3_params)
from sim3_scenes import EUROC_K, solver_scene

LOOP = dict(probability=0.99, min_inliers=20, max_iterations=300)  # LoopClosing.cc:296
FLOAT_FIELDS = ("best_scale", "best_R", "best_t", "best_T12")
INT_FIELDS = ("n", "min_inliers", "max_iterations", "iterations", "best_inliers")


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("n,seed", [(40, 1), (120, 2), (400, 3), (1000, 4)])
def test_restatement_recovers_truth(n, seed):
    """find() on noise-free inliers with 30% permuted rows: FOUND, the inlier
    mask is the non-permuted set (for these seeds no permuted pair falls inside
    both bounds, checked with the restatement), and (s, R, t) is the truth.
    Worst error of the restatement over these four seeds, measured on the CPU:
    s 1.2e-7, R 8.5e-8, t 1.1e-6; the bounds are 4x that."""
    X1, X2, s1, s2, K, (s, Rm, t), out = solver_scene(n, seed, 0.3)
    T, inl, ni, fl, _, st, _ = R.run(X1, X2, s1, s2, K, K, 7, [300], **LOOP)[0]
    assert fl == GF_SIM3_FOUND
    assert np.array_equal(inl.astype(bool), ~out) and ni == (~out).sum()
    es = abs(float(st["best_scale"][0]) - s)
    eR = np.abs(st["best_R"][0].reshape(3, 3) - Rm).max()
    et = np.abs(st["best_t"][0] - t).max()
    print(f"n={n} seed={seed}: |ds|={es:.3e} |dR|={eR:.3e} |dt|={et:.3e}")
    assert es <= 4.8e-7 and eR <= 3.4e-7 and et <= 4.4e-6
    T = T.reshape(4, 4)
    assert T[:3, :3].tobytes() == (st["best_R"][0].reshape(3, 3) * st["best_scale"][0]).tobytes()
    assert np.array_equal(T[:3, 3], st["best_t"][0]) and np.array_equal(T[3], [0, 0, 0, 1])


@pytest.mark.parametrize("n", [0, 5, 6, 19, 20, 21, 100, 5000])
def test_sim3_init_matches_restatement(n):
    """gf_sim3_init (library host code) == the restatement's SetRansacParameters, byte for byte."""
    for kw in (dict(probability=0.99, min_inliers=6, max_iterations=300), LOOP):
        a = np.zeros(1, SIM3_STATE_DTYPE)
        check(lib().gf_sim3_init(n, ptr(sim3_params(**kw)), ptr(a)))
        assert a.tobytes() == R.init(n, **kw).tobytes()
        assert 1 <= a["max_iterations"][0] <= 300 and a["n"][0] == n and a["min_inliers"][0] == kw["min_inliers"]


def test_bound_is_truncated_to_size_t():
    """mvnMaxError is a vector<size_t>: at octave 0 the bound is 9, not 9.21. A
    correspondence whose error in image 1 lies between the two is an outlier;
    one just under 9 is an inlier."""
    X1, X2, s1, s2, K, (s, Rm, t), _ = solver_scene(30, 11, 0.0)
    s1[:] = 1.0
    s2[:] = np.float32(1.2 ** 14)  # image 2 never decides
    fx = K[0]
    for i, d in ((3, 3.02), (4, 2.96)):  # d^2 = 9.12 and 8.76
        X1[i, 0] += np.float32(d * X1[i, 2] / fx)
    # the test's own premise, from the truth: the projection of X2 into image 1
    for i, lo, hi in ((3, 9.0, 9.21), (4, 8.0, 9.0)):
        p = s * Rm @ X2[i].astype(np.float64) + t
        du = fx * (X1[i, 0] / X1[i, 2] - p[0] / p[2])
        assert lo + 0.02 < du * du < hi - 0.02
    T, inl, ni, fl, _, _, _ = R.run(X1, X2, s1, s2, K, K, 5, [300], **LOOP)[0]
    assert fl == GF_SIM3_FOUND
    assert inl[3] == 0 and inl[4] == 1 and ni == 29


def test_iteration_accounting():
    """Three draws per iteration run; a call runs while mnIterations < max and
    its own count is not reached (:158); bNoMore once max is reached."""
    X1, X2, s1, s2, K, _, out = solver_scene(30, 12, 0.6)  # 12 consistent rows < 20
    res = R.run(X1, X2, s1, s2, K, K, 11, [2, 3, 5], probability=0.99, min_inliers=20, max_iterations=8)
    assert [r[4] for r in res] == [6, 15, 24]
    assert [int(r[5]["iterations"][0]) for r in res] == [2, 5, 8]
    assert [r[3] for r in res] == [0, 0, GF_SIM3_NOMORE]
    assert all(r[2] == 0 and not r[1].any() for r in res)


def test_too_few_correspondences():
    """N < mRansacMinInliers: bNoMore, no Sim3, no rand() draws (:146-150)."""
    X1, X2, s1, s2, K, _, _ = solver_scene(19, 13, 0.0)
    res = R.run(X1, X2, s1, s2, K, K, 3, [5, 5], **LOOP)
    assert [r[3] for r in res] == [GF_SIM3_NOMORE] * 2 and [r[4] for r in res] == [0, 0]
    assert all(int(r[5]["iterations"][0]) == 0 for r in res)


def test_n_equal_min_inliers_never_succeeds():
    """N == mRansacMinInliers: one iteration (:130-131), and the return needs
    more than mRansacMinInliers inliers (:192), so even 20 consistent
    correspondences of 20 end with bNoMore."""
    X1, X2, s1, s2, K, _, _ = solver_scene(20, 14, 0.0)
    res = R.run(X1, X2, s1, s2, K, K, 3, [5, 5], **LOOP)
    T, inl, ni, fl, draws, st, bm = res[0]
    assert st["max_iterations"][0] == 1 and st["iterations"][0] == 1 and draws == 3
    assert fl == GF_SIM3_NOMORE and ni == 0 and not inl.any() and not T.any()
    assert st["best_inliers"][0] == 20 and bm.all()
    assert res[1][3] == GF_SIM3_NOMORE and res[1][4] == 3


def _draw_sets(seed, n, iterations):
    """The minimal sets of :163-177 replayed on the pre-drawn rand() values."""
    rv = R.rand_values(seed, 3 * iterations)
    sets = []
    for it in range(iterations):
        avail, ids = list(range(n)), []
        for i in range(3):
            randi = int((float(rv[3 * it + i]) / 2147483648.0) * len(avail))
            idx = avail[randi]
            ids.append(idx)
            if idx < len(avail):
                avail[idx] = avail[-1]  # position idx, the value drawn (:175)
            avail.pop()
        sets.append(ids)
    return sets


def test_duplicate_draws_are_degenerate_sets():
    """With 4 correspondences the write to position idx (:175) repeats an index
    inside a set (the third draw repeats the second). Two distinct points leave
    the rotation about their axis free: such an iteration does not reach 4
    inliers and the loop goes on; every other iteration returns at once."""
    X1, X2, s1, s2, K, _, _ = solver_scene(4, 46, 0.0)
    n_dup = 0
    for seed in range(1001, 1041):
        sets = _draw_sets(seed, 4, 10)
        first_good = next(i for i, ids in enumerate(sets) if len(set(ids)) == 3)
        n_dup += first_good
        T, inl, ni, fl, draws, st, _ = R.run(X1, X2, s1, s2, K, K, seed, [10], probability=0.99, min_inliers=3,
                                             max_iterations=300)[0]
        assert fl == GF_SIM3_FOUND and ni == 4 and draws == 3 * (first_good + 1), (seed, sets[:3])
    assert n_dup > 0


def test_nan_hypothesis_is_stored_as_best_and_terminates():
    """Coincident points give a 0/0 angle-axis factor and a NaN transform; NaN
    comparisons make every correspondence an outlier, and 0 >= 0 stores the NaN
    hypothesis as best. A NaN coordinate takes the Jacobi sweeps to their bound.
    Both end with bNoMore after max_iterations."""
    X1, X2, s1, s2, K, _, _ = solver_scene(6, 15, 0.0)
    A1, A2 = np.repeat(X1[:1], 6, 0), np.repeat(X2[:1], 6, 0)
    B1 = X1.copy()
    B1[:] = np.nan
    for P1, P2 in ((A1, A2), (B1, X2)):
        res = R.run(P1, P2, s1, s2, K, K, 9, [5, 300], probability=0.99, min_inliers=3, max_iterations=12)
        assert [r[3] for r in res] == [0, GF_SIM3_NOMORE] and [r[4] for r in res] == [15, 36]
        for r in res:
            assert np.isnan(r[5]["best_T12"][0][:12]).all() and r[5]["best_inliers"][0] == 0 and r[2] == 0


# ------------------------------------------------------------------ GPU
def _rng_after(seed, calls):
    g = np.zeros(1, RNG_DTYPE)
    check(lib().gf_rng_seed(ptr(g), ctypes.c_uint32(seed)))
    if calls:
        sink = np.zeros(calls, np.int32)  # held: gf_rng_next writes `calls` values into it
        check(lib().gf_rng_next(ptr(g), ptr(sink), calls))
    return g


def _assert_state_equal(got, want, where):
    for k in INT_FIELDS:
        assert got[k][0] == want[k][0], (where, k, got[k][0], want[k][0])
    for k in FLOAT_FIELDS:
        a, b = np.atleast_1d(got[k][0]), np.atleast_1d(want[k][0])
        if np.isnan(b).any():  # NaN payloads are not part of the contract
            assert np.array_equal(a, b, equal_nan=True), (where, k, a, b)
        else:
            assert a.tobytes() == b.tobytes(), (where, k, a, b)


def _degenerate(kind, X1, X2):
    if kind == "same":  # coincident points: NaN transform from the 0/0 angle-axis factor
        X1[:], X2[:] = X1[0], X2[0]
    elif kind == "nan":  # NaN coordinates: the Jacobi sweeps run to their bound
        X1[:] = np.nan


# n, outliers, min_inliers, calls, 3-D noise, seed[, degenerate kind]
CASES = [(2, 0.0, 20, [5], 0.0, 1),
         (4, 0.0, 3, [5, 5, 5], 0.0, 46),  # first set [1, 3, 3]
         (6, 0.0, 3, [5, 300], 0.0, 15, "same"),
         (6, 0.0, 3, [5, 300], 0.0, 16, "nan"),
         (4, 0.0, 3, [5, 5, 5], 0.0, 2),
         (20, 0.0, 20, [5], 0.0, 3),
         (21, 0.3, 20, [5, 5, 5, 300], 0.0, 4),
         (64, 0.5, 20, [5, 5, 300], 0.0, 5),
         (65, 0.5, 20, [5, 5, 300], 0.0, 6),
         (257, 0.6, 20, [5, 300], 0.0, 7),
         (1000, 0.45, 20, [5, 5], 0.0, 8),
         (300, 0.3, 20, [5, 5, 300], 0.005, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:3]) + "-" + str(c[5]))
def test_sim3_iterate_gpu_bit_exact(case):
    from gf_orb_slam_amd.matcher import default_context

    n, outl, min_inl, calls, noise, seed = case[:6]
    X1, X2, s1, s2, K, _, _ = solver_scene(n, seed, outl, noise)
    _degenerate(case[6] if len(case) > 6 else "", X1, X2)
    prm = dict(probability=0.99, min_inliers=min_inl, max_iterations=300)
    ref = R.run(X1, X2, s1, s2, K, K, 1000 + seed, calls, **prm)
    ctx = default_context()
    st = np.zeros(1, SIM3_STATE_DTYPE)
    check(lib().gf_sim3_init(n, ptr(sim3_params(**prm)), ptr(st)))
    g = _rng_after(1000 + seed, 0)
    bm = np.zeros(max(n, 1), np.uint8)
    for c, it in enumerate(calls):
        To, io, no, fo, ro, sto, bmo = ref[c]
        T = np.zeros(16, np.float32)
        inl = np.zeros(max(n, 1), np.uint8)
        ni = np.zeros(1, np.int32)
        fl = np.zeros(1, np.int32)
        check(lib().gf_sim3_iterate(ctx.handle, ptr(X1), ptr(X2), ptr(s1), ptr(s2), ptr(K), ptr(K), ptr(st), ptr(bm),
                                    it, ptr(g), ptr(T), ptr(inl), ptr(ni), ptr(fl)))
        assert fl[0] == fo and ni[0] == no, (c, fl[0], fo, ni[0], no)
        assert T.tobytes() == To.tobytes(), (c, T, To)
        assert np.array_equal(inl[:n], io), c
        assert np.array_equal(bm[:n], bmo), c
        _assert_state_equal(st, sto, c)
        assert g.tobytes() == _rng_after(1000 + seed, ro).tobytes(), c


@pytest.mark.gpu
def test_sim3_batch_dev_matches_reference():
    """gf_sim3_iterate_dev: 24 independent solvers (ragged sizes, own rand()
    streams) in one launch, two successive calls; each equals its own
    single-problem restatement."""
    import torch

    from gf_orb_slam_amd.matcher import default_context

    dev = torch.device("cuda:0")
    sizes = [15, 40, 300, 9, 120, 800, 64, 33] * 3
    cap = max(sizes)
    B = len(sizes)
    x1 = np.zeros((B, cap, 3), np.float32)
    x2 = np.zeros((B, cap, 3), np.float32)
    g1 = np.ones((B, cap), np.float32)
    g2 = np.ones((B, cap), np.float32)
    st = np.zeros(B, SIM3_STATE_DTYPE)
    rng = np.zeros(B, RNG_DTYPE)
    ref = []
    calls = [5, 300]
    K = np.asarray(EUROC_K, np.float32)
    for b, n in enumerate(sizes):
        X1, X2, s1, s2, _, _, _ = solver_scene(n, 100 + b, 0.4)
        x1[b, :n], x2[b, :n], g1[b, :n], g2[b, :n] = X1, X2, s1, s2
        check(lib().gf_sim3_init(n, ptr(sim3_params(**LOOP)), ptr(st[b:b + 1])))
        rng[b:b + 1] = _rng_after(500 + b, 0)
        ref.append(R.run(X1, X2, s1, s2, K, K, 500 + b, calls, **LOOP))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    d1, d2, dg1, dg2, dst, drng = t(x1), t(x2), t(g1), t(g2), t(st), t(rng)
    dbm = torch.zeros(B * cap, dtype=torch.uint8, device=dev)
    dT = torch.zeros(B * 16, dtype=torch.float32, device=dev)
    dinl = torch.zeros(B * cap, dtype=torch.uint8, device=dev)
    dn = torch.zeros(B, dtype=torch.int32, device=dev)
    dfl = torch.zeros(B, dtype=torch.int32, device=dev)
    ctx = default_context()
    for c, it in enumerate(calls):
        check(lib().gf_sim3_iterate_dev(ctx.handle, B, ptr(d1), ptr(d2), ptr(dg1), ptr(dg2), cap, ptr(K), ptr(K),
                                        ptr(dst), ptr(dbm), it, 300, ptr(drng), ptr(dT), ptr(dinl), ptr(dn),
                                        ptr(dfl), ctx.stream))
        check(lib().gf_ctx_sync(ctx.handle))
        T = dT.cpu().numpy().reshape(B, 16)
        inl = dinl.cpu().numpy().reshape(B, cap)
        bmh = dbm.cpu().numpy().reshape(B, cap)
        sth = dst.cpu().numpy().view(SIM3_STATE_DTYPE)
        g = drng.cpu().numpy().view(RNG_DTYPE)
        fl, nn = dfl.cpu().numpy(), dn.cpu().numpy()
        for b, n in enumerate(sizes):
            To, io, no, fo, ro, sto, bmo = ref[b][c]
            assert fl[b] == fo and nn[b] == no, (b, c, fl[b], fo, nn[b], no)
            assert T[b].tobytes() == To.tobytes(), (b, c)
            assert np.array_equal(inl[b, :n], io), (b, c)
            assert np.array_equal(bmh[b, :n], bmo), (b, c)
            _assert_state_equal(sth[b:b + 1], sto, (b, c))
            assert g[b:b + 1].tobytes() == _rng_after(500 + b, ro).tobytes(), (b, c)


@pytest.mark.gpu
def test_sim3solver_class_indexing():
    """The Sim3Solver mirror: NULL / bad / unindexed points are skipped (ctor
    :62-103) and vbInliers comes back indexed by KF1 keypoint (:195-197)."""
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
    from gf_orb_slam_amd.sim3 import Rand

    n, n1, n2 = 200, 260, 240
    X1, X2, _, _, K, (s, Rm, t), out = solver_scene(n, 21, 0.3)
    r = np.random.default_rng(0)
    level_s2 = (1.2 ** (2 * np.arange(8))).astype(np.float32)
    # both keyframes at the identity: world = camera, one map point per row of X1 and of X2
    mp_pos = np.concatenate([X1, X2]).astype(np.float32)
    slot1, slot2 = r.permutation(n1)[:n], r.permutation(n2)[:n]
    kf = []
    for nk, slot, first in ((n1, slot1, 0), (n2, slot2, n)):
        kps = np.zeros(nk, KEYPOINT_DTYPE)
        kps["octave"] = r.integers(0, 8, nk)
        ids = np.full(nk, -1, np.int32)
        ids[slot] = first + np.arange(n)
        kf.append(Sim3KeyFrame(np.eye(4, dtype=np.float32), kps, ids, EUROC_K, level_s2))
    matched12 = np.full(n1, -1, np.int32)
    matched12[slot1] = n + np.arange(n)
    bad = np.zeros(2 * n, bool)
    bad[[0, 1, n + 2]] = True                  # pMP1 bad, pMP1 bad, pMP2 bad
    kf[1].mp_ids[slot2[3]] = -1                # pMP2 not indexed in KF2
    matched12[slot1[4]] = -1                   # no match
    spare = np.setdiff1d(np.arange(n1), slot1)[0]
    matched12[spare] = n + 5                   # KF1 slot without a map point of its own
    skipped = np.array([0, 1, 2, 3, 4])
    solver = Sim3Solver(kf[0], kf[1], matched12, mp_pos, bad)
    assert solver.N == n - 5
    keep = np.setdiff1d(np.arange(n), skipped)
    assert np.array_equal(np.sort(solver.kp_idx), np.sort(slot1[keep]))
    solver.set_ransac_parameters(**LOOP)
    T12, no_more, vb, ninl = solver.iterate(300, Rand(3))
    assert T12 is not None and not no_more
    assert abs(solver.estimated_scale() - s) < 1e-4 and np.abs(solver.estimated_rotation() - Rm).max() < 1e-4
    assert np.abs(solver.estimated_translation() - t).max() < 1e-3
    expect = np.zeros(n1, bool)
    expect[slot1[keep]] = ~out[keep]
    assert np.array_equal(vb, expect) and ninl == expect.sum()


# ------------------------------------------------------------------ SearchBySim3
def _info(sc):
    from gf_orb_slam_amd.matcher import FrameInfo

    return FrameInfo.make(*sc["camera"])


def _ref_search(sc, matches12=None, s=None, Rm=None, t=None, th=7.5, swap=False):
    a, b = ("2", "1") if swap else ("1", "2")
    return R.search_by_sim3(_info(sc), sc["T" + a], sc["kps" + a], sc["desc" + a], sc["ids" + a], sc["T" + b],
                            sc["kps" + b], sc["desc" + b], sc["ids" + b], sc["mps"], sc["mp_desc"], sc["mp_bad"],
                            sc["matches12"] if matches12 is None else matches12, sc["s"] if s is None else s,
                            sc["R"] if Rm is None else Rm, sc["t"] if t is None else t, th)


def _gpu_search(sc, s=None, Rm=None, t=None, th=7.5):
    from gf_orb_slam_amd.sim3 import search_by_sim3

    lv = (1.2 ** (2 * np.arange(8))).astype(np.float32)
    kf1 = Sim3KeyFrame(sc["T1"], sc["kps1"], sc["ids1"], sc["camera"][2:], lv)
    kf2 = Sim3KeyFrame(sc["T2"], sc["kps2"], sc["ids2"], sc["camera"][2:], lv)
    return search_by_sim3(_info(sc), kf1, sc["desc1"], kf2, sc["desc2"], sc["mps"], sc["mp_desc"], sc["matches12"],
                          sc["s"] if s is None else s, sc["R"] if Rm is None else Rm, sc["t"] if t is None else t, th,
                          mp_bad=sc["mp_bad"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_search_by_sim3_restatement_properties(seed):
    """On a scene with known point-to-keypoint assignment and the true Sim3:
    pre-matched slots are kept, the number of matches grows by nfound, every new
    pair is one-to-one and is found from the other side as well, and nfound is
    the number of shared points that are neither pre-matched nor bad, each
    matched to its partner."""
    from sim3_scenes import matcher_scene

    sc = matcher_scene(300, seed, n_only=40, prematched=0.3, bad=0.05)
    n1, ns = sc["n1"], sc["n_shared"]
    m_in = sc["matches12"]
    m_out, nf = _ref_search(sc)
    assert np.array_equal(m_out[m_in >= 0], m_in[m_in >= 0])
    assert (m_out >= 0).sum() == (m_in >= 0).sum() + nf
    new = (m_out >= 0) & (m_in < 0)
    assert len(np.unique(m_out[m_out >= 0])) == (m_out >= 0).sum()  # one-to-one, the pre-matched ones included
    free = np.ones(ns, bool)
    free[sc["pre"]] = False
    free &= ~sc["mp_bad"][:ns] & ~sc["mp_bad"][n1:n1 + ns]
    expect = np.full(n1, -1, np.int32)
    expect[sc["slot1"][np.nonzero(free)[0]]] = n1 + np.nonzero(free)[0]
    assert nf == free.sum() and np.array_equal(np.where(new, m_out, -1), expect)
    # mutual: the search from KF2's side with the inverse Sim3 pairs the same keypoints
    s, Rm, t = float(sc["s"]), sc["R"].astype(np.float64), sc["t"].astype(np.float64)
    back = np.full(sc["n2"], -1, np.int32)
    slot_of2 = {int(i): k for k, i in enumerate(sc["ids2"]) if i >= 0}
    for i1 in np.nonzero(m_in >= 0)[0]:
        back[slot_of2[int(m_in[i1])]] = sc["ids1"][i1]
    b_out, nb = _ref_search(sc, back, np.float32(1 / s), Rm.T.astype(np.float32), (-Rm.T @ t / s).astype(np.float32),
                            swap=True)
    pairs12 = {(int(i1), slot_of2[int(m_out[i1])]) for i1 in np.nonzero(new)[0]}
    slot_of1 = {int(i): k for k, i in enumerate(sc["ids1"]) if i >= 0}
    pairs21 = {(slot_of1[int(b_out[i2])], int(i2)) for i2 in np.nonzero((b_out >= 0) & (back < 0))[0]}
    assert nb == nf and pairs12 == pairs21


BOUND_EXPECT = {"max_on": 0, "max_below": 1, "min_on": 1, "min_below": 0, "z0": 0}


@pytest.mark.parametrize("kind", sorted(BOUND_EXPECT))
def test_search_by_sim3_restatement_image_bounds(kind):
    """KeyFrame::IsInImage is min <= u < max; depth 0 passes the `< 0.0` test
    and fails IsInImage through inf / NaN."""
    from sim3_scenes import bound_scene

    m, nf = _ref_search(bound_scene(kind))
    assert nf == BOUND_EXPECT[kind] and list(m) == ([1] if nf else [-1])


def test_search_by_sim3_restatement_tie_order():
    from sim3_scenes import tie_scene

    m, nf = _ref_search(tie_scene())
    assert nf == 1 and list(m) == [-1, 1]


# kwargs of matcher_scene, Sim3 translation offset, th
SEARCH_CASES = [(dict(n_shared=0, seed=1), 0.0, 7.5),
                (dict(n_shared=1, seed=2), 0.0, 7.5),
                (dict(n_shared=60, seed=3, n_only=10), 0.0, 7.5),
                (dict(n_shared=60, seed=4, n_only=10, prematched=0.4), 0.0, 7.5),
                (dict(n_shared=900, seed=5, n_only=200), 0.0, 7.5),
                (dict(n_shared=900, seed=6, n_only=200, prematched=0.3, bad=0.1, behind=30, out_of_range=40), 0.0, 7.5),
                (dict(n_shared=300, seed=7, n_only=60, prematched=0.2, bad=0.05, behind=10, out_of_range=10), 0.01, 7.5),
                (dict(n_shared=300, seed=8, n_only=60), 0.03, 10.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEARCH_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c[0].items()))
def test_search_by_sim3_gpu_bit_exact(case):
    from sim3_scenes import matcher_scene

    kw, off, th = case
    sc = matcher_scene(**kw)
    t = (sc["t"] + np.float32(off)).astype(np.float32)  # a Sim3 that is off by a few pixels
    mo, nfo = _ref_search(sc, t=t, th=th)
    mg, nfg = _gpu_search(sc, t=t, th=th)
    assert nfg == nfo and np.array_equal(mg, mo)
    if kw["n_shared"] >= 60 and off == 0.0:
        assert nfo > kw["n_shared"] // 4  # the case exercises matches, not only rejections


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(BOUND_EXPECT))
def test_search_by_sim3_gpu_image_bounds(kind):
    from sim3_scenes import bound_scene

    sc = bound_scene(kind)
    mg, nfg = _gpu_search(sc)
    mo, nfo = _ref_search(sc)
    assert nfg == nfo == BOUND_EXPECT[kind] and np.array_equal(mg, mo)


@pytest.mark.gpu
def test_search_by_sim3_tie_order():
    """Two keypoints with identical descriptors inside one window, the
    higher-index one in a lower grid column: the column-major first wins, in
    both directions (the pair agrees only then)."""
    from sim3_scenes import tie_scene

    sc = tie_scene()
    mg, nfg = _gpu_search(sc)
    mo, nfo = _ref_search(sc)
    assert nfg == nfo == 1 and list(mg) == list(mo) == [-1, 1]


@pytest.mark.gpu
def test_compute_sim3_pair():
    """LoopClosing::ComputeSim3 up to OptimizeSim3 on two synthetic keyframes of
    one scene: a true candidate (returns a Sim3 whose inliers are all true
    correspondences; SearchBySim3 does not reduce its matches) and a false one
    (KF2's keypoints and descriptors over scrambled map point positions: BoW
    matches, no consistent geometry, discarded with bNoMore). The results equal
    the same loop run on the restatement, the shared rand() state included."""
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary, search_by_bow
    from gf_orb_slam_amd.sim3 import Rand, compute_sim3
    from sim3_scenes import matcher_scene

    sc = matcher_scene(300, 31, n_only=40)
    n1, n2, ns = sc["n1"], sc["n2"], sc["n_shared"]
    lv = (1.2 ** (2 * np.arange(8))).astype(np.float32)
    K = sc["camera"][2:]
    # the false candidate's own map points: KF2's, positions permuted
    mps = np.concatenate([sc["mps"], sc["mps"][n1:][np.random.default_rng(5).permutation(n2)]])
    mp_desc = np.concatenate([sc["mp_desc"], sc["mp_desc"][n1:]])
    ids3 = np.where(sc["ids2"] >= 0, sc["ids2"] + n2, -1).astype(np.int32)
    voc = ORBVocabulary(synth.synth_vocabulary(7, k=10, L=3))
    fv = [voc.transform(d, 4)[2] for d in (sc["desc1"], sc["desc2"])]
    cur = (Sim3KeyFrame(sc["T1"], sc["kps1"], sc["ids1"], K, lv), sc["desc1"], fv[0])
    true_c = (Sim3KeyFrame(sc["T2"], sc["kps2"], sc["ids2"], K, lv), sc["desc2"], fv[1])
    false_c = (Sim3KeyFrame(sc["T2"], sc["kps2"], ids3, K, lv), sc["desc2"], fv[1])
    info = _info(sc)

    def ref_loop(cands, seed):
        rand = [R.rand_values(seed, 3000), 0]
        res = [dict(T12=None, matches=None, discarded=None) for _ in cands]
        solvers = {}
        for i, (kf, desc, f) in enumerate(cands):
            nm, m12 = search_by_bow(1, 0.75, True, (cur[2], cur[1], cur[0].kps, cur[0].mp_ids),
                                    (f, desc, kf.kps, kf.mp_ids))
            if nm < 20:
                res[i]["discarded"] = "few_matches"
                continue
            py = Sim3Solver(cur[0], kf, m12, mps["pos"])
            solvers[i] = (py, m12, R.RefSolver(py.X1, py.X2, py.sigma2_1, py.sigma2_2, py.K1, py.K2, rand, **LOOP))
        active = len(solvers)
        while active > 0:
            for i in sorted(solvers):
                if res[i]["discarded"]:
                    continue
                py, m12, rs = solvers[i]
                T, inl, ni, fl, _ = rs.iterate(5)
                if fl & GF_SIM3_NOMORE:
                    res[i]["discarded"] = "no_more"
                    active -= 1
                if fl & GF_SIM3_FOUND:
                    vb = np.zeros(n1, bool)
                    vb[py.kp_idx[inl.astype(bool)]] = True
                    m = np.where(vb, m12, -1).astype(np.int32)
                    kf, desc, _ = cands[i]
                    st = rs.state
                    m, _ = R.search_by_sim3(info, cur[0].Tcw, cur[0].kps, cur[1], cur[0].mp_ids, kf.Tcw, kf.kps, desc,
                                            kf.mp_ids, mps, mp_desc, None, m, st["best_scale"][0], st["best_R"][0],
                                            st["best_t"][0], 7.5)
                    res[i].update(T12=T.reshape(4, 4), matches=m, vb=vb)
                    return res, rand[1]
        return res, rand[1]

    for cands, want in (([false_c, true_c], [None, None]), ([false_c], ["no_more"])):
        rng = Rand(77)
        got = compute_sim3(info, cur, cands, mps, mp_desc, rng)
        ref, draws = ref_loop(cands, 77)
        assert [g["discarded"] for g in got] == [r["discarded"] for r in ref] == want
        assert rng.state.tobytes() == _rng_after(77, draws).tobytes()
        for g, r in zip(got, ref):
            assert (g["T12"] is None) == (r["T12"] is None)
            if g["T12"] is not None:
                assert g["T12"].tobytes() == r["T12"].tobytes() and np.array_equal(g["matches"], r["matches"])
    got = compute_sim3(info, cur, [false_c, true_c], mps, mp_desc, Rand(77))
    ref, _ = ref_loop([false_c, true_c], 77)
    g, vb = got[1], ref[1]["vb"]
    assert got[0]["T12"] is None and g["T12"] is not None and g["n_inliers"] == vb.sum() > 20
    truth = np.full(n1, -1, np.int32)
    truth[sc["slot1"][:ns]] = n1 + np.arange(ns)
    _, bow12 = search_by_bow(1, 0.75, True, (cur[2], cur[1], cur[0].kps, cur[0].mp_ids),
                             (true_c[2], true_c[1], true_c[0].kps, true_c[0].mp_ids))
    assert np.array_equal(bow12[vb], truth[vb])                      # every inlier is a true correspondence
    assert (g["matches"] >= 0).sum() >= vb.sum()                      # SearchBySim3 does not reduce them
    assert np.array_equal(g["matches"][vb], bow12[vb])
    assert abs(g["s"] - float(sc["s"])) < 1e-3 and np.abs(g["R"] - sc["R"]).max() < 1e-3


@pytest.mark.gpu
def test_sim3_dev_truncated_call():
    """gf_sim3_iterate_dev with max_iterations below the call's loop count: the
    problem runs max_iterations iterations (as a call of that count would) and
    is flagged TRUNCATED; a problem that returns a Sim3 inside the bound is not."""
    import torch

    from gf_orb_slam_amd.matcher import default_context
    from gf_orb_slam_amd.sim3 import GF_SIM3_TRUNCATED

    dev = torch.device("cuda:0")
    n = 30
    K = np.asarray(EUROC_K, np.float32)
    scenes = [solver_scene(n, 12, 0.6), solver_scene(n, 11, 0.0)]  # never found / found at once
    st = np.zeros(2, SIM3_STATE_DTYPE)
    rng = np.zeros(2, RNG_DTYPE)
    ref = []
    for b, (X1, X2, s1, s2, _, _, _) in enumerate(scenes):
        check(lib().gf_sim3_init(n, ptr(sim3_params(**LOOP)), ptr(st[b:b + 1])))
        rng[b:b + 1] = _rng_after(40 + b, 0)
        ref.append(R.run(X1, X2, s1, s2, K, K, 40 + b, [4], **LOOP)[0])
    assert ref[0][3] == 0 and ref[1][3] == GF_SIM3_FOUND and st["max_iterations"][0] > 10
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    cat = lambda k: np.stack([np.asarray(s[k], np.float32) for s in scenes])  # noqa: E731
    d1, d2, dg1, dg2, dst, drng = t(cat(0)), t(cat(1)), t(cat(2)), t(cat(3)), t(st), t(rng)
    dbm = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
    dT = torch.zeros(2 * 16, dtype=torch.float32, device=dev)
    dinl = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
    dn = torch.zeros(2, dtype=torch.int32, device=dev)
    dfl = torch.zeros(2, dtype=torch.int32, device=dev)
    ctx = default_context()
    check(lib().gf_sim3_iterate_dev(ctx.handle, 2, ptr(d1), ptr(d2), ptr(dg1), ptr(dg2), n, ptr(K), ptr(K), ptr(dst),
                                    ptr(dbm), 10, 4, ptr(drng), ptr(dT), ptr(dinl), ptr(dn), ptr(dfl), ctx.stream))
    check(lib().gf_ctx_sync(ctx.handle))
    fl = dfl.cpu().numpy()
    assert fl[0] == GF_SIM3_TRUNCATED and fl[1] == GF_SIM3_FOUND
    sth = dst.cpu().numpy().view(SIM3_STATE_DTYPE)
    g = drng.cpu().numpy().view(RNG_DTYPE)
    T = dT.cpu().numpy().reshape(2, 16)
    for b in range(2):
        To, io, no, _, ro, sto, bmo = ref[b]
        _assert_state_equal(sth[b:b + 1], sto, b)
        assert T[b].tobytes() == To.tobytes() and dn[b].item() == no
        assert np.array_equal(dinl.cpu().numpy().reshape(2, n)[b], io)
        assert np.array_equal(dbm.cpu().numpy().reshape(2, n)[b], bmo)
        assert g[b:b + 1].tobytes() == _rng_after(40 + b, ro).tobytes()
