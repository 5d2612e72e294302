"""Two-frame problems for the initial map (Tracking::CreateInitialMap):
``two_view`` runs the CPU oracle's initialiser on ``synth_two_view`` and adds
descriptors; ``hand_made`` builds the initialiser's output directly, for the
shapes and ties the tests need (any n1, duplicated KFcur indices, depths with
ties, untriangulated matches)."""
from __future__ import annotations

import ctypes

import numpy as np

from gf_orb_slam_amd._lib import check, lib, ptr
from gf_orb_slam_amd.initializer import INIT_RESULT_DTYPE
from gf_orb_slam_amd.matcher import FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
from gf_orb_slam_amd.pnp import RNG_DTYPE
from gf_orb_slam_amd.synth import synth_two_view

W, H, F = 752, 480, 458.0
INFO = FrameInfo.make(W, H, F, F, W / 2, H / 2)


def rng_state(seed):
    r = np.zeros(1, RNG_DTYPE)
    check(lib().gf_rng_seed(ptr(r), ctypes.c_uint32(seed)))
    return r


def _desc(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def two_view(seed, mask=0, **kw) -> dict:
    """synth_two_view(seed, **kw) through the oracle's Initializer::Initialize
    (rand() seeded with the scene seed). mask: that many triangulated matches
    (the first ones in index order) are reported as not triangulated, to step
    the point count down."""
    import oracle_lib as O

    d = synth_two_view(seed, **kw)
    rng = np.random.default_rng(1000 + seed)
    rc, res, p3d, tri = O.initialize(d["K"], d["kps1"], d["kps2"], d["matches12"], rng_state(seed))
    assert rc == 0
    tri = tri.copy()
    if mask:
        idx = np.nonzero((d["matches12"] >= 0) & (tri != 0))[0][:mask]
        tri[idx] = 0
    return dict(info=INFO, K=d["K"], kps1=d["kps1"], desc1=_desc(rng, len(d["kps1"])), kps2=d["kps2"],
                desc2=_desc(rng, len(d["kps2"])), matches12=d["matches12"].copy(), init=res, p3d=p3d, tri=tri)


def _kps(rng, n):
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(5, W - 5, n), rng.uniform(5, H - 5, n)
    k["size"], k["class_id"] = 31.0, -1
    k["octave"] = rng.integers(0, 8, n)
    return k


def hand_made(seed, n1, n2=None, nmatch=None, tri_frac=0.8, dup=0, tie_depths=False, ok=1, negative=False) -> dict:
    """The initialiser's output made by hand: n1 / n2 keypoints, nmatch
    matches at random indices (an injection, then ``dup`` matches redirected
    to an already used KFcur keypoint), a fraction marked triangulated, points
    in front of both cameras (tie_depths: z drawn from three values;
    negative: behind KFini, for the median test)."""
    rng = np.random.default_rng(seed)
    n2 = n1 + 7 if n2 is None else n2
    nmatch = min(n1, n2) if nmatch is None else nmatch
    m = np.full(n1, -1, np.int32)
    src = np.sort(rng.choice(n1, nmatch, replace=False)) if nmatch else np.zeros(0, np.int64)
    m[src] = rng.choice(n2, nmatch, replace=False) if nmatch else []
    tri = np.zeros(n1, np.uint8)
    tri[src] = rng.random(nmatch) < tri_frac
    tri[(m < 0) & (rng.random(n1) < 0.1)] = 1  # flags on unmatched keypoints mean nothing
    good = src[tri[src] != 0]
    z = rng.choice([2.0, 3.0, 5.0], n1) if tie_depths else rng.uniform(2.0, 8.0, n1)
    if negative:
        z = -z
    p3d = np.c_[rng.uniform(-1, 1, n1) * z, rng.uniform(-0.6, 0.6, n1) * z, z].astype(np.float32)
    for q in range(min(dup, len(good) // 2)):  # two triangulated matches (of one 3-D point) share one KFcur keypoint
        m[good[2 * q + 1]] = m[good[2 * q]]
        p3d[good[2 * q + 1]] = p3d[good[2 * q]]
    res = np.zeros(1, INIT_RESULT_DTYPE)
    res["ok"], res["model"], res["nmatches"] = ok, 1, nmatch
    a = 0.05
    res["R21"][0] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32).reshape(9)
    res["t21"][0] = np.array([-0.95, 0.05, 0.3], np.float32)
    # matched keypoints sit near the projections of their point, so the bundle adjustment has a minimum to find
    k1, k2 = _kps(rng, n1), _kps(rng, n2)
    R, t = res["R21"][0].reshape(3, 3).astype(np.float64), res["t21"][0].astype(np.float64)
    for i in src:
        X = p3d[i].astype(np.float64)
        X2 = R @ X + t
        k1["x"][i], k1["y"][i] = F * X[0] / X[2] + W / 2 + rng.normal(0, 0.5), F * X[1] / X[2] + H / 2 + rng.normal(0, 0.5)
        k2["x"][m[i]], k2["y"][m[i]] = (F * X2[0] / X2[2] + W / 2 + rng.normal(0, 0.5),
                                        F * X2[1] / X2[2] + H / 2 + rng.normal(0, 0.5))
    return dict(info=INFO, K=np.array([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1]], np.float32), kps1=k1,
                desc1=_desc(rng, n1), kps2=k2, desc2=_desc(rng, n2), matches12=m, init=res, p3d=p3d,
                tri=tri)


def device_batch(scs):
    """Scenes as the [P, cap...] device tensors of initial_map_points_device."""
    import torch

    P = len(scs)
    c1 = max(1, max(len(s["kps1"]) for s in scs))
    c2 = max(1, max(len(s["kps2"]) for s in scs))
    k1, k2 = np.zeros((P, c1), KEYPOINT_DTYPE), np.zeros((P, c2), KEYPOINT_DTYPE)
    d1, d2 = np.zeros((P, c1, 32), np.uint8), np.zeros((P, c2, 32), np.uint8)
    n1, n2 = np.zeros(P, np.int32), np.zeros(P, np.int32)
    m, init = np.full((P, c1), -1, np.int32), np.zeros(P, INIT_RESULT_DTYPE)
    p3d, tri = np.zeros((P, c1, 3), np.float32), np.zeros((P, c1), np.uint8)
    for p, s in enumerate(scs):
        a, b = len(s["kps1"]), len(s["kps2"])
        n1[p], n2[p] = a, b
        k1[p, :a], k2[p, :b], d1[p, :a], d2[p, :b] = s["kps1"], s["kps2"], s["desc1"], s["desc2"]
        m[p, :a], init[p], p3d[p, :a], tri[p, :a] = s["matches12"], s["init"][0], s["p3d"], s["tri"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    return (dev(k1.view(np.uint8).reshape(P, c1, 28)), dev(d1), dev(n1), dev(k2.view(np.uint8).reshape(P, c2, 28)),
            dev(d2), dev(n2), dev(m), dev(init.view(np.uint8).reshape(P, 200)), dev(p3d), dev(tri))


def args(sc: dict) -> tuple:
    """The positional arguments of initmap_ref.points / tracking.create_initial_map after info."""
    return (sc["kps1"], sc["desc1"], sc["kps2"], sc["desc2"], sc["matches12"], sc["init"], sc["p3d"], sc["tri"])
