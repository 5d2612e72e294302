"""ctypes loader of tests/helpers/libsim3optref.so, the tests' CPU restatement
of Optimizer::OptimizeSim3 and of the Sim3 SearchByProjection
(tests/helpers/sim3opt_ref.cpp), and the scene generators of
tests/test_sim3_optimize.py."""
import ctypes
import os

import numpy as np

from gf_orb_slam_amd._lib import ptr
from sim3_scenes import EUROC_K, H, W, _rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K2_CAM = (435.2, 435.9, 380.1, 236.7)  # a second camera: K1 != K2
_ref = None


def ref():
    global _ref
    if _ref is None:
        _ref = ctypes.CDLL(os.path.join(ROOT, "tests", "helpers", "libsim3optref.so"))
        _ref.sim3optref_optimize.restype = ctypes.c_int
        _ref.sim3optref_search_projection.restype = ctypes.c_int
        _ref.sim3optref_jacobian.restype = None
        _ref.sim3optref_quat_from_R.restype = None
        _ref.sim3optref_scw.restype = None
    return _ref


def quat_from_R(R):
    q = np.zeros(4, np.float64)
    Rf = np.ascontiguousarray(R, np.float32).reshape(9)  # held in a name until the call has read it
    ref().sim3optref_quat_from_R(ptr(Rf), ptr(q))
    return q


def scw(gScm, Tmw):
    """mScw as LoopClosing.cc:343-345 builds it (g2o::Sim3 product, then
    Converter::toCvMat) -> (Scw 4x4 float32, gScw 8 doubles)."""
    S = np.zeros(16, np.float32)
    g = np.zeros(8, np.float64)
    a, T = np.ascontiguousarray(gScm, np.float64).reshape(8), np.ascontiguousarray(Tmw, np.float32).reshape(16)
    ref().sim3optref_scw(ptr(a), ptr(T), ptr(S), ptr(g))
    return S.reshape(4, 4), g


def optimize(X1, X2, z1, z2, w1, w2, K1, K2, S12, th2=10.0):
    """-> dict: nin, S (8 doubles), inlier [n], its (2), trials (2), asked
    (round-two iteration count asked for, 0 = returned before it), nbad,
    by_count (2: the round ended on its iteration count, not on a Terminate of
    the LM, so a larger count would have run another iteration), chi2 [n, 4]
    (e12, e21 at the first check, e12, e21 at the second; NaN = not tested)."""
    c = lambda a, k: np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, k))  # noqa: E731
    X1, X2, z1, z2 = c(X1, 3), c(X2, 3), c(z1, 2), c(z2, 2)
    w1, w2 = np.ascontiguousarray(w1, np.float32).reshape(-1), np.ascontiguousarray(w2, np.float32).reshape(-1)
    n = len(X1)
    S = np.ascontiguousarray(S12, np.float64).reshape(8).copy()
    inl = np.zeros(max(n, 1), np.uint8)
    stats = np.zeros(8, np.int32)
    chi2 = np.zeros((max(n, 1), 4), np.float64)
    K1 = np.ascontiguousarray(K1, np.float32).reshape(4)
    K2 = np.ascontiguousarray(K2, np.float32).reshape(4)
    nin = ref().sim3optref_optimize(n, ptr(X1), ptr(X2), ptr(z1), ptr(z2), ptr(w1), ptr(w2), ptr(K1), ptr(K2),
                                    ctypes.c_float(th2), ptr(S), ptr(inl), ptr(stats), ptr(chi2))
    return dict(nin=int(nin), S=S, inlier=inl[:n].copy(), its=stats[0:2].copy(), trials=stats[2:4].copy(),
                asked=int(stats[4]), nbad=int(stats[5]), by_count=stats[6:8].astype(bool),
                chi2=chi2[:n].copy())


def jacobian(S, X1, X2, K1, K2):
    """The restatement's central-difference Jacobians of one pair -> (J12, J21), 2 x 7 each."""
    d = lambda a, k: np.ascontiguousarray(a, np.float64).reshape(k)  # noqa: E731
    J12, J21 = np.zeros((2, 7)), np.zeros((2, 7))
    S, X1, X2, K1, K2 = d(S, 8), d(X1, 3), d(X2, 3), d(K1, 4), d(K2, 4)
    ref().sim3optref_jacobian(ptr(S), ptr(X1), ptr(X2), ptr(K1), ptr(K2), ptr(J12), ptr(J21))
    return J12, J21


def search_projection(info, Scw, kps, desc, mps, mp_desc, mp_bad, points, matched, th=10):
    """The restated SearchByProjection(pKF, Scw, ...) -> (matched, nmatches)."""
    c = np.ascontiguousarray
    m = c(matched, np.int32).copy()
    S = c(Scw, np.float32).reshape(16)
    kps, desc, mps, mp_desc = c(kps), c(desc, np.uint8), c(mps), c(mp_desc, np.uint8)
    pts = c(points, np.int32).reshape(-1)
    bad = None if mp_bad is None else c(np.asarray(mp_bad).astype(np.uint8))
    nm = ref().sim3optref_search_projection(ctypes.byref(info), ptr(S), ptr(kps), ptr(desc), len(kps), ptr(mps),
                                            ptr(mp_desc), ptr(bad), ptr(pts) if len(pts) else None, len(pts), ptr(m),
                                            int(th))
    return m, int(nm)


# ------------------------------------------------------------------ scenes
def _project(X, K):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


def opt_scene(n, seed, outliers=0.0, noise=0.0, K1=EUROC_K, K2=K2_CAM):
    """n pairs of a noise-free two-view scene with a ground-truth (s, R, t):
    X1 in camera 1 (inside both images), X2 = R^T (X1 - t) / s in camera 2, the
    keypoints their exact projections (+ `noise` pixels of Gaussian noise),
    octaves U{0..7}. A fraction `outliers` of the pairs is permuted (X2 and z2
    rows shifted cyclically among themselves). The start estimate is 3 degrees,
    5% in scale and a few centimetres off. -> dict."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.5, 2.0)
    R = _rot(*rng.uniform(-0.3, 0.3, 3))
    t = rng.uniform(-0.5, 0.5, 3)
    X1 = np.zeros((0, 3))
    while len(X1) < n:
        z = rng.uniform(2, 8, 4 * max(n, 8))
        u, v = rng.uniform(20, W - 20, len(z)), rng.uniform(20, H - 20, len(z))
        c = np.stack([(u - K1[2]) / K1[0] * z, (v - K1[3]) / K1[1] * z, z], 1)
        c2 = (c - t) @ R / s
        ok = c2[:, 2] > 0.5
        p2 = _project(np.where(ok[:, None], c2, 1.0), K2)
        ok &= (p2[:, 0] > 20) & (p2[:, 0] < W - 20) & (p2[:, 1] > 20) & (p2[:, 1] < H - 20)
        X1 = np.concatenate([X1, c[ok]])
    X1 = X1[:n].astype(np.float32)
    X2 = ((X1.astype(np.float64) - t) @ R / s).astype(np.float32)
    z1 = _project(X1.astype(np.float64), K1)
    z2 = _project(X2.astype(np.float64), K2)
    if noise:
        z1 = z1 + rng.normal(0, noise, z1.shape)
        z2 = z2 + rng.normal(0, noise, z2.shape)
    oct1, oct2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    lv = np.float32(1.2) ** (2 * np.arange(8, dtype=np.float32))
    lv = lv.astype(np.float32)
    out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k >= 2:
        idx = np.sort(rng.permutation(n)[:k])
        out[idx] = True
        X2[idx] = X2[np.roll(idx, 1)]
        z2[idx] = z2[np.roll(idx, 1)]
    # the start: 3 degrees about a random axis, 5% scale, a few centimetres
    ax = rng.normal(0, 1, 3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(3.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    dR = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    s0, R0, t0 = np.float32(s * 1.05), (dR @ R).astype(np.float32), (t + rng.uniform(-0.03, 0.03, 3)).astype(np.float32)
    S0 = np.zeros(8, np.float64)
    S0[:4] = quat_from_R(R0)
    S0[4:7] = t0.astype(np.float64)
    S0[7] = float(s0)
    return dict(X1=X1, X2=X2, z1=z1.astype(np.float32), z2=z2.astype(np.float32),
                w1=(np.float32(1) / lv[oct1]).astype(np.float32), w2=lv[oct2].astype(np.float32), oct1=oct1, oct2=oct2,
                K1=np.asarray(K1, np.float32), K2=np.asarray(K2, np.float32), truth=(s, R, t), out=out, S0=S0)


def args(sc):
    return (sc["X1"], sc["X2"], sc["z1"], sc["z2"], sc["w1"], sc["w2"], sc["K1"], sc["K2"], sc["S0"])


def s_R_t(S):
    """8 doubles -> (s, R, t) with R = toRotationMatrix() of the quaternion."""
    from gf_orb_slam_amd.optimizer import sim3_from_g2o

    return sim3_from_g2o(S)


# ------------------------------------------------------- projection scenes
LEVELS = 8


def _info():
    from gf_orb_slam_amd.matcher import FrameInfo

    return FrameInfo.make(W, H, *EUROC_K)


def _f32_project(pos, K=EUROC_K):
    """The float32 projection of the search for an identity pose: invz = 1/z,
    u = fx*(X*invz) + cx."""
    f = np.float32
    X, Y, Z = (f(c) for c in pos)
    invz = f(1) / Z
    return f(f(K[0]) * f(X * invz)) + f(K[2]), f(f(K[1]) * f(Y * invz)) + f(K[3])


def tiny_proj_scene(kps, pts, matched=None):
    """Identity Scw. kps: list of (x, y, octave, desc[32] or byte); pts: list of
    dicts pos, level (predicted: ratio = 1.2^(level - 0.5)), desc, and
    optionally min_dist / max_dist / normal / bad. The candidates are all the
    points in list order. -> dict."""
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    def d32(d):
        return np.full(32, d, np.uint8) if np.isscalar(d) else np.asarray(d, np.uint8)

    k = np.zeros(len(kps), KEYPOINT_DTYPE)
    kd = np.zeros((len(kps), 32), np.uint8)
    for i, (x, y, o, d) in enumerate(kps):
        k["x"][i], k["y"][i], k["octave"][i] = x, y, o
        kd[i] = d32(d)
    mps = np.zeros(len(pts), MAP_POINT_DTYPE)
    md = np.zeros((len(pts), 32), np.uint8)
    bad = np.zeros(len(pts), bool)
    for i, p in enumerate(pts):
        pos = np.asarray(p["pos"], np.float32)
        dist = float(np.sqrt((pos.astype(np.float64) ** 2).sum()))
        mps["pos"][i] = pos
        mps["min_dist"][i] = p.get("min_dist", dist / 1.2 ** (p.get("level", 1) - 0.5))
        mps["max_dist"][i] = p.get("max_dist", mps["min_dist"][i] * np.float32(1.2 ** 12))
        mps["normal"][i] = p.get("normal", pos / np.float32(dist))
        md[i] = d32(p.get("desc", 0))
        bad[i] = p.get("bad", False)
    m = np.full(len(kps), -1, np.int32) if matched is None else np.asarray(matched, np.int32)
    return dict(Scw=np.eye(4, dtype=np.float32), kps=k, desc=kd, mps=mps, mp_desc=md, mp_bad=bad,
                points=np.arange(len(pts), dtype=np.int32), matched=m)


def point_at(u, v, z=4.0, K=EUROC_K):
    """A float32 camera point that projects near (u, v), and its exact float32 projection."""
    pos = np.array([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], np.float32)
    return pos, _f32_project(pos, K)


def flip_bits(desc, nbits):
    """A copy of the 32-byte descriptor with its first `nbits` bits flipped."""
    d = np.array(desc, np.uint8).copy()
    for b in range(nbits):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def proj_scene(nkp, ncand, seed, scale=1.0, prematched=0.1, bad=0.05, crowd=0.3):
    """A keyframe of nkp keypoints and ncand candidate map points under a random
    pose, Scw = scale * (Rcw | tcw). The first nkp-ish candidates own a keypoint
    near their projection (octave = predicted level or one below, descriptor a
    few bits off); a fraction `crowd` of the others are near-copies of an
    earlier candidate (same place, close descriptor), so that candidates
    contend for one keypoint. -> dict."""
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    rng = np.random.default_rng(seed)
    K = EUROC_K
    T = np.eye(4)
    T[:3, :3] = _rot(*rng.uniform(-0.3, 0.3, 3))
    T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    z = rng.uniform(2, 8, ncand)
    u, v = rng.uniform(-40, W + 40, ncand), rng.uniform(-40, H + 40, ncand)
    C = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
    behind = rng.random(ncand) < 0.03
    C[behind, 2] *= -1
    base = rng.integers(0, 256, (ncand, 32), dtype=np.uint8)
    for i in range(nkp, ncand):
        if rng.random() < crowd:
            j = int(rng.integers(0, nkp))
            C[i] = C[j] * (1 + rng.uniform(-1e-3, 1e-3))
            base[i] = base[j]
    Ow = -T[:3, :3].T @ T[:3, 3]
    pos = (C - T[:3, 3]) @ T[:3, :3]
    a = rng.integers(0, 7, ncand)
    dist = np.linalg.norm(pos - Ow, axis=1)
    mps = np.zeros(ncand, MAP_POINT_DTYPE)
    mps["pos"] = pos
    mps["min_dist"] = dist / 1.2 ** (a + 0.5)
    mps["max_dist"] = mps["min_dist"] * np.float32(1.2 ** 8)
    far = rng.random(ncand) < 0.04
    mps["max_dist"][far] = (dist * 0.9)[far]
    nrm = (pos - Ow) / dist[:, None]
    tilt = rng.random(ncand) < 0.05  # viewed from more than 60 degrees
    nrm[tilt] = np.cross(nrm[tilt], [0.3, 0.5, 0.8])
    nrm[tilt] /= np.linalg.norm(nrm[tilt], axis=1)[:, None]
    mps["normal"] = nrm
    from sim3_scenes import _flip

    mp_desc = _flip(rng, base)
    kps = np.zeros(nkp, KEYPOINT_DTYPE)
    kps["x"] = K[0] * C[:nkp, 0] / C[:nkp, 2] + K[2] + rng.uniform(-3, 3, nkp)
    kps["y"] = K[1] * C[:nkp, 1] / C[:nkp, 2] + K[3] + rng.uniform(-3, 3, nkp)
    kps["octave"] = a[:nkp] + 1 - (rng.random(nkp) < 0.3) - 2 * (rng.random(nkp) < 0.05)
    order = rng.permutation(nkp)
    kps = kps[order]
    desc = _flip(rng, base[:nkp])[order]
    matched = np.full(nkp, -1, np.int32)
    slot_of = np.argsort(order)
    for j in np.nonzero(rng.random(nkp) < prematched)[0]:
        matched[slot_of[j]] = j
    Scw = T.copy()
    Scw[:3] *= scale
    return dict(Scw=Scw.astype(np.float32), kps=kps, desc=desc, mps=mps, mp_desc=mp_desc,
                mp_bad=rng.random(ncand) < bad, points=rng.permutation(ncand).astype(np.int32), matched=matched)


def ref_search(sc, th=10, **over):
    a = dict(sc, **over)
    return search_projection(_info(), a["Scw"], a["kps"], a["desc"], a["mps"], a["mp_desc"], a["mp_bad"], a["points"],
                             a["matched"], th)
