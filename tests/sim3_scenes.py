"""Scene generators for tests/test_sim3.py."""
import numpy as np

EUROC_K = (458.654, 457.296, 367.215, 248.375)
W, H = 752, 480


def _rot(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rz = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    Ry = np.array([[cc, 0, sc], [0, 1, 0], [-sc, 0, cc]])
    return Rz @ Rx @ Ry


def _flip(rng, base, nbits=3):
    """Copies of 32-byte descriptors with up to `nbits` bits flipped each."""
    d = base.copy()
    for row in d:
        for _ in range(int(rng.integers(0, nbits + 1))):
            row[rng.integers(0, 32)] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return d


def _pose(rng):
    T = np.eye(4)
    T[:3, :3] = _rot(*rng.uniform(-0.2, 0.2, 3))
    T[:3, 3] = rng.uniform(-0.3, 0.3, 3)
    return T


def _to_world(T, Xc):
    return (Xc - T[:3, 3]) @ T[:3, :3]  # rows: R^T (x - t)


def matcher_scene(n_shared, seed, n_only=0, prematched=0.0, bad=0.0, behind=0, out_of_range=0, K=EUROC_K):
    """Two keyframes of one scene, in maps related by a ground-truth Sim3
    (Xc1 = s R Xc2 + t). `n_shared` physical points are seen by both: map point
    p in KF1's map, n1 + p in KF2's, a keypoint each (slot tables permuted),
    descriptors a few bits apart. Scale-invariance distances put the predicted
    level of each projection at the partner keypoint's octave or one above.
    n_only: extra points per keyframe seen by it alone; prematched: fraction of
    shared points already in matches12; bad: fraction of all map points bad;
    behind: KF1 points behind camera 2; out_of_range: shared points whose
    projection falls outside [min_dist, max_dist]. -> dict."""
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    s = rng.uniform(0.5, 2.0)
    R = _rot(*rng.uniform(-0.15, 0.15, 3))
    t = rng.uniform(-0.3, 0.3, 3)

    def proj(X):
        return np.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)

    def cam_points(m):
        z = rng.uniform(2, 8, m)
        u, v = rng.uniform(30, W - 30, m), rng.uniform(30, H - 30, m)
        return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)

    X1 = np.zeros((0, 3))
    while len(X1) < n_shared:  # shared points: inside both images with a margin
        c = cam_points(4 * max(n_shared, 8))
        c2 = (c - t) @ R / s
        p2 = proj(c2)
        ok = (c2[:, 2] > 0.5) & (p2[:, 0] > 30) & (p2[:, 0] < W - 30) & (p2[:, 1] > 30) & (p2[:, 1] < H - 30)
        X1 = np.concatenate([X1, c[ok]])
    X1 = X1[:n_shared]
    X2 = (X1 - t) @ R / s
    only1, only2 = cam_points(n_only), cam_points(n_only)
    hind2 = cam_points(behind) * [1, 1, -1]  # camera 2 coordinates, behind it
    hind1 = s * hind2 @ R.T + t
    C1 = np.concatenate([X1, only1, hind1])  # camera-1 coordinates of KF1's map points
    C2 = np.concatenate([X2, only2])
    n1, n2 = len(C1), len(C2)
    T1, T2 = _pose(rng), _pose(rng)
    pos = np.concatenate([_to_world(T1, C1), _to_world(T2, C2)])
    nmp = n1 + n2
    mps = np.zeros(nmp, MAP_POINT_DTYPE)
    mps["pos"] = pos
    # predicted level of a point in the other camera: ratio = 1.2^(a + 0.5) -> level a + 1
    a1, a2 = rng.integers(0, 7, n1), rng.integers(0, 7, n2)
    other1 = np.linalg.norm((C1 - t) @ R / s, axis=1)   # KF1's points seen from camera 2
    other2 = np.linalg.norm(s * C2 @ R.T + t, axis=1)   # KF2's points seen from camera 1
    mps["min_dist"][:n1] = other1 / 1.2 ** (a1 + 0.5)
    mps["min_dist"][n1:] = other2 / 1.2 ** (a2 + 0.5)
    mps["max_dist"] = mps["min_dist"] * np.float32(1.2 ** 8)
    for p in range(min(out_of_range, n_shared)):
        if p % 2:
            mps["min_dist"][p] = other1[p] * 1.5
            mps["max_dist"][p] = other1[p] * 6
        else:
            mps["max_dist"][p] = other1[p] * 0.9
    base = rng.integers(0, 256, (nmp, 32), dtype=np.uint8)
    base[n1:n1 + n_shared] = base[:n_shared]
    mp_desc = _flip(rng, base)
    slot1, slot2 = rng.permutation(n1), rng.permutation(n2)
    kf, desc = [], []
    for (C, slot, first, a_other) in ((C1, slot1, 0, a2), (C2, slot2, n1, a1)):
        n = len(C)
        kps = np.zeros(n, KEYPOINT_DTYPE)
        uv = proj(C)
        kps["x"][slot], kps["y"][slot] = uv[:, 0], uv[:, 1]
        octave = rng.integers(0, 8, n)
        # the partner's map point predicts level a + 1 here: octave a + 1 or a
        octave[:n_shared] = a_other[:n_shared] + 1 - (rng.random(n_shared) < 0.3)
        kps["octave"][slot] = octave
        ids = np.full(n, -1, np.int32)
        ids[slot] = first + np.arange(n)
        d = np.zeros((n, 32), np.uint8)
        d[slot] = _flip(rng, base[first:first + n])
        kf.append((kps, ids))
        desc.append(d)
    matches12 = np.full(n1, -1, np.int32)
    pre = np.nonzero(rng.random(n_shared) < prematched)[0]
    matches12[slot1[pre]] = n1 + pre
    mp_bad = rng.random(nmp) < bad
    return dict(camera=(W, H) + tuple(K), T1=T1.astype(np.float32), T2=T2.astype(np.float32), kps1=kf[0][0],
                ids1=kf[0][1], desc1=desc[0], kps2=kf[1][0], ids2=kf[1][1], desc2=desc[1], mps=mps, mp_desc=mp_desc,
                mp_bad=mp_bad, matches12=matches12, s=np.float32(s), R=R.astype(np.float32), t=t.astype(np.float32),
                slot1=slot1, slot2=slot2, n_shared=n_shared, n1=n1, n2=n2, pre=pre)


def _tiny_scene(kp1, kp2, ids1, ids2, pos, K=EUROC_K):
    """Identity poses and identity Sim3, all descriptors equal, every map point
    predicting level 1, every keypoint at octave 1."""
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    def kps(xy):
        k = np.zeros(len(xy), KEYPOINT_DTYPE)
        k["x"], k["y"] = np.asarray(xy, np.float32).reshape(-1, 2).T
        k["octave"] = 1
        return k

    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    mps = np.zeros(len(pos), MAP_POINT_DTYPE)
    mps["pos"] = pos
    d = np.maximum(np.linalg.norm(pos.astype(np.float64), axis=1), 1e-3)
    mps["min_dist"] = d / 1.2 ** 0.5
    mps["max_dist"] = mps["min_dist"] * np.float32(1.2 ** 8)
    eye = np.eye(4, dtype=np.float32)
    z = lambda n: np.zeros((n, 32), np.uint8)  # noqa: E731
    return dict(camera=(W, H) + tuple(K), T1=eye, T2=eye.copy(), kps1=kps(kp1), ids1=np.asarray(ids1, np.int32),
                desc1=z(len(kp1)), kps2=kps(kp2), ids2=np.asarray(ids2, np.int32), desc2=z(len(kp2)), mps=mps,
                mp_desc=z(len(pos)), mp_bad=np.zeros(len(pos), bool), matches12=np.full(len(kp1), -1, np.int32),
                s=np.float32(1), R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32))


def _x_for_u(u_target, K=EUROC_K):
    """A float32 X with fx*X + cx == u_target exactly in float32 arithmetic (depth 1)."""
    fx, cx = np.float32(K[0]), np.float32(K[2])
    x = np.float32((np.float32(u_target) - cx) / fx)
    for cand in [x] + [f(x, k) for k in range(1, 200) for f in (_up, _down)]:
        if np.float32(fx * cand) + cx == np.float32(u_target):
            return cand
    raise AssertionError("no float32 X reaches the target column")


def _up(x, k):
    for _ in range(k):
        x = np.nextafter(x, np.float32(np.inf))
    return x


def _down(x, k):
    for _ in range(k):
        x = np.nextafter(x, np.float32(-np.inf))
    return x


def bound_scene(kind, K=EUROC_K):
    """One KF1 map point whose projection into image 2 sits on an image bound
    (KeyFrame::IsInImage: min <= u < max), with a partner that matches it back
    whenever the projection is accepted. kind: max_on (u == 752, rejected),
    max_below (largest float under 752, accepted), min_on (u == 0, accepted),
    min_below (rejected), z0 (depth 0 passes `< 0.0` and fails IsInImage)."""
    fy, cy = K[1], K[3]
    u_kp = {"max_on": 745.0, "max_below": 745.0,"min_on": 2.0, "min_below": 2.0, "z0": 375.0}[kind]
    fx32, cx32 = np.float32(K[0]), np.float32(K[2])
    yv = np.float32((240.0 - cy) / fy)
    if kind == "z0":
        a = [0.0, 0.0, 0.0]
    else:
        bound = np.float32(W if kind.startswith("max") else 0)
        x = _x_for_u(bound, K)
        if kind.endswith("below"):
            while np.float32(fx32 * x) + cx32 >= bound:
                x = _down(x, 1)
        a = [x, yv, 1.0]
    b = [np.float32((u_kp - K[2]) / K[0]), yv, 1.0]  # KF2's point, seen in image 1 at KF1's keypoint
    return _tiny_scene([(u_kp, 240.0)], [(u_kp, 240.0)], [0], [1], [a, b], K)


def tie_scene(K=EUROC_K):
    """Two keypoints with identical descriptors inside one window, in both
    keyframes: index 1 at x = 394 (grid column 34), index 0 at x = 406 (column
    35). GetFeaturesInArea lists column 34 first, so index 1 wins the tie in
    both directions and the pair (1, 1) agrees; the lowest index would give
    (1 -> 0) and no match."""
    kp = [(406.0, 240.0), (394.0, 240.0)]
    p = [np.float32((400.0 - K[2]) / K[0] * 4), np.float32((240.0 - K[3]) / K[1] * 4), 4.0]
    return _tiny_scene(kp, kp, [-1, 0], [-1, 1], [p, p], K)


def solver_scene(n, seed, outliers=0.3, noise=0.0, K=EUROC_K):
    """n points in camera 1 (z in 2..8, inside the 752x480 frustum), a
    ground-truth (s, R, t) with s in [0.5, 2] and X2 = R^T (X1 - t) / s,
    octaves U{0..7} (sigma^2 = 1.2^(2 oct)) for both keypoints. A fraction
    `outliers` of the X2 rows is permuted among themselves (a cyclic shift, so
    no row stays in place); `noise` is 3-D Gaussian noise on X2 as a fraction
    of its depth. -> X1, X2, sigma2_1, sigma2_2, K, (s, R, t), outlier flags."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    z = rng.uniform(2, 8, n)
    u = rng.uniform(0, W, n)
    v = rng.uniform(0, H, n)
    X1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    s = rng.uniform(0.5, 2.0)
    R = _rot(*rng.uniform(-0.3, 0.3, 3))
    t = rng.uniform(-0.5, 0.5, 3)
    X2 = (X1 - t) @ R / s  # rows: R^T (x - t) / s
    if noise:
        X2 = X2 + rng.normal(0, 1, (n, 3)) * (noise * np.abs(X2[:, 2:3]))
    s1 = (1.2 ** (2 * rng.integers(0, 8, n))).astype(np.float32)
    s2 = (1.2 ** (2 * rng.integers(0, 8, n))).astype(np.float32)
    out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k >= 2:
        idx = np.sort(rng.permutation(n)[:k])
        out[idx] = True
        X2[idx] = X2[np.roll(idx, 1)]
    return (np.ascontiguousarray(X1, np.float32), np.ascontiguousarray(X2, np.float32), s1, s2,
            np.asarray(K, np.float32), (s, R, t), out)
