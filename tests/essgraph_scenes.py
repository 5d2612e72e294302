"""Scene generator of the essential-graph tests (tests/test_essgraph_cpu.py,
tests/test_essgraph_gpu.py): a closed trajectory with accumulated rotation,
translation and scale drift, a branching spanning tree, covisibility weights on
both sides of 100, optional past loop edges and kf_id gaps, a loop between the
last keyframe and an early one, and map points with mixed references.

A scene is the argument tuple of gf_orb_slam_amd.optimizer.EssGraphArrays:
(map, loop_kf, cur_kf, NonCorrectedSim3, CorrectedSim3, LoopConnections)."""
import numpy as np

import essgraph_ref as R


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose_inverse_f32(T):
    """KeyFrame::GetPoseInverse in float: [R^T | -R^T t]."""
    T = np.asarray(T, np.float32)
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = T[:3, :3].T
    Twc[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Twc


def propagate(Tcw, cur, neighbours, Scw):
    """LoopClosing.cc:432-459 through the restatement's Sim3 arithmetic ->
    (NonCorrectedSim3, CorrectedSim3), dicts over `neighbours` and cur."""
    Twc = pose_inverse_f32(Tcw[cur])
    non, cor = {}, {cur: np.asarray(Scw, np.float64).copy()}
    for i in list(neighbours) + [cur]:
        Tiw = np.asarray(Tcw[i], np.float32)
        if i != cur:
            Tic = (Tiw @ Twc).astype(np.float32)
            cor[i] = R.sim_mul(R.sim_from_pose(Tic), Scw)
        non[i] = R.sim_from_pose(Tiw)
    return non, cor


def make_scene(N, seed, past_loops=False, gaps=False, npts=300, drift=1.0):
    rng = np.random.default_rng(seed)
    # true poses on a circle, the camera looking along the tangent
    ang = 2 * np.pi * np.arange(N) / N
    Twc_true = []
    for a in ang:
        T = np.eye(4)
        T[:3, :3] = _rot(0.05 * np.sin(3 * a), 0.0, a)
        T[:3, 3] = [5 * np.cos(a), 5 * np.sin(a), 0.3 * np.sin(2 * a)]
        Twc_true.append(T)
    # accumulated drift D_i = (s, Rd, td): world point p -> s Rd p + td
    s, Rd, td = 1.0, np.eye(3), np.zeros(3)
    sD, Tcw = [], []
    for i in range(N):
        if i:
            s *= 1.0 + drift * rng.uniform(0.001, 0.004)
            Rd = _rot(*(drift * rng.uniform(-0.003, 0.003, 3))) @ Rd
            td = td + drift * rng.uniform(-0.01, 0.01, 3)
        Twc = np.eye(4)
        Twc[:3, :3] = Rd @ Twc_true[i][:3, :3]
        Twc[:3, 3] = s * (Rd @ Twc_true[i][:3, 3]) + td
        sD.append(s)
        Tcw.append(np.linalg.inv(Twc).astype(np.float32))
    Tcw = np.stack(Tcw)
    cur, loop = N - 1, (1 if N >= 4 else 0)
    # mg2oScw: the current keyframe as the loop side sees it, at the loop side's scale
    Tc = np.linalg.inv(Twc_true[cur])
    sc = sD[cur] / sD[loop]
    Scw = np.zeros(8)
    Scw[:4] = R.sim_from_pose(Tc.astype(np.float32))[:4]
    Scw[4:7] = sc * Tc[:3, 3]
    Scw[7] = sc

    # covisibility: weights fall off with the id distance
    W = {}
    for i in range(N):
        for j in range(i + 1, min(N, i + 7)):
            w = int(260 * np.exp(-(j - i) / 2.5) + rng.integers(-25, 26))
            if w >= 15:
                W[(i, j)] = w
    # the loop side seen from the current keyframe and its neighbours after the fusion
    near_cur = [k for k in range(max(0, cur - 3), cur) if k != loop]
    near_loop = [k for k in range(max(0, loop - 1), min(N - 4, loop + 3)) if k not in near_cur and k != cur]
    lc = {cur: {loop}}
    W[(min(cur, loop), max(cur, loop))] = 40  # kept by the (current, loop) exception
    wsel = [130, 60, 101, 99, 150, 100]
    q = 0
    for a in [cur] + near_cur:
        for b in near_loop:
            if (a, b) == (cur, loop) or a == b:
                continue
            key = (min(a, b), max(a, b))
            if key in W:
                continue
            w = wsel[q % len(wsel)]
            q += 1
            W[key] = w
            if q % 4 != 0:  # every fourth new link is not a loop connection: a plain covisibility edge
                lc.setdefault(a, set()).add(b)
    cov = []
    for i in range(N):
        nb = [(w, (a if b == i else b)) for (a, b), w in W.items() if i in (a, b)]
        nb.sort(key=lambda t: (-t[0], t[1]))
        cov.append(([n for _, n in nb], [w for w, _ in nb]))
    # spanning tree with a few branches
    parent = np.arange(-1, N - 1)
    for i in range(5, N, 7):
        parent[i] = i - int(rng.integers(2, 4))
    loop_edges = [[] for _ in range(N)]
    if past_loops:
        for a, b in ((N // 2, N // 6), ((3 * N) // 4, N // 3)):
            if a != b and abs(a - b) > 7:
                loop_edges[a].append(b)
                loop_edges[b].append(a)
    kf_id = np.cumsum(rng.integers(1, 4, N)) if gaps else np.arange(N)

    neighbours = sorted(cov[cur][0])
    neighbours = [k for k in neighbours if k != loop] if N > 3 else [k for k in neighbours if k != loop]
    non, cor = propagate(Tcw, cur, neighbours, Scw)

    # map points around their reference keyframe
    ref = rng.integers(0, N, npts)
    pos = np.zeros((npts, 3), np.float32)
    for m in range(npts):
        Twc = np.linalg.inv(Tcw[ref[m]].astype(np.float64))
        pos[m] = (Twc[:3, :3] @ rng.uniform([-1, -1, 2], [1, 1, 6]) + Twc[:3, 3]).astype(np.float32)
    ref = np.where(rng.random(npts) < 0.1, -1, ref)
    bad = rng.random(npts) < 0.1
    ckeys = sorted(cor)
    cref = np.where(rng.random(npts) < 0.3, np.asarray(ckeys)[rng.integers(0, len(ckeys), npts)], -1)
    map_ = dict(kf_id=kf_id, Tcw=Tcw, parent=parent, cov=cov, loop_edges=loop_edges, pos=pos, bad=bad, ref=ref,
                corrected_ref=cref)
    return (map_, loop, cur, non, cor, {k: sorted(v) for k, v in lc.items()})


def scale_chain(M, D):
    """The closed-form problem: keyframes 0..M with identity rotation and zero
    translation, parent = i - 1, loop keyframe 0, only the current keyframe M
    corrected, by the log-scale D, LoopConnections = {M: {0}}. EdgeSim3's error is
    then the log-scale difference alone and keyframe i ends at the log scale
    i D / (M + 1). The poses [R | t/s] stay the identity; point i (reference
    keyframe i) shows the scale: it is multiplied by s_before / s_after."""
    N = M + 1
    Tcw = np.stack([np.eye(4, dtype=np.float32)] * N)
    non = {M: np.array([0, 0, 0, 1, 0, 0, 0, 1.0], np.float64)}
    cor = {M: np.array([0, 0, 0, 1, 0, 0, 0, np.exp(D)], np.float64)}
    cov = [([], []) for _ in range(N)]
    pos = np.array([[1.0, 2.0, 3.0]], np.float32) * (1 + 0.1 * np.arange(N, dtype=np.float32))[:, None]
    map_ = dict(kf_id=np.arange(N), Tcw=Tcw, parent=np.arange(-1, N - 1), cov=cov,
                loop_edges=[[] for _ in range(N)], pos=pos, bad=np.zeros(N, bool), ref=np.arange(N),
                corrected_ref=np.full(N, -1))
    return (map_, 0, M, non, cor, {M: [0]})
