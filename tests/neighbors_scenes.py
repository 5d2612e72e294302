"""A synthetic map for SearchInNeighbors: six good neighbours and a bad one
around a new keyframe that overlaps all of them, every world point seen from
every pose, several map points per world point (near-duplicates held by
different keyframes), with the situations the serial reference is sensitive to
planted on purpose (see ``neighbors_scene``)."""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd import synth
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, FrameInfo
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

NLEVELS, SCALE = 8, 1.2
SF = np.array([np.float32(1.0)] * NLEVELS, np.float32)
for _i in range(1, NLEVELS):
    SF[_i] = np.float32(SF[_i - 1] * np.float32(SCALE))
N_GOOD = 6          # keyframes 0 .. 5
BAD_KF = N_GOOD     # a neighbour with isBad() set
CUR = N_GOOD + 1    # the new keyframe
KF_ID = np.array([3, 5, 6, 8, 11, 12, 14, 17], np.int32)  # mnId: increasing, not the index


def _level(dist, min_dist):
    return np.minimum(np.searchsorted(SF.astype(np.float64), dist / min_dist, side="left"), NLEVELS - 1)


def neighbors_scene(seed=5, n_world=400, see=0.9, kp_extra=10, n_good=N_GOOD):
    """-> dict with the LoopMap / RefWorld constructor arrays (``info, kf_kps,
    kf_desc, kf_mp, mps, mp_desc, mp_bad, observations, kf_bad, kf_Tcw, ref_kf,
    kf_id``), ``cur``, ``bad_kf`` and ``roles`` (world point -> role). Keyframes
    0 .. n_good-1 are the good neighbours, then the bad one, then the new one.

    A world point w has a base descriptor; every keyframe that sees it has a
    keypoint at its projection whose row is the base with up to 10 bits
    flipped. Its map points ("instances") sit within a millimetre of it. Roles:
      old       up to three instances, each held by some of one third of the
                neighbours; the new keyframe's keypoint is free: the backward
                call adds the first and replaces the others by it;
      new       an instance seen by the new keyframe and one neighbour (a point
                CreateNewMapPoints just made). In a fifth of them another
                neighbour holds an older instance: the forward call adds and
                replaces by the occupant. Up to two more neighbours hold a rival
                instance at a keypoint whose row is far from the base (as
                ``brepl`` below): the forward search reaches the descriptors and
                misses, the backward search replaces the rival by the occupant;
      tracked   an instance seen by the new keyframe and two neighbours;
      none      keypoints without a map point.
    The new keyframe sees every world point but half of the ``none`` ones, so
    that few entries of its slot table are NULL, and every point it holds comes
    back as a backward candidate that is already in it; the ``old`` instances
    and the rivals are the backward candidates that reach the descriptors.
    Planted:
      twin      two keypoints of the new keyframe hold two instances; every
                neighbour's keypoint is free: the second is replaced by the first
                (forward, by an earlier candidate) and Replace erases its slot;
      fkeep     a neighbour's keypoint holds a bad point, the new keyframe a good one;
      stale     the new keyframe tracks an instance whose descriptor is far from
                every row, and holds a fresh instance at a second keypoint; two
                neighbours hold the tracked one. Replace into it recomputes its
                descriptor, after which it matches where it did not;
      brepl     a neighbour's keypoint row is far from the base while the instance it
                holds has a descriptor near it: the forward search misses, the
                backward search replaces it by the new keyframe's occupant;
      bkeep     the new keyframe's keypoint holds a bad point, a neighbour a good one."""
    rng = np.random.default_rng(seed)
    cam = synth.CAMERAS["euroc"]
    w, h = cam[0], cam[1]
    info = FrameInfo.make(*cam, nlevels=NLEVELS, scale_factor=SCALE)
    BAD_KF, CUR = n_good, n_good + 1  # noqa: N806
    nkf = CUR + 1
    X = np.stack([rng.uniform(-2.2, 2.2, n_world), rng.uniform(-1.4, 1.4, n_world), rng.uniform(4, 8, n_world)], 1)
    poses = [synth.look_pose(rng, 0.12, 1.0).astype(np.float32) for _ in range(nkf)]
    O0 = -(poses[0][:3, :3].astype(np.float64).T @ poses[0][:3, 3])
    d0 = np.linalg.norm(X - O0, axis=1)
    level = rng.integers(1, 6, n_world)
    min_dist = d0 / (SF[level] * 0.97)
    normal = (X - O0) / d0[:, None]
    base = rng.integers(0, 256, (n_world, 32), dtype=np.uint8)

    names = ["twin", "fkeep", "stale", "brepl", "bkeep"]
    perm = rng.permutation(n_world)
    roles, lo = {}, 0
    for nme, cnt in zip(names, [8, 6, 8, 8, 6]):
        for i in perm[lo:lo + cnt]:
            roles[int(i)] = nme
        lo += cnt
    for i in perm[lo:]:
        roles[int(i)] = str(rng.choice(["old", "new", "tracked", "none"], p=[0.18, 0.57, 0.21, 0.04]))

    pts = dict(pos=[], desc=[], world=[], bad=[], ref=[])

    def instance(wi, desc=None, bad=False, ref=-1):
        pts["pos"].append(X[wi] + rng.normal(0, 5e-4, 3))
        pts["desc"].append(synth.flip_bits(rng, base[wi:wi + 1], 5)[0] if desc is None else desc)
        pts["world"].append(wi)
        pts["bad"].append(bad)
        pts["ref"].append(ref)
        return len(pts["world"]) - 1

    far = lambda wi: synth.flip_bits(rng, base[wi:wi + 1] ^ np.uint8(0xF0), 4)[0]  # 128 bits from the base  # noqa: E731

    # which keyframes see which world point; planted points are seen by all
    sees = rng.uniform(size=(nkf, n_world)) < see
    for wi, r in roles.items():
        if r in names:
            sees[:, wi] = True
        sees[CUR, wi] = r != "none" or rng.uniform() < 0.5
    # slot plan: (keyframe, world point) -> instance, and a second keypoint of the new keyframe
    plan, second, row_far = {}, {}, set()
    good = list(range(n_good))
    nb_all = good + [BAD_KF]
    thirds = [nb_all[i::3] for i in range(3)]
    for wi in range(n_world):
        r = roles[wi]
        seen_nb = [k for k in nb_all if sees[k, wi]]
        if r == "old":
            for third in thirds:
                ks = [k for k in third if sees[k, wi] and rng.uniform() < 0.85]
                if ks and rng.uniform() < 0.9:
                    p = instance(wi, ref=ks[0])
                    plan.update({(k, wi): p for k in ks})
        elif r == "new" and sees[CUR, wi] and seen_nb:
            nb = int(rng.choice(seen_nb))
            p = instance(wi, ref=CUR)
            plan[(CUR, wi)] = plan[(nb, wi)] = p
            others = [int(k) for k in rng.permutation([k for k in seen_nb if k != nb and k != BAD_KF])]
            if others and rng.uniform() < 0.2:
                k = others.pop()
                plan[(k, wi)] = instance(wi, ref=k)
            for k in others[:2]:
                if rng.uniform() < 0.6:
                    plan[(k, wi)] = instance(wi, ref=k)
                    row_far.add((k, wi))
        elif r == "tracked" and sees[CUR, wi] and len(seen_nb) >= 2:
            ks = [int(k) for k in rng.choice(seen_nb, 2, replace=False)]
            p = instance(wi, ref=min(ks))
            plan.update({(k, wi): p for k in ks + [CUR]})
        elif r == "twin":
            plan[(CUR, wi)] = instance(wi, ref=CUR)
            second[wi] = instance(wi, ref=CUR)
        elif r == "fkeep":
            plan[(CUR, wi)] = instance(wi, ref=CUR)
            for k in rng.choice(good, 2, replace=False):
                plan[(int(k), wi)] = instance(wi, bad=True)
        elif r == "stale":
            ka, kb = (int(k) for k in rng.choice(good, 2, replace=False))
            p = instance(wi, desc=far(wi), ref=min(ka, kb))
            plan.update({(ka, wi): p, (kb, wi): p, (CUR, wi): p})
            second[wi] = instance(wi, ref=CUR)
        elif r == "brepl":
            k = int(rng.choice(good))
            plan[(k, wi)] = instance(wi, ref=k)
            row_far.add((k, wi))
            for k2 in nb_all:  # nobody else sees it: the new keyframe's instance stays where it is
                if k2 != k:
                    sees[k2, wi] = False
            plan[(CUR, wi)] = instance(wi, ref=CUR)
        elif r == "bkeep":
            plan[(CUR, wi)] = instance(wi, bad=True)
            k = int(rng.choice(good))
            plan[(k, wi)] = instance(wi, ref=k)

    nmp = len(pts["world"])
    wid = np.asarray(pts["world"])
    mps = np.zeros(nmp, MAP_POINT_DTYPE)
    mps["pos"] = np.asarray(pts["pos"])
    mps["normal"] = normal[wid]
    mps["min_dist"] = min_dist[wid]
    mps["max_dist"] = mps["min_dist"] * SF[-1] * 1.2
    mp_desc = np.asarray(pts["desc"], np.uint8)
    mp_bad = np.asarray(pts["bad"], bool)

    kf_kps, kf_desc, kf_mp = [], [], []
    for j, T in enumerate(poses):
        u, v, z = synth.project(T.astype(np.float64), X, cam)
        Oj = -(T[:3, :3].astype(np.float64).T @ T[:3, 3])
        lvl = _level(np.linalg.norm(X - Oj, axis=1), min_dist)
        rows = []  # (x, y, octave, desc row, slot)
        for wi in range(n_world):
            if not sees[j, wi] or not (z[wi] > 0 and 4 <= u[wi] < w - 4 and 4 <= v[wi] < h - 4):
                continue
            x, y = u[wi] + rng.uniform(-0.6, 0.6), v[wi] + rng.uniform(-0.6, 0.6)
            octv = max(int(lvl[wi]) - int(rng.uniform() < 0.3), 0)
            row = far(wi) if (j, wi) in row_far else synth.flip_bits(rng, base[wi:wi + 1], 10)[0]
            rows.append((x, y, octv, row, plan.get((j, wi), -1)))
            if j == CUR and wi in second:
                rows.append((x + 0.4, y - 0.3, octv, synth.flip_bits(rng, base[wi:wi + 1], 10)[0], second[wi]))
        for _ in range(kp_extra):
            rows.append((rng.uniform(0, w - 1), rng.uniform(0, h - 1), int(rng.integers(0, NLEVELS)),
                         rng.integers(0, 256, 32, dtype=np.uint8), -1))
        order = rng.permutation(len(rows))
        kps = np.zeros(len(order), KEYPOINT_DTYPE)
        desc = np.zeros((len(order), 32), np.uint8)
        slots = np.full(len(order), -1, np.int32)
        for k, o in enumerate(order):
            kps["x"][k], kps["y"][k], kps["octave"][k], desc[k], slots[k] = rows[o]
        kps["size"], kps["class_id"] = 31 * SF[kps["octave"]], -1
        kf_kps.append(kps), kf_desc.append(desc), kf_mp.append(slots)

    # a bad point keeps its slot but has no observations (SetBadFlag cleared them; the slot is planted)
    observations = [dict() for _ in range(nmp)]
    for k, s in enumerate(kf_mp):
        for idx in np.nonzero(s >= 0)[0]:
            if not mp_bad[s[idx]]:
                observations[int(s[idx])][k] = int(idx)
    ref_kf = np.asarray(pts["ref"], np.int32)
    for p, o in enumerate(observations):
        if o and ref_kf[p] not in o:
            ref_kf[p] = min(o)
    kf_bad = np.zeros(nkf, bool)
    kf_bad[BAD_KF] = True
    return dict(info=info, kf_kps=kf_kps, kf_desc=kf_desc, kf_mp=kf_mp, mps=mps, mp_desc=mp_desc, mp_bad=mp_bad,
                observations=observations, kf_bad=kf_bad, kf_Tcw=np.stack(poses), ref_kf=ref_kf,
                kf_id=KF_ID.copy() if nkf == len(KF_ID) else (3 + 2 * np.arange(nkf)).astype(np.int32),
                cur=CUR, bad_kf=BAD_KF, roles=roles, world=wid)


_KEYS = ("info", "kf_kps", "kf_desc", "kf_mp", "mps", "mp_desc", "mp_bad", "observations", "kf_bad")


def ref_world(sc):
    """The restatement's world of the scene, its covisibility graph built by
    UpdateConnections of every keyframe in index order (the bad one included:
    it was good when it was connected)."""
    from neighbors_ref import RefWorld

    kw = {k: sc[k] for k in ("kf_Tcw", "ref_kf", "kf_id")}
    good = np.zeros(len(sc["kf_bad"]), bool)
    w = RefWorld(*[sc[k] for k in _KEYS[:-1]], kf_bad=good, **kw)
    for k in range(len(sc["kf_kps"])):
        w.update_connections(k)
    for k in np.nonzero(sc["kf_bad"])[0]:
        w.set_bad_kf(k)
    return w


def loop_map(sc, **kw):
    """The LoopMap of the scene, prepared as :func:`ref_world`."""
    from gf_orb_slam_amd.loopmap import LoopMap

    m = LoopMap(*[sc[k] for k in _KEYS[:-1]], kf_bad=None, kf_Tcw=sc["kf_Tcw"], ref_kf=sc["ref_kf"], kf_id=sc["kf_id"],
                **kw)
    for k in range(m.nkf):
        m.update_connections(k)
    m.kf_bad[:] = sc["kf_bad"]
    return m


_CACHE = {}


def small():
    if "small" not in _CACHE:
        _CACHE["small"] = neighbors_scene()
    return _CACHE["small"]
