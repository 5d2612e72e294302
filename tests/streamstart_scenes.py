"""Start requests for gf_frontend_start_streams: ``mapupdate_scenes``-style
graphs of chosen sizes read as a delta against the empty map, a random frame
that becomes mLastFrame, optional keyframe database rows; and the map a
``MonoInitializer`` / ``create_initial_map`` makes of an ``initmap_scenes``
problem (device)."""
import numpy as np

import mapupdate_scenes as S
from gf_orb_slam_amd.localmap import StreamStart
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

EMPTY = dict(mp=np.zeros(0, MAP_POINT_DTYPE), desc=np.zeros((0, 32), np.uint8), graph=S.graph_of([], [], [], [], []))


def graph_map(seed, nmp, nkf, slots=(1, 40), obs=None, odd_offsets=False):
    """``mapupdate_scenes.random_map``; obs (int): exactly that many
    observations in total."""
    m = S.random_map(seed, nmp, nkf, slots=slots, odd_offsets=odd_offsets)
    if obs is not None:
        m = S.evolve(seed + 1000, m, obs=int(obs), cov=False, obs_most=max(4, nkf))
        assert len(m["graph"]["mp_obs"]) == obs
    return m


def keypoints(rng, n):
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = rng.uniform(0, 752, n).astype(np.float32)
    k["y"] = rng.uniform(0, 480, n).astype(np.float32)
    k["size"] = 31.0
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.uniform(20, 200, n).astype(np.float32)
    k["octave"] = rng.integers(0, 8, n)
    k["class_id"] = -1
    return k


def pose(rng):
    a = rng.normal(size=(3, 3))
    q, _ = np.linalg.qr(a)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = q.astype(np.float32)
    T[:3, 3] = rng.uniform(-1, 1, 3).astype(np.float32)
    return T


def db_rows(m, transform, seed):
    """One database row set per keyframe of the map (random keypoints and
    descriptors, one per slot) -> (pipeline.KeyframeDB of rows, kps, desc)."""
    from gf_orb_slam_amd.pipeline import KeyframeDB

    rng = np.random.default_rng(seed)
    ns = np.diff(m["graph"]["kf_mp_off"])
    kps = [keypoints(rng, int(n)) for n in ns]
    desc = [rng.integers(0, 256, (int(n), 32), dtype=np.uint8) for n in ns]
    return KeyframeDB(kps, desc, transform), kps, desc


def request(stream, m, n_last, seed, rows=None, frame_id=None, since_reloc=None) -> StreamStart:
    """The start of ``stream`` on map ``m`` with a random last frame of n_last
    keypoints, about two thirds of which hold a point of the map."""
    rng = np.random.default_rng(seed)
    d = S.diff(stream, EMPTY, m)
    d.kf_rows = rows
    nmp = len(m["mp"])
    kp2mp = np.where(rng.random(n_last) < 0.66, rng.integers(0, max(nmp, 1), n_last), -1) if nmp else np.full(n_last, -1)
    fid = int(rng.integers(1, 5000)) if frame_id is None else frame_id
    return StreamStart(d, keypoints(rng, n_last), rng.integers(0, 256, (n_last, 32), dtype=np.uint8), kp2mp, pose(rng),
                       timestamp=float(rng.uniform(0, 100)), frame_id=fid,
                       since_reloc=int(rng.integers(0, 40)) if since_reloc is None else since_reloc)


def initial_loopmap(seed, voc=None):
    """CreateInitialMap of ``initmap_scenes.two_view(seed)`` on the device ->
    (LoopMap, scene, report)."""
    import initmap_scenes
    from gf_orb_slam_amd import tracking

    sc = initmap_scenes.two_view(seed)
    m, rep = tracking.create_initial_map(initmap_scenes.INFO, sc["K"], *initmap_scenes.args(sc), voc=voc)
    assert m is not None, rep
    return m, sc, rep


def refusal_cases(cap, M, transform):
    """Requests gf_frontend_start_streams must refuse, on a four-stream front
    end (map_cap M >= cap + 2) whose stream 1 has a growable database of max_kf
    4 and max_rows 200, stream 2 a fixed one and streams 0 and 3 none -> ({name: (request, code)}, the two
    valid requests that travel with them, the map they start)."""
    m = graph_map(600, 20, 2, slots=(3, 9))

    def req(b, mm=m, n_last=10, **kw):
        rows = db_rows(mm, transform, 77)[0] if b == 1 and len(mm["graph"]["kf_bad"]) else None
        r = request(b, mm, n_last, 41, rows=rows)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def with_delta(b, **kw):
        r = req(b)
        for k, v in kw.items():
            setattr(r.map, k, np.asarray(v, getattr(r.map, k).dtype))
        return r

    r_kp = req(0)
    r_kp.kp2mp = r_kp.kp2mp.copy()
    r_kp.kp2mp[3] = 20
    r_obs = req(0)
    r_obs.map.obs_kf = r_obs.map.obs_kf.copy()
    r_obs.map.obs_kf[0] = 2
    r_rows = req(1)
    r_rows.map.kf_rows = db_rows(graph_map(601, 10, 1, slots=(3, 9)), transform, 78)[0]  # one keyframe's rows for two
    norows = req(1)
    norows.map.kf_rows = None
    big = np.zeros(cap + 1, KEYPOINT_DTYPE)
    i32 = lambda v: np.asarray(v, np.int32)  # noqa: E731

    def raw(b=0, **kw):
        """The valid request with arrays of its delta replaced as they are."""
        r = req(b)
        for k, v in kw.items():
            setattr(r.map, k, v if isinstance(v, (bool, np.ndarray)) else i32(v))
        return r

    assert M >= cap + 2
    # 64 keyframes of cap + 1 slots: one more than the 64 x cap slot capacity allows in each
    wide = graph_map(605, 10, 64, slots=(cap + 1, cap + 1), obs=0)
    # cap + 2 points that all 64 keyframes observe: 128 observations above the capacity
    many = graph_map(606, cap + 2, 64, slots=(1, 2), obs=0)
    r_obs_cap = req(0, mm=many, n_last=0)
    r_obs_cap.map.obs_mp = np.arange(cap + 2, dtype=np.int32)
    r_obs_cap.map.obs_off = (64 * np.arange(cap + 3)).astype(np.int32)
    r_obs_cap.map.obs_kf = np.tile(np.arange(64, dtype=np.int32), cap + 2)
    bad = {
        "a rewritten point": (with_delta(0, set_mp_idx=[0], set_mp=m["mp"][:1], set_mp_desc=m["desc"][:1]), -1),
        "a bad point": (with_delta(0, bad_mp=[1]), -1),
        "a bad keyframe": (with_delta(0, bad_kf=[0]), -1),
        "a slot write": (with_delta(0, slot_kf=[0], slot_idx=[0], slot_val=[1]), -1),
        "kp2mp out of range": (r_kp, -1),
        "reference keyframe out of range": (req(0, ref_kf=2), -1),
        "an observation of a keyframe out of range": (r_obs, -1),
        "stream out of range": (req(4), -1),
        "stream named twice": (req(0), -1),
        "rows without a database": (request(0, m, 5, 1, rows=db_rows(m, transform, 79)[0]), -1),
        "rows that differ from the keyframes": (r_rows, -1),
        "more keypoints than the capacity": (req(0, kps=big, desc=np.zeros((cap + 1, 32), np.uint8),
                                                 kp2mp=np.full(cap + 1, -1, np.int32)), -3),
        "more points than map_cap": (req(0, mm=graph_map(602, M + 1, 1, slots=(1, 5))), -3),
        "more than 64 keyframes": (req(0, mm=graph_map(603, 10, 65, slots=(1, 2))), -3),
        "more database rows than max_rows": (req(1, mm=graph_map(604, 10, 3, slots=(70, 80))), -3),
        "more slots than the capacity": (req(0, mm=wide, n_last=0), -3),
        "more observations than the capacity": (r_obs_cap, -3),
        "more covisibility entries than keyframes squared": (raw(has_cov=True, kf_cov_off=[0, 3, 5],
                                                                 kf_cov=[1, 0, 1, 0, 1]), -3),
        "more keyframes than the database's max_kf": (req(1, mm=graph_map(607, 10, 5, slots=(2, 4))), -3),
        "an observation row that is not ascending": (raw(obs_mp=[0], obs_off=[0, 2], obs_kf=[1, 0]), -1),
        "two observation rows for one point": (raw(obs_mp=[3, 3], obs_off=[0, 1, 2], obs_kf=[0, 1]), -1),
        "keyframe offsets that are not ascending": (raw(new_kf_off=[0, 5, 3]), -1),
        "covisibility offsets that are not ascending": (raw(has_cov=True, kf_cov_off=[0, 2, 1], kf_cov=[1, 0]), -1),
        "a slot value out of range": (raw(new_kf_mp=np.where(np.arange(len(req(0).map.new_kf_mp)) == 1, 20,
                                                              req(0).map.new_kf_mp).astype(np.int32)), -1),
        "a covisible keyframe out of range": (raw(has_cov=True, kf_cov_off=[0, 1, 1], kf_cov=[2]), -1),
        "a fixed database": (req(2), -4),
        "a growable database without rows": (norows, -4),
    }
    return bad, [req(0), req(3)], m
