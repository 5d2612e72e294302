"""Map compaction on the device (csrc/mapcompact.hip, gf_frontend_compact_maps)
against the serial restatement (tests/helpers/mapcompact_ref.cpp): every map
field, the graph and every index holder over the shapes at which the kernels
can go wrong, the pins, the refusals, then a compaction inside a tracked
sequence: a stream compacted of everything bad against its untouched twin
(eager and through a graph captured before the compaction), and a window
against the oracle chain on the restricted map; the closed loop tracker ->
keyframe -> mapper -> feed_back with a compaction in it, below and past the
capacities; last the growable keyframe database that follows a compaction. Every comparison of the feature's own outputs is byte equality."""
import numpy as np
import pytest

import mapcompact_ref as R
import mapcompact_scenes as CS
import mapupdate_scenes as S
import oracle_chain as C
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.localmap import MapCompact, MapDelta, MapRemap
from gf_orb_slam_amd.pipeline import STATS, FrontEnd

pytestmark = pytest.mark.gpu

POINT_FIELDS = ["map", "map_desc", "views", "mp_H", "mp_info", "mp_uv", "mp_upd"]
HOLDERS = ["kp2mp", "nkp", "last_kp2mp", "last_nkp", "left", "stats", "reloc", "nmp"]
NLEFT = STATS.index("nleft")


# ---------------------------------------------------------------- 1. tables against the restatement
def _frontend(maps, M, nfeatures=150, seed=0, free=()):
    """A front end over ``maps`` (one per stream) whose buffers hold random
    per-point state on the used rows and sentinels past them, and frame state
    (current frame, last frame, leftovers) that holds random points; the
    streams in ``free`` hold none, so that everything listed can go."""
    B = len(maps)
    fe = FrontEnd("euroc", nfeatures, B, M, 100)
    rng = np.random.default_rng(seed)
    for b, m in enumerate(maps):
        fe.set_map(b, m["mp"], m["desc"])
        fe.set_covis(b, m["graph"])
    st = {k: fe.read(k) for k in POINT_FIELDS + HOLDERS}
    for b, m in enumerate(maps):
        n = len(m["mp"])
        for k in ("map", "map_desc", "views", "mp_upd"):
            st[k][b, n:].view(np.uint8)[...] = S.SENTINEL
        st["views"][b, :n].view(np.uint8)[...] = rng.integers(0, 256, st["views"][b, :n].view(np.uint8).shape)
        st["mp_upd"][b, :n] = rng.integers(-5, 3, n)
        for k in ("mp_H", "mp_info", "mp_uv"):
            st[k][b] = rng.normal(size=st[k][b].shape)
        st["reloc"][b].view(np.uint8)[...] = rng.integers(0, 256, st["reloc"][b].view(np.uint8).shape)
        hold = n > 0 and b not in free
        for k, nk in (("kp2mp", "nkp"), ("last_kp2mp", "last_nkp")):
            st[nk][b] = int(rng.integers(fe.cap // 2, fe.cap + 1)) if hold else 0
            st[k][b] = np.where(rng.random(fe.cap) < 0.2, rng.integers(0, max(n, 1), fe.cap), -1) if n else -1
        st["left"][b] = rng.integers(0, max(n, 1), fe.M)
        st["stats"][NLEFT, b] = int(rng.integers(0, n + 1))
    for k in POINT_FIELDS + HOLDERS:
        if k != "nmp":
            fe.write(k, st[k])
    return fe


def _states(fe, has_db=()):
    """The restatement's State of every stream, from the device."""
    st = {k: fe.read(k) for k in POINT_FIELDS + HOLDERS}
    out = []
    for b in range(fe.B):
        n = int(st["nmp"][b])
        g = fe.covis(b)
        out.append(R.State(fe.M, fe.cap, dict(g, mp_bad=g["mp_bad"][:n]), point_rows={k: st[k][b] for k in POINT_FIELDS},
                           kf_rows=dict(reloc=st["reloc"][b]), has_db=b in has_db, kp2mp=st["kp2mp"][b],
                           nkp=st["nkp"][b], last_kp2mp=st["last_kp2mp"][b], last_nkp=st["last_nkp"][b],
                           left=st["left"][b], nleft=st["stats"][NLEFT, b]))
    return out, st


def _assert_device_equals(fe, states, st0, what):
    """Every map field, the graph and every index holder of every stream equal
    the restatement's state (which, for a stream not named, is what it was)."""
    now = {k: fe.read(k) for k in POINT_FIELDS + HOLDERS}
    assert now["stats"].tobytes() == st0["stats"].tobytes() and now["nkp"].tobytes() == st0["nkp"].tobytes(), what
    assert now["last_nkp"].tobytes() == st0["last_nkp"].tobytes(), what
    for b, s in enumerate(states):
        tag = f"{what}: stream {b}"
        assert int(now["nmp"][b]) == s.nmp, tag
        for k in POINT_FIELDS:
            assert now[k][b].tobytes() == s.point_rows[k].tobytes(), f"{tag}: {k}"
        assert now["reloc"][b].tobytes() == s.kf_rows["reloc"].tobytes(), f"{tag}: reloc"
        for k in ("kp2mp", "last_kp2mp", "left"):
            assert np.array_equal(now[k][b], getattr(s, k)), f"{tag}: {k}"
        assert R.same_graph(fe.covis(b), s.graph()) == [], tag


def _same_remap(got: MapRemap, want: MapRemap, tag):
    assert (got.nkf, got.nmp, got.n_kept_kf, got.n_kept_mp) == (want.nkf, want.nmp, want.n_kept_kf, want.n_kept_mp), tag
    assert np.array_equal(got.kf_remap, want.kf_remap) and np.array_equal(got.mp_remap, want.mp_remap), tag


def _round(fe, plan, seed, what):
    """plan: {stream: (keyframe pattern, point pattern)} of mapcompact_scenes.drops."""
    rng = np.random.default_rng(seed)
    states, st0 = _states(fe)
    reqs, want = [], []
    for b, (pk, pm) in plan.items():
        req = MapCompact(b, CS.drops(pk, states[b].nkf, rng), CS.drops(pm, states[b].nmp, rng))
        rc, rm = states[b].apply(req)
        assert rc == 0, (what, b)
        reqs.append(req)
        want.append(rm)
    got = fe.compact_maps(reqs)
    for g, w in zip(got, want):
        _same_remap(g, w, f"{what}: stream {w.stream}")
    _assert_device_equals(fe, states, st0, what)
    return want


def _append(fe, b, seed, **kw):
    """A map delta into the room the compaction freed: gf_frontend_update_maps
    places it from the host mirrors the compaction left."""
    st = {k: fe.read(k) for k in ("map", "map_desc", "nmp")}
    n = int(st["nmp"][b])
    m0 = dict(mp=st["map"][b][:n].copy(), desc=st["map_desc"][b][:n].copy(), graph=fe.covis(b))
    m1 = S.evolve(seed, m0, **kw)
    fe.update_maps(S.diff(b, m0, m1))
    st = {k: fe.read(k) for k in ("map", "map_desc", "nmp")}
    n1 = int(st["nmp"][b])
    got = dict(mp=st["map"][b][:n1].copy(), desc=st["map_desc"][b][:n1].copy(), graph=fe.covis(b))
    assert n1 == len(m1["mp"]) and S.same_map(got, m1) == [], f"stream {b}: the appended map differs"


def test_point_counts_and_drop_patterns():
    """nmp of 1, 63, 64, 65, 255, 256, 257 and map_cap; index 0 only, the last
    only, none, every other, everything droppable; two rounds per front end,
    then an update_maps that appends into the freed room."""
    M = 300
    maps = [S.random_map(40 + i, n, 6, slots=(0, 30), odd_offsets=True)
            for i, n in enumerate((1, 63, 64, 65, 255, 256, 257, M))]
    fe = _frontend(maps, M, free={0, 3, 6})
    _round(fe, {0: ("none", "first"), 1: ("none", "first"), 2: ("none", "last"), 3: ("first", "all"),
                4: ("alternate", "alternate"), 5: ("random", "first"), 6: ("none", "all"), 7: ("last", "first")},
           1, "round 0")
    assert fe.read("nmp")[[0, 3, 6]].tolist() == [0, 0, 0]
    _round(fe, {1: ("first", "alternate"), 2: ("random", "random"), 4: ("none", "none"), 5: ("all", "all"),
                7: ("random", "alternate"), 0: ("none", "none")}, 2, "round 1")
    for b, kw in ((0, dict(new_mp=5, new_kf=1)), (3, dict(new_mp=M, obs="all")), (5, dict(new_mp=40, new_kf=2, rewrite=3)),
                  (7, dict(new_mp=100, new_kf=1, slot_writes=20, bad_mp=3))):
        _append(fe, b, 60 + b, **kw)
    fe.close()


def test_keyframe_counts():
    """1, 2, 63 and 64 keyframes; 64 -> 1; every keyframe gone (observation
    rows and covisibility lists emptied, slot rows gone)."""
    maps = [S.random_map(50, 40, 1, slots=(1, 9)), S.random_map(51, 40, 2, slots=(0, 9), odd_offsets=True),
            S.random_map(52, 40, 63, slots=(0, 9)), S.random_map(53, 40, 64, slots=(0, 9), odd_offsets=True)]
    fe = _frontend(maps, 48)
    rm = _round(fe, {0: ("all", "none"), 1: ("first", "first"), 2: ("alternate", "random"), 3: ("none", "none")}, 3,
                "round 0")
    assert rm[0].nkf == 0 and rm[0].nmp == 40
    g = fe.covis(0)
    assert len(g["mp_obs"]) == 0 and len(g["kf_mp"]) == 0
    # 64 -> 1: everything but keyframe 17
    states, st0 = _states(fe)
    req = MapCompact(3, np.setdiff1d(np.arange(64), [17]))
    rc, want = states[3].apply(req)
    assert rc == 0 and want.nkf == 1
    _same_remap(fe.compact_maps(req)[0], want, "64 -> 1")
    _assert_device_equals(fe, states, st0, "64 -> 1")
    _append(fe, 0, 70, new_kf=3, new_mp=2, obs="all")
    _append(fe, 3, 71, new_kf=63, new_kf_slots=(0, 5), obs="some")
    fe.close()


def test_observation_and_slot_totals():
    """Totals of 1023 .. 1025 and 4095 .. 4097 observations, across the
    chunk widths of the scan and of the copy home."""
    totals = (1023, 1024, 1025, 4095, 4096, 4097)
    maps = []
    for i, t in enumerate(totals):
        m = S.random_map(80 + i, 1030, 12, slots=(70, 90))
        maps.append(S.evolve(90 + i, m, obs=t, cov=False))
    fe = _frontend(maps, 1100, free={1, 4})
    assert [len(fe.covis(b)["mp_obs"]) for b in range(6)] == list(totals)
    _round(fe, {0: ("none", "first"), 1: ("first", "none"), 2: ("last", "last"), 3: ("none", "first"),
                4: ("random", "all"), 5: ("alternate", "alternate")}, 4, "round 0")
    _round(fe, {b: ("random", "random") for b in range(6)}, 5, "round 1")
    _append(fe, 4, 99, new_mp=1100, new_kf=2, obs="all")
    fe.close()


def test_stream_subsets():
    """Stream 0 only, the last only, a non-contiguous subset, all; a stream not
    named is byte-identical before and after."""
    maps = [S.random_map(20 + b, 90, 6, odd_offsets=True) for b in range(4)]
    fe = _frontend(maps, 128)
    both = ("random", "random")
    for r, plan in enumerate(({0: both}, {3: both}, {2: both, 0: both}, {0: both, 1: both, 2: both, 3: both},
                              {1: ("none", "none")})):
        _round(fe, plan, 10 + r, f"round {r}")
    fe.close()


# ---------------------------------------------------------------- 3. refusals
def test_refusals_leave_every_stream_untouched():
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
    from gf_orb_slam_amd.pipeline import KeyframeDB

    M = 48
    maps = [S.random_map(30, 40, 6, odd_offsets=True), S.random_map(31, 40, 9, slots=(0, 3)),
            S.random_map(32, 40, 3, slots=(5, 9))]
    fe = FrontEnd("euroc", 150, 4, M, 100)  # stream 3: a map without a graph
    rng = np.random.default_rng(1)
    for b, m in enumerate(maps):
        fe.set_map(b, m["mp"], m["desc"])
        fe.set_covis(b, m["graph"])
    fe.set_map(3, maps[0]["mp"], maps[0]["desc"])
    dvoc = ORBVocabulary(synth.synth_vocabulary_fast(11, k=10, L=5))
    n2 = np.diff(maps[2]["graph"]["kf_mp_off"])
    db = KeyframeDB([np.zeros(n, KEYPOINT_DTYPE) for n in n2],
                    [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in n2], dvoc.transform)
    fe.set_kfdb(2, db)
    fields = POINT_FIELDS + HOLDERS

    def snapshot():
        return {k: fe.read(k).tobytes() for k in fields}, [fe.covis(b) for b in range(3)]

    before, graphs = snapshot()
    good0, good2 = MapCompact(0, [1], [0, 5]), MapCompact(2, drop_mp=[3])
    bad = {
        "point out of range": (MapCompact(1, drop_mp=[40]), -1),
        "negative keyframe": (MapCompact(1, drop_kf=[-1]), -1),
        "keyframe out of range": (MapCompact(1, drop_kf=[9]), -1),
        "duplicate point": (MapCompact(1, drop_mp=[7, 2, 7]), -1),
        "duplicate keyframe": (MapCompact(1, drop_kf=[0, 0]), -1),
        "stream named twice": (MapCompact(0, drop_mp=[1]), -1),
        "no graph": (MapCompact(3, drop_mp=[1]), -1),
        "stream out of range": (MapCompact(4, drop_mp=[1]), -1),
        "a fixed database with drop_kf": (MapCompact(2, drop_kf=[1]), -4),
    }
    for name, (r, code) in bad.items():
        others = [g for g in (good0, good2) if g.stream != r.stream or name == "stream named twice"]
        for call in ([r] + others, others + [r]):
            with pytest.raises(GFError) as e:
                fe.compact_maps(call)
            assert e.value.code == code, (name, str(e.value))
            now, g = snapshot()
            assert all(now[k] == before[k] for k in fields), name
            assert all(R.same_graph(a, b) == [] for a, b in zip(g, graphs)), name
    # the valid requests pass, the points-only one on the stream with a database included
    rm = fe.compact_maps([good2, good0])
    assert (rm[0].nmp, rm[0].nkf, rm[1].nmp, rm[1].nkf) == (39, 3, 38, 5)
    # an empty request: identity remaps, nothing touched
    mid, _ = snapshot()
    rm = fe.compact_maps([MapCompact(1), MapCompact(0)])
    assert rm[0].identity() and rm[0].mp_remap.tolist() == list(range(40)) and rm[0].kf_remap.tolist() == list(range(9))
    assert rm[1].identity() and rm[1].nmp == 38 and snapshot()[0] == mid
    assert fe.compact_maps([]) == []
    fe.close()


# ---------------------------------------------------------------- 2. / 4. / 5. inside a tracked sequence
G, SEED, BUDGET = 2600, 4, 400
_SC = {}


def _scene():
    """The scene of test_track_loss_gpu, one stream's worth."""
    if not _SC:
        import test_track_loss_gpu as TL
        from gf_orb_slam_amd import synth

        voc = synth.synth_vocabulary_fast(11, k=10, L=5)
        W, fr, gmaps, dbs, fe, T, V, dvoc = TL._scene_setup(1, G, SEED, voc)
        fe.close()
        _SC.update(W=W, fr=fr, gm=gmaps[0], T=T, V=V, voc=voc, dvoc=dvoc)
    return _SC


def _twins(keyframes=False, budget=BUDGET):
    """Two streams on the same scene, map, graph and std::rand() seed."""
    import torch

    sc = _scene()
    W, gm = sc["W"], sc["gm"]
    fe = FrontEnd("euroc", 1000, 2, G, budget)
    fe.set_vocab(sc["dvoc"])
    for b in range(2):
        fe.set_map(b, gm["mp"], gm["desc"])
        fe.set_covis(b, gm["graph"])
        fe.set_rng(b, 7)
    fe.set_source(torch.from_numpy(sc["fr"]).cuda().contiguous(), [W.scene_of[0]] * 2, [W.phase[0]] * 2)
    fe.bootstrap(np.repeat(sc["T"][:1], 2, 0), np.repeat(sc["V"][:1], 2, 0), 0.0)
    if keyframes:
        fe.enable_keyframes()
    return fe


def _held(st, b):
    """The map indices stream b's frame state holds."""
    a = np.concatenate([st["kp2mp"][b][:int(st["nkp"][b])], st["last_kp2mp"][b][:int(st["last_nkp"][b])]])
    return np.unique(a[a >= 0])


def test_pins():
    """Everything listed: what the current frame, the last frame and the
    pending outbox keyframe hold survives, so does the reference keyframe; the
    counts say so, and the taken keyframe's slots carry the new indices."""
    fe = _twins(keyframes=True, budget=100)  # the budget at which the scene makes a keyframe within four steps
    k = 0
    while not fe.keyframe_state()["pending"].all():
        k += 1
        assert k <= 4, "no keyframe within four steps"
        fe.step()
    # the frames let go of half of their points (on both twins), so that the outbox keyframe alone holds those
    for key in ("kp2mp", "last_kp2mp"):
        a = fe.read(key)
        a[:, ::2] = -1
        fe.write(key, a)
    st = C.read_state(fe)
    ks = fe.keyframe_state()
    ref = int(ks["ref"][0])
    assert st["kp2mp"][0].tobytes() == st["kp2mp"][1].tobytes() and ref >= 0
    n, nkf = int(st["nmp"][0]), len(fe.covis(0)["kf_bad"])
    rm = fe.compact_maps(MapCompact(0, np.arange(nkf), np.arange(n)))[0]
    kfs = {q["stream"]: q for q in fe.take_keyframes()}
    assert set(kfs) == {0, 1}
    old_slots = kfs[1]["slots"]  # the twin's: the old indices
    held = np.union1d(_held(st, 0), np.unique(old_slots[old_slots >= 0]))
    assert len(held) > len(_held(st, 0)) + 50, "the outbox keyframe pins nothing of its own"
    assert rm.nmp == len(held) == rm.n_kept_mp and np.array_equal(np.nonzero(rm.mp_remap >= 0)[0], held)
    assert rm.nkf == 1 == rm.n_kept_kf and rm.kf_remap[ref] == 0 and fe.keyframe_state()["ref"][0] == 0
    assert np.array_equal(kfs[0]["slots"], MapRemap.apply(rm.mp_remap, old_slots))
    now = C.read_state(fe)
    for key in ("kp2mp", "last_kp2mp"):
        assert np.array_equal(now[key][0], MapRemap.apply(rm.mp_remap, st[key][0])), key
        assert now[key][1].tobytes() == st[key][1].tobytes(), key
    assert now["map"][0][:rm.nmp].tobytes() == st["map"][0][held].tobytes()
    g = fe.covis(0)  # the pinned points keep rows that hold the reference keyframe alone, or nothing
    assert len(g["kf_bad"]) == 1 and set(g["mp_obs"].tolist()) <= {0} and len(g["mp_obs_off"]) == rm.nmp + 1
    fe.close()


PER_POINT = ("map", "map_desc", "views", "mp_H", "mp_info", "mp_uv", "mp_upd")
INDEXED = ("kp2mp", "last_kp2mp")
SKIP = ("clock", "nmp", "left")


def _invisible_run(captured):
    """Both twins get the same points and one keyframe turned bad; stream 0 is
    compacted of everything bad. -> the states after each following step, the
    remap, the graphs at the end."""
    fe = _twins(keyframes=True)
    fe.set_keyframe_state(accept=0)  # the rule is evaluated (GF_KF_REF), no keyframe leaves
    fe.step()
    if captured:
        fe.capture_graph()
    fe.step()
    st = C.read_state(fe)
    rng = np.random.default_rng(3)
    n, g = int(st["nmp"][0]), fe.covis(0)
    nkf, ref = len(g["kf_bad"]), int(fe.keyframe_state()["ref"][0])
    free = np.setdiff1d(np.arange(n), _held(st, 0))
    bad_mp = np.sort(rng.choice(free, 400, replace=False))
    bad_mp = np.union1d(bad_mp, [free[0], free[-1]])
    bad_kf = [k for k in range(nkf) if k != ref][:2]
    # MapPoint::SetBadFlag erases the point from its keyframes' slots (MapPoint.cc:140-160): a bad point is in none
    hit = np.nonzero(np.isin(g["kf_mp"], bad_mp))[0]
    slot_kf = np.searchsorted(g["kf_mp_off"], hit, side="right") - 1
    fe.update_maps([MapDelta(b, bad_mp=bad_mp, bad_kf=bad_kf, slot_kf=slot_kf, slot_idx=hit - g["kf_mp_off"][slot_kf],
                             slot_val=np.full(len(hit), -1)) for b in range(2)])
    rm = fe.compact_maps(MapCompact(0, bad_kf, bad_mp))[0]
    assert rm.n_kept_mp == 0 and rm.n_kept_kf == 0 and rm.nmp == n - len(bad_mp) and rm.nkf == nkf - 2
    steps = []
    for _ in range(3):
        fe.step()
        steps.append(C.read_state(fe))
    out = dict(steps=steps, rm=rm, graphs=[fe.covis(0), fe.covis(1)], ks=fe.keyframe_state())
    fe.close()
    return out


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_a_compaction_of_bad_items_is_invisible(captured):
    run = _invisible_run(captured)
    rm = run["rm"]
    keep = rm.mp_remap >= 0
    n0 = len(keep)
    for i, s in enumerate(run["steps"]):
        tag = f"step {i + 1} after the compaction: "
        for k in C.FIELDS:
            if k in SKIP:
                continue
            a, b = s[k][0], s[k][1]
            if k in PER_POINT:
                assert a[:rm.nmp].tobytes() == b[:n0][keep].tobytes(), tag + k
            elif k in INDEXED:
                assert np.array_equal(a, MapRemap.apply(rm.mp_remap, b)), tag + k
                assert not np.any((b >= 0) & (MapRemap.apply(rm.mp_remap, b) < 0)), tag + k + ": a bad point is matched"
            elif k == "stats":
                assert np.array_equal(s[k][:, 0], s[k][:, 1]), tag + k
            elif k == "reloc":  # rows per keyframe
                assert a[:rm.nkf].tobytes() == b[:len(rm.kf_remap)][rm.kf_remap >= 0].tobytes(), tag + k
            else:
                assert a.tobytes() == b.tobytes(), tag + k
        nl = int(s["stats"][NLEFT, 0])
        assert np.array_equal(s["left"][0][:nl], MapRemap.apply(rm.mp_remap, s["left"][1][:nl])), tag + "left"
        assert int(s["nmp"][0]) == rm.nmp and int(s["nmp"][1]) == n0
    ks = run["ks"]
    assert ks["ref"][0] == rm.kf_remap[ks["ref"][1]] and ks["ref_matches"][0] == ks["ref_matches"][1]
    # the graphs: the compacted one is the twin's restricted to what stayed
    sc = _scene()
    twin = dict(mp=sc["gm"]["mp"], desc=sc["gm"]["desc"], graph=run["graphs"][1])
    want, _, _ = CS.restrict(twin, rm.kf_remap >= 0, keep)
    assert R.same_graph(run["graphs"][0], want["graph"]) == []


def test_a_window_equals_the_chain_on_the_restricted_map():
    """Good keyframes and their points dropped: the next step equals the
    oracle chain built on the restricted map and loaded with the device state
    after the call."""
    import test_track_loss_gpu as TL

    sc = _scene()
    fe = _twins(keyframes=True)
    fe.set_keyframe_state(accept=0)
    for _ in range(2):
        fe.step()
    st = C.read_state(fe)
    g = fe.covis(0)
    nkf, ref = len(g["kf_bad"]), int(fe.keyframe_state()["ref"][0])
    # the window: the reference keyframe, its first covisibles and the newest keyframes, half of the graph
    cov = S.rows_of(g["kf_cov_off"], g["kf_cov"])[ref]
    keep_kf = list(dict.fromkeys([ref] + [int(c) for c in cov] + list(range(nkf - 1, -1, -1))))[:nkf // 2]
    drop_kf = np.setdiff1d(np.arange(nkf), keep_kf)
    slots = S.rows_of(g["kf_mp_off"], g["kf_mp"])
    seen = np.unique(np.concatenate([slots[k] for k in keep_kf]))
    drop_mp = np.setdiff1d(np.arange(int(st["nmp"][0])), seen[seen >= 0])
    assert len(drop_kf) >= nkf // 2 and len(drop_mp) > 100
    rm = fe.compact_maps(MapCompact(0, drop_kf, drop_mp))[0]
    assert rm.nkf == nkf - len(drop_kf) and rm.nmp < int(st["nmp"][0]) - 100
    upd = C.read_state(fe)
    n1 = rm.nmp
    m1 = dict(mp=upd["map"][0][:n1].copy(), desc=upd["map_desc"][0][:n1].copy(), graph=fe.covis(0))
    twin = dict(mp=sc["gm"]["mp"], desc=sc["gm"]["desc"], graph=g)
    want, _, _ = CS.restrict(twin, rm.kf_remap >= 0, rm.mp_remap >= 0)
    assert S.same_map(m1, want) == []
    ch = C.Chain("euroc", 1000, G, BUDGET)
    ch.set_map(m1["mp"], m1["desc"])
    ch.set_covis(m1["graph"])
    ch.set_kfdb(None)
    ch.set_vocab(sc["voc"])
    ch.load_from(upd, 0)
    ch.write("reloc", upd["reloc"][0])
    fe.step()
    ch.step(sc["fr"][sc["W"].scene_of[0], (sc["W"].phase[0] + 3) % sc["W"].period])
    after = C.read_state(fe)
    TL._compare(after, ch, 0, "the step after the window: ")
    # the untouched twin went on as if nothing had happened next to it
    assert int(after["nmp"][1]) == int(st["nmp"][1]) and R.same_graph(fe.covis(1), g) == []
    fe.close()


# ---------------------------------------------------------------- the closed loop with a compaction in it
def test_closed_loop_feed_back_compacts_the_real_front_end():
    """Tracker -> keyframe -> mapper -> feed_back as in test_mapupdate_gpu's closed
    loop, then feed_back(compact_at=...) with limits below the map's size: the
    default policy's window goes through the real front end, with its pins and
    the device-decided remaps applied to the shadow and the id maps. The front
    end then holds covis_graph_from_loopmap through the id maps, the delta of
    the unchanged LoopMap is empty, and the next step equals the chain on the
    compacted map. (The loop past the 64-keyframe capacity itself is not
    tested here.)"""
    import torch

    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import tracking
    from gf_orb_slam_amd.localmapping import LocalMapper

    sc = _scene()
    W, gm, voc, dvoc, fr = sc["W"], sc["gm"], sc["voc"], sc["dvoc"], sc["fr"]
    M = len(gm["mp"]) + 1400  # room for what CreateNewMapPoints appends
    fe = FrontEnd("euroc", 1000, 1, M, 100)
    fe.set_vocab(dvoc)
    fe.set_map(0, gm["mp"], gm["desc"])
    fe.set_covis(0, gm["graph"])
    fe.set_rng(0, 7)
    fe.set_source(torch.from_numpy(fr).cuda().contiguous(), W.scene_of, W.phase)
    fe.bootstrap(sc["T"], sc["V"], 0.0)
    m = tracking.loopmap_from_global_map(TL.INFO, gm, voc=dvoc)
    nkf0 = m.nkf
    fb = tracking.MapFeedback(fe, 0, m)
    ins = tracking.KeyFrameInserter(fe, [LocalMapper(m, dvoc)], feedback=[fb])
    fe.enable_keyframes()
    k = 0
    while not fe.keyframe_state()["pending"][0]:
        k += 1
        assert k <= 4, "no keyframe within four steps"
        fe.step()
    assert ins.pump() == [(0, nkf0)]
    ins.run_mapper(0)
    assert len(ins.feed_back()) == 1
    n_before, held = len(fb.mp), _held(C.read_state(fe), 0)
    ref = int(fe.keyframe_state()["ref"][0])
    # the map is below the capacities: limits below its size make feed_back compact it to a window of 12
    assert ins.feed_back(streams=[0], compact_at=dict(kf=20, keep_kf=12)) == []
    assert not fb._identity and 12 <= len(fb.kf_id) <= 13 and len(fb.mp) < n_before  # 13: a pinned reference keyframe
    assert fb.kf_index[ref] >= 0 and np.all(fb.mp_index[held] >= 0), "a pinned item left the shadow"
    assert fb.kf_index[nkf0] == len(fb.kf_id) - 1, "the newest keyframe is not the last of the window"
    assert len(m.mps) >= n_before and m.nkf == nkf0 + 1  # the LoopMap never shrinks
    st = C.read_state(fe)
    n = len(fb.mp)
    g = fe.covis(0)
    assert int(st["nmp"][0]) == n and st["map"][0][:n].tobytes() == np.asarray(m.mps)[fb.mp_id].tobytes()
    assert np.array_equal(st["map_desc"][0][:n], np.asarray(m.mp_desc)[fb.mp_id])
    assert R.same_graph(g, tracking._graph_through(m, fb.mp_id, fb.kf_id)) == [] and R.same_graph(g, fb.graph) == []
    assert fb.delta().empty()
    fb.commit()
    print(f"compacted {n_before} -> {n} points, {nkf0 + 1} -> {len(fb.kf_id)} keyframes")
    # the next step tracks the compacted map
    ch = C.Chain("euroc", 1000, M, 100)
    ch.set_map(st["map"][0][:n], st["map_desc"][0][:n])
    ch.set_covis(g)
    ch.set_kfdb(None)
    ch.set_vocab(voc)
    ch.load_from(st, 0)
    ch.write("reloc", st["reloc"][0])
    fe.step()
    ch.step(fr[W.scene_of[0], (W.phase[0] + k + 1) % W.period])
    TL._compare(C.read_state(fe), ch, 0, "the step after the compaction: ")
    # and a later keyframe's slots come back in LoopMap ids through the id maps
    j = 0
    while not fe.keyframe_state()["pending"][0] and j < 12:
        j += 1
        fe.step()
    print(f"a second keyframe after {j} steps: {bool(fe.keyframe_state()['pending'][0])}")
    if fe.keyframe_state()["pending"][0]:
        assert ins.pump() == [(0, nkf0 + 1)]
        s = m.slots[nkf0 + 1]
        assert np.all(s < len(m.mps)) and np.all(np.isin(s[s >= 0], fb.mp_id)), "slots not translated to LoopMap ids"
    fe.close()


# ---------------------------------------------------------------- 7. past the cap
def _padded(gm, nkf):
    """The map with bad, empty keyframes appended up to ``nkf``."""
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    g = gm["graph"]
    k0 = len(g["kf_bad"])
    pad = nkf - k0
    graph = dict(g, kf_bad=np.concatenate([np.asarray(g["kf_bad"], np.uint8), np.ones(pad, np.uint8)]),
                 kf_mp_off=np.concatenate([g["kf_mp_off"], np.full(pad, g["kf_mp_off"][-1], np.int32)]),
                 kf_cov_off=np.concatenate([g["kf_cov_off"], np.full(pad, g["kf_cov_off"][-1], np.int32)]))
    Tcw = np.concatenate([np.asarray(gm["kf_Tcw"], np.float32).reshape(k0, 4, 4),
                          np.tile(np.eye(4, dtype=np.float32), (pad, 1, 1))])
    return dict(gm, graph=graph, kf_kps=list(gm["kf_kps"]) + [np.zeros(0, KEYPOINT_DTYPE)] * pad,
                kf_desc=list(gm["kf_desc"]) + [np.zeros((0, 32), np.uint8)] * pad, kf_Tcw=Tcw), k0


def test_closed_loop_past_the_keyframe_and_point_capacity():
    """The closed loop on a graph padded with bad, empty keyframes to 63 and a
    map_cap 400 above the map (one mapper pass appends a keyframe and about 230
    points). On the second pass the delta as it stands is refused with
    GF_ERR_CAP and leaves the stream untouched: the limit. With
    feed_back(compact_at=...) the loop runs that pass and one more; then the
    front end holds covis_graph_from_loopmap through the id maps and the next
    step equals the chain."""
    import torch

    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import tracking
    from gf_orb_slam_amd.bow import FeatureVector
    from gf_orb_slam_amd.localmapping import LocalMapper

    sc = _scene()
    W, voc, dvoc, fr = sc["W"], sc["voc"], sc["dvoc"], sc["fr"]
    gm, k_real = _padded(sc["gm"], 63)
    M = len(gm["mp"]) + 400
    fe = FrontEnd("euroc", 1000, 1, M, 100)
    fe.set_vocab(dvoc)
    fe.set_map(0, gm["mp"], gm["desc"])
    fe.set_covis(0, gm["graph"])
    fe.set_rng(0, 7)
    fe.set_source(torch.from_numpy(fr).cuda().contiguous(), W.scene_of, W.phase)
    fe.bootstrap(sc["T"], sc["V"], 0.0)
    m = tracking.loopmap_from_global_map(TL.INFO, gm, voc=None)
    for k in range(k_real):  # ComputeBoW of the real keyframes (the padding has no descriptors)
        words, values, fv = dvoc.transform(m.kf_desc[k], 4)
        m.kf_bow[k] = (words, values)
        m.kf_fv[k] = fv if isinstance(fv, FeatureVector) else FeatureVector(*fv)
    fb = tracking.MapFeedback(fe, 0, m)
    ins = tracking.KeyFrameInserter(fe, [LocalMapper(m, dvoc)], feedback=[fb])
    fe.enable_keyframes()
    steps, refused = 0, 0
    for p in range(3):
        j = 0
        while not fe.keyframe_state()["pending"][0]:
            j += 1
            assert j <= 16, f"pass {p}: no keyframe within sixteen steps"
            fe.step()
        steps += j
        assert ins.pump() == [(0, 63 + p)]
        ins.run_mapper(0)
        d = fb.delta()
        fb.discard()
        over = len(fb.graph["kf_bad"]) + 1 > 64 or len(fb.mp) + len(d.new_mp) > M
        assert over == (p == 1), f"pass {p}: {len(fb.graph['kf_bad'])} keyframes, {len(fb.mp)} + {len(d.new_mp)} points"
        if over:  # the limit the compaction removes: refused, nothing touched
            before = C.read_state(fe, ["map", "nmp", "mp_upd", "kp2mp"])
            g0 = fe.covis(0)
            with pytest.raises(GFError) as e:
                fe.update_maps(d)
            assert e.value.code == -3, str(e.value)
            now = C.read_state(fe, ["map", "nmp", "mp_upd", "kp2mp"])
            assert all(now[k].tobytes() == before[k].tobytes() for k in now) and R.same_graph(fe.covis(0), g0) == []
            refused += 1
        sent = ins.feed_back(compact_at=dict(keep_kf=12))
        assert len(sent) == 1 and len(sent[0].new_kf_off) == 2
        print(f"pass {p}: {len(fb.kf_id)} keyframes, {len(fb.mp)} points in the front end; {m.nkf}, {len(m.mps)} in the map")
    assert refused == 1 and not fb._identity and m.nkf == 66 and len(fb.kf_id) <= 15
    st = C.read_state(fe)
    n, g = len(fb.mp), fe.covis(0)
    assert int(st["nmp"][0]) == n and st["map"][0][:n].tobytes() == np.asarray(m.mps)[fb.mp_id].tobytes()
    assert R.same_graph(g, tracking._graph_through(m, fb.mp_id, fb.kf_id)) == []
    ch = C.Chain("euroc", 1000, M, 100)
    ch.set_map(st["map"][0][:n], st["map_desc"][0][:n])
    ch.set_covis(g)
    ch.set_kfdb(None)
    ch.set_vocab(voc)
    ch.load_from(st, 0)
    ch.write("reloc", st["reloc"][0])
    fe.step()
    ch.step(fr[W.scene_of[0], (W.phase[0] + steps + 1) % W.period])
    TL._compare(C.read_state(fe), ch, 0, "the step after three passes: ")
    fe.close()


# ---------------------------------------------------------------- 6. the keyframe database
def _growable_db(m, dvoc, seed, max_kf=64, room=200):
    """A growable KeyframeDB over the keyframes of the map's graph (random
    keypoints and descriptors, one row per slot), and what it was built from."""
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
    from gf_orb_slam_amd.pipeline import KeyframeDB

    rng = np.random.default_rng(seed)
    ns = np.diff(m["graph"]["kf_mp_off"])
    kps = [rng.integers(0, 200, (n, KEYPOINT_DTYPE.itemsize), dtype=np.uint8).view(KEYPOINT_DTYPE).reshape(-1) for n in ns]
    desc = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in ns]
    return KeyframeDB(kps, desc, dvoc.transform, max_kf=max_kf, max_rows=int(ns.sum()) + room), kps, desc


def test_compacted_database_equals_one_built_from_the_kept_keyframes():
    """KeyFrameDatabase::erase: after a compaction that drops keyframes, the
    stream's growable database read back (rows, offsets, inverted file) equals,
    bit for bit, a database built from the kept keyframes; so do its host
    arrays. Two rounds; a database on a stream not named is untouched."""
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.pipeline import KeyframeDB

    dvoc = ORBVocabulary(synth.synth_vocabulary_fast(11, k=10, L=5))
    maps = [S.random_map(70, 60, 9, slots=(1, 25), odd_offsets=True), S.random_map(71, 60, 64, slots=(1, 12)),
            S.random_map(72, 60, 2, slots=(3, 9)), S.random_map(73, 60, 12, slots=(1, 30))]
    fe = _frontend(maps, 64)
    built = [_growable_db(m, dvoc, 80 + b) for b, m in enumerate(maps)]
    for b in range(3):  # stream 3 keeps a database nobody compacts
        fe.set_kfdb(b, built[b][0])
    fe.set_kfdb(3, built[3][0])
    untouched = built[3][0].read(fe.ctx)
    for r, plan in enumerate(({0: ("first", "random"), 1: ("alternate", "none"), 2: ("last", "first")},
                              {0: ("random", "none"), 1: ("random", "random"), 2: ("none", "last")})):
        rms = _round(fe, plan, 20 + r, f"database round {r}")
        for rm in rms:
            b = rm.stream
            db, kps, desc = built[b]
            keep = np.nonzero(rm.kf_remap >= 0)[0]
            kps, desc = [kps[k] for k in keep], [desc[k] for k in keep]
            built[b] = (db, kps, desc)
            want = KeyframeDB(kps, desc, dvoc.transform, max_kf=64, max_rows=db.max_rows)
            got, ref = db.read(fe.ctx), want.read(fe.ctx)
            assert got["nkf"] == len(keep) == ref["nkf"]
            for k in ref:
                assert np.asarray(got[k]).tobytes() == np.asarray(ref[k]).tobytes(), f"round {r} stream {b}: {k}"
            for k in KeyframeDB._ARRAYS:
                assert getattr(db, k).tobytes() == getattr(want, k).tobytes(), f"round {r} stream {b}: host {k}"
    now = built[3][0].read(fe.ctx)
    assert all(np.asarray(now[k]).tobytes() == np.asarray(untouched[k]).tobytes() for k in now)
    fe.close()


def test_lost_stream_relocalises_against_a_kept_keyframe():
    """A tracked stream with a growable database is compacted to a window
    (keyframes and their database rows go), then loses track on blank frames
    and relocalises against the keyframes that stayed; every step after the
    compaction equals the chain on the restricted map and database."""
    import torch

    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import scene, synth
    from gf_orb_slam_amd.pipeline import KeyframeDB, TR

    voc = synth.synth_vocabulary_fast(11, k=10, L=5)
    W0 = scene.Workload("euroc", 1, n_scenes=1, period=32, seed=SEED)
    blank = [(W0.scene_of[0], (W0.phase[0] + k) % 32) for k in (4, 5)]
    W, fr, gmaps, dbs, fe0, T, V, dvoc = TL._scene_setup(1, G, SEED, voc, blank=blank)
    fe0.close()
    gm = gmaps[0]
    db = KeyframeDB(gm["kf_kps"], gm["kf_desc"], dvoc.transform, max_kf=64,
                    max_rows=sum(len(k) for k in gm["kf_kps"]) + 2000)
    fe = FrontEnd("euroc", 1000, 1, G, 100)
    fe.set_vocab(dvoc)
    fe.set_map(0, gm["mp"], gm["desc"])
    fe.set_covis(0, gm["graph"])
    fe.set_kfdb(0, db)
    fe.set_rng(0, 7)
    fe.set_source(torch.from_numpy(fr).cuda().contiguous(), W.scene_of, W.phase)
    fe.bootstrap(T, V, 0.0)
    fe.enable_keyframes()
    fe.set_keyframe_state(accept=0)
    for _ in range(2):
        fe.step()
    st = C.read_state(fe)
    g = fe.covis(0)
    nkf, ref = len(g["kf_bad"]), int(fe.keyframe_state()["ref"][0])
    cov = S.rows_of(g["kf_cov_off"], g["kf_cov"])[ref]
    keep_kf = list(dict.fromkeys([ref] + [int(c) for c in cov] + list(range(nkf - 1, -1, -1))))[:nkf // 2]
    drop_kf = np.setdiff1d(np.arange(nkf), keep_kf)
    slots = S.rows_of(g["kf_mp_off"], g["kf_mp"])
    seen = np.unique(np.concatenate([slots[k] for k in keep_kf]))
    drop_mp = np.setdiff1d(np.arange(int(st["nmp"][0])), seen[seen >= 0])
    rm = fe.compact_maps(MapCompact(0, drop_kf, drop_mp))[0]
    assert rm.nkf == nkf - len(drop_kf) == db.nkf
    dev = C.read_state(fe)
    n1, g1 = rm.nmp, fe.covis(0)
    mp1, desc1 = dev["map"][0][:n1].copy(), dev["map_desc"][0][:n1].copy()
    assert np.array_equal(np.diff(db.kp_off), np.diff(g1["kf_mp_off"]))
    relocalised = False
    for k in range(3, 11):
        before = dev
        fe.step()
        dev = C.read_state(fe)
        ch = C.Chain("euroc", 1000, G, 100)
        ch.set_map(mp1, desc1)
        ch.set_covis(g1)
        ch.set_kfdb(db)
        ch.set_vocab(voc)
        ch.load_from(before, 0)
        ch.write("reloc", before["reloc"][0])
        ch.step(fr[W.scene_of[0], (W.phase[0] + k) % W.period])
        TL._compare(dev, ch, 0, f"step {k} after the compaction: ")
        relocalised |= int(dev["track"][0][TR["path"]]) == 3 and int(dev["track"][0][TR["ok"]]) == 1
    assert relocalised, "the stream did not relocalise against the kept keyframes"
    fe.close()
