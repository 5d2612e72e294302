"""Map feedback on the device (csrc/mapupdate.hip, gf_frontend_update_maps)
against the serial restatement (tests/helpers/mapupdate_ref.cpp): the tables
over the shapes at which the kernels can go wrong, the refusals, then a
constructed delta inside a tracked sequence against the oracle chain (eager and
through a captured graph) and the closed loop tracker -> keyframe -> mapper ->
map -> tracker. Every comparison of the feature's own outputs is byte
equality."""
import numpy as np
import pytest

import mapupdate_ref as R
import mapupdate_scenes as S
import oracle_chain as C
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.localmap import MapDelta
from gf_orb_slam_amd.pipeline import FrontEnd

pytestmark = pytest.mark.gpu

MAP_FIELDS = ["map", "map_desc", "nmp", "views", "mp_H", "mp_info", "mp_uv", "mp_upd", "last_pos", "last_kp2mp",
              "last_nkp"]


# ---------------------------------------------------------------- 1. tables against the restatement
def _frontend(maps, M, nfeatures=150, seed=0):
    """A front end over ``maps`` (one per stream) whose buffers hold random
    per-point state on the used rows and sentinels past them, with a last frame
    that matches random points."""
    B = len(maps)
    fe = FrontEnd("euroc", nfeatures, B, M, 100)
    rng = np.random.default_rng(seed)
    for b, m in enumerate(maps):
        fe.set_map(b, m["mp"], m["desc"])
        fe.set_covis(b, m["graph"])
    st = {k: fe.read(k) for k in MAP_FIELDS}
    for b, m in enumerate(maps):
        n = len(m["mp"])
        for k in ("map", "map_desc", "views", "mp_upd"):
            st[k][b, n:].view(np.uint8)[...] = S.SENTINEL
        st["views"][b, :n].view(np.uint8)[...] = rng.integers(0, 256, st["views"][b, :n].view(np.uint8).shape)
        st["mp_upd"][b, :n] = rng.integers(-5, 3, n)
        for k in ("mp_H", "mp_info", "mp_uv"):
            st[k][b] = rng.normal(size=st[k][b].shape)
        nk = int(rng.integers(fe.cap // 2, fe.cap + 1))
        st["last_nkp"][b] = nk
        st["last_kp2mp"][b] = rng.integers(-1, n, fe.cap) if n else -1
        st["last_pos"][b].view(np.uint8)[...] = S.SENTINEL
    for k in MAP_FIELDS:
        if k != "nmp":
            fe.write(k, st[k])
    return fe


def _states(fe, has_db=()):
    """The restatement's State of every stream, from the device."""
    st = {k: fe.read(k) for k in MAP_FIELDS}
    out = []
    for b in range(fe.B):
        n = int(st["nmp"][b])
        g = fe.covis(b)
        s = R.State(fe.M, fe.cap, st["map"][b], st["map_desc"][b], dict(g, mp_bad=g["mp_bad"][:n]),
                    views=st["views"][b], upd=st["mp_upd"][b], last_kp2mp=st["last_kp2mp"][b],
                    last_nkp=int(st["last_nkp"][b]), last_pos=st["last_pos"][b], has_db=b in has_db)
        out.append(s)
    return out, st


def _assert_device_equals(fe, states, st0, named, what):
    """Every map field and the graph of every stream equal the restatement's
    state (named streams) or what they were (the others); the per-point state
    the delta does not own is untouched everywhere."""
    now = {k: fe.read(k) for k in MAP_FIELDS}
    for k in ("mp_H", "mp_info", "mp_uv", "last_kp2mp", "last_nkp"):
        assert now[k].tobytes() == st0[k].tobytes(), f"{what}: {k} changed"
    for b, s in enumerate(states):
        tag = f"{what}: stream {b} ({'named' if b in named else 'not named'})"
        assert int(now["nmp"][b]) == s.nmp, tag
        for k, ref in (("map", s.map), ("map_desc", s.desc), ("views", s.views), ("mp_upd", s.upd),
                       ("last_pos", s.last_pos)):
            assert now[k][b].tobytes() == ref.tobytes(), f"{tag}: {k}"
        assert R.same_graph(fe.covis(b), s.graph()) == [], tag


def _run_rounds(maps, M, rounds, nfeatures=150):
    """rounds: a list of {stream: evolve keywords or a function map -> MapDelta}."""
    fe = _frontend(maps, M, nfeatures)
    for r, plan in enumerate(rounds):
        states, st0 = _states(fe)
        deltas = []
        for b, kw in plan.items():
            m0 = S.map_of_state(states[b])
            d = kw(m0, b) if callable(kw) else S.diff(b, m0, S.evolve(31 * r + b, m0, **kw))
            assert states[b].apply(d) == 0, (r, b)
            deltas.append(d)
        fe.update_maps(deltas)
        _assert_device_equals(fe, states, st0, set(plan), f"round {r}")
    fe.close()


def test_point_counts_at_the_tile_edges():
    """nmp after the update at 1, 63, 64, 65, 256, 257 and map_cap."""
    maps = [S.random_map(1, 0, 3), S.random_map(2, 60, 5), S.random_map(3, 60, 5), S.random_map(4, 60, 5)]
    _run_rounds(maps, 300, [{0: dict(new_mp=1), 1: dict(new_mp=3), 2: dict(new_mp=4, rewrite=60),
                             3: dict(new_mp=5, rewrite=1)},
                            {0: dict(new_mp=255, rewrite=1), 1: dict(new_mp=194, rewrite=63), 2: dict(new_mp=236),
                             3: dict(new_mp=0, rewrite=65)}])


def test_observation_rows():
    """Rows growing from empty, shrinking to empty, the first and the last
    point's row, every row, no row; then totals crossing the scan's and the
    copy's widths."""
    empty = S.random_map(5, 130, 7, obs_most=0)
    maps = [empty, S.random_map(6, 130, 7), S.random_map(7, 130, 7), S.random_map(8, 130, 7)]
    _run_rounds(maps, 200, [{0: dict(obs="grow", cov=False), 1: dict(obs="shrink", cov=False),
                             2: dict(obs="ends", new_mp=3, cov=False), 3: dict(obs="all", new_mp=2)},
                            {0: dict(obs="none", rewrite=5, cov=False), 1: dict(obs="all"), 3: dict(obs="ends")}])
    big = [S.random_map(9 + i, n, 12) for i, n in enumerate((1020, 1020, 1030, 1030))]
    _run_rounds(big, 1100, [{0: dict(new_mp=4, obs=1024), 1: dict(new_mp=5, obs=1025), 2: dict(obs=4096),
                             3: dict(obs=4097)},
                            {0: dict(obs=1023), 1: dict(new_mp=75, obs="some"), 2: dict(obs=4095), 3: dict(obs=8193)}])


def test_keyframe_rows_and_slot_writes():
    """Slot rows appended when nkf is 0 and when it becomes 64; slot writes at
    the first and the last slot of rows at odd offsets."""
    def ends(m, b):
        off = m["graph"]["kf_mp_off"]
        rows = [k for k in range(len(off) - 1) if off[k] % 2 == 1 and off[k + 1] - off[k] >= 2]
        assert rows
        kf = np.repeat(rows, 2)
        idx = np.ravel([(0, off[k + 1] - off[k] - 1) for k in rows])
        cur = m["graph"]["kf_mp"][off[kf] + idx]
        return MapDelta(b, slot_kf=kf, slot_idx=idx, slot_val=np.where(cur == 7, 8, 7))

    maps = [S.random_map(11, 50, 0), S.random_map(12, 50, 62, slots=(0, 9), odd_offsets=True),
            S.random_map(13, 50, 63, slots=(0, 9)), S.random_map(14, 50, 9, odd_offsets=True)]
    _run_rounds(maps, 64, [{0: dict(new_kf=2, new_mp=2), 1: dict(new_kf=2, slot_writes=30),
                            2: dict(new_kf=1, new_kf_slots=(0, 0), cov=False), 3: ends},
                           {0: dict(new_kf=1, slot_writes=20, cov=False, obs="none"), 1: ends, 3: dict(slot_writes=200)}])


def test_single_items_and_stream_subsets():
    """Only appended points, only rewritten points, an empty delta; stream 0
    only, the last stream only, a non-contiguous subset, all streams."""
    maps = [S.random_map(20 + b, 90, 6, odd_offsets=True) for b in range(4)]
    only_new = dict(new_mp=17, obs="none", cov=False)
    only_set = dict(rewrite=30, obs="none", cov=False)
    both = dict(new_mp=3, new_kf=1, rewrite=9, bad_mp=4, bad_kf=1, slot_writes=15)
    _run_rounds(maps, 256, [{0: only_new, 1: only_set, 2: lambda m, b: MapDelta(b)}, {0: both}, {3: both},
                            {0: both, 2: both}, {0: both, 1: both, 2: both, 3: both}, {1: lambda m, b: MapDelta(b)}])


# ---------------------------------------------------------------- 2. refusals
def test_refusals_leave_every_stream_untouched():
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE
    from gf_orb_slam_amd.pipeline import KeyframeDB

    M = 48
    maps = [S.random_map(30, 40, 6, odd_offsets=True), S.random_map(31, 40, 64, slots=(0, 3)),
            S.random_map(32, 40, 3, slots=(5, 9))]
    fe = _frontend(maps, M)
    rng = np.random.default_rng(1)
    dvoc = ORBVocabulary(synth.synth_vocabulary_fast(11, k=10, L=5))
    n2 = np.diff(maps[2]["graph"]["kf_mp_off"])
    db = KeyframeDB([np.zeros(n, KEYPOINT_DTYPE) for n in n2],
                    [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in n2], dvoc.transform)
    fe.set_kfdb(2, db)
    states, st0 = _states(fe, has_db={2})
    m = [S.map_of_state(s) for s in states]
    good0 = S.diff(0, m[0], S.evolve(40, m[0], new_mp=2, rewrite=3, slot_writes=4))
    good2 = S.diff(2, m[2], S.evolve(41, m[2], new_mp=1, rewrite=2))
    bad = {
        "65 keyframes": (S.diff(1, m[1], S.evolve(42, m[1], new_kf=1, cov=False, obs="none")), -3),
        "map_cap + 1 points": (S.diff(1, m[1], S.evolve(43, m[1], new_mp=9, cov=False, obs="none")), -3),
        "slot value out of range": (MapDelta(1, slot_kf=[5], slot_idx=[0], slot_val=[40]), -1),
        "observation row not ascending": (MapDelta(1, obs_rows={3: [2, 1]}), -1),
        "duplicate stream": (S.diff(0, m[0], S.evolve(44, m[0], rewrite=1, cov=False, obs="none")), -1),
        "appended keyframe with a database": (MapDelta(2, new_kf=[[0, 1]]), -4),
    }
    assert np.diff(maps[1]["graph"]["kf_mp_off"])[5] > 0
    for name, (d, code) in bad.items():
        b = d.stream
        if name != "duplicate stream":
            assert states[b].copy().apply(d) == code, name  # the restatement's verdict
        others = [g for g in (good0, good2) if g.stream != b or name == "duplicate stream"]
        for call in ([d] + others, others + [d]):
            with pytest.raises(GFError) as e:
                fe.update_maps(call)
            assert e.value.code == code, (name, str(e.value))
            _assert_device_equals(fe, states, st0, set(), name)
    # the valid deltas pass, the one on the stream with a database included
    assert states[0].apply(good0) == 0 and states[2].apply(good2) == 0
    fe.update_maps([good2, good0])
    _assert_device_equals(fe, states, st0, {0, 2}, "after the refusals")
    fe.close()


# ---------------------------------------------------------------- 3. / 4. a constructed delta in a tracked sequence
G, SEED, K_BEFORE, N_WITHHELD = 2600, 4, 2, 12
# With the scene's usual budget of 100 good features the last frame alone fills the budget on every step, and
# SearchReferencePointsInFrustum leaves at once with the leftovers of the stale mbTrackInView flags
# (Tracking.cc:3231-3249): a point that enters the map then is never looked at, in the reference as here. A budget
# above the last frame's matches makes the step search the local map, where the appended points are.
BUDGET = 400
_RUNS = {}


def _chain(m, voc, M, budget):
    """An oracle chain over the map dict ``m`` without a keyframe database."""
    ch = C.Chain("euroc", 1000, M, budget)
    ch.set_map(m["mp"], m["desc"])
    ch.set_covis(m["graph"])
    ch.set_kfdb(None)
    ch.set_vocab(voc)
    return ch


def _voc():
    from gf_orb_slam_amd import synth

    return synth.synth_vocabulary_fast(11, k=10, L=5)


def _permuted(gm, last):
    """The map with the points ``last`` moved to the highest indices."""
    n = len(gm["mp"])
    keep = np.setdiff1d(np.arange(n), last)
    old_of_new = np.concatenate([keep, np.asarray(last, np.int64)])
    new_of_old = np.empty(n, np.int32)
    new_of_old[old_of_new] = np.arange(n, dtype=np.int32)
    g = gm["graph"]
    kf_mp = np.where(g["kf_mp"] >= 0, new_of_old[np.maximum(g["kf_mp"], 0)], -1).astype(np.int32)
    obs = S.rows_of(g["mp_obs_off"], g["mp_obs"])
    g1 = S.graph_of(S.rows_of(g["kf_mp_off"], kf_mp), g["kf_bad"], S.rows_of(g["kf_cov_off"], g["kf_cov"]),
                    np.asarray(g["mp_bad"])[old_of_new], [obs[i] for i in old_of_new])
    return dict(mp=gm["mp"][old_of_new].copy(), desc=gm["desc"][old_of_new].copy(), graph=g1)


def _withheld(m1, n0):
    """M0 / G0: the map without the points >= n0 and without the last keyframe."""
    g = m1["graph"]
    last = len(g["kf_bad"]) - 1
    kf_rows = [np.where(r >= n0, -1, r).astype(np.int32) for r in S.rows_of(g["kf_mp_off"], g["kf_mp"])[:last]]
    cov = [r[r != last] for r in S.rows_of(g["kf_cov_off"], g["kf_cov"])[:last]]
    obs = [r[r != last] for r in S.rows_of(g["mp_obs_off"], g["mp_obs"])[:n0]]
    return dict(mp=m1["mp"][:n0].copy(), desc=m1["desc"][:n0].copy(),
                graph=S.graph_of(kf_rows, g["kf_bad"][:last], cov, g["mp_bad"][:n0], obs))


def _feedback_scene():
    """The scene of test_track_loss_gpu with B = 2, and for stream 0 the full
    map permuted so that N_WITHHELD points the chain newly matches on step
    K_BEFORE + 1 come last (M1 / G1), and the map without them (M0 / G0)."""
    if "scene" in _RUNS:
        return _RUNS["scene"]
    import test_track_loss_gpu as TL

    voc = _voc()
    W, fr, gmaps, dbs, fe, T, V, dvoc = TL._scene_setup(2, G, SEED, voc)
    fe.close()
    s0 = W.scene_of[0]
    ch = _chain(gmaps[s0], voc, G, BUDGET)
    ch.set_rng(7)
    ch.bootstrap(fr[s0, W.phase[0] % W.period], T[0], V[0])
    seen = []
    for k in range(1, K_BEFORE + 2):
        ch.step(fr[s0, (W.phase[0] + k) % W.period])
        seen.append(np.unique(ch.read("kp2mp")[:int(ch.read("nkp"))]))
    # the points step K_BEFORE + 1 matches afresh: the local-map searches found them, not the last frame, so a
    # tracker that receives them between the two steps can find them the same way
    fresh = np.setdiff1d(seen[-1][seen[-1] >= 0], seen[-2])
    assert len(fresh) >= N_WITHHELD, len(fresh)
    m1 = _permuted(gmaps[s0], fresh[:N_WITHHELD])
    n0 = len(m1["mp"]) - N_WITHHELD
    sc = dict(W=W, fr=fr, gmaps=gmaps, dbs=dbs, T=T, V=V, dvoc=dvoc, voc=voc, m1=m1, m0=_withheld(m1, n0), n0=n0)
    _RUNS["scene"] = sc
    return sc


def _feedback_run(captured):
    """K_BEFORE steps on M0, the delta M0 -> M1' (M1 with a few tracked points
    moved and one matched point bad), one more step. -> the states read after
    every step and around the update, the delta, M1'."""
    import torch

    sc = _feedback_scene()
    W, fr, T, V = sc["W"], sc["fr"], sc["T"], sc["V"]
    fe = FrontEnd("euroc", 1000, 2, G, BUDGET)
    fe.set_vocab(sc["dvoc"])
    fe.set_map(0, sc["m0"]["mp"], sc["m0"]["desc"])
    fe.set_covis(0, sc["m0"]["graph"])  # no database on the stream that gets a keyframe
    gm = sc["gmaps"][W.scene_of[1]]
    fe.set_map(1, gm["mp"], gm["desc"])
    fe.set_covis(1, gm["graph"])
    fe.set_kfdb(1, sc["dbs"][W.scene_of[1]])
    for b in range(2):
        fe.set_rng(b, 7 + b)
    fe.set_source(torch.from_numpy(fr).cuda().contiguous(), W.scene_of, W.phase)
    fe.bootstrap(T, V, 0.0)
    out = dict(steps=[])
    for k in range(1, K_BEFORE + 1):
        if captured and k == 2:  # the first step ran eagerly (it sizes the context's scratch)
            fe.capture_graph()
        fe.step()
        out["steps"].append(C.read_state(fe))
    before = out["steps"][-1]
    # M1': tracked points moved by a small offset, one matched point bad
    n0 = sc["n0"]
    tracked = np.unique(before["kp2mp"][0][:int(before["nkp"][0])])
    tracked = tracked[(tracked >= 0) & (tracked < n0)]
    assert len(tracked) > 20
    m1 = dict(mp=sc["m1"]["mp"].copy(), desc=sc["m1"]["desc"], graph={k: v.copy() for k, v in sc["m1"]["graph"].items()})
    moved, bad = tracked[1:9], int(tracked[0])
    m1["mp"]["pos"][moved] += np.float32(1e-3)
    m1["graph"]["mp_bad"][bad] = 1
    delta = S.diff(0, sc["m0"], m1)
    assert len(delta.new_mp) == N_WITHHELD and len(delta.new_kf_off) == 2 and len(delta.slot_kf) > 0
    assert delta.set_mp_idx.tolist() == moved.tolist() and delta.bad_mp.tolist() == [bad]
    fe.update_maps(delta)
    out["updated"] = C.read_state(fe)
    out["graphs"] = [fe.covis(0), fe.covis(1)]
    fe.step()
    out["steps"].append(C.read_state(fe))
    fe.close()
    out.update(delta=delta, m1=m1, moved=moved, bad=bad)
    return out


def test_state_survives_and_the_tracker_sees_the_change():
    import test_track_loss_gpu as TL

    sc = _feedback_scene()
    run = _RUNS["eager"] = _feedback_run(False)
    before, upd, after, m1, n0 = run["steps"][K_BEFORE - 1], run["updated"], run["steps"][K_BEFORE], run["m1"], sc["n0"]
    # the update itself: the map of stream 0 is M1', stream 1 and every per-point state row are untouched
    n1 = len(m1["mp"])
    assert int(upd["nmp"][0]) == n1 and upd["map"][0][:n1].tobytes() == m1["mp"].tobytes()
    assert np.array_equal(upd["map_desc"][0][:n1], m1["desc"]) and R.same_graph(run["graphs"][0], m1["graph"]) == []
    assert R.same_graph(run["graphs"][1], sc["gmaps"][sc["W"].scene_of[1]]["graph"]) == []
    for k in ("mp_H", "mp_info", "mp_upd", "mp_uv", "views"):
        assert upd[k][0][:n0].tobytes() == before[k][0][:n0].tobytes(), k
        assert upd[k][1].tobytes() == before[k][1].tobytes(), k
    for k in C.FIELDS:
        if k not in ("map", "map_desc", "nmp", "last_pos", "mp_upd", "views"):
            assert upd[k].tobytes() == before[k].tobytes(), k
    assert upd["map"][1].tobytes() == before["map"][1].tobytes() and int(upd["nmp"][1]) == int(before["nmp"][1])
    assert np.all(upd["mp_upd"][0][n0:n1] == -1000) and not upd["views"][0][n0:n1].view(np.uint8).any()
    # GF_FE_LAST_POS follows the moved points, and nothing else of it moved
    lk = before["last_kp2mp"][0][:int(before["last_nkp"][0])]
    rows = np.nonzero(np.isin(lk, run["moved"]))[0]
    assert len(rows) > 0 and np.array_equal(upd["last_pos"][0][rows], m1["mp"]["pos"][lk[rows]])
    rest = np.setdiff1d(np.arange(upd["last_pos"].shape[1]), rows)
    assert upd["last_pos"][0][rest].tobytes() == before["last_pos"][0][rest].tobytes()
    assert upd["last_pos"][1].tobytes() == before["last_pos"][1].tobytes()
    # the next step equals the chain built on M1' / G1' and loaded with the device state
    s0 = sc["W"].scene_of[0]
    img = sc["fr"][s0, (sc["W"].phase[0] + K_BEFORE + 1) % sc["W"].period]
    ch = _chain(m1, sc["voc"], G, BUDGET)
    ch.load_from(upd, 0)
    ch.write("reloc", upd["reloc"][0])
    ch.step(img)
    TL._compare(after, ch, 0, "the step after the update: ")
    for name, kp in (("chain", ch.read("kp2mp")), ("device", after["kp2mp"][0])):
        assert np.any(kp >= n0), f"{name}: no withheld point is matched after the update"
        assert run["bad"] not in kp.tolist(), f"{name}: the bad point is still in the frame"
    assert run["bad"] in before["kp2mp"][0].tolist()


def test_the_same_run_through_a_captured_graph():
    eager = _RUNS.get("eager") or _feedback_run(False)
    cap = _feedback_run(True)
    assert R.same_graph(cap["graphs"][0], eager["graphs"][0]) == []
    pairs = list(zip(cap["steps"], eager["steps"])) + [(cap["updated"], eager["updated"])]
    for i, (a, b) in enumerate(pairs):
        for k in C.FIELDS:
            if k != "clock":
                assert a[k].tobytes() == b[k].tobytes(), (i, k)


# ---------------------------------------------------------------- 5. the closed loop
def test_closed_loop_tracker_keyframe_mapper_map_tracker():
    import torch

    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import tracking
    from gf_orb_slam_amd.localmapping import LocalMapper

    voc = _voc()
    W, fr, gmaps, dbs, fe0, T, V, dvoc = TL._scene_setup(1, G, 4, voc)
    fe0.close()
    gm = gmaps[0]
    M = len(gm["mp"]) + 1400  # room for what CreateNewMapPoints appends
    fe = FrontEnd("euroc", 1000, 1, M, 100)
    fe.set_vocab(dvoc)
    fe.set_map(0, gm["mp"], gm["desc"])
    fe.set_covis(0, gm["graph"])  # no database: the graph is about to grow
    fe.set_rng(0, 7)
    fe.set_source(torch.from_numpy(fr).cuda().contiguous(), W.scene_of, W.phase)
    fe.bootstrap(T, V, 0.0)
    m = tracking.loopmap_from_global_map(TL.INFO, gm, voc=dvoc)
    nkf0, nmp0 = m.nkf, len(m.mps)
    fb = tracking.MapFeedback(fe, 0, m)
    ins = tracking.KeyFrameInserter(fe, [LocalMapper(m, dvoc)], feedback=[fb])
    assert ins.feed_back() == []  # no mapper ran
    fe.enable_keyframes()
    k = 0
    while not fe.keyframe_state()["pending"][0]:
        k += 1
        assert k <= 4, "no keyframe within four steps"
        fe.step()
    assert ins.pump() == [(0, nkf0)]
    rep = ins.run_mapper(0)
    assert rep["to_loop_closer"] == nkf0
    sent = ins.feed_back()
    assert len(sent) == 1 and len(sent[0].new_kf_off) == 2 and ins.feed_back() == []
    print(f"the mapper appended {len(m.mps) - nmp0} points, rewrote {len(sent[0].set_mp_idx)}, "
          f"replaced {len(sent[0].obs_mp)} observation rows, wrote {len(sent[0].slot_kf)} slots")
    g, want = fe.covis(0), tracking.covis_graph_from_loopmap(m)
    assert R.same_graph(g, want) == []
    n = len(m.mps)
    st = C.read_state(fe)
    assert int(st["nmp"][0]) == n and st["map"][0][:n].tobytes() == m.mps.tobytes()
    assert np.array_equal(st["map_desc"][0][:n], m.mp_desc)
    off = g["kf_mp_off"]
    assert len(g["kf_bad"]) == nkf0 + 1 and np.array_equal(g["kf_mp"][off[nkf0]:off[nkf0 + 1]], m.slots[nkf0])
    assert (m.slots[nkf0] >= 0).sum() > 15
    # the next step tracks the mapper's map
    ch = _chain(dict(mp=m.mps, desc=m.mp_desc, graph=want), voc, M, 100)
    ch.load_from(st, 0)
    ch.write("reloc", st["reloc"][0])
    fe.step()
    ch.step(fr[0, (W.phase[0] + k + 1) % W.period])
    TL._compare(C.read_state(fe), ch, 0, "the step after the feedback: ")
    fe.close()
