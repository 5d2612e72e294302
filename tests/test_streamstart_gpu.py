"""Stream start, park and reset on the device (csrc/streamstart.hip,
gf_frontend_start_streams, gf_frontend_set_lifecycle): a started stream against
the serial restatement (tests/streamstart_ref.py) and against a twin front end
given the same state through set_map / set_covis / set_kfdb / write, over the
shapes at which the kernels can go wrong; the refusals; the third tracking
state (a parked stream's carried state is byte-identical) and the reset rule
inside a tracked sequence against the oracle chain; a parked stream started
again; a start between replays of a captured graph; and the path from the
monocular initialiser to a tracked stream. Every comparison of the feature's
own outputs is byte equality."""
import numpy as np
import pytest

import mapupdate_ref as MR
import mapupdate_scenes as S
import oracle_chain as C
import streamstart_ref as R
import streamstart_scenes as SS
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.pipeline import KF, STATS, TR, FrontEnd, KeyframeDB

pytestmark = pytest.mark.gpu

NLEFT = STATS.index("nleft")
FIELDS = R.WRITTEN + R.UNTOUCHED
_VOC = {}


def _dvoc():
    if not _VOC:
        from gf_orb_slam_amd import synth
        from gf_orb_slam_amd.bow import ORBVocabulary

        _VOC["tree"] = synth.synth_vocabulary_fast(11, k=10, L=5)
        _VOC["dev"] = ORBVocabulary(_VOC["tree"])
    return _VOC["dev"]


def _snapshot(fe, dbs=None):
    st = {k: fe.read(k) for k in FIELDS + ("stats",)}
    try:
        ks = fe.keyframe_state()
    except GFError:
        ks = None
    return dict(st=st, graphs=[fe.covis(b) for b in range(fe.B)], ks=ks,
                dbs={b: db.read(fe.ctx) for b, db in (dbs or {}).items()})


def _stream(snap, b):
    """One stream of a snapshot as the restatement takes it."""
    out = {k: snap["st"][k][b].copy() for k in FIELDS}
    out["graph"] = snap["graphs"][b]
    out["nleft"] = int(snap["st"]["stats"][NLEFT, b])
    out["kf"] = {w: int(snap["ks"][w][b]) for w in KF} if snap["ks"] is not None else None
    return out


def _assert_stream(got, want, tag, fields=FIELDS):
    for k in fields:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), f"{tag}: {k}"
    assert MR.same_graph(got["graph"], want["graph"]) == [], tag
    assert got["nleft"] == want["nleft"] and got["kf"] == want["kf"], f"{tag}: {got['kf']} / {want['kf']}"


def _same_db(a, b, tag):
    assert a["nkf"] == b["nkf"], tag
    for k in b:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{tag}: database {k}"


def _scribble(fe, seed):
    """Sentinels and random state in every buffer a start must overwrite or
    must leave alone, so that either mistake shows."""
    rng = np.random.default_rng(seed)
    for k in ("map", "map_desc", "views", "last_kps", "last_desc", "last_pos", "reloc", "left"):
        a = fe.read(k)
        a.view(np.uint8)[...] = S.SENTINEL
        fe.write(k, a)
    for k, lo, hi in (("mp_upd", -5, 3), ("last_kp2mp", -1, 1), ("kp2mp", -1, 1), ("outlier", 0, 2), ("last_outlier", 0, 2)):
        a = fe.read(k)
        fe.write(k, rng.integers(lo, hi, a.shape).astype(a.dtype))
    for k in ("mp_H", "mp_info", "mp_uv", "velocity", "Xv", "Xv_next", "base", "Tcw_last", "t_prev", "t_cur"):
        a = fe.read(k)
        fe.write(k, rng.normal(size=a.shape).astype(a.dtype))
    a = fe.read("track")
    a[:, 1:6] = rng.integers(0, 50, (fe.B, 5))  # every word a start sets but STATE; the two spare words stay 0
    fe.write("track", a)
    st = fe.read("stats")
    st[NLEFT] = rng.integers(0, 5, fe.B)
    fe.write("stats", st)


def _empty_frontend(B, M, dbs=(), keyframes=True, max_rows=4000, seed=1, max_kf=64):
    """A front end made by enable_lifecycle alone: every stream parked on an
    empty graph; streams in ``dbs`` get an empty growable database."""
    fe = FrontEnd("euroc", 1000, B, M, 100)
    fe.set_vocab(_dvoc())
    fe.enable_lifecycle()
    assert fe.lifecycle().tolist() == [2] * B
    held = {}
    for b in dbs:
        held[b] = KeyframeDB([], [], _dvoc().transform, max_kf=max_kf, max_rows=max_rows)
        fe.set_kfdb(b, held[b])
    if keyframes:
        fe.enable_keyframes()
    _scribble(fe, seed)
    return fe, held


def _start_and_check(fe, dbs, reqs, built, tag):
    """Send the requests; every stream (named or not) equals the restatement,
    every database one built from the request's rows. -> the snapshot after."""
    before = _snapshot(fe, dbs)
    fe.start_streams(reqs)
    after = _snapshot(fe, dbs)
    named = {r.stream: r for r in reqs}
    for b in range(fe.B):
        want = R.start(_stream(before, b), named[b]) if b in named else _stream(before, b)
        _assert_stream(_stream(after, b), want, f"{tag}: stream {b}")
    for b, db in dbs.items():
        if b not in named:
            _same_db(after["dbs"][b], before["dbs"][b], f"{tag}: stream {b} (not named)")
            continue
        kps, desc = built.get(b, ([], []))
        want = KeyframeDB(kps, desc, _dvoc().transform, max_kf=db.max_kf, max_rows=db.max_rows)
        _same_db(after["dbs"][b], want.read(fe.ctx), f"{tag}: stream {b}")
        for k in KeyframeDB._ARRAYS:
            assert getattr(db, k).tobytes() == getattr(want, k).tobytes(), f"{tag}: stream {b}: host {k}"
    return after


def _requests(fe, plan, seed, dbs=()):
    """plan: {stream: (map, n_last)} -> (requests, {stream: (kps, desc)} of the database rows)."""
    reqs, built = [], {}
    for i, (b, (m, n_last)) in enumerate(plan.items()):
        rows = None
        if b in dbs and len(m["graph"]["kf_bad"]):
            rows, kps, desc = SS.db_rows(m, _dvoc().transform, seed + 50 + i)
            built[b] = (kps, desc)
        reqs.append(SS.request(b, m, n_last, seed + i, rows=rows))
    return reqs, built


# ---------------------------------------------------------------- 1. state equality
def _twin_of(fe, snap, reqs, built, dbs, M):
    """An uncaptured front end given the same state the only way there was
    before: set_map, set_covis, set_kfdb of a database built from the same
    keyframes, and write of the last-frame, tracking and keyframe fields."""
    tw = FrontEnd("euroc", 1000, fe.B, M, 100)
    tw.set_vocab(_dvoc())
    named = {r.stream: r for r in reqs}
    for b in range(fe.B):
        r = named[b]
        tw.set_map(b, r.map.new_mp, r.map.new_mp_desc)
        tw.set_covis(b, R.graph_of_delta(r.map))
        if b in dbs:
            kps, desc = built.get(b, ([], []))
            dbs[b]["twin"] = KeyframeDB(kps, desc, _dvoc().transform, max_kf=64, max_rows=dbs[b]["max_rows"])
            tw.set_kfdb(b, dbs[b]["twin"])
    tw.enable_keyframes()
    w = {k: tw.read(k) for k in ("last_kps", "last_desc", "last_nkp", "last_kp2mp", "last_outlier", "last_pos",
                                 "Tcw_last", "t_prev", "t_cur", "track", "kp2mp", "outlier")}
    for b, r in named.items():
        n = len(r.kps)
        w["last_kps"][b, :n], w["last_desc"][b, :n], w["last_kp2mp"][b, :n] = r.kps, r.desc, r.kp2mp
        w["last_outlier"][b, :n] = 0
        w["last_pos"][b, :n] = np.where(r.kp2mp[:, None] >= 0, r.map.new_mp["pos"][np.maximum(r.kp2mp, 0)], 0) if n else 0
        w["last_nkp"][b], w["Tcw_last"][b], w["t_prev"][b], w["t_cur"][b] = n, r.Tcw, r.timestamp, r.timestamp
        w["track"][b, :6] = (0, 0, r.since_reloc, 2, r.frame_id, 1)
        w["kp2mp"][b], w["outlier"][b] = -1, 0
    for k, a in w.items():
        tw.write(k, a)
    # what a start leaves alone is whatever the stream held: the twin gets the same bytes
    for k in ("mp_H", "mp_info", "mp_uv", "velocity", "rng"):
        tw.write(k, snap["st"][k])
    ks = fe.keyframe_state()
    tw.set_keyframe_state(**{k: ks[k] for k in KF})
    return tw


def test_shapes_against_the_restatement_and_a_twin():
    """nmp 1, 63, 64, 65, 255, 256, 257 and map_cap; 1, 2 and 64 keyframes;
    n_last 0, 1, 255, 256, 257 and the capacity; observation totals 1023, 1024
    and 1025; every stream starts from nothing (a front end made by
    enable_lifecycle alone). Then the same streams are started a second time,
    on smaller maps while they hold a larger one and a pending keyframe."""
    M = 300
    fe, dbs = _empty_frontend(8, M, dbs=(0, 2, 4, 7))
    cap = fe.cap
    shapes = [(1, 1, None, 0), (63, 2, None, 1), (64, 64, None, 255), (65, 1, None, 256), (255, 5, 1023, 257),
              (256, 5, 1024, cap), (257, 5, 1025, 10), (M, 2, None, 20)]
    plan = {b: (SS.graph_map(100 + b, n, k, slots=(1, 9) if k == 64 else (1, 40), obs=o, odd_offsets=b % 2 == 1), nl)
            for b, (n, k, o, nl) in enumerate(shapes)}
    reqs, built = _requests(fe, plan, 7, dbs)
    after = _start_and_check(fe, dbs, reqs, built, "first start")
    assert fe.lifecycle().tolist() == [0] * 8
    assert [len(g["mp_obs"]) for g in after["graphs"][4:7]] == [1023, 1024, 1025]
    # the twin, set up the only way possible before
    info = {b: dict(max_rows=db.max_rows) for b, db in dbs.items()}
    tw = _twin_of(fe, after, reqs, built, info, M)
    a, t = _snapshot(fe, dbs), _snapshot(tw, {b: info[b]["twin"] for b in info})
    for b, r in enumerate(reqs):
        n, nl = len(r.map.new_mp), len(r.kps)
        for k in C.Chain.STATE:
            count = n if k in ("map", "map_desc", "views", "mp_H", "mp_info", "mp_uv", "mp_upd") else \
                nl if k.startswith("last_") and k != "last_nkp" else None
            x, y = a["st"][k][b], t["st"][k][b]
            if count is not None:
                x, y = x[:count], y[:count]
            assert x.tobytes() == y.tobytes(), f"twin: stream {b}: {k}"
        assert MR.same_graph(a["graphs"][b], t["graphs"][b]) == [], f"twin: stream {b}"
        assert all(a["ks"][w][b] == t["ks"][w][b] for w in KF), f"twin: stream {b}: keyframe words"
    for b in dbs:
        _same_db(a["dbs"][b], t["dbs"][b], f"twin: stream {b}")
    tw.close()
    # a second start of every stream: smaller maps onto larger ones, a pending keyframe of the old map dropped
    fe.set_keyframe_state(accept=0, pending=1, abort=1, since=9, decision=65, ref=0, seq=3)
    plan2 = {b: (SS.graph_map(200 + b, max(1, n // 3), 1 + b % 3, slots=(1, 15)), 5 + 30 * b)
             for b, (n, k, o, nl) in enumerate(shapes)}
    reqs2, built2 = _requests(fe, plan2, 9, dbs)
    after2 = _start_and_check(fe, dbs, reqs2, built2, "second start")
    assert not after2["ks"]["pending"].any() and after2["ks"]["seq"].tolist() == [3] * 8
    assert fe.take_keyframes() == []
    # rows past the new counts kept their bytes (the first start's)
    for b, (n, _, _, _) in enumerate(shapes):
        n2 = len(reqs2[b].map.new_mp)
        assert after2["st"]["map"][b][n2:n].tobytes() == after["st"]["map"][b][n2:n].tobytes()
    fe.close()


def test_stream_subsets():
    """First, last, alternate and all streams named; the streams not named are
    byte-identical to those of an untouched twin front end; an empty call
    changes nothing."""
    M = 128
    fe, dbs = _empty_frontend(4, M, dbs=(0, 3), seed=3)
    tw, tdbs = _empty_frontend(4, M, dbs=(0, 3), seed=3)
    maps = {b: SS.graph_map(300 + b, 90, 6, odd_offsets=True) for b in range(4)}
    first = {b: (maps[b], 40 + b) for b in range(4)}
    for f, d in ((fe, dbs), (tw, tdbs)):  # both hold the same maps to begin with
        reqs, built = _requests(f, first, 11, d)
        _start_and_check(f, d, reqs, built, "set-up")
    untouched = _snapshot(tw, tdbs)
    touched = set()
    for r, names in enumerate(([0], [3], [0, 2], [3, 2, 1, 0])):
        plan = {b: (SS.graph_map(400 + 10 * r + b, 30 + 17 * b, 1 + b), 17 * b) for b in names}
        reqs, built = _requests(fe, plan, 20 + r, dbs)
        after = _start_and_check(fe, dbs, reqs, built, f"round {r}")
        touched |= set(names)
        for b in set(range(4)) - touched:
            _assert_stream(_stream(after, b), _stream(untouched, b), f"round {r}: stream {b} against the twin")
    mid = _snapshot(fe, dbs)
    fe.start_streams([])
    now = _snapshot(fe, dbs)
    for b in range(4):
        _assert_stream(_stream(now, b), _stream(mid, b), f"empty call: stream {b}")
    fe.close()
    tw.close()


# ---------------------------------------------------------------- 2. refusals
def test_refusals_leave_every_stream_untouched():
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    M = 1400  # above the keypoint capacity, so that a map can pass the observation capacity of 64 x cap
    fe, dbs = _empty_frontend(4, M, dbs=(1,), max_rows=200, seed=5, max_kf=4)
    cap = fe.cap
    base = {b: (SS.graph_map(500 + b, 40, 3, slots=(2, 9)), 30) for b in range(3)}
    reqs, built = _requests(fe, base, 31, dbs)
    _start_and_check(fe, dbs, reqs, built, "set-up")
    # stream 2: a fixed database over its three keyframes; stream 3 stays empty
    n2 = np.diff(base[2][0]["graph"]["kf_mp_off"])
    rng = np.random.default_rng(2)
    fixed = KeyframeDB([np.zeros(n, KEYPOINT_DTYPE) for n in n2],
                       [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in n2], _dvoc().transform)
    fe.set_kfdb(2, fixed)
    before = _snapshot(fe, dbs)
    bad, good, m = SS.refusal_cases(cap, M, _dvoc().transform)
    kinds = {0: None, 1: (4, 200), 2: "fixed", 3: None}
    for name, (r, code) in bad.items():
        others = [g for g in good if g.stream != r.stream or name == "stream named twice"]
        for call in ([r] + others, others + [r]):
            with pytest.raises(GFError) as e:
                fe.start_streams(call)
            assert e.value.code == code, (name, str(e.value))
            named = [0] if name == "stream named twice" else []
            assert R.verdict(r, cap, M, named=named, nstreams=4, db=kinds.get(r.stream)) == code, name
            now = _snapshot(fe, dbs)
            for b in range(4):
                _assert_stream(_stream(now, b), _stream(before, b), f"{name}: stream {b}")
            _same_db(now["dbs"][1], before["dbs"][1], name)
            assert dbs[1].nkf == 3, name
    # the valid requests pass afterwards: the mirrors were put back
    reqs, built = _requests(fe, {0: (m, 10), 1: (m, 4), 3: (m, 0)}, 43, dbs)
    _start_and_check(fe, dbs, reqs, built, "after the refusals")
    fe.close()


# ---------------------------------------------------------------- 3. park and reset inside a tracked sequence
G, SEED = 2600, 4
_SC = {}


def _scene(n_kf):
    """test_track_loss_gpu's scene on two streams; stream 0's frames 5 and 6
    are blank. Maps of n_kf keyframes, fixed databases."""
    if n_kf not in _SC:
        import test_track_loss_gpu as TL
        from gf_orb_slam_amd import scene

        W0 = scene.Workload("euroc", 2, n_scenes=2, period=32, seed=SEED)
        blank = [(W0.scene_of[0], (W0.phase[0] + k) % 32) for k in (5, 6)]
        _dvoc()
        W, fr, gmaps, dbs, fe, T, V, dvoc = TL._scene_setup(2, G, SEED, _VOC["tree"], blank=blank, n_kf=n_kf)
        fe.close()
        _SC[n_kf] = dict(W=W, fr=fr, gmaps=gmaps, dbs=dbs, T=T, V=V, dvoc=dvoc)
    return _SC[n_kf]


def _tracked(sc, lifecycle, growable=False, keyframes=False, frames=None):
    """A front end over the scene (or over ``frames`` in its place),
    bootstrapped. growable: stream 0 gets a growable copy of its database (a
    start can empty that one)."""
    import torch

    W = sc["W"]
    fe = FrontEnd("euroc", 1000, 2, G, 100)
    fe.set_vocab(sc["dvoc"])
    held = []
    for b in range(2):
        gm = sc["gmaps"][W.scene_of[b]]
        fe.set_map(b, gm["mp"], gm["desc"])
        fe.set_covis(b, gm["graph"])
        db = sc["dbs"][W.scene_of[b]]
        if growable and b == 0:
            db = KeyframeDB(gm["kf_kps"], gm["kf_desc"], sc["dvoc"].transform, max_kf=64,
                            max_rows=sum(len(k) for k in gm["kf_kps"]) + 2000)
        held.append(db)
        fe.set_kfdb(b, db)
        fe.set_rng(b, 7 + b)
    fe.set_source(torch.from_numpy(sc["fr"] if frames is None else frames).cuda().contiguous(), W.scene_of, W.phase)
    if lifecycle:
        fe.enable_lifecycle()
    fe.bootstrap(sc["T"], sc["V"], 0.0)
    if keyframes:
        fe.enable_keyframes()
        fe.set_keyframe_state(accept=0)
    return fe, held


def _chain_step(sc, dbs, before, b, k):
    import test_track_loss_gpu as TL

    W = sc["W"]
    s = W.scene_of[b]
    ch = TL._chain(sc["gmaps"][s], dbs[b], _VOC["tree"], G)
    ch.load_from(before, b)
    ch.write("reloc", before["reloc"][b])
    ch.step(sc["fr"][s, (W.phase[b] + k) % W.period])
    return ch


def _run_against_the_chain(sc, fe, dbs, nsteps):
    import test_track_loss_gpu as TL

    dev = C.read_state(fe)
    log = []
    for k in range(1, nsteps + 1):
        before = dev
        fe.step()
        dev = C.read_state(fe)
        for b in range(2):
            TL._compare(dev, _chain_step(sc, dbs, before, b, k), b, f"step {k}: ")
        log.append([tuple(int(dev["track"][b][TR[w]]) for w in ("state", "path", "ok")) for b in range(2)])
    return log


def test_switch_off_five_keyframes_equals_the_chain():
    """The parent's behaviour: without the switch a stream that loses track
    on a map of five keyframes is LOST (state 1), and every field of every
    step equals the oracle chain."""
    sc = _scene(5)
    fe, dbs = _tracked(sc, lifecycle=False)
    log = _run_against_the_chain(sc, fe, dbs, 8)
    assert log[4][0][0] == 1 and all(r[b][0] != 2 for r in log for b in range(2)), log
    fe.close()


def test_six_keyframes_lost_and_relocalises_like_the_chain():
    """With the switch on and six keyframes the rule does not fire: the
    stream is LOST and relocalises, every step equal to the chain."""
    sc = _scene(6)
    fe, dbs = _tracked(sc, lifecycle=True)
    log = _run_against_the_chain(sc, fe, dbs, 11)
    assert log[4][0][0] == 1 and all(r[0][0] != 2 for r in log), log
    assert any(r[0] == (0, 3, 1) for r in log[6:]), f"stream 0 did not relocalise: {log}"
    fe.close()


CARRIED = ("last_kps", "last_desc", "last_nkp", "last_kp2mp", "last_outlier", "last_pos", "Tcw_last", "velocity",
           "t_prev", "map", "map_desc", "nmp", "views", "mp_H", "mp_info", "mp_uv", "mp_upd", "rng", "reloc", "Xv",
           "Xv_next", "base", "left", "hist")


def test_five_keyframes_park_restart_and_the_other_stream():
    """With the switch on and five keyframes the stream is in state 2 after
    the step that lost it and stays there on frames it could relocalise on:
    its carried state is byte-identical, PATH 4, OK 0, Tcw zeros, and
    poll_resets reports it once. The other stream equals a twin front end
    without the switch, byte for byte. Started again on its own map with a last
    frame recorded earlier (one loop of the source later), the stream tracks,
    every field equal to the chain."""
    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import tracking
    from gf_orb_slam_amd.localmap import StreamStart

    sc = _scene(5)
    fe, dbs = _tracked(sc, lifecycle=True, growable=True, keyframes=True)
    tw, _ = _tracked(sc, lifecycle=False, growable=True, keyframes=True)
    ins = tracking.KeyFrameInserter(fe, {0: None})
    rec = None
    for k in range(1, 6):
        fe.step()
        tw.step()
        if k == 1:
            rec = C.read_state(fe)  # the last frame a restart can use: frame 1 of the loop
        assert ins.poll_resets() == ([0] if k == 5 else [])
    assert fe.lifecycle().tolist() == [2, 0] and tw.lifecycle().tolist() == [1, 0]
    parked, ks0, g0, db0 = C.read_state(fe), fe.keyframe_state(), fe.covis(0), dbs[0].read(fe.ctx)
    for k in range(6, 34):
        fe.step()
        tw.step()
        if k in (6, 9, 33):
            now, other = C.read_state(fe), C.read_state(tw)
            for f in CARRIED:
                assert now[f][0].tobytes() == parked[f][0].tobytes(), f"step {k}: {f} of the parked stream changed"
            tr = now["track"][0]
            assert (tr[TR["state"]], tr[TR["path"]], tr[TR["ok"]], tr[TR["vel"]]) == (2, 4, 0, 0), (k, tr)
            assert tr[TR["query"]] == parked["track"][0][TR["query"]] + k - 5 and not now["Tcw"][0].any()
            assert now["t_cur"][0] > parked["t_cur"][0] and now["nkp"][0] >= 0
            fl = int(now["stats"][STATS.index("flags"), 0])
            assert not fl & (2048 | 4096) and fl & 8192, (k, fl)
            ks = fe.keyframe_state()
            assert all(ks[w][0] == ks0[w][0] for w in KF), f"step {k}: keyframe words of the parked stream changed"
            assert MR.same_graph(fe.covis(0), g0) == []
            _same_db(dbs[0].read(fe.ctx), db0, f"step {k}")
            for f in C.FIELDS:  # the other stream: as if nothing had happened next to it
                if f not in ("clock", "stats"):
                    assert now[f][1].tobytes() == other[f][1].tobytes(), f"step {k}: {f} of the other stream"
            assert np.array_equal(now["stats"][:, 1], other["stats"][:, 1])
    assert ins.poll_resets() == []
    tw.close()
    # the restart: the stream's own map, its database rows, the frame recorded after step 2
    W = sc["W"]
    gm = sc["gmaps"][W.scene_of[0]]
    m = dict(mp=gm["mp"], desc=gm["desc"], graph=gm["graph"])
    d = S.diff(0, SS.EMPTY, m)
    d.kf_rows = KeyframeDB(gm["kf_kps"], gm["kf_desc"], sc["dvoc"].transform)
    n = int(rec["last_nkp"][0])
    req = StreamStart(d, rec["last_kps"][0][:n], rec["last_desc"][0][:n], rec["last_kp2mp"][0][:n], rec["Tcw_last"][0],
                      timestamp=float(rec["t_prev"][0]), frame_id=int(rec["track"][0][TR["query"]]), since_reloc=40)
    before = _snapshot(fe, {0: dbs[0]})
    fe.start_streams(req)
    after = _snapshot(fe, {0: dbs[0]})
    _assert_stream(_stream(after, 0), R.start(_stream(before, 0), req), "restart")
    _assert_stream(_stream(after, 1), _stream(before, 1), "restart: the other stream")
    assert fe.lifecycle().tolist() == [0, 0] and dbs[0].nkf == 5
    # a twin at the same place of the source, given the state the only way there was before: it holds the same
    # map and database already (set_map / set_covis / set_kfdb); the last frame, the words and the fresh per-point
    # state are written from the request, not from the front end under test; what a start leaves alone (MP_H,
    # MP_INFO, MP_UV, the velocity matrix, the rand() state) is whatever the stream held
    tw, _ = _tracked(sc, lifecycle=True, growable=True, keyframes=True)
    for k in range(1, 34):
        tw.step()
    dev = C.read_state(fe)
    nm = len(gm["mp"])
    w = {f: tw.read(f) for f in ("last_kps", "last_desc", "last_nkp", "last_kp2mp", "last_outlier", "last_pos", "Tcw_last",
                                 "t_prev", "t_cur", "track", "views", "mp_upd", "Xv", "Xv_next", "base", "reloc")}
    w["last_kps"][0, :n], w["last_desc"][0, :n], w["last_kp2mp"][0, :n] = req.kps, req.desc, req.kp2mp
    w["last_outlier"][0, :n] = 0
    w["last_pos"][0, :n] = np.where(req.kp2mp[:, None] >= 0, gm["mp"]["pos"][np.maximum(req.kp2mp, 0)], 0)
    w["last_nkp"][0], w["Tcw_last"][0], w["t_prev"][0], w["t_cur"][0] = n, req.Tcw, req.timestamp, req.timestamp
    w["track"][0, :6] = (0, 0, req.since_reloc, 2, req.frame_id, 1)
    w["views"][0, :nm].view(np.uint8)[...] = 0
    w["mp_upd"][0, :nm] = -1000
    for f in ("Xv", "Xv_next", "base"):
        w[f][0] = 0
    w["reloc"][0].view(np.uint8)[...] = 0
    for f, a in w.items():
        tw.write(f, a)
    for f in ("mp_H", "mp_info", "mp_uv", "velocity", "rng"):
        a = tw.read(f)
        a[0] = dev[f][0]
        tw.write(f, a)
    tw.set_keyframe_state(0, since=0, pending=0, abort=0, decision=0, ref=req.ref_kf)
    for k in (34, 35, 36):  # the loop's frames 2, 3 and 4; frame 5 is blank again
        prev = dev
        fe.step()
        tw.step()
        dev, other = C.read_state(fe), C.read_state(tw)
        TL._compare(dev, _chain_step(sc, dbs, prev, 0, k), 0, f"step {k} after the restart: ")
        for f in C.FIELDS:
            if f not in ("clock", "stats"):
                assert dev[f][0].tobytes() == other[f][0].tobytes(), f"step {k} after the restart: {f} against the twin"
        assert np.array_equal(dev["stats"][:, 0], other["stats"][:, 0]), f"step {k}"
        tr = dev["track"][0]
        assert tr[TR["state"]] == 0 and tr[TR["ok"]] == 1, (k, tr)
    kf, kt = fe.keyframe_state(), tw.keyframe_state()
    assert all(kf[w][0] == kt[w][0] for w in KF)
    tw.close()
    fe.close()


# ---------------------------------------------------------------- 4. a start between replays of a captured graph
def _restrict_points(g, keep):
    from gf_orb_slam_amd.tracking import restrict_graph

    mp_remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return restrict_graph(g, np.arange(len(g["kf_bad"]), dtype=np.int32), mp_remap)


def _captured_run(captured):
    sc = _scene(5)
    fe, dbs = _tracked(sc, lifecycle=True, growable=True, keyframes=True)
    fe.step()  # the first step allocates the context's scratch, which a capture cannot
    if captured:
        fe.capture_graph()
    fe.step()
    rec = C.read_state(fe)  # frame 2 of the loop; frames 3 and 4 follow, frame 5 is blank: the stream parks again
    gm = sc["gmaps"][sc["W"].scene_of[0]]
    # a smaller map of the same scene: every second point, the graph restricted to them
    keep = np.arange(len(gm["mp"])) % 2 == 0
    g = _restrict_points(gm["graph"], keep)
    m = dict(mp=gm["mp"][keep], desc=gm["desc"][keep], graph=g)
    d = S.diff(0, SS.EMPTY, m)
    d.kf_rows = KeyframeDB(gm["kf_kps"], gm["kf_desc"], sc["dvoc"].transform)
    remap = np.cumsum(keep) - 1
    n = int(rec["last_nkp"][0])
    kp = rec["last_kp2mp"][0][:n]
    kp = np.where((kp >= 0) & keep[np.maximum(kp, 0)], remap[np.maximum(kp, 0)], -1)
    from gf_orb_slam_amd.localmap import StreamStart

    fe.start_streams(StreamStart(d, rec["last_kps"][0][:n], rec["last_desc"][0][:n], kp, rec["Tcw_last"][0],
                                 timestamp=float(rec["t_prev"][0]), frame_id=int(rec["track"][0][TR["query"]]),
                                 since_reloc=40))
    out = [_snapshot(fe, {0: dbs[0]})]
    for _ in range(3):
        fe.step()
        out.append(_snapshot(fe, {0: dbs[0]}))
    fe.close()
    return out


def test_start_between_replays_of_a_captured_graph_equals_eager():
    eager, graph = _captured_run(False), _captured_run(True)
    for i, (a, b) in enumerate(zip(eager, graph)):
        for s in range(2):
            _assert_stream(_stream(b, s), _stream(a, s), f"snapshot {i}: stream {s}")
        assert np.array_equal(a["st"]["stats"], b["st"]["stats"]), f"snapshot {i}"
        _same_db(b["dbs"][0], a["dbs"][0], f"snapshot {i}")
    tr = eager[-2]["st"]["track"][0]
    assert tr[TR["state"]] == 0 and tr[TR["ok"]] == 1, "the started stream does not track"
    assert eager[-1]["st"]["track"][0][TR["state"]] == 2, "the blank frame did not park it again"


# ---------------------------------------------------------------- 5. from the initialiser
def test_from_the_initialiser_to_a_started_stream():
    """Two views through MonoInitializer.feed until WORKING, then
    KeyFrameInserter.start on a captured front end whose other stream tracks
    a scene map: the started stream equals the restatement, and the growable
    database holds the two keyframes."""
    import initmap_scenes
    import searchinit_scenes
    from gf_orb_slam_amd import tracking

    sc = _scene(5)
    fe, dbs = _tracked(sc, lifecycle=True, growable=True, keyframes=True)
    fe.step()
    fe.capture_graph()
    fe.step()
    two = searchinit_scenes.two_view(1)
    mono = tracking.MonoInitializer(searchinit_scenes.INFO, two["K"], initmap_scenes.rng_state(1), voc=sc["dvoc"])
    state = None
    for fk, fd in ((two["kps1"], two["desc1"]), (two["kps2"], two["desc2"])):
        state, m, rep = mono.feed(fk, fd)
    assert state == tracking.WORKING and m.nkf == 2
    ins = tracking.KeyFrameInserter(fe, {})
    before = _snapshot(fe, {0: dbs[0]})
    req = ins.start(0, m, two["kps2"], two["desc2"], frame_id=1, timestamp=0.05, voc=sc["dvoc"])
    assert len(req.kps) <= fe.cap and (len(req.kps) == len(two["kps2"]) or np.all(req.kp2mp >= 0))
    after = _snapshot(fe, {0: dbs[0]})
    want = R.start(_stream(before, 0), req)
    want["kf"] = dict(want["kf"], accept=1, stop=0)  # the inserter hands mbAcceptKeyFrames back
    _assert_stream(_stream(after, 0), want, "from the initialiser")
    _assert_stream(_stream(after, 1), _stream(before, 1), "the other stream")
    fb = ins.feedback[0]
    assert np.array_equal(fb.mp_id, np.arange(len(m.mps))) and np.array_equal(fb.kf_id, [0, 1]) and fb.delta().empty()
    assert MR.same_graph(after["graphs"][0], tracking.covis_graph_from_loopmap(m)) == []
    built = KeyframeDB(m.kf_kps, m.kf_desc, sc["dvoc"].transform, max_kf=64, max_rows=dbs[0].max_rows)
    _same_db(after["dbs"][0], built.read(fe.ctx), "the two keyframes")
    assert dbs[0].nkf == 2
    fe.step()  # the captured graph replays over the started stream
    assert fe.lifecycle()[1] == 0
    fe.close()


def test_image_level_loop_from_two_frames_to_a_tracked_stream():
    """The oracle's initialiser accepts two frames of a rendered room four
    apart, so the whole loop runs on images: both frames are extracted on the
    device, MonoInitializer.feed makes the map, KeyFrameInserter.start puts it
    on stream 0 of a captured front end whose other stream tracks its scene
    map, and the next ten frames track, every field equal to the chain. Then a
    blank frame loses the stream and the second view's image relocalises it
    against the two keyframes of its database, equal to the chain as well."""
    import initmap_scenes
    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import ORBextractor, tracking

    sc = _scene(5)
    W = sc["W"]
    s0, p0 = W.scene_of[0], W.phase[0]
    V1, V2 = 8, 12  # the two views, as steps of the source
    fr = sc["fr"].copy()
    fr[s0, (p0 + V2 + 11) % 32] = 100                        # a blank frame after ten tracked ones
    fr[s0, (p0 + V2 + 12) % 32] = fr[s0, (p0 + V2) % 32]    # then the second view's image again
    fe, dbs = _tracked(sc, lifecycle=False, growable=True, keyframes=True, frames=fr)
    fe.step()
    fe.capture_graph()
    for _ in range(2, V2 + 1):
        fe.step()
    ex = ORBextractor(1000, 1.2, 8, 1, 20)
    K = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]], np.float32)
    mono = tracking.MonoInitializer(TL.INFO, K, initmap_scenes.rng_state(1), voc=sc["dvoc"])
    for v in (V1, V2):
        kps, desc = ex(fr[s0, (p0 + v) % 32])
        state, m, rep = mono.feed(kps, desc)
    assert state == tracking.WORKING and m.nkf == 2 and len(m.mps) >= 100, (state, rep)
    now = C.read_state(fe)
    ins = tracking.KeyFrameInserter(fe, {})
    req = ins.start(0, m, kps, desc, frame_id=int(now["track"][0][TR["query"]]), timestamp=float(now["t_cur"][0]),
                    voc=sc["dvoc"])
    fe.set_keyframe_state(0, accept=0)  # no keyframe leaves: the map stays the initialiser's
    assert len(req.kps) == len(kps) and dbs[0].nkf == 2
    gm = dict(mp=np.asarray(m.mps), desc=np.asarray(m.mp_desc), graph=tracking.covis_graph_from_loopmap(m))
    dev = C.read_state(fe)
    assert int(dev["nmp"][0]) == len(m.mps) and MR.same_graph(fe.covis(0), gm["graph"]) == []
    for k in range(V2 + 1, V2 + 13):
        before = dev
        fe.step()
        dev = C.read_state(fe)
        ch = TL._chain(gm, dbs[0], _VOC["tree"], G)
        ch.load_from(before, 0)
        ch.write("reloc", before["reloc"][0])
        ch.step(fr[s0, (p0 + k) % 32])
        TL._compare(dev, ch, 0, f"step {k}: ")
        tr = dev["track"][0]
        st = (int(tr[TR["state"]]), int(tr[TR["path"]]), int(tr[TR["ok"]]))
        if k <= V2 + 10:
            assert st == (0, 2, 1), f"step {k}: the started stream does not track: {st}"  # < 4 keyframes: TrackPreviousFrame
        elif k == V2 + 11:
            assert st[0] == 1, f"the blank frame did not lose the stream: {st}"
        else:
            assert st == (0, 3, 1), f"the second view's image did not relocalise the stream: {st}"
    assert fe.lifecycle()[1] == 0
    fe.close()
