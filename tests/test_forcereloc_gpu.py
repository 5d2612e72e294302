"""Forced relocalisation on the device (gf_frontend_force_relocalisation,
k_force_reloc, the forced branch of k_reloc_cand) against the oracle chain on
the scene of forcereloc_scenes.py: a B = 2 front end, stream 0 acted on, stream
1 the control. The chain cannot be told a candidate list; the tests give the
covisibility row of C[-1] the entries C[:-1], so that the forced list is the
list C the chain's DetectRelocalisationCandidates returns
(test_forcereloc_cpu.py pins that premise on the CPU's renderings; here C is
taken from the oracle on the device's renderings, and every test that edits a
row asserts that the edit leaves the chain's list unchanged)."""
import numpy as np
import pytest

import forcereloc_scenes as FS
import kfdb_grow_scenes as GS
import oracle_chain as C
from gf_orb_slam_amd._lib import GFError
from gf_orb_slam_amd.localmap import MapCompact
from gf_orb_slam_amd.pipeline import STATS, TR, FrontEnd

pytestmark = pytest.mark.gpu

_S = {}


def _scene():
    if _S:
        return _S
    import torch

    import oracle_lib as O
    from gf_orb_slam_amd.bow import ORBVocabulary

    voc = GS.vocabulary()
    W = GS.workload()
    frames = W.render_all("cuda").contiguous()
    blank = frames.clone()
    for s, i in GS.blank_frames(W):
        blank[s, i] = 100
    gmaps = W.build_global_maps(lambda im: O.extract(im), GS.G)
    dvoc = ORBVocabulary(voc)
    _, m1, rows = GS.maps_of(W, gmaps, dvoc.transform)
    gm1 = gmaps[W.scene_of[1]]
    rows1 = [(k, d) + tuple(dvoc.transform(d)) for k, d in zip(gm1["kf_kps"], gm1["kf_desc"])]
    T, V = W.boot_state()
    torch.cuda.synchronize()
    _S.update(W=W, frames=frames, fr=frames.cpu().numpy(), blank=blank, fr_blank=blank.cpu().numpy(), voc=voc, dvoc=dvoc,
              m1=m1, rows=rows, gm=gmaps[W.scene_of[0]], gm1=gm1, rows1=rows1, T=T, V=V, db=GS.database(rows),
              control={})
    return _S


def _frontend(sc, m, blank=False, growable=False):
    W, rows = sc["W"], sc["rows"]
    fe = FrontEnd("euroc", 1000, 2, GS.G, GS.BUDGET)
    fe.set_vocab(sc["dvoc"])
    fe.set_map(0, m["mp"], m["desc"])
    fe.set_covis(0, m["graph"])
    kw = dict(max_kf=len(rows) + 2, max_rows=sum(len(r[0]) for r in rows) + 100) if growable else {}
    fe.set_kfdb(0, GS.database(rows, **kw))
    fe.set_map(1, sc["gm1"]["mp"], sc["gm1"]["desc"])
    fe.set_covis(1, sc["gm1"]["graph"])
    fe.set_kfdb(1, GS.database(sc["rows1"]))
    for b in range(2):
        fe.set_rng(b, 7 + b)
    fe.set_source(sc["blank"] if blank else sc["frames"], W.scene_of, W.phase)
    fe.bootstrap(sc["T"], sc["V"], 0.0)
    return fe


def _run(k, m, request=None, captured=False, blank=False, growable=False, between=None):
    """Steps 1 .. k - 1, the request, (``between``), step k, step k + 1 -> the
    states around them and the candidate lists of step k."""
    sc = _scene()
    fe = _frontend(sc, m, blank, growable)
    for j in range(1, k):
        if captured and j == 2:  # the first step ran eagerly (it sizes the context's scratch)
            fe.capture_graph()
        fe.step()
    out = dict(before=C.read_state(fe))
    if request is not None:
        request(fe)
    out["pending"] = C.read_state(fe)
    if between is not None:
        out["between"] = between(fe)
        out["pending2"] = C.read_state(fe)
    fe.step()
    out["after"] = C.read_state(fe)
    out["cands"] = fe.reloc_candidates()
    fe.step()
    out["after2"] = C.read_state(fe)
    fe.close()
    return out


def _control(k, blank=False):
    """The states after steps k and k + 1 of a run with no request (stream 1 is
    the control of every test), and the one before step k."""
    sc = _scene()
    key = (k, blank)
    if key not in sc["control"]:
        r = _run(k, sc["m1"], blank=blank)
        sc["control"][key] = (r["after"], r["after2"], r["before"])
    return sc["control"][key]


def _cands(k, blank=False):
    """C: what DetectRelocalisationCandidates returns for frame k to a stream
    that is LOST there, on the unedited graph (the oracle, from the device's
    state before the step). The frames are the device's renderings, so the
    lists are taken here and not from the CPU pin; the tests that edit a row
    assert that the edit leaves the list unchanged."""
    sc = _scene()
    key = ("cands", k, blank)
    if key not in sc["control"]:
        before = _control(k, blank)[2]
        ch = FS.chain_step(sc["m1"], sc["db"], sc["voc"], FS.lost(before), 0, _frame(sc, 0, k, blank))
        oc, _, _ = GS.candidates(ch, before["reloc"][0], sc["db"], sc["m1"]["graph"], sc["voc"])
        n = int(ch.read("nkp"))
        nm = [FS.bow_matches(sc["rows"], sc["m1"]["graph"], int(c), ch.read("desc")[:n], ch.read("kps")[:n], sc["voc"])
              for c in oc]
        print(f"step {k}: the chain's candidates {oc.tolist()}, SearchByBoW matches {nm}, "
              f"relocalised {bool(ch.stats()['flags'] & 32768)}")
        sc["control"][key] = [int(c) for c in oc]
    return sc["control"][key]


def _assert_control(run, k, blank=False):
    """Stream 1 is byte-identical, in every field, to the same run without the
    request (the clock record holds device timestamps and is not compared)."""
    for name, ref in zip(("after", "after2"), _control(k, blank)[:2]):
        for f in C.FIELDS:
            if f == "clock":
                continue
            a, o = run[name][f], ref[f]
            if f == "stats":
                a, o = a[:, 1], o[:, 1]
            else:
                a, o = a[1], o[1]
            assert a.tobytes() == o.tobytes(), f"stream 1 {f} differs at step {k + (name == 'after2')}"


def _assert_request_wrote(run, kf, b=0):
    """The request wrote GF_TR_FORCE, GF_TR_FORCE_KF and GF_TR_SINCE of the
    stream and nothing else of any stream."""
    before, pend = run["before"], run["pending"]
    want = before["track"].copy()
    want[b, TR["force"]], want[b, TR["force_kf"]], want[b, TR["since"]] = 1, kf, 0
    assert np.array_equal(pend["track"], want), (pend["track"], want)
    for f in C.FIELDS:
        if f not in ("track", "clock"):
            assert pend[f].tobytes() == before[f].tobytes(), f


def _stats(state, b=0):
    return {n: int(state["stats"][i, b]) for i, n in enumerate(STATS)}


def _frame(sc, b, k, blank=False):
    return FS.frame(sc["W"], sc["fr_blank"] if blank else sc["fr"], b, k)


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("k,captured", [(3, False), (6, False), (6, True), (8, False)])
def test_forced_step_equals_the_lost_chain(k, captured):
    sc = _scene()
    cands = _cands(k)
    assert len(cands) >= 2, "one candidate: the row edit would be an emptied row"
    m = FS.edited(sc["m1"], cands)
    run = _run(k, m, lambda fe: fe.force_relocalisation([0], [cands[-1]]), captured=captured)
    _assert_request_wrote(run, cands[-1])
    before, after = run["before"], run["after"]
    ch = FS.chain_step(m, sc["db"], sc["voc"], FS.lost(before), 0, _frame(sc, 0, k))
    oc, _, _ = GS.candidates(ch, before["reloc"][0], sc["db"], m["graph"], sc["voc"])
    assert oc.tolist() == cands, "the premise: the chain's candidates on the edited graph"
    assert run["cands"][0].tolist() == cands
    FS.compare(after, ch, 0, f"forced step {k}: ", reloc=before["reloc"][0], flags=FS.FORCED)
    tr = after["track"][0]
    st = _stats(after)
    print(f"step {k}: list {run['cands'][0].tolist()}, flags {st['flags']:#x}, nGood {st['reloc']}, ransac {st['ransac']}")
    assert (tr[TR["force"]], tr[TR["force_kf"]], tr[TR["since"]], tr[TR["state"]], tr[TR["path"]]) == (0, 0, 0, 0, 3)
    assert st["flags"] & FS.FORCED and st["flags"] & 32768 and st["ncand"] == len(cands)
    # the next step tracks on: TrackPreviousFrame, since SINCE < 2
    ch2 = FS.chain_step(m, sc["db"], sc["voc"], after, 0, _frame(sc, 0, k + 1))
    FS.compare(run["after2"], ch2, 0, f"step {k + 1}: ")
    assert int(run["after2"]["track"][0][TR["path"]]) == 2 and not _stats(run["after2"])["flags"] & FS.FORCED
    _assert_control(run, k)


# ---------------------------------------------------------------- 2. the natural list
def test_the_window_around_the_last_keyframe():
    sc = _scene()
    g = sc["m1"]["graph"]
    want = FS.forced_list(g["kf_cov_off"], g["kf_cov"], 23)
    assert len(want) == 10 and g["kf_cov_off"][24] - g["kf_cov_off"][23] == 11
    run = _run(4, sc["m1"], lambda fe: fe.force_relocalisation(0, 23))
    _assert_request_wrote(run, 23)
    assert run["cands"][0].tolist() == want and len(run["cands"][1]) == 0
    st, tr = _stats(run["after"]), run["after"]["track"][0]
    assert st["flags"] & 4096 and st["flags"] & 32768 and st["flags"] & FS.FORCED, hex(st["flags"])
    assert st["ncand"] == 10 and (tr[TR["state"]], tr[TR["force"]], tr[TR["force_kf"]], tr[TR["since"]]) == (0, 0, 0, 0)
    assert run["after"]["reloc"][0].tobytes() == run["before"]["reloc"][0].tobytes()
    _assert_control(run, 4)


# ---------------------------------------------------------------- 3. failure
def test_a_failed_forced_relocalisation_leaves_a_lost_stream():
    sc = _scene()
    m = sc["m1"]
    run = _run(4, m, lambda fe: fe.force_relocalisation([0], [0]))
    _assert_request_wrote(run, 0)
    before, after = run["before"], run["after"]
    assert run["cands"][0].tolist() == [0]
    ch = FS.chain_step(m, None, sc["voc"], FS.lost(before), 0, _frame(sc, 0, 4))
    FS.compare(after, ch, 0, "failed forced step: ", reloc=before["reloc"][0], flags=FS.FORCED, stats=dict(ncand=1))
    tr = after["track"][0]
    assert (tr[TR["state"]], tr[TR["vel"]], tr[TR["force"]], tr[TR["force_kf"]]) == (1, 0, 0, 0)
    assert not _stats(after)["flags"] & 32768
    # from the next frame on the database is asked again
    ch2 = FS.chain_step(m, sc["db"], sc["voc"], after, 0, _frame(sc, 0, 5))
    FS.compare(run["after2"], ch2, 0, "the step after the failure: ")
    st = _stats(run["after2"])
    assert st["flags"] & 4096 and not st["flags"] & FS.FORCED and st["ncand"] >= 1
    assert run["after2"]["reloc"][0].tobytes() != before["reloc"][0].tobytes(), "the database was not asked"
    _assert_control(run, 4)


# ---------------------------------------------------------------- 4. forced while LOST
def test_forced_while_lost():
    sc = _scene()
    assert _cands(4, blank=True) == [23]
    m = dict(mp=sc["m1"]["mp"], desc=sc["m1"]["desc"], graph=FS.with_row(sc["m1"]["graph"], 23, []))
    run = _run(4, m, lambda fe: fe.force_relocalisation([0], [23]), blank=True)
    before, after = run["before"], run["after"]
    assert int(before["track"][0][TR["state"]]) == 1, "stream 0 is not LOST before the request"
    _assert_request_wrote(run, 23)
    ch = FS.chain_step(m, sc["db"], sc["voc"], FS.lost(before), 0, _frame(sc, 0, 4, True))
    oc, _, _ = GS.candidates(ch, before["reloc"][0], sc["db"], m["graph"], sc["voc"])
    assert oc.tolist() == [23] and run["cands"][0].tolist() == [23]
    FS.compare(after, ch, 0, "forced while LOST: ", reloc=before["reloc"][0], flags=FS.FORCED)
    assert _stats(after)["flags"] & 32768 and int(after["track"][0][TR["state"]]) == 0
    _assert_control(run, 4, blank=True)


# ---------------------------------------------------------------- 5. a moved map
def _similarity():
    a, b = np.deg2rad(4.0), np.deg2rad(-3.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return 1.05, Rz @ Ry, np.array([0.3, -0.2, 0.15])


def test_loop_corrected_on_a_moved_map():
    """Every position and pose of stream 0's LoopMap goes through one
    similarity, normals and depths are updated as correct_loop updates them,
    and ``KeyFrameInserter.loop_corrected`` carries the map to the front end
    and forces the relocalisation: the step equals the chain on the moved
    map."""
    import test_track_loss_gpu as TL
    from gf_orb_slam_amd import tracking
    from gf_orb_slam_amd.localmapping import LocalMapper

    sc = _scene()
    k = 6
    gm = GS.keyframe_last(sc["gm"], GS.MOVED_KF)
    K = len(gm["kf_kps"])
    gm["kf_Tcw"] = np.asarray(sc["gm"]["kf_Tcw"])[[i for i in range(K) if i != GS.MOVED_KF] + [GS.MOVED_KF]]
    lm = tracking.loopmap_from_global_map(TL.INFO, gm)
    m = dict(mp=gm["mp"], desc=gm["desc"], graph=tracking.covis_graph_from_loopmap(lm))
    fe = _frontend(sc, m)
    fb = tracking.MapFeedback(fe, 0, lm)
    ins = tracking.KeyFrameInserter(fe, {0: LocalMapper(lm, sc["dvoc"])}, feedback={0: fb})
    for _ in range(1, k):
        fe.step()
    before = C.read_state(fe)
    # the correction
    s, R, t = _similarity()
    pos = np.asarray(lm.mps["pos"], np.float64)
    lm.mps["pos"] = (s * pos @ R.T + t).astype(np.float32)
    T = np.asarray(lm.Tcw, np.float64).reshape(-1, 4, 4)
    for i in range(len(T)):
        Rc = T[i, :3, :3] @ R.T
        T[i, :3, 3] = s * T[i, :3, 3] - Rc @ t
        T[i, :3, :3] = Rc
    lm.Tcw[:] = T.astype(np.float32).reshape(np.asarray(lm.Tcw).shape)
    lm.update_normal_and_depth_batch(np.nonzero(~np.asarray(lm.mp_bad).astype(bool))[0])
    # the candidates the chain finds on the moved map, and the row edit that makes them the forced list
    moved = dict(mp=np.asarray(lm.mps).copy(), desc=gm["desc"], graph=m["graph"])
    assert np.abs(moved["mp"]["pos"] - gm["mp"]["pos"]).max() > 0.1
    lost = FS.lost(before)
    lost["map"][0][:len(moved["mp"])] = moved["mp"]
    ch0 = FS.chain_step(moved, sc["db"], sc["voc"], lost, 0, _frame(sc, 0, k))
    c0, _, _ = GS.candidates(ch0, before["reloc"][0], sc["db"], moved["graph"], sc["voc"])
    c0 = [int(c) for c in c0]
    assert len(c0) >= 1, "the chain finds no candidate on the moved map"
    lm.ordered[c0[-1]] = list(c0[:-1])
    sent = ins.loop_corrected(0, last_kf=c0[-1])
    assert sent == c0[-1]
    pend = C.read_state(fe)
    n = len(moved["mp"])
    assert pend["map"][0][:n].tobytes() == moved["mp"].tobytes(), "the moved map did not reach the front end"
    want = FS.with_row(m["graph"], c0[-1], c0[:-1])
    got = fe.covis(0)
    assert np.array_equal(got["kf_cov"], want["kf_cov"]) and np.array_equal(got["kf_cov_off"], want["kf_cov_off"])
    tr = pend["track"][0]
    assert (tr[TR["force"]], tr[TR["force_kf"]], tr[TR["since"]]) == (1, c0[-1], 0)
    fe.step()
    after = C.read_state(fe)
    cands = fe.reloc_candidates()[0].tolist()
    fe.close()
    moved_e = dict(mp=moved["mp"], desc=moved["desc"], graph=want)
    ch = FS.chain_step(moved_e, sc["db"], sc["voc"], FS.lost(pend), 0, _frame(sc, 0, k))
    oc, _, _ = GS.candidates(ch, pend["reloc"][0], sc["db"], want, sc["voc"])
    assert oc.tolist() == c0, "the premise: the row edit changes the chain's candidates on the moved map"
    assert cands == c0
    FS.compare(after, ch, 0, "forced step on the moved map: ", reloc=pend["reloc"][0], flags=FS.FORCED)
    st = _stats(after)
    print(f"moved map: list {cands}, flags {st['flags']:#x}, nGood {st['reloc']}")
    ref = _control(k)[0]
    for f in C.FIELDS:
        if f != "clock":
            a, o = (after[f][:, 1], ref[f][:, 1]) if f == "stats" else (after[f][1], ref[f][1])
            assert a.tobytes() == o.tobytes(), f"stream 1 {f} differs"


# ---------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing():
    sc = _scene()
    fe = _frontend(sc, sc["m1"])
    fe.step()
    before = C.read_state(fe, ["track", "reloc"])
    bad = {"stream below range": ([-1], [0]), "stream above range": ([2], [0]), "named twice": ([0, 0], [1, 2]),
           "named twice beside a valid one": ([1, 0, 1], [0, 0, 0]), "last_kf above the graph": ([0], [24]),
           "last_kf below -1": ([0], [-2]), "a valid stream beside a bad keyframe": ([1, 0], [0, 24])}
    for name, (ss, kf) in bad.items():
        with pytest.raises(GFError) as e:
            fe.force_relocalisation(ss, kf)
        assert e.value.code == -1, (name, str(e.value))
        now = C.read_state(fe, ["track", "reloc"])
        assert all(now[f].tobytes() == before[f].tobytes() for f in now), name
    fe.force_relocalisation([], [])  # nothing named: nothing launched
    assert fe.read("track").tobytes() == before["track"].tobytes()
    fe.close()
    # no keyframe graph, no vocabulary, no database
    fe = FrontEnd("euroc", 1000, 2, GS.G, GS.BUDGET)
    fe.set_map(0, sc["m1"]["mp"], sc["m1"]["desc"])
    fe.set_covis(0, sc["m1"]["graph"])
    fe.set_map(1, sc["gm1"]["mp"], sc["gm1"]["desc"])
    before = fe.read("track")
    steps = (("no vocabulary", [0], None), ("no keyframe graph", [1], lambda: fe.set_vocab(sc["dvoc"])),
             ("no database", [0], None), ("no database on this stream", [0], lambda: fe.set_kfdb(1, None)))
    for name, ss, prepare in steps:
        if prepare is not None:
            prepare()
        with pytest.raises(GFError) as e:
            fe.force_relocalisation(ss)
        assert e.value.code == -1, (name, str(e.value))
        assert fe.read("track").tobytes() == before.tobytes(), name
    fe.close()


# ---------------------------------------------------------------- 8. compaction between request and step
def test_compaction_pins_and_renumbers_the_pending_keyframe():
    sc = _scene()
    k = 6
    cands = _cands(k)
    assert len(cands) >= 2 and 0 not in cands
    m = FS.edited(sc["m1"], cands)
    run = _run(k, m, lambda fe: fe.force_relocalisation([0], [cands[-1]]), growable=True,
               between=lambda fe: fe.compact_maps(MapCompact(0, [0, cands[-1]], []))[0])
    rm = run["between"]
    assert rm.kf_remap[0] == -1 and rm.n_kept_kf == 1 and rm.nkf == 23, "keyframe 0 left, the pending keyframe stayed"
    want = [int(rm.kf_remap[c]) for c in cands]
    assert want == [c - 1 for c in cands]
    tr = run["pending2"]["track"][0]
    assert (tr[TR["force"]], tr[TR["force_kf"]]) == (1, want[-1])
    assert run["pending2"]["track"][1].tobytes() == run["pending"]["track"][1].tobytes()
    assert run["cands"][0].tolist() == want
    st, tr = _stats(run["after"]), run["after"]["track"][0]
    assert st["flags"] & FS.FORCED and st["ncand"] == 2 and (tr[TR["force"]], tr[TR["force_kf"]]) == (0, 0)
    _assert_control(run, k)


# ---------------------------------------------------------------- 9. a parked stream
def test_a_parked_stream_keeps_the_request_and_a_start_clears_it():
    import streamstart_scenes as SS

    sc = _scene()
    fe = _frontend(sc, sc["m1"], growable=True)
    fe.step()
    fe.step()
    tr = fe.read("track")
    tr[0, TR["state"]] = 2  # parked
    fe.write("track", tr)
    fe.force_relocalisation([0], [23])
    before = C.read_state(fe)
    assert tuple(before["track"][0][[TR["state"], TR["force"], TR["force_kf"], TR["since"]]]) == (2, 1, 23, 0)
    fe.step()
    after = C.read_state(fe)
    tr = after["track"][0]
    assert (tr[TR["state"]], tr[TR["path"]], tr[TR["force"]], tr[TR["force_kf"]]) == (2, 4, 1, 23), tr
    assert len(fe.reloc_candidates()[0]) == 0 and not _stats(after)["flags"] & FS.FORCED
    for f in C.Chain.STATE:  # the carried state of a parked stream stays byte-identical (t_cur is a step output)
        if f not in ("track", "t_cur"):
            assert after[f][0].tobytes() == before[f][0].tobytes(), f
    small = SS.graph_map(700, 20, 2, slots=(3, 9))
    rows = SS.db_rows(small, sc["dvoc"].transform, 3)[0]
    fe.start_streams([SS.request(0, small, 12, 5, rows=rows)])
    tr = fe.read("track")[0]
    assert (tr[TR["state"]], tr[TR["force"]], tr[TR["force_kf"]]) == (0, 0, 0), tr
    fe.close()
