"""The scene the forced-relocalisation tests share (test_forcereloc_cpu.py pins
it with the oracle chain alone, test_forcereloc_gpu.py runs it on the device):
the scene of kfdb_grow_scenes.py (Workload "euroc", B = 2, two scenes, seed 4,
phase offset 12, the map m1 of 2600 points and 24 keyframes with keyframe 11
moved last, the database of all 24 keyframes), with no blank frames unless a
test asks for them. Stream 0 is the one acted on, stream 1 the control.

The oracle chain cannot be told a candidate list, but the forced list is a
function of an input the tests own: when C is what
DetectRelocalisationCandidates returns for a frame, and the covisibility row of
C[-1] is given the entries C[:-1], a relocalisation forced with last_kf = C[-1]
has the candidate list C. The forced step must then equal a chain loaded with
the state before the step and GF_TR_STATE = 1, GF_TR_SINCE = 0, in everything
but the keyframes' query state (the forced path leaves it) and flag 65536."""
from __future__ import annotations

import numpy as np

import kfdb_grow_scenes as GS
import mapupdate_scenes as S
import oracle_chain as C
import oracle_lib as O
from gf_orb_slam_amd.pipeline import STATS, TR

# step k -> the candidates of the LOST-at-k chain (test_forcereloc_cpu.py pins them)
CANDS = {3: [6, 15], 6: [23, 6], 8: [12, 9]}
FORCED = 65536


def forced_list(cov_off, cov, kf: int) -> list:
    """Relocalisation's candidates under mbForceRelocalisation (Tracking.cc:
    3866-3879): GetBestCovisibilityKeyFrames(9) of the keyframe, in the row's
    order, then the keyframe."""
    row = np.asarray(cov[cov_off[kf]:cov_off[kf + 1]], np.int32)
    return [int(c) for c in row[:9]] + [int(kf)]


def with_row(graph: dict, kf: int, entries) -> dict:
    """The graph with the covisibility row of ``kf`` replaced by ``entries``."""
    cov = S.rows_of(graph["kf_cov_off"], graph["kf_cov"])
    cov[kf] = np.asarray(entries, np.int32)
    return S.graph_of(S.rows_of(graph["kf_mp_off"], graph["kf_mp"]), graph["kf_bad"], cov, graph["mp_bad"],
                      S.rows_of(graph["mp_obs_off"], graph["mp_obs"]))


def edited(m: dict, cands) -> dict:
    """Map ``m`` whose row of cands[-1] is cands[:-1]: forcing with cands[-1] gives ``cands``."""
    return dict(mp=m["mp"], desc=m["desc"], graph=with_row(m["graph"], int(cands[-1]), cands[:-1]))


def lost(state: dict, b: int = 0) -> dict:
    """The state with stream b LOST and just relocalised-from (STATE 1, SINCE
    0) and no request pending: what a chain that stands for a forced step is
    loaded with."""
    st = {k: np.array(v, copy=True) for k, v in state.items()}
    st["track"][b, TR["state"]] = 1
    st["track"][b, TR["since"]] = 0
    st["track"][b, TR["force"]] = 0
    st["track"][b, TR["force_kf"]] = 0
    return st


def chain_step(m, db, voc, state, b, img):
    """A chain over map ``m`` loaded with stream b of ``state``, one step on ``img``."""
    ch = GS.chain(m, db, voc)
    ch.load_from(state, b)
    ch.write("reloc", state["reloc"][b])
    ch.step(img)
    return ch


EXACT = ["kps", "desc", "nkp", "kp2mp", "score", "outlier", "last_kps", "last_desc", "last_nkp", "last_kp2mp",
         "last_outlier", "last_pos", "views", "mp_upd", "rng", "t_prev", "t_cur", "track"]


def compare(dev, ch, b, prefix, reloc=None, flags=0, stats=None):
    """Every carried field and statistic of stream b against the chain (the
    bounds of test_track_loss_gpu._compare). ``reloc``: what the keyframes'
    query state must be (default: the chain's); ``flags``: bits the device
    sets beyond the chain's; ``stats``: {name: value} of statistics that differ
    by rule."""
    n = int(ch.read("nkp"))
    for k in EXACT:
        a, o = dev[k][b], ch.read(k)
        if k in ("kps", "desc"):  # a frame with fewer keypoints leaves the device buffer's tail as it was
            a, o = a[:n], o[:n]
        assert np.array_equal(a, o), f"{prefix}{k} differs (stream {b}): {a if a.size < 10 else ''} {o if o.size < 10 else ''}"
    want = ch.read("reloc") if reloc is None else reloc
    assert dev["reloc"][b].tobytes() == np.asarray(want).tobytes(), f"{prefix}reloc differs (stream {b})"
    nl = int(ch.stats()["nleft"])
    assert np.array_equal(dev["left"][b][:nl], ch.read("left")[:nl]), f"{prefix}leftovers differ (stream {b})"
    for k in ("Tcw", "velocity", "Tcw_last"):
        a, o = dev[k][b].astype(np.float64), ch.read(k).astype(np.float64)
        assert np.all(np.abs(a - o) <= 1e-5 * np.maximum(1, np.abs(o))), f"{prefix}{k} differs (stream {b})"
    for k in ("Xv", "Xv_next", "base", "mp_H", "mp_info", "mp_uv"):
        np.testing.assert_allclose(dev[k][b], ch.read(k), rtol=1e-9, atol=1e-12, err_msg=f"{prefix}{k} (stream {b})")
    sd, so = dev["stats"][:, b].copy(), ch.read("stats").copy()
    so[STATS.index("flags")] |= flags
    for name, v in (stats or {}).items():
        so[STATS.index(name)] = v
    assert np.array_equal(sd, so), f"{prefix}stage counters differ (stream {b}): " + str(
        {STATS[i]: (int(sd[i]), int(so[i])) for i in range(len(STATS)) if sd[i] != so[i]})


def bow_matches(rows, graph, kf: int, desc, kps, voc) -> int:
    """SearchByBoW(keyframe kf, frame) match count (ORBmatcher(0.75, true))."""
    _, _, fv = O.bow_transform(voc, desc, 4)
    r = rows[kf]
    slots = S.rows_of(graph["kf_mp_off"], graph["kf_mp"])[kf]
    return O.match_bow(0, 0.75, True, ((r[4].nodes, r[4].start, r[4].feats), r[1], r[0], slots),
                       (fv, desc, kps, np.full(len(desc), -1, np.int32)))[0]


_CPU = {}


def cpu_scene() -> dict:
    """The scene on the CPU with the chain's states after steps 0 .. 9 of
    stream 0 (tracking every frame on the full map and database)."""
    if _CPU:
        return _CPU
    voc = GS.vocabulary()
    W = GS.workload()
    fr = W.render_all("cpu").numpy()
    gmaps = W.build_global_maps(lambda im: O.extract(im), GS.G, device="cpu")
    _, m1, rows = GS.maps_of(W, gmaps, GS.oracle_transform(voc))
    db = GS.database(rows)
    T, V = W.boot_state()
    ch = GS.chain(m1, db, voc)
    ch.set_rng(7)
    ch.bootstrap(fr[W.scene_of[0], W.phase[0] % W.period], T[0], V[0])
    states = [GS.chain_state(ch)]
    for k in range(1, 10):
        ch.step(frame(W, fr, 0, k))
        states.append(GS.chain_state(ch))
    _CPU.update(voc=voc, W=W, fr=fr, m1=m1, rows=rows, db=db, states=states)
    return _CPU


def frame(W, fr, b, k):
    return fr[W.scene_of[b], (W.phase[b] + k) % W.period]


def lost_at(sc, k, m=None, db="full"):
    """The LOST-at-k chain: the state after step k - 1 with STATE 1 and SINCE
    0, one step on frame k over map ``m`` (default m1) -> (chain, candidates of
    the step or None without a database)."""
    m = m or sc["m1"]
    d = sc["db"] if db == "full" else db
    st = lost(sc["states"][k - 1])
    ch = chain_step(m, d, sc["voc"], st, 0, frame(sc["W"], sc["fr"], 0, k))
    if d is None:
        return ch, None
    cands, _, _ = GS.candidates(ch, st["reloc"][0], d, m["graph"], sc["voc"])
    return ch, [int(c) for c in cands]
