"""Micro-benchmark of the resident map tables on one GPU. Prints one JSON object
per line and writes them to profiles/maptables/bench.json.

  --part a   kernel times on the KeyFrameCulling bench map (scripts/
             kfcull_bench.py: 101 keyframes, observation rows of 8 on average)
             from the library's HIP-event profiler, the median of five rounds
             of 40 launches: gf_map_tables_apply_dev for the journal of one
             ProcessNewKeyFrame (one OBS_SET per associated point, distinct
             rows) and for the journal of one SearchInNeighbors on the
             neighbours bench (scripts/neighbors_bench.py), and
             gf_map_tables_move_dev of the whole table; next to each the tests'
             restatement on one host core. The observation table is restored
             before every apply launch (a copy on torch's stream, not timed),
             so that every launch inserts.
  --part b   whole stages by their own clocks, attached and unattached in the
             same run (the median of three runs after a warm-up):
             process_new_keyframe, keyframe_culling with nothing and with five
             keyframes culled, local_bundle_adjustment on the ten-keyframe map
             of scripts/lbamap_bench.py; the cost of attaching; and a run of
             ten keyframes through the table-touching stages on the bench map
             (process_new_keyframe, map_point_culling, 100 new points per
             keyframe with two observations each in CreateNewMapPoints' place,
             keyframe_culling; the bench map has no geometry, so the search and
             the adjustment are left out) with the regrows, the flushes and
             the slack (capacity / live entries) it ends with.
  --part c   ten keyframes through the whole LocalMapper.step on the
             neighbours bench scene (a map of 14 keyframes, ten more inserted
             one by one), unattached and attached after a warm-up of both: the
             stages' host-clock seconds summed over the ten steps, the regrows,
             flushes, launches and slack; the two maps end equal.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]


def _new_keyframe(n_points, rng):
    import kfcull_bench as KB
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    kps = np.zeros(KB.NSLOTS, KEYPOINT_DTYPE)
    kps["octave"] = rng.integers(0, 8, KB.NSLOTS)
    desc = rng.integers(0, 256, (KB.NSLOTS, 32), dtype=np.uint8)
    slots = rng.choice(n_points, KB.NSLOTS, replace=False).astype(np.int32)
    slots[rng.random(KB.NSLOTS) < 0.2] = -1
    return kps, desc, slots, np.eye(4, dtype=np.float32)


def _geometry(m, rng):
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.matcher import FrameInfo

    n = len(m.mps)
    m.info = FrameInfo.make(*synth.CAMERAS["euroc"], nlevels=8, scale_factor=1.2)
    m.mps["pos"] = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)], 1)


def _time_apply(ctx, t, label):
    """Kernel time of the pending journal of ``t`` (not flushed) and the
    restatement's time on host copies."""
    import torch

    import kfcull_bench as KB
    import maptables_ref as R
    from gf_orb_slam_amd._lib import check, lib, ptr

    t._append_new()
    slot_g, slot_v, bad_p, row_ids, row_op_off, ops, counts = t.journal_arrays()
    parts = [slot_g, slot_v, bad_p, row_ids, row_op_off, ops.reshape(-1)]
    at = np.concatenate([[0], np.cumsum([len(a) for a in parts])])
    d = torch.from_numpy(np.concatenate(parts).astype(np.int32)).cuda()
    p = [ptr(d[int(o):]) for o in at[:-1]]
    d_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    # room for the journal: the regrow a flush would run first
    final = np.fromiter((len(t.map.obs[q]) for q in row_ids), np.int32, len(row_ids))
    regrown = bool(np.any(final > t.h_obs_off[row_ids + 1] - t.h_obs_off[row_ids]))
    if regrown:
        need = t.live.copy()
        need[row_ids] = np.maximum(t.live[row_ids], final)
        t._regrow(t._offsets(t._cap(need)))
    b, n = t.b, t.sizes()
    keep = {k: b[k].view().clone() for k in ("slots", "mp_bad", "obs_gkp")}

    def launch():
        for k, v in keep.items():
            b[k].view().copy_(v)
        torch.cuda.current_stream().synchronize()
        check(lib().gf_map_tables_apply_dev(ctx.handle, n["nkf"], n["nkp"], ptr(b["kf_off"].a), ptr(b["slots"].a),
                                            n["nmp"], ptr(b["mp_bad"].a), ptr(b["obs_off"].a), ptr(b["obs_gkp"].a),
                                            n["nobs"], len(slot_g), p[0], p[1], len(bad_p), p[2], len(row_ids), p[3],
                                            p[4], len(ops), p[5], ptr(d_status), ctx.stream))
        ctx.sync()

    host = t.download()
    launch()
    assert d_status.cpu().numpy()[:2].tolist() == [0, 0]
    want = {k: host[k].copy() for k in host}
    st = R.apply(want["kf_off"], want["slots"], want["mp_bad"], want["obs_off"], want["obs_gkp"], slot_g, slot_v, bad_p,
                 row_ids, row_op_off, ops)
    got = t.download()
    assert st.tolist() == [0, 0] and all(got[k].tobytes() == want[k].tobytes() for k in want), \
        "the device and the restatement disagree"
    cpu = []
    for _ in range(5):
        w = {k: host[k].copy() for k in host}
        t0 = time.perf_counter()
        R.apply(w["kf_off"], w["slots"], w["mp_bad"], w["obs_off"], w["obs_gkp"], slot_g, slot_v, bad_p, row_ids,
                row_op_off, ops)
        cpu.append(time.perf_counter() - t0)
    rounds = []
    for _ in range(5):
        pr = KB.prof(ctx, launch, 40)["k_tables_apply"]
        rounds.append(round(1e3 * pr[0] / pr[1], 2))
    for k, v in keep.items():  # as before the journal, which stays pending
        b[k].view().copy_(v)
    torch.cuda.current_stream().synchronize()
    kinds = np.bincount(ops[:, 0], minlength=3) if len(ops) else np.zeros(3, int)
    return {f"{label}_rows": len(row_ids), f"{label}_ops_set_erase_clear": kinds.tolist(),
            f"{label}_max_ops_per_row": int(counts.max()) if len(counts) else 0, f"{label}_slot_writes": len(slot_g),
            f"{label}_bad_flags": len(bad_p), f"{label}_regrown_first": regrown, f"{label}_k_tables_apply_us": rounds,
            f"{label}_k_tables_apply_us_median": KB.med(rounds),
            f"{label}_restatement_us_1core": round(KB.med(cpu) * 1e6, 1)}


def part_a():
    import torch

    import kfcull_bench as KB
    import maptables_ref as R
    import neighbors_scenes as NS
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd._lib import check, lib, ptr
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    rng = np.random.default_rng(2)
    m, _ = KB.bench_map()
    t = m.attach_tables(ctx=ctx)
    n = t.sizes()
    res = {"part": "a", "keyframes": m.nkf, "map_points": n["nmp"], "observations": int(t.live.sum()),
           "capacity": n["nobs"], "slack": round(t.slack(), 3)}
    # the journal of one ProcessNewKeyFrame: the association of :177-192
    cur = m.add_keyframe(*_new_keyframe(len(m.mps), rng))
    for i, p in enumerate(m.slots[cur]):
        if p >= 0 and not m.mp_bad[p]:
            m.add_observation(int(p), cur, i)
    res.update(_time_apply(ctx, t, "pnk"))
    # the whole table moved to the capacities the policy gives it now
    t.flush()
    new_off = t._offsets(t._cap(t.live))
    d_off = torch.from_numpy(new_off).cuda()
    d_new = torch.empty(int(new_off[-1]), dtype=torch.int32, device="cuda")
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b = t.b

    def move():
        check(lib().gf_map_tables_move_dev(ctx.handle, t.nmp, ptr(b["obs_off"].a), ptr(b["obs_gkp"].a), b["obs_gkp"].n,
                                           ptr(d_off), ptr(d_new), len(d_new), ptr(d_status), ctx.stream))

    move()
    ctx.sync()
    host = t.download()
    want = np.empty(int(new_off[-1]), np.int32)
    assert R.move(host["obs_off"], host["obs_gkp"], new_off, want).tolist() == [0] == d_status.cpu().numpy().tolist()
    assert d_new.cpu().numpy().tobytes() == want.tobytes(), "the device and the restatement disagree"
    cpu = []
    for _ in range(5):
        t0 = time.perf_counter()
        R.move(host["obs_off"], host["obs_gkp"], new_off, want)
        cpu.append(time.perf_counter() - t0)
    rounds = []
    for _ in range(5):
        pr = KB.prof(ctx, move, 40)["k_tables_move"]
        rounds.append(round(1e3 * pr[0] / pr[1], 2))
    res.update(move_rows=t.nmp, move_entries_old=b["obs_gkp"].n, move_entries_new=int(new_off[-1]),
               k_tables_move_us=rounds, k_tables_move_us_median=KB.med(rounds),
               move_restatement_us_1core=round(KB.med(cpu) * 1e6, 1))
    # the journal of one SearchInNeighbors on the neighbours bench
    sc = NS.neighbors_scene(7, n_world=1150, n_good=22)
    m2 = NS.loop_map(sc)
    t2 = m2.attach_tables(ctx=ctx)
    LM.search_in_neighbors(m2, sc["cur"], ctx=ctx)
    res.update(sin_keyframes=m2.nkf, sin_map_points=len(m2.mps), **_time_apply(ctx, t2, "sin"))
    return res


def _runs(make, stage, keys, attach):
    """Four runs (the first is the warm-up) of ``stage(map)`` on fresh maps ->
    the median laps in ms, the attach time apart."""
    import kfcull_bench as KB

    runs, attach_ms, rep = [], [], None
    for _ in range(4):
        m = make()
        if attach:
            t0 = time.perf_counter()
            m.attach_tables()
            attach_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rep = stage(m)
        runs.append(dict(rep["times"], total=time.perf_counter() - t0))
    out = {k + "_ms": [round(1e3 * r[k], 3) for r in runs[1:]] for k in keys + ("total",)}
    out.update({k + "_ms_median": KB.med(out[k + "_ms"]) for k in keys + ("total",)})
    if attach:
        out["attach_ms_median"] = round(KB.med(attach_ms[1:]), 2)
    return out, rep


def part_b():
    import kfcull_bench as KB
    import lbamap_scenes
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    voc = ORBVocabulary(synth.synth_vocabulary(7, k=10, L=3), ctx=ctx)
    out = []
    # process_new_keyframe
    base, _ = KB.bench_map()
    _geometry(base, np.random.default_rng(2))
    kf = _new_keyframe(len(base.mps), np.random.default_rng(3))

    def pnk(m):
        cur = m.add_keyframe(*kf)
        return LM.process_new_keyframe(m, cur, voc, [], levelsup=2, ctx=ctx)

    keys = ("bow", "association", "tables", "launch", "apply")
    for attach in (False, True):
        laps, rep = _runs(lambda: copy.deepcopy(base), pnk, keys, attach)
        out.append({"part": "b", "stage": "process_new_keyframe", "attached": attach, "keyframes": base.nkf + 1,
                    "associated": len(rep["associated"]), **laps})
    # keyframe_culling, nothing culled and five culled
    keys = ("upload", "launch", "walk", "refresh")
    for redundant in ((), (10, 30, 50, 70, 90)):
        base, cur = KB.bench_map(redundant=redundant)
        for attach in (False, True):
            laps, rep = _runs(lambda: copy.deepcopy(base), lambda m: LM.keyframe_culling(m, cur, ctx=ctx), keys, attach)
            out.append({"part": "b", "stage": "keyframe_culling", "attached": attach, "culled": len(rep["culled"]),
                        "points_bad": len(rep["points_bad"]), "launches": rep["launches"], **laps})
    # local_bundle_adjustment on the ten-keyframe map
    sc = lbamap_scenes.parity(per_start=150)
    base = lbamap_scenes.parity_map(sc)
    keys = ("tables", "assembly", "download", "solve", "writeback", "update")
    for attach in (False, True):
        laps, rep = _runs(lambda: copy.deepcopy(base), lambda m: LM.local_bundle_adjustment(m, sc["cur"], ctx=ctx), keys,
                          attach)
        out.append({"part": "b", "stage": "local_bundle_adjustment", "attached": attach, "keyframes": base.nkf,
                    "edges": rep["nedges"], "iterations": list(rep["iterations"]), **laps})
    # ten keyframes through the table-touching stages
    rng = np.random.default_rng(5)
    for attach in (False, True):
        m, _ = KB.bench_map()
        _geometry(m, np.random.default_rng(2))
        t = m.attach_tables() if attach else None
        recent, secs = [], dict(process_new_keyframe=0.0, map_point_culling=0.0, new_points=0.0, keyframe_culling=0.0)
        rng = np.random.default_rng(5)
        culled = 0
        for _ in range(10):
            cur = m.add_keyframe(*_new_keyframe(len(m.mps), rng))
            t0 = time.perf_counter()
            LM.process_new_keyframe(m, cur, voc, recent, levelsup=2, ctx=ctx)
            t1 = time.perf_counter()
            recent = LM.map_point_culling(m, recent, cur)
            t2 = time.perf_counter()
            free = np.nonzero(m.slots[cur] < 0)[0][:100]
            for i1 in free:  # the bookkeeping of CreateNewMapPoints (:393-406) for made-up points
                k2 = int(rng.integers(0, KB.NCAND))  # one of the generated keyframes, which have NSLOTS keypoints
                i2 = int(rng.integers(0, KB.NSLOTS))
                p = m.new_map_point(rng.uniform(-1, 1, 3) + (0, 0, 6), cur)
                m.add_observation(p, k2, i2), m.add_observation(p, cur, int(i1))
                m.add_map_point(cur, p, int(i1)), m.add_map_point(k2, p, i2)
                recent.append(p)
            t3 = time.perf_counter()
            culled += len(LM.keyframe_culling(m, cur, ctx=ctx)["culled"])
            t4 = time.perf_counter()
            for k, v in zip(secs, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                secs[k] += v
        row = {"part": "b", "stage": "ten_keyframes", "attached": attach, "keyframes": m.nkf, "map_points": len(m.mps),
               "culled": culled, **{k + "_ms_total": round(1e3 * v, 2) for k, v in secs.items()}}
        if attach:
            t.flush()
            t.check()
            row.update(regrows=t.regrows, flushes=t.flushes, rebuilds=t.rebuilds, launches=t.launches,
                       slack=round(t.slack(), 3), capacity=t.sizes()["nobs"], live=int(t.live.sum()))
        out.append(row)
    return out


def _step_map(first):
    """The neighbours bench scene as tracking leaves it before keyframe
    ``first``: a LoopMap of the keyframes below it, the later ones' observations
    taken out of the maps, the graph built by UpdateConnections in index order,
    and the later keyframes as ``add_keyframe`` tuples."""
    import neighbors_scenes as NS
    from gf_orb_slam_amd.loopmap import LoopMap

    sc = NS.neighbors_scene(7, n_world=1150, n_good=22)
    obs = [{k: i for k, i in o.items() if k < first} for o in sc["observations"]]
    ref = np.asarray([r if r < first else (min(o) if o else -1) for r, o in zip(sc["ref_kf"], obs)], np.int32)
    m = LoopMap(sc["info"], sc["kf_kps"][:first], sc["kf_desc"][:first], sc["kf_mp"][:first], sc["mps"], sc["mp_desc"],
                mp_bad=sc["mp_bad"], observations=obs, kf_Tcw=sc["kf_Tcw"][:first], ref_kf=ref, kf_id=sc["kf_id"][:first])
    for k in range(m.nkf):
        m.update_connections(k)
    new = [(sc["kf_kps"][k], sc["kf_desc"][k], sc["kf_mp"][k], sc["kf_Tcw"][k], int(sc["kf_id"][k]))
           for k in range(first, len(sc["kf_kps"]))]
    return m, new


def part_c():
    """Ten keyframes through the whole LocalMapper.step on the neighbours bench
    scene (24 keyframes of about 1160 keypoints: a map of 14, ten inserted one
    by one), unattached and attached: seconds per stage summed over the ten
    steps, and with tables the regrows, flushes, launches and slack."""
    import covis_ref
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    voc = ORBVocabulary(synth.synth_vocabulary(7, k=10, L=3), ctx=ctx)
    out, maps = [], []
    for attach in (False, True, False, True):  # the first pair is the warm-up
        m, new = _step_map(14)
        for k in range(m.nkf):
            words, values, fv = voc.transform(m.kf_desc[k], 2)
            m.kf_bow[k], m.kf_fv[k] = (words, values), fv
        t0 = time.perf_counter()
        mapper = LM.LocalMapper(m, voc, ctx=ctx, levelsup=2, resident=attach)
        attach_ms = 1e3 * (time.perf_counter() - t0)
        secs = {name: 0.0 for name in LM.LocalMapper.STAGES}
        culled = 0
        for kf in new:
            rep = mapper.step(mapper.insert_keyframe(*kf))
            for name in rep["order"]:
                secs[name] += rep[name]["seconds"]
            culled += len(rep["keyframe_culling"]["report"]["culled"])
        row = {"part": "c", "stage": "ten_local_mapper_steps", "attached": attach, "keyframes": m.nkf,
               "map_points": len(m.mps), "observations": int(sum(len(o) for o in m.obs)), "culled": culled,
               **{name + "_ms_total": round(1e3 * v, 2) for name, v in secs.items()},
               "total_ms": round(1e3 * sum(secs.values()), 2)}
        if attach:
            t = m.tables
            t.flush()
            t.check()
            row.update(attach_ms=round(attach_ms, 2), regrows=t.regrows, flushes=t.flushes, rebuilds=t.rebuilds,
                       launches=t.launches, slack=round(t.slack(), 3), capacity=t.sizes()["nobs"],
                       live=int(t.live.sum()))
        maps.append(m)
        out.append(row)
    covis_ref.assert_same_maps(maps[2], maps[3])
    return out[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c", "all"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maptables", "bench.json"))
    a = ap.parse_args()
    lines = []
    for part, fn in (("a", lambda: [part_a()]), ("b", part_b), ("c", part_c)):
        if a.part in (part, "all"):
            for r in fn():
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    if a.part == "all":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
