"""Micro-benchmark of KeyFrameCulling on one GPU. Prints one JSON object per
part.

  --part a   the one-launch count: one current keyframe with 100 candidates of
             1000 slots, observation rows of 8 on average, through
             gf_keyframe_culling_counts_dev (kernel time from the library's
             HIP-event profiler; the median of five rounds of 40 launches,
             alternating without and with the flags plane), and the tests'
             restatement of the count on one host core.
  --part b   a whole localmapping.keyframe_culling on that map, by its own
             clocks: table build and upload, launches, the host walk
             (set_bad_keyframe) and the refreshes after a cull; once as
             generated and once with five candidates made redundant (all
             their keypoints at the top level), which are culled.
"""
import argparse
import copy
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCAND, NSLOTS, ROW = 100, 1000, 8


def bench_map(seed=1, redundant=()):
    """NCAND candidate keyframes of NSLOTS keypoints and a current keyframe
    that lists them all; every point is observed by a Poisson(ROW) number of
    distinct candidates (at least one), octaves uniform in 0..7."""
    from gf_orb_slam_amd.loopmap import LoopMap
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    rng = np.random.default_rng(seed)
    fill = np.zeros(NCAND, np.int64)
    slots = np.full((NCAND, NSLOTS), -1, np.int32)
    obs = []
    while fill.min() < int(0.8 * NSLOTS):
        free = np.nonzero(fill < NSLOTS)[0]
        k = min(max(int(rng.poisson(ROW)), 1), len(free))
        kfs = np.sort(rng.choice(free, k, replace=False))
        p = len(obs)
        obs.append({int(kf): int(fill[kf]) for kf in kfs})
        slots[kfs, fill[kfs]] = p
        fill[kfs] += 1
    kps = []
    for kf in range(NCAND + 1):
        kp = np.zeros(NSLOTS if kf < NCAND else 0, KEYPOINT_DTYPE)
        kp["octave"] = 7 if kf in redundant else rng.integers(0, 8, len(kp))
        kps.append(kp)
    nmp = len(obs)
    m = LoopMap(None, kps, [np.zeros((len(k), 32), np.uint8) for k in kps], list(slots) + [np.zeros(0, np.int32)],
                np.zeros(nmp, MAP_POINT_DTYPE), np.zeros((nmp, 32), np.uint8), observations=obs,
                kf_id=np.arange(1, NCAND + 2))
    cur = NCAND
    for kf in range(NCAND):
        m.add_connection(cur, kf, 2 * NCAND - kf)
        m.add_connection(kf, cur, 2 * NCAND - kf)
        m.parent[kf] = kf - 1 if kf else cur
    return m, cur


def prof(ctx, fn, reps):
    from gf_orb_slam_amd._lib import check, lib

    check(lib().gf_prof_enable(ctx.handle, 1))
    check(lib().gf_prof_reset(ctx.handle))
    for _ in range(reps):
        fn()
    check(lib().gf_ctx_sync(ctx.handle))
    out, i = {}, 0
    name, ms, cnt = ctypes.create_string_buffer(64), ctypes.c_double(), ctypes.c_int()
    while lib().gf_prof_report(ctx.handle, i, name, 64, ctypes.byref(ms), ctypes.byref(cnt)) == 0:
        out[name.value.decode()] = (ms.value, cnt.value)
        i += 1
    check(lib().gf_prof_enable(ctx.handle, 0))
    return out


med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731


def part_a():
    import torch

    import kfcull_ref as R
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd._lib import check, lib, ptr
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    m, cur = bench_map()
    tables = LM.culling_tables(m)[:6]
    cand = np.asarray(m.ordered[cur], np.int32)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in tables + (cand,)]
    d_counts = torch.zeros(len(cand) * 2, dtype=torch.int32, device="cuda")
    d_flags = torch.zeros(len(tables[2]), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def launch(flags):
        check(lib().gf_keyframe_culling_counts_dev(ctx.handle, len(tables[0]) - 1, len(tables[2]), ptr(d[0]), ptr(d[1]),
                                                   ptr(d[2]), len(tables[3]), ptr(d[3]), ptr(d[4]), ptr(d[5]),
                                                   len(tables[5]), len(cand), ptr(d[6]), ptr(d_counts),
                                                   ptr(d_flags) if flags else None, ctx.stream))

    launch(True)
    ctx.sync()
    want = R.counts(*tables, cand)
    assert np.array_equal(d_counts.cpu().numpy().reshape(-1, 2), want), "the device and the restatement disagree"
    t0 = time.perf_counter()
    for _ in range(5):
        R.counts(*tables, cand)
    cpu = (time.perf_counter() - t0) / 5
    rounds = {False: [], True: []}
    for _ in range(5):  # alternating
        for flags in (False, True):
            p = prof(ctx, lambda: launch(flags), 40)["k_kfcull_count"]
            rounds[flags].append(round(1e3 * p[0] / p[1], 2))
    return {"part": "a", "candidates": len(cand), "slots": NSLOTS, "map_points": len(tables[3]),
            "observations": len(tables[5]), "mean_row": round(len(tables[5]) / len(tables[3]), 2),
            "nmps_total": int(want[:, 0].sum()), "nredundant_total": int(want[:, 1].sum()),
            "k_kfcull_count_us": rounds[False], "k_kfcull_count_flags_us": rounds[True],
            "k_kfcull_count_us_median": med(rounds[False]), "k_kfcull_count_flags_us_median": med(rounds[True]),
            "restatement_us_1core": round(cpu * 1e6, 1)}


def part_b():
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    out = []
    for redundant in ((), (10, 30, 50, 70, 90)):
        base, cur = bench_map(redundant=redundant)
        runs = []
        for _ in range(4):  # the first is the warm-up
            m = copy.deepcopy(base)
            t0 = time.perf_counter()
            rep = LM.keyframe_culling(m, cur, ctx=ctx)
            runs.append(dict(rep["times"], total=time.perf_counter() - t0))
        ms = lambda k: [round(1e3 * r[k], 2) for r in runs[1:]]  # noqa: E731
        out.append({"part": "b", "planted_redundant": len(redundant), "candidates": len(rep["candidates"]),
                    "culled": len(rep["culled"]), "points_bad": len(rep["points_bad"]), "launches": rep["launches"],
                    "upload_ms": ms("upload"), "launch_ms": ms("launch"), "walk_ms": ms("walk"),
                    "refresh_ms": ms("refresh"), "total_ms": ms("total"),
                    **{k + "_ms_median": med(ms(k)) for k in ("upload", "launch", "walk", "refresh", "total")}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], required=True)
    a = ap.parse_args()
    for res in ([part_a()] if a.part == "a" else part_b()):
        print(json.dumps(res))


if __name__ == "__main__":
    main()
