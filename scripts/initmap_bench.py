"""Micro-benchmark of CreateInitialMap on one GPU. Prints one JSON object per
part and writes them to profiles/initmap/bench.json.

  --part a   the two stages alone: k_initmap_points and k_initmap_finish on a
             batch of 1 and of 256 two-view problems (synth_two_view seeds 1,
             2, 3, 5 through the oracle's initialiser, 252-268 points each;
             stage 2 fed the oracle's BA output). Kernel time from the
             library's HIP-event profiler: the median of five rounds of 40
             launches.
  --part b   256 initial maps through both stages and the plan
             (tracking.create_initial_maps_device), host clock per map, next
             to the tests' restatement plus the oracle's BundleAdjustment on
             one host core and to single calls (batches of one).
  --part c   one whole tracking.create_initial_map on the host clock, with
             its laps.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
SEEDS = (1, 2, 3, 5)


def scenes():
    import initmap_scenes as S

    return [S.two_view(s) for s in SEEDS]


def batch_of(scs, P):
    import initmap_scenes as S

    return S.device_batch([scs[p % len(scs)] for p in range(P)])


def part_a():
    import ctypes

    import torch

    import initmap_ref as R
    import initmap_scenes as S
    import kfcull_bench as KB
    from gf_orb_slam_amd import tracking as TR
    from gf_orb_slam_amd._lib import check, lib
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    scs = scenes()
    refs = [R.create(S.INFO, *S.args(sc)) for sc in scs]
    res = {"part": "a", "points": [a["npts"] for a, _ in refs], "keypoints": len(scs[0]["kps1"])}
    for P in (1, 256):
        tens = batch_of(scs, P)
        arg, out = TR.initial_map_points_device(S.INFO, *tens, ctx=ctx)
        pts = TR.InitMapPoints(*[out[k].data_ptr() for k in TR._PT_FIELDS])
        keep = [[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in
                 (b["ba_Tcw"].reshape(2, 16), b["ba_pos"], np.array([b["ba_iterations"], -1], np.int32))]
                for _, b in refs]
        tabs = torch.tensor([[keep[p % len(keep)][k].data_ptr() for p in range(P)] for k in range(3)],
                            dtype=torch.int64, device="cuda")
        rep, mps = TR.initial_map_finish_device(S.INFO, arg, out, tabs[0], tabs[1], tabs[2], ctx=ctx)
        torch.cuda.synchronize()
        r = rep.cpu().numpy().view(TR.REPORT_DTYPE).reshape(-1)
        assert all(int(r[p]["status"]) == refs[p % len(refs)][1]["status"] for p in range(P))

        def launch():
            check(lib().gf_initial_map_points_dev(ctx.handle, ctypes.byref(S.INFO), P, ctypes.byref(arg),
                                                  ctypes.byref(pts), ctx.stream))
            check(lib().gf_initial_map_finish_dev(ctx.handle, ctypes.byref(S.INFO), P, ctypes.byref(arg),
                                                  ctypes.byref(pts), tabs[0].data_ptr(), tabs[1].data_ptr(),
                                                  tabs[2].data_ptr(), 100, rep.data_ptr(), mps.data_ptr(), ctx.stream))

        rounds = {"k_initmap_points": [], "k_initmap_finish": []}
        for _ in range(5):
            p = KB.prof(ctx, launch, 40)
            for k in rounds:
                rounds[k].append(round(1e3 * p[k][0] / p[k][1], 2))
        for k, v in rounds.items():
            res[f"P{P}_{k}_us"] = v
            res[f"P{P}_{k}_us_median"] = KB.med(v)
    return res


def part_b():
    import torch

    import initmap_ref as R
    import initmap_scenes as S
    import kfcull_bench as KB
    from gf_orb_slam_amd import tracking as TR

    scs = scenes()
    P = 256
    tens = batch_of(scs, P)
    runs = []
    for _ in range(4):  # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = TR.create_initial_maps_device(S.INFO, *tens)
        runs.append(dict(out["times"], total=time.perf_counter() - t0, steps=out["ba_steps"]))
    ones = [batch_of([sc], 1) for sc in scs]
    single = []
    for i in range(1 + 16):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        TR.create_initial_maps_device(S.INFO, *ones[i % len(ones)])
        single.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for sc in scs:
        R.create(S.INFO, *S.args(sc))
    cpu = (time.perf_counter() - t0) / len(scs)
    keys = ("points", "plan", "solve", "finish", "total")
    us = lambda k: [round(1e6 * r[k] / P, 1) for r in runs[1:]]  # noqa: E731
    return {"part": "b", "maps": P, "ba_steps": runs[-1]["steps"], **{k + "_us_per_map": us(k) for k in keys},
            **{k + "_us_per_map_median": KB.med(us(k)) for k in keys},
            "single_call_us_per_map_median": round(1e6 * KB.med(single[1:]), 1),
            "restatement_plus_oracle_ba_us_per_map_1core": round(1e6 * cpu, 1)}


def part_c():
    import initmap_scenes as S
    import kfcull_bench as KB
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd import tracking as TR
    from gf_orb_slam_amd.bow import ORBVocabulary

    voc = ORBVocabulary(synth.synth_vocabulary(7, k=10, L=3))
    sc = S.two_view(1)
    runs = []
    for _ in range(4):  # the first is the warm-up
        t0 = time.perf_counter()
        m, rep = TR.create_initial_map(S.INFO, sc["K"], *S.args(sc), voc=voc, levelsup=2)
        runs.append(dict(rep["times"], total=time.perf_counter() - t0))
    keys = tuple(runs[0])
    ms = lambda k: [round(1e3 * r[k], 2) for r in runs[1:]]  # noqa: E731
    return {"part": "c", "points": rep["npts"], "ba_iterations": rep["ba_iterations"],
            **{k + "_ms": ms(k) for k in keys}, **{k + "_ms_median": KB.med(ms(k)) for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c", "all"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initmap", "bench.json"))
    a = ap.parse_args()
    lines = [json.dumps(fn()) for p, fn in (("a", part_a), ("b", part_b), ("c", part_c)) if a.part in (p, "all")]
    for line in lines:
        print(line)
    if a.part == "all":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
