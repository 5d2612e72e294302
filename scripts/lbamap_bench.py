"""Micro-benchmark of LocalBundleAdjustment on a LoopMap on one GPU. Prints one
JSON object per part.

  --part a   the graph assembly: the KeyFrameCulling bench map
             (scripts/kfcull_bench.py: 100 keyframes of 1000 slots, rows of 8 on
             average), the current keyframe with its first 31 covisibles as the
             local list, through gf_lba_graph_dev (the six kernels' span from
             the library's HIP-event profiler; the median of five rounds of 40
             calls), and the tests' restatement of the assembly on one host
             core.
  --part b   a whole localmapping.local_bundle_adjustment by its own clocks:
             tables (build and upload), assembly, download, solve, write-back
             and update, on the tests' parity scene grown to about 1200 points.
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

NLOCAL = 32
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731


def part_a():
    import kfcull_bench as KB
    import lbamap_ref as R
    import lbamap_scenes as S
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    m, cur = KB.bench_map()
    m.info = S.info()
    keep = m.ordered[cur][:NLOCAL - 1]
    m.weights[cur] = {k: m.weights[cur][k] for k in keep}
    m.update_best_covisibles(cur)
    local = LM.lba_local_keyframes(m, cur)
    t = LM._LBATables(m, ctx)
    t.launch(local)
    g = t.download()
    w = R.RefWorld.from_loopmap(m)
    want = w.graph(cur, m.ordered[cur])
    for name in R.PROBLEM:
        assert np.asarray(g[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    cov = np.asarray(m.ordered[cur], np.int32)
    t0 = time.perf_counter()
    for _ in range(5):
        R.lib().lr_graph(w.h, int(cur), len(cov), ctypes.c_void_p(cov.ctypes.data))
    cpu = (time.perf_counter() - t0) / 5
    rounds = []
    for _ in range(5):
        p = KB.prof(ctx, lambda: t.launch(local), 40)["k_lba_graph"]
        rounds.append(round(1e3 * p[0] / p[1], 2))
    return {"part": "a", "local_keyframes": len(local), "slots": KB.NSLOTS, "map_points": len(m.mps),
            "observations": len(t.t["obs_gkp"]), "problem_keyframes": g["nkf"], "problem_points": g["npts"],
            "problem_edges": g["nedges"], "k_lba_graph_us": rounds, "k_lba_graph_us_median": med(rounds),
            "restatement_us_1core": round(cpu * 1e6, 1)}


def part_b():
    import lbamap_scenes as S
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    sc = S.parity(per_start=150)
    base = S.parity_map(sc)
    runs = []
    for _ in range(4):  # the first is the warm-up
        m = copy.deepcopy(base)
        t0 = time.perf_counter()
        rep = LM.local_bundle_adjustment(m, sc["cur"], ctx=ctx)
        runs.append(dict(rep["times"], total=time.perf_counter() - t0))
    keys = ("tables", "assembly", "download", "solve", "writeback", "update", "total")
    ms = lambda k: [round(1e3 * r[k], 2) for r in runs[1:]]  # noqa: E731
    return {"part": "b", "local_keyframes": len(rep["local_kfs"]), "fixed_keyframes": len(rep["fixed_kfs"]),
            "points": rep["npts"], "edges": rep["nedges"], "iterations": list(rep["iterations"]),
            "erased": rep["erased"], "points_bad": len(rep["points_bad"]), **{k + "_ms": ms(k) for k in keys},
            **{k + "_ms_median": med(ms(k)) for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], required=True)
    a = ap.parse_args()
    print(json.dumps(part_a() if a.part == "a" else part_b()))


if __name__ == "__main__":
    main()
