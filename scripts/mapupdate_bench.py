"""Measurement of map feedback ("Map feedback") -> one JSON object:

  (a) one FrontEnd.update_maps call for 1, 8 and 256 streams of a 256-stream
      front end, every delta with the shape of one mapper pass on the EuRoC
      workload (one appended 1000-slot keyframe, 59 appended points, about a
      thousand rewritten points, several hundred replaced observation rows, a
      new covisibility table): kernel time as the median of five rounds of 40
      calls from the kernels' own dispatch timestamps (the library's profiler,
      gf_prof_*), in rounds of their own; and on the host clock the time of
      the call itself (it enqueues and returns) and of the call to completion
      (40 calls, then one synchronisation);
  (b) the same change made without the entry: set_map + set_covis per stream
      and the per-point fields the set call resets (GF_FE_MP_UPD, GF_FE_VIEWS)
      read before and written back with gf_frontend_read / _write; host clock,
      alternated with (a) round by round in the same process.

A round starts from the same maps (set_map + set_covis, untimed) and applies
40 successive deltas, which takes the streams from 24 to 64 keyframes.

python scripts/mapupdate_bench.py [--out profiles/mapupdate/bench.json]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CALLS, NKF0, NMP0, NEW_MP, SLOTS = 40, 24, 1700, 59, 1000  # 1700 + 40 x 59 points: inside the 4096 a map holds


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=[round(x, 4) for x in v])


def mapper_passes():
    """The start map of a stream and CALLS successive (delta, map after it)."""
    import mapupdate_scenes as S

    m = S.random_map(1, NMP0, NKF0, slots=(SLOTS, SLOTS), obs_most=6)
    start, out = m, []
    for i in range(CALLS):
        nxt = S.evolve(100 + i, m, new_mp=NEW_MP, new_kf=1, new_kf_slots=(SLOTS, SLOTS), rewrite=1000, bad_mp=20,
                       slot_writes=300, obs="some", cov=True, obs_most=6)  # "some": a tenth of the rows
        out.append((S.diff(0, m, nxt), nxt))
        m = nxt
    return start, out


def for_stream(d, b):
    c = copy.copy(d)
    c.stream = b
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gf_orb_slam_amd.pipeline import FrontEnd

    B = args.batch
    M = NMP0 + CALLS * NEW_MP
    start, passes = mapper_passes()
    fe = FrontEnd("euroc", 1000, B, M, 100)
    res = dict(shape=dict(batch=B, nfeatures=1000, map_cap=M, calls_per_round=CALLS, keyframes=[NKF0, NKF0 + CALLS],
                          delta=dict(new_kf_slots=SLOTS, new_mp=NEW_MP,
                                     set_mp=int(np.median([len(d.set_mp_idx) for d, _ in passes])),
                                     obs_rows=int(np.median([len(d.obs_mp) for d, _ in passes])),
                                     slot_writes=int(np.median([len(d.slot_kf) for d, _ in passes])))),
               a_update_maps={}, b_set_map_set_covis={}, ratio_b_over_a_host_complete={})

    def reset(n):
        for b in range(n):
            fe.set_map(b, start["mp"], start["desc"])
            fe.set_covis(b, start["graph"])
        fe.sync()

    def run_a(n):
        t_call = []
        fe.sync()
        t0 = time.perf_counter()
        for d, _ in passes:
            ds = [for_stream(d, b) for b in range(n)]
            t1 = time.perf_counter()
            fe.update_maps(ds)
            t_call.append(time.perf_counter() - t1)
        fe.sync()
        return (time.perf_counter() - t0) / CALLS * 1e3, statistics.median(t_call) * 1e3

    def run_b(n, reps=2):
        """The parent's way, `reps` of the 40 passes."""
        fe.sync()
        t0 = time.perf_counter()
        for _, m in passes[:reps]:
            upd, views = fe.read("mp_upd"), fe.read("views")
            for b in range(n):
                fe.set_map(b, m["mp"], m["desc"])
                fe.set_covis(b, m["graph"])
            fe.write("mp_upd", upd)
            fe.write("views", views)
        fe.sync()
        return (time.perf_counter() - t0) / reps * 1e3

    kernels = ["k_mu_rows", "k_mu_obs_scan", "k_mu_obs_rows", "k_mu_finish"]
    for n in sorted({1, min(8, B), B}):
        reset(n)
        run_a(n)  # the first call allocates the staging
        total, call, old, kern, per = [], [], [], [], {k: [] for k in kernels}
        for _ in range(args.rounds):
            reset(n)
            a = run_a(n)
            total.append(a[0])
            call.append(a[1])
            reset(n)
            old.append(run_b(n))
        for _ in range(args.rounds):  # kernel times in rounds of their own
            reset(n)
            fe.prof_enable(True)
            fe.prof_reset()
            run_a(n)
            rep = fe.prof_report()
            fe.prof_enable(False)
            kern.append(sum(rep[k][0] for k in kernels if k in rep) / CALLS * 1e3)
            for k in kernels:
                per[k].append(rep[k][0] / max(rep[k][1], 1) * 1e3 if k in rep else 0.0)
        res["a_update_maps"][str(n)] = dict(kernels_us=spread(kern), per_kernel_us={k: spread(v) for k, v in per.items()},
                                            host_call_ms=spread(call), host_complete_ms=spread(total))
        res["b_set_map_set_covis"][str(n)] = dict(host_ms=spread(old))
        res["ratio_b_over_a_host_complete"][str(n)] = statistics.median(old) / statistics.median(total)
    fe.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
