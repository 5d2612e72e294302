"""Measurement of the relocalisation database that grows ("Map
feedback") -> one JSON object:

  (a) one FrontEnd.update_maps call that appends a 1000-keypoint keyframe (its
      graph row and its database rows) to streams whose databases hold 8, 32
      and 63 keyframes, for 1, 8 and 256 streams of a 256-stream front end in
      one call: kernel time of the append (k_kg_scan, k_kg_merge, k_kg_finish)
      as the median of five rounds from the kernels' own dispatch timestamps
      (the library's profiler, gf_prof_*), in rounds of their own; and on the
      host clock the time of the call itself (it enqueues and returns) and of
      the call to completion (the call, then one synchronisation);
  (b) the only way before the entry existed: detach the database, send the
      same delta without rows, rebuild the whole database on the host with
      gf_kfdb_create and attach it with gf_frontend_set_kfdb, per stream; host
      clock to completion, alternated with (a) call by call in the same process.

A database at its size takes one append, so every call starts from streams
reset to that size (set_covis and a fresh database per stream, untimed). A
round is 40 calls for 1 and 8 streams and 2 calls for 256 streams, where the
reset of 256 databases is what takes the time.

python scripts/kfdb_bench.py [--out profiles/kfdb/bench.json]
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

NKP, NWORDS, VOCAB, NODES, NMP = 1000, 900, 100000, 100, 64
CALLS = {1: 40, 8: 40, 256: 2}
KERNELS = ["k_kg_scan", "k_kg_merge", "k_kg_finish"]


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=[round(x, 4) for x in v])


def clone(db):
    """The same host arrays behind a device database of its own."""
    c = copy.copy(db)
    c._dev = {}
    if c.growable:
        c.reserve()  # host arrays of its own at the capacities
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kfdb_ref as R
    import mapupdate_scenes as S
    from gf_orb_slam_amd.localmap import MapDelta
    from gf_orb_slam_amd.pipeline import FrontEnd

    B = args.batch
    rng = np.random.default_rng(1)
    kfs = [R.keyframe(rng, NKP, np.sort(rng.choice(VOCAB, NWORDS, replace=False)), nodes_per=NODES) for _ in range(64)]
    fe = FrontEnd("euroc", 1000, B, NMP, 100)
    res = dict(shape=dict(batch=B, keypoints=NKP, words=NWORDS, vocabulary=VOCAB, fv_nodes=NODES, calls_per_round=CALLS,
                          rounds=args.rounds),
               a_update_maps_kfdb={}, b_rebuild_and_set_kfdb={}, ratio_b_over_a_host_complete={})
    mp, desc = S.points(rng, NMP)
    slots = np.full(NKP, -1, np.int32)
    for N in (8, 32, 63):
        graph = S.graph_of([slots] * N, np.zeros(N), [np.zeros(0, np.int32)] * N, np.zeros(NMP), [np.zeros(0, np.int32)] * NMP)
        base, grown, rows = R.db_of(kfs[:N]), R.db_of(kfs[:N + 1]), R.db_of(kfs[N:N + 1])
        base_g = R.db_of(kfs[:N], max_kf=64, max_rows=(N + 1) * NKP)

        def reset(n, growable):
            for b in range(n):
                fe.set_covis(b, graph)  # detaches the stream's database
                fe.set_kfdb(b, clone(base_g if growable else base))
            fe.sync()

        def run_a(n):
            ds = [MapDelta(b, new_kf=[slots], kf_rows=rows) for b in range(n)]
            fe.sync()
            t0 = time.perf_counter()
            fe.update_maps(ds)
            t1 = time.perf_counter()
            fe.sync()
            return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3

        def run_b(n):
            ds = [MapDelta(b, new_kf=[slots]) for b in range(n)]
            fe.sync()
            t0 = time.perf_counter()
            for b in range(n):
                fe.set_kfdb(b, None)
            fe.update_maps(ds)
            for b in range(n):
                fe.set_kfdb(b, clone(grown))
            fe.sync()
            return (time.perf_counter() - t0) * 1e3

        for b in range(B):
            fe.set_map(b, mp, desc)
        for n in sorted({1, min(8, B), B}):
            calls = CALLS.get(n, 2)
            reset(n, True)
            run_a(n)  # the first call of a size allocates the staging
            total, call, old, kern, per = [], [], [], [], {k: [] for k in KERNELS}
            for _ in range(args.rounds):
                ta, tc, tb = [], [], []
                for _ in range(calls):
                    reset(n, True)
                    a = run_a(n)
                    ta.append(a[0])
                    tc.append(a[1])
                    reset(n, False)
                    tb.append(run_b(n))
                total.append(statistics.median(ta))
                call.append(statistics.median(tc))
                old.append(statistics.median(tb))
            for _ in range(args.rounds):  # kernel times in rounds of their own
                fe.prof_reset()
                for _ in range(calls):
                    reset(n, True)  # creating a database appends too: the profiler is on around the call only
                    fe.prof_enable(True)
                    run_a(n)
                    fe.prof_enable(False)
                rep = fe.prof_report()
                kern.append(sum(rep[k][0] for k in KERNELS if k in rep) / calls * 1e3)
                for k in KERNELS:
                    per[k].append(rep[k][0] / max(rep[k][1], 1) * 1e3 if k in rep else 0.0)
            key = f"{N}kf_{n}streams"
            res["a_update_maps_kfdb"][key] = dict(kernels_us=spread(kern), per_kernel_us={k: spread(v) for k, v in per.items()},
                                                  host_call_ms=spread(call), host_complete_ms=spread(total))
            res["b_rebuild_and_set_kfdb"][key] = dict(host_ms=spread(old))
            res["ratio_b_over_a_host_complete"][key] = statistics.median(old) / statistics.median(total)
            print(key, "kernels", round(statistics.median(kern), 2), "us; call to completion",
                  round(statistics.median(total), 3), "ms; rebuild", round(statistics.median(old), 3), "ms", flush=True)
    fe.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
