"""Measurement of map compaction ("Map compaction") -> one JSON object:

  (a) one FrontEnd.compact_maps call for 1, 8 and 256 streams of a 256-stream
      front end, every stream holding a 64-keyframe map of about 4000 points
      of which a quarter goes (every fourth keyframe and point): kernel time
      as the median of five rounds from the kernels' own dispatch timestamps
      (the library's profiler, gf_prof_*), in rounds of their own; and on the
      host clock the call to completion (it synchronises itself);
  (b) the only way before the entry: read the per-point fields and the index
      holders, restrict them on the host, set_map + set_covis per stream,
      write the fields back; host clock, alternated with (a) round by round in
      the same process.

A round starts from the same maps (set_map + set_covis, untimed).

python scripts/mapcompact_bench.py [--out profiles/mapcompact/bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NKF, NMP, SLOTS = 64, 4000, 1000
POINT_FIELDS = ("views", "mp_H", "mp_info", "mp_uv", "mp_upd")
INDEX_FIELDS = ("kp2mp", "last_kp2mp", "left")
KERNELS = ["k_mc_mark", "k_mc_scan", "k_mc_move", "k_mc_obs_rows", "k_mc_finish"]


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=[round(x, 4) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mapupdate_scenes as S
    from gf_orb_slam_amd.localmap import MapCompact, MapRemap
    from gf_orb_slam_amd.pipeline import FrontEnd
    from gf_orb_slam_amd.tracking import restrict_graph

    B, M = args.batch, 4096
    start = S.random_map(1, NMP, NKF, slots=(SLOTS, SLOTS), obs_most=6)
    drop_kf, drop_mp = np.arange(0, NKF, 4), np.arange(0, NMP, 4)
    kf_remap, mp_remap = np.full(NKF, -1, np.int32), np.full(NMP, -1, np.int32)
    kf_remap[np.setdiff1d(np.arange(NKF), drop_kf)] = np.arange(NKF - len(drop_kf))
    mp_remap[np.setdiff1d(np.arange(NMP), drop_mp)] = np.arange(NMP - len(drop_mp))
    fe = FrontEnd("euroc", 1000, B, M, 100)
    res = dict(shape=dict(batch=B, nfeatures=1000, map_cap=M, keyframes=NKF, points=NMP, slots_per_keyframe=SLOTS,
                          observations=int(len(start["graph"]["mp_obs"])), dropped_keyframes=len(drop_kf),
                          dropped_points=len(drop_mp)),
               a_compact_maps={}, b_read_restrict_set_write={}, ratio_b_over_a_host_complete={})

    def reset(n):
        for b in range(n):
            fe.set_map(b, start["mp"], start["desc"])
            fe.set_covis(b, start["graph"])
        fe.sync()

    def run_a(n):
        fe.sync()
        t0 = time.perf_counter()
        rm = fe.compact_maps([MapCompact(b, drop_kf, drop_mp) for b in range(n)])
        dt = (time.perf_counter() - t0) * 1e3
        got = {(r.nkf, r.nmp, r.n_kept_kf, r.n_kept_mp) for r in rm}
        assert got == {(NKF - len(drop_kf), NMP - len(drop_mp), 0, 0)}, got
        return dt

    def run_b(n):
        """The way before the entry."""
        keep = mp_remap >= 0
        n1 = int(keep.sum())
        g1 = restrict_graph(start["graph"], kf_remap, mp_remap)
        fe.sync()
        t0 = time.perf_counter()
        st = {k: fe.read(k) for k in POINT_FIELDS + INDEX_FIELDS}
        for b in range(n):
            for k in POINT_FIELDS:
                st[k][b][:n1] = st[k][b][:NMP][keep]
            for k in INDEX_FIELDS:
                st[k][b] = MapRemap.apply(mp_remap, np.where(st[k][b] < NMP, st[k][b], -1))
            fe.set_map(b, start["mp"][keep], start["desc"][keep])
            fe.set_covis(b, g1)
        for k in POINT_FIELDS + INDEX_FIELDS:
            fe.write(k, st[k])
        fe.sync()
        return (time.perf_counter() - t0) * 1e3

    for n in sorted({1, min(8, B), B}):
        reset(n)
        run_a(n)  # the first call allocates the tables
        total, old, kern, per = [], [], [], {k: [] for k in KERNELS}
        for _ in range(args.rounds):
            reset(n)
            total.append(run_a(n))
            reset(n)
            old.append(run_b(n))
        for _ in range(args.rounds):  # kernel times in rounds of their own
            reset(n)
            fe.prof_enable(True)
            fe.prof_reset()
            run_a(n)
            rep = fe.prof_report()
            fe.prof_enable(False)
            kern.append(sum(rep[k][0] for k in KERNELS if k in rep) * 1e3)
            for k in KERNELS:
                per[k].append(rep[k][0] * 1e3 if k in rep else 0.0)
        res["a_compact_maps"][str(n)] = dict(kernels_us=spread(kern), per_kernel_us={k: spread(v) for k, v in per.items()},
                                             host_complete_ms=spread(total))
        res["b_read_restrict_set_write"][str(n)] = dict(host_ms=spread(old))
        res["ratio_b_over_a_host_complete"][str(n)] = statistics.median(old) / statistics.median(total)
    fe.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
