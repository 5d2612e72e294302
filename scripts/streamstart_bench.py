"""Measurement of gf_frontend_start_streams ("Stream start, park
and reset") -> one JSON object:

  (a) one FrontEnd.start_streams call for 1, 8 and 256 streams of a
      256-stream front end, every start shaped like an initial map on the EuRoC
      workload (2 keyframes of 1000 keypoints, about 250 points, a last frame
      of 1000 keypoints, the two keyframes' database rows): kernel time per
      call as the median of five rounds of 40 calls from the kernels' own
      dispatch timestamps (the library's profiler, gf_prof_*), in rounds of
      their own; and on the host clock the call to completion (a
      synchronisation after it);
  (b) the only way before the entry, on an uncaptured front end: synchronise,
      then per stream set_map, set_covis and set_kfdb of a rebuilt database,
      and write of the last-frame, tracking and keyframe fields; host clock,
      alternated with (a) round by round in the same process.

python scripts/streamstart_bench.py [--out profiles/streamstart/bench.json]
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

NKF, NMP, NKP, CALLS = 2, 250, 1000, 40
KERNELS = ["k_ss_install", "k_mu_rows", "k_mu_obs_scan", "k_mu_obs_rows", "k_mu_finish", "k_kg_scan", "k_kg_merge",
           "k_kg_finish"]
WRITTEN = ("last_kps", "last_desc", "last_nkp", "last_kp2mp", "last_outlier", "last_pos", "Tcw_last", "t_prev", "t_cur",
           "track")


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=[round(x, 4) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mapupdate_scenes as S
    import streamstart_ref as R
    import streamstart_scenes as SS
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.pipeline import KF, FrontEnd, KeyframeDB

    B, M = args.batch, 2000
    dvoc = ORBVocabulary(synth.synth_vocabulary_fast(11, k=10, L=5))
    m = S.random_map(1, NMP, NKF, slots=(NKP, NKP), obs_most=2)
    rows, kf_kps, kf_desc = SS.db_rows(m, dvoc.transform, 2)
    bow = [(rows.bow_words[rows.bow_off[k]:rows.bow_off[k + 1]], rows.bow_values[rows.bow_off[k]:rows.bow_off[k + 1]])
           for k in range(NKF)]
    graph = m["graph"]

    def frontend(lifecycle):
        fe = FrontEnd("euroc", 1000, B, M, 100)
        fe.set_vocab(dvoc)
        if lifecycle:
            fe.enable_lifecycle()
            for b in range(B):
                fe.set_kfdb(b, KeyframeDB([], [], dvoc.transform, max_kf=64, max_rows=2 * NKF * NKP))
        else:
            for b in range(B):
                fe.set_map(b, m["mp"], m["desc"])
                fe.set_covis(b, graph)
        fe.enable_keyframes()
        return fe

    fe, old = frontend(True), frontend(False)
    reqs = [SS.request(b, m, NKP, 10 + b, rows=rows) for b in range(B)]
    res = dict(shape=dict(batch=B, nfeatures=1000, map_cap=M, keyframes=NKF, points=NMP, slots_per_keyframe=NKP,
                          last_frame_keypoints=NKP, observations=int(len(graph["mp_obs"])), database_rows=NKF * NKP,
                          calls_per_kernel_round=CALLS),
               a_start_streams={}, b_set_map_covis_kfdb_write={}, ratio_b_over_a_host_complete={})

    def run_a(n):
        fe.sync()
        t0 = time.perf_counter()
        fe.start_streams(reqs[:n])
        fe.sync()
        return (time.perf_counter() - t0) * 1e3

    def run_b(n):
        """The way before the entry (the BowVectors are given, as the rows of (a) are)."""
        old.sync()
        t0 = time.perf_counter()
        for b in range(n):
            old.set_map(b, m["mp"], m["desc"])
            old.set_covis(b, graph)
            old.set_kfdb(b, dbs[b])
        w = {k: old.read(k) for k in WRITTEN}
        for b in range(n):
            r = reqs[b]
            w["last_kps"][b, :NKP], w["last_desc"][b, :NKP], w["last_kp2mp"][b, :NKP] = r.kps, r.desc, r.kp2mp
            w["last_outlier"][b, :NKP] = 0
            w["last_pos"][b, :NKP] = np.where(r.kp2mp[:, None] >= 0, m["mp"]["pos"][np.maximum(r.kp2mp, 0)], 0)
            w["last_nkp"][b], w["Tcw_last"][b], w["t_prev"][b], w["t_cur"][b] = NKP, r.Tcw, r.timestamp, r.timestamp
            w["track"][b, :6] = (0, 0, r.since_reloc, 2, r.frame_id, 1)
        for k, a in w.items():
            old.write(k, a)
        ks = old.keyframe_state()
        for word, v in (("since", 0), ("pending", 0), ("abort", 0), ("decision", 0), ("ref", NKF - 1)):
            ks[word][:n] = v
        old.set_keyframe_state(**{k: ks[k] for k in KF})
        old.sync()
        return (time.perf_counter() - t0) * 1e3

    # a database row needs its FeatureVector too: take it from the rows once
    from gf_orb_slam_amd.bow import FeatureVector

    fvs = []
    for k in range(NKF):
        a, b_ = rows.fv_off[k], rows.fv_off[k + 1]
        st = rows.fv_start[a:b_ + 1] - rows.fv_start[a]
        fvs.append(FeatureVector(rows.fv_nodes[a:b_], st, rows.fv_feats[rows.fv_start[a]:rows.fv_start[b_]]))

    def rebuilt_db():
        it = iter([(bow[k][0], bow[k][1], fvs[k]) for k in range(NKF)])
        return KeyframeDB(kf_kps, kf_desc, lambda d: next(it), max_kf=64, max_rows=2 * NKF * NKP)

    assert R.verdict(reqs[0], fe.cap, M, nstreams=B, db=(64, 2 * NKF * NKP)) == 0
    for n in sorted({1, min(8, B), B}):
        run_a(n)  # the first call allocates the staging
        total, prev, kern, per = [], [], [], {k: [] for k in KERNELS}
        for _ in range(args.rounds):
            total.append(run_a(n))
            t0 = time.perf_counter()
            dbs = [rebuilt_db() for _ in range(n)]  # the rebuilt databases' host arrays, counted with (b)
            build = (time.perf_counter() - t0) * 1e3
            prev.append(run_b(n) + build)
        for _ in range(args.rounds):  # kernel times in rounds of their own
            fe.sync()
            fe.prof_enable(True)
            fe.prof_reset()
            for _ in range(CALLS):
                fe.start_streams(reqs[:n])
            fe.sync()
            rep = fe.prof_report()
            fe.prof_enable(False)
            kern.append(sum(rep[k][0] for k in KERNELS if k in rep) * 1e3 / CALLS)
            for k in KERNELS:
                per[k].append(rep[k][0] * 1e3 / CALLS if k in rep else 0.0)
        res["a_start_streams"][str(n)] = dict(kernels_us_per_call=spread(kern),
                                              per_kernel_us={k: spread(v) for k, v in per.items()},
                                              host_complete_ms=spread(total))
        res["b_set_map_covis_kfdb_write"][str(n)] = dict(host_ms=spread(prev))
        res["ratio_b_over_a_host_complete"][str(n)] = statistics.median(prev) / statistics.median(total)
    fe.close()
    old.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
