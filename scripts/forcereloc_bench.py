"""Measurement of gf_frontend_force_relocalisation ("Forced
relocalisation") -> one JSON object:

  (a) one FrontEnd.force_relocalisation call for 1, 8 and 256 streams of a
      256-stream front end whose streams hold a keyframe graph and a
      database: kernel time per call as the median of five rounds of 40
      calls from the kernel's own dispatch timestamps (the library's profiler,
      gf_prof_*), in rounds of their own; and on the host clock the call to
      completion (a synchronisation after it);
  (b) on the B = 2 front end of the tests' scene (2600 points, 24 keyframes):
      one step with stream 0 forced (the window around keyframe 23: ten
      candidates) against one plain step of the same front end, alternated,
      host clock to completion, median of five rounds.

Nobody's numbers yet: reported, not gated on.

python scripts/forcereloc_bench.py [--out profiles/forcereloc/bench.json]
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

NKF, NMP, NKP, CALLS = 8, 250, 200, 40


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=[round(x, 4) for x in v])


def request_cost(B, rounds):
    import mapupdate_scenes as S
    import streamstart_scenes as SS
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.pipeline import TR, FrontEnd

    dvoc = ORBVocabulary(synth.synth_vocabulary_fast(11, k=10, L=5))
    m = S.random_map(1, NMP, NKF, slots=(NKP, NKP), obs_most=2)
    rows = SS.db_rows(m, dvoc.transform, 2)[0]
    fe = FrontEnd("euroc", 1000, B, 2000, 100)
    fe.set_vocab(dvoc)
    for b in range(B):
        fe.set_map(b, m["mp"], m["desc"])
        fe.set_covis(b, m["graph"])
        fe.set_kfdb(b, rows)
    out = {}
    streams = np.arange(B, dtype=np.int32)
    kfs = (streams % NKF).astype(np.int32)
    for n in sorted({1, min(8, B), B}):
        fe.force_relocalisation(streams[:n], kfs[:n])  # the first call allocates the staging
        fe.sync()
        total, kern = [], []
        for _ in range(rounds):
            fe.sync()
            t0 = time.perf_counter()
            fe.force_relocalisation(streams[:n], kfs[:n])
            fe.sync()
            total.append((time.perf_counter() - t0) * 1e3)
        for _ in range(rounds):  # kernel times in rounds of their own
            fe.sync()
            fe.prof_enable(True)
            fe.prof_reset()
            for _ in range(CALLS):
                fe.force_relocalisation(streams[:n], kfs[:n])
            fe.sync()
            rep = fe.prof_report()
            fe.prof_enable(False)
            kern.append(rep["k_force_reloc"][0] * 1e3 / CALLS)
        out[str(n)] = dict(kernel_us_per_call=spread(kern), host_complete_ms=spread(total))
    tr = fe.read("track")
    assert np.all(tr[:, TR["force"]] == 1) and np.array_equal(tr[:, TR["force_kf"]], kfs)
    fe.close()
    return dict(shape=dict(batch=B, keyframes=NKF, calls_per_kernel_round=CALLS), calls=out)


def step_cost(rounds):
    import kfdb_grow_scenes as GS
    import oracle_lib as O
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.pipeline import FrontEnd

    voc = GS.vocabulary()
    W = GS.workload()
    frames = W.render_all("cuda").contiguous()
    gmaps = W.build_global_maps(lambda im: O.extract(im), GS.G)
    dvoc = ORBVocabulary(voc)
    _, m1, rows = GS.maps_of(W, gmaps, dvoc.transform)
    gm1 = gmaps[W.scene_of[1]]
    rows1 = [(k, d) + tuple(dvoc.transform(d)) for k, d in zip(gm1["kf_kps"], gm1["kf_desc"])]
    fe = FrontEnd("euroc", 1000, 2, GS.G, GS.BUDGET)
    fe.set_vocab(dvoc)
    fe.set_map(0, m1["mp"], m1["desc"])
    fe.set_covis(0, m1["graph"])
    fe.set_kfdb(0, GS.database(rows))
    fe.set_map(1, gm1["mp"], gm1["desc"])
    fe.set_covis(1, gm1["graph"])
    fe.set_kfdb(1, GS.database(rows1))
    for b in range(2):
        fe.set_rng(b, 7 + b)
    fe.set_source(frames, W.scene_of, W.phase)
    T, V = W.boot_state()
    fe.bootstrap(T, V, 0.0)
    for _ in range(3):
        fe.step()

    def step():
        fe.sync()
        t0 = time.perf_counter()
        fe.step()
        fe.sync()
        return (time.perf_counter() - t0) * 1e3

    plain, forced, flags = [], [], []
    for _ in range(rounds):
        plain.append(step())
        fe.force_relocalisation([0], [23])
        forced.append(step())
        flags.append(int(fe.stats()["flags"][0]))
        fe.step()  # TrackPreviousFrame after the relocalisation: not the plain step measured
        fe.step()
    fe.close()
    assert all(f & 65536 for f in flags)
    return dict(plain_step_ms=spread(plain), forced_step_ms=spread(forced), forced_flags=[hex(f) for f in flags],
                candidates=10, relocalised=[bool(f & 32768) for f in flags])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(a_force_relocalisation=request_cost(args.batch, args.rounds), b_forced_step=step_cost(args.rounds))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
