"""Micro-benchmark of UpdateConnections / ProcessNewKeyFrame on one GPU. Prints
one JSON object per part and writes them to profiles/covis/bench.json.

  --part a   the counting and ordering on the KeyFrameCulling bench map
             (scripts/kfcull_bench.py: 100 keyframes of 1000 slots, observation
             rows of 8 on average) through gf_update_connections_dev, for one
             query and for all 100 in one launch (kernel time from the
             library's HIP-event profiler; the median of five rounds of 40
             launches), next to the tests' restatement on one host core and
             LoopMap.update_connections in Python.
  --part b   a whole localmapping.process_new_keyframe on that map for a new
             keyframe of 1000 slots holding points of the map, by its own
             clocks: BoW, association, table build and upload, launch and
             download, apply.
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


def part_a():
    import torch

    import covis_ref as R
    import kfcull_bench as KB
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd._lib import check, lib, ptr
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    m, cur = KB.bench_map()
    t = LM.culling_tables(m)
    tables = (t[0], t[2], t[3], t[4], t[5])
    nkf = m.nkf
    cand = np.asarray(m.ordered[cur], np.int32)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in tables]
    res = {"part": "a", "keyframes": nkf, "slots": KB.NSLOTS, "map_points": len(tables[2]),
           "observations": len(tables[4]), "mean_row": round(len(tables[4]) / len(tables[2]), 2)}
    for label, query in (("1", cand[:1]), ("100", cand)):
        nq = len(query)
        d_q = torch.from_numpy(np.ascontiguousarray(query)).cuda()
        d_out = torch.zeros((3 * nkf + 1) * nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        row = nq * nkf

        def launch():
            check(lib().gf_update_connections_dev(ctx.handle, nkf, len(tables[1]), ptr(d[0]), ptr(d[1]), len(tables[2]),
                                                  ptr(d[2]), ptr(d[3]), ptr(d[4]), len(tables[4]), nq, ptr(d_q),
                                                  ptr(d_out), ptr(d_out[3 * row:]), ptr(d_out[row:]),
                                                  ptr(d_out[2 * row:]), ctx.stream))

        launch()
        ctx.sync()
        out = d_out.cpu().numpy()
        want = R.counts(*tables, query)
        got = (out[:row].reshape(nq, nkf), out[3 * row:], out[row:2 * row].reshape(nq, nkf),
               out[2 * row:3 * row].reshape(nq, nkf))
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "the device and the restatement disagree"
        t0 = time.perf_counter()
        for _ in range(5):
            R.counts(*tables, query)
        cpu = (time.perf_counter() - t0) / 5
        walk = copy.deepcopy(m)
        t0 = time.perf_counter()
        for k in query:
            walk.update_connections(int(k))
        py = time.perf_counter() - t0
        rounds = []
        for _ in range(5):
            p = KB.prof(ctx, launch, 40)["k_update_connections"]
            rounds.append(round(1e3 * p[0] / p[1], 2))
        res.update({f"q{label}_k_update_connections_us": rounds,
                    f"q{label}_k_update_connections_us_median": KB.med(rounds),
                    f"q{label}_restatement_us_1core": round(cpu * 1e6, 1),
                    f"q{label}_python_update_connections_us": round(py * 1e6, 1),
                    f"q{label}_listed_total": int(want[1].sum()), f"q{label}_weight_total": int(want[0].sum())})
    return res


def part_b():
    import kfcull_bench as KB
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd import synth
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.matcher import FrameInfo
    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE, default_context

    ctx = default_context()
    base, _ = KB.bench_map()
    rng = np.random.default_rng(2)
    info = FrameInfo.make(*synth.CAMERAS["euroc"], nlevels=8, scale_factor=1.2)
    n = len(base.mps)
    base.mps["pos"] = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)], 1)
    voc = ORBVocabulary(synth.synth_vocabulary(7, k=10, L=3), ctx=ctx)
    kps = np.zeros(KB.NSLOTS, KEYPOINT_DTYPE)
    kps["octave"] = rng.integers(0, 8, KB.NSLOTS)
    desc = rng.integers(0, 256, (KB.NSLOTS, 32), dtype=np.uint8)
    slots = rng.choice(n, KB.NSLOTS, replace=False).astype(np.int32)
    slots[rng.random(KB.NSLOTS) < 0.2] = -1
    runs = []
    for _ in range(4):  # the first is the warm-up
        m = copy.deepcopy(base)
        m.info = info
        cur = m.add_keyframe(kps, desc, slots, np.eye(4, dtype=np.float32))
        t0 = time.perf_counter()
        rep = LM.process_new_keyframe(m, cur, voc, [], levelsup=2, ctx=ctx)
        runs.append(dict(rep["times"], total=time.perf_counter() - t0))
    keys = ("bow", "association", "tables", "launch", "apply", "total")
    ms = lambda k: [round(1e3 * r[k], 2) for r in runs[1:]]  # noqa: E731
    return {"part": "b", "keyframes": m.nkf, "slots": KB.NSLOTS, "associated": len(rep["associated"]),
            "n_ordered": rep["n_ordered"], **{k + "_ms": ms(k) for k in keys},
            **{k + "_ms_median": KB.med(ms(k)) for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "all"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis", "bench.json"))
    a = ap.parse_args()
    lines = [json.dumps(fn()) for p, fn in (("a", part_a), ("b", part_b)) if a.part in (p, "all")]
    for line in lines:
        print(line)
    if a.part == "all":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
