"""Micro-benchmark of SearchForInitialization and Tracking::Initialize on one
GPU. Prints one JSON object per part and writes them to
profiles/searchinit/bench.json.

  --part a   the matcher's kernels on 1 and 256 problems of the EuRoC shape
             (752 x 480, 1000 keypoints a frame, a fifth of them level 0, a
             few tens of level-0 candidates in a 200 x 200 window). The two
             paths alternate in one session: the candidate lists (k_si_grid,
             k_si_cand, k_si_resolve) and GF_SI_DIRECT (the same kernels, every
             query walking its window inside the ordered pass). Kernel time
             from the library's HIP-event profiler: the median of five rounds
             of 40 launches. vbPrevMatched is updated in place, so after the
             warm-up launch every launch sees the matched positions.
  --part b   the tests' restatement on one host core, per problem.
  --part c   one whole MonoInitializer.feed (second frame of two_view(1): the
             matcher, the gate, the initialiser, CreateInitialMap) on the host
             clock, with its laps.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
NSCENES = 16


def euroc(seed, n=1000):
    import searchinit_scenes as S

    rng = np.random.default_rng(8000 + seed)
    xy1 = rng.uniform([5, 5], [S.W - 5, S.H - 5], (n, 2))
    perm = rng.permutation(n)
    xy2 = xy1[perm] + rng.normal(0, 15.0, (n, 2))
    lvl = np.where(rng.random(n) < 0.2, 0, rng.integers(1, 8, n))
    a1 = rng.uniform(0, 360, n)
    d1 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    d2 = np.stack([S.flip(rng, d1[i], rng.integers(0, 30)) for i in perm])
    k1, k2 = S.kparr(xy1, lvl, a1), S.kparr(xy2, lvl[perm], (a1[perm] - 10.0) % 360.0)
    return dict(kps1=k1, desc1=d1, kps2=k2, desc2=d2, prev=S.prev_of(k1))


def device_batch(scs):
    import torch

    from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

    P, c = len(scs), len(scs[0]["kps1"])
    st = lambda k, dt: np.ascontiguousarray(np.stack([np.ascontiguousarray(s[k], dt) for s in scs]))  # noqa: E731
    dev = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    n = torch.full((P,), c, dtype=torch.int32, device="cuda")
    return (dev(st("kps1", KEYPOINT_DTYPE).view(np.uint8).reshape(P, c, 28)), dev(st("desc1", np.uint8)), n,
            dev(st("kps2", KEYPOINT_DTYPE).view(np.uint8).reshape(P, c, 28)), dev(st("desc2", np.uint8)), n.clone(),
            dev(st("prev", np.float32)))


def part_a():
    import torch

    import kfcull_bench as KB
    import searchinit_ref as R
    import searchinit_scenes as S
    from gf_orb_slam_amd._lib import check, lib
    from gf_orb_slam_amd.matcher import GF_SI_DIRECT
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    scs = [euroc(s) for s in range(NSCENES)]
    refs = [R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"]) for s in scs]
    again = [R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], r[2]) for s, r in zip(scs, refs)]
    lvl0 = [int((s["kps1"]["octave"] == 0).sum()) for s in scs]
    k2 = scs[0]["kps2"]
    cands = [int(((k2["octave"] == 0) & (np.abs(k2["x"] - x) <= 100) & (np.abs(k2["y"] - y) <= 100)).sum())
             for x, y in scs[0]["prev"][scs[0]["kps1"]["octave"] == 0]]
    res = {"part": "a", "keypoints": 1000, "level0_queries": lvl0[:4], "nmatches": [r[0] for r in refs[:4]],
           "candidates_per_window_median": int(np.median(cands)), "candidates_per_window_max": int(max(cands))}
    names = {0: ("k_si_grid", "k_si_cand", "k_si_resolve"), GF_SI_DIRECT: ("k_si_grid", "k_si_cand_direct",
                                                                            "k_si_resolve_direct")}
    for P in (1, 256):
        tens = device_batch([scs[p % NSCENES] for p in range(P)])
        c = tens[0].shape[1]
        m12 = torch.empty((P, c), dtype=torch.int32, device="cuda")
        nm = torch.zeros(P, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def launch(flags):
            check(lib().gf_search_for_initialization_batch_dev(
                ctx.handle, ctypes.byref(S.INFO), P, tens[0].data_ptr(), tens[1].data_ptr(), c, tens[2].data_ptr(),
                tens[3].data_ptr(), tens[4].data_ptr(), c, tens[5].data_ptr(), 100, ctypes.c_float(0.9), 1, flags,
                tens[6].data_ptr(), m12.data_ptr(), nm.data_ptr(), ctx.stream))

        # warm-up, and both paths agree with the restatement's first and second call
        for flags, want in ((0, refs), (GF_SI_DIRECT, again)):
            launch(flags)
            check(lib().gf_ctx_sync(ctx.handle))
            got = nm.cpu().numpy()
            assert all(int(got[p]) == want[p % NSCENES][0] for p in range(P)), (flags, got[:4])
        rounds = {}
        for _ in range(5):
            for flags, tag in ((0, "lists"), (GF_SI_DIRECT, "direct")):
                p = KB.prof(ctx, lambda: launch(flags), 40)
                tot = 0.0
                for k in names[flags]:
                    us = 1e3 * p[k][0] / p[k][1]
                    rounds.setdefault(f"{tag}_{k}", []).append(round(us, 2))
                    tot += us
                rounds.setdefault(f"{tag}_total", []).append(round(tot, 2))
        for k, v in rounds.items():
            res[f"P{P}_{k}_us"] = v
            res[f"P{P}_{k}_us_median"] = KB.med(v)
    return res


def part_b():
    import searchinit_ref as R
    import searchinit_scenes as S

    scs = [euroc(s) for s in range(NSCENES)]
    runs = []
    for _ in range(4):  # the first is the warm-up
        t0 = time.perf_counter()
        for s in scs:
            R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"])
        runs.append(round(1e6 * (time.perf_counter() - t0) / len(scs), 1))
    return {"part": "b", "restatement_us_per_problem_1core": runs[1:],
            "restatement_us_per_problem_1core_median": sorted(runs[1:])[1]}


def part_c():
    import initmap_scenes
    import kfcull_bench as KB
    import searchinit_scenes as S
    from gf_orb_slam_amd import tracking as TR

    sc = S.two_view(1)
    runs = []
    for _ in range(4):  # the first is the warm-up
        mi = TR.MonoInitializer(S.INFO, sc["K"], initmap_scenes.rng_state(1))
        mi.feed(sc["kps1"], sc["desc1"])
        t0 = time.perf_counter()
        state, m, rep = mi.feed(sc["kps2"], sc["desc2"])
        runs.append(dict(mi.times, total=time.perf_counter() - t0))
        assert state == TR.WORKING
    keys = tuple(runs[0])
    ms = lambda k: [round(1e3 * r[k], 2) for r in runs[1:]]  # noqa: E731
    return {"part": "c", "nmatches": rep["nmatches"], "points": rep["npts"], "ba_iterations": rep["ba_iterations"],
            **{k + "_ms": ms(k) for k in keys}, **{k + "_ms_median": KB.med(ms(k)) for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c", "all"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "searchinit", "bench.json"))
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
