"""Micro-benchmark of the SearchInNeighbors kernels on one GPU. Prints one JSON
object per run.

  --part a   the backward shape: one 1000-keypoint keyframe against 16k
             candidates through gf_fuse_search_dev (kernel time from the
             library's HIP-event profiler), beside gf_fuse_dev on the same
             gathered inputs, alternating, and the tests' restatement on one
             core. --chunks a,b,c sweeps the candidates per workgroup
             (gf_fuse_search_set_chunk), one JSON line per value.
  --part b   a whole localmapping.search_in_neighbors on a map of 22 good
             neighbours at ~1000 keypoints (20 first-neighbour targets and
             some 50 second-neighbour entries), split by timing wrappers
             around the library's own functions into the two launches
             (uploads, kernel, downloads), the host walks (searches redone
             inside them included) and the update pass.
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


def part_a(chunks):
    import torch

    import lmap_scenes as S
    from gf_orb_slam_amd._lib import check, lib, ptr
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE, FuseProblem, FuseSearchProblem
    from gf_orb_slam_amd.orb import default_context
    from neighbors_ref import RefWorld

    ctx = default_context()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sc = S.fuse_scene(21, nmp=15000, nkp=1000, dup=1000)
    kf, m = sc["kf"], len(sc["mps"])
    info = sc["info"]
    d_kps, d_desc = t(kf.mvKeysUn.view(np.uint8)), t(kf.mDescriptors)
    d_mps, d_md, d_skip = t(sc["mps"].view(np.uint8)), t(sc["mp_desc"]), t(sc["skip"])
    # gf_fuse_search_dev: the gathered rows are the map, the candidates its ids in order
    d_pts = t(np.arange(m, dtype=np.int32))
    d_res = torch.zeros(m * 2, dtype=torch.int32, device=dev)
    sp = (FuseSearchProblem * 1)(FuseSearchProblem.make(sc["Tcw"], sc["Ow"], d_kps, d_desc, kf.N, d_pts, d_skip, m, 3.0,
                                                        d_res))
    search = lambda: check(lib().gf_fuse_search_dev(ctx.handle, ctypes.byref(info), 1, sp, ptr(d_mps), ptr(d_md),  # noqa: E731
                                                    None, m, ctx.stream))
    # gf_fuse_dev on the same inputs
    bufs = [d_kps, d_desc, t(sc["kf_mp"]), t(sc["kf_bad"]), d_mps, d_md, d_skip, t(sc["ids"]),
            torch.zeros(m * 3, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)]
    fp = (FuseProblem * 1)(FuseProblem.make(sc["Tcw"], sc["Ow"], bufs, kf.N, m, 3.0))
    fuse = lambda: check(lib().gf_fuse_dev(ctx.handle, ctypes.byref(info), 1, fp, ctx.stream))  # noqa: E731
    search(), fuse()
    ctx.sync()
    kp_s = d_res.cpu().numpy().reshape(-1, 2)[:, 0]
    kp_f = bufs[8].cpu().numpy().reshape(-1, 3)[:, 0]
    assert np.array_equal(kp_s, kp_f), "gf_fuse_search_dev and gf_fuse_dev disagree"
    # the restatement on one core: skip as the bad flag, which leaves at the same place
    mps = np.ascontiguousarray(sc["mps"], MAP_POINT_DTYPE)
    w = RefWorld(info, [kf.mvKeysUn], [kf.mDescriptors], [np.full(kf.N, -1, np.int32)], mps, sc["mp_desc"],
                 mp_bad=sc["skip"], observations=[dict() for _ in range(m)], kf_Tcw=sc["Tcw"][None])
    pts = np.arange(m, dtype=np.int32)
    r = w.fuse(0, pts)
    assert np.array_equal(r["kp"], kp_s), "restatement disagrees"
    t0 = time.perf_counter()
    for _ in range(5):
        w.fuse(0, pts)
    cpu = (time.perf_counter() - t0) / 5
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    out = []
    for chunk in chunks:
        check(lib().gf_fuse_search_set_chunk(ctx.handle, chunk))
        search()
        ctx.sync()
        assert np.array_equal(d_res.cpu().numpy().reshape(-1, 2)[:, 0], kp_s), "the result depends on the chunk"
        rounds = {"k_fuse_search": [], "k_fuse": []}
        for _ in range(5):  # alternating
            for name, fn in (("k_fuse_search", search), ("k_fuse", fuse)):
                p = prof(ctx, fn, 40)[name]
                rounds[name].append(round(1e3 * p[0] / p[1], 2))
        out.append({"part": "a", "chunk": chunk, "keypoints": kf.N, "candidates": m, "fused": int((kp_s >= 0).sum()),
                    "workgroups": (m + chunk - 1) // chunk, "k_fuse_search_us": rounds["k_fuse_search"],
                    "k_fuse_us": rounds["k_fuse"], "k_fuse_search_us_median": med(rounds["k_fuse_search"]),
                    "k_fuse_us_median": med(rounds["k_fuse"]), "restatement_us_1core": round(cpu * 1e6, 1)})
    return out


def part_b():
    import neighbors_scenes as S
    from gf_orb_slam_amd import localmapping as LM
    from gf_orb_slam_amd.orb import default_context

    from gf_orb_slam_amd.loopmap import LoopMap

    ctx = default_context()
    sc = S.neighbors_scene(7, n_world=1150, n_good=22)
    base = S.loop_map(sc)
    # time spent in the library's own phases; a phase entered inside another one counts for the outer one
    acc, depth = {}, [0]

    def timed(owner, name, key):
        fn = getattr(owner, name)

        def wrapper(*a, **kw):
            if depth[0]:
                return fn(*a, **kw)
            depth[0] += 1
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                acc[key] = acc.get(key, 0.0) + time.perf_counter() - t0
                depth[0] -= 1
        setattr(owner, name, wrapper)

    timed(LM._DeviceMap, "__init__", "launch")
    timed(LM._DeviceMap, "search", "launch")
    timed(LM, "_fuse_walk", "walk")
    timed(LoopMap, "compute_distinctive_descriptors", "update")
    timed(LoopMap, "update_normal_and_depth_batch", "update")
    timed(LoopMap, "update_connections", "update")
    runs = []
    for _ in range(4):  # the first is the warm-up
        m = copy.deepcopy(base)
        acc.clear()
        t0 = time.perf_counter()
        rep = LM.search_in_neighbors(m, sc["cur"], ctx=ctx)
        total = time.perf_counter() - t0
        runs.append(dict(acc, total=total))
    t = rep["targets"]
    ms = lambda k: [round(1e3 * r[k], 2) for r in runs[1:]]  # noqa: E731
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    launch, walk, update, total = (med(ms(k)) for k in ("launch", "walk", "update", "total"))
    return {"part": "b", "keyframes": base.nkf, "keypoints_cur": len(base.kf_kps[sc["cur"]]), "map_points": len(base.mps),
            "targets": len(t), "distinct_targets": len(set(t)), "backward_candidates": len(rep["candidates"]),
            "forward_fused": int(sum(f["nFused"] for f in rep["forward"])), "backward_fused": rep["backward"]["nFused"],
            "researched": rep["researched"], "research_changed": rep["research_changed"],
            "launch_ms": ms("launch"), "walk_ms": ms("walk"), "update_ms": ms("update"), "total_ms": ms("total"),
            "launch_ms_median": launch, "walk_ms_median": walk, "update_ms_median": update,
            "walk_share_of_total": round(walk / total, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], required=True)
    ap.add_argument("--chunks", default="64,128,256,512,1024,2048")
    a = ap.parse_args()
    for res in (part_a([int(c) for c in a.chunks.split(",")]) if a.part == "a" else [part_b()]):
        print(json.dumps(res))


if __name__ == "__main__":
    main()
