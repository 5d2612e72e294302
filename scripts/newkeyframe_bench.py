"""Measurement of the NeedNewKeyFrame / CreateNewKeyFrame stage (DESIGN.md,
"NeedNewKeyFrame / CreateNewKeyFrame") -> one JSON object:

  (a) kernel time of k_need_keyframe at the bench shape (B = 256, 1000
      features) with 0, 8 and 256 streams creating, and of the hand-over's
      kernels (k_keyframe_scan + k_keyframe_pack) for 8 and 256 keyframes:
      median of five rounds of 40 launches, from the kernels' own dispatch
      timestamps (the library's profiler, gf_prof_*), in a run of their own;
  (b) step time at the bench shape on keyframe-graph streams, the stage off
      and on with nobody creating, alternated round by round in one process
      (host clock around synchronised runs of `--steps` steps), with the
      spread of each; with --tree-a the "off" figure of another built checkout
      (e.g. the parent commit's) against this one's, alternated process by
      process;
  (c) host clock of one take_keyframes for 1, 8 and 256 keyframes and of one
      pump() + run_mapper() on a stream's map.

python scripts/newkeyframe_bench.py [--out profiles/newkeyframe/bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

# GF_BENCH_TREE: another checkout of the project (built) whose package the --off-only child measures
ROOT = os.environ.get("GF_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(B, nmap, scenes, n_kf=24):
    """A front end of B keyframe-graph streams over `scenes` rendered loops."""
    import torch

    from gf_orb_slam_amd import ORBextractor, scene
    from gf_orb_slam_amd.pipeline import FrontEnd

    W = scene.Workload("euroc", B, n_scenes=scenes, period=32, seed=0)
    frames = W.render_all("cuda").contiguous()
    ex = ORBextractor(1000, 1.2, 8, 1, 20)
    gmaps = W.build_global_maps(lambda im: ex(im), nmap, n_kf=n_kf, device="cuda")
    fe = FrontEnd("euroc", 1000, B, nmap, 100)
    T, V = W.boot_state()
    for b in range(B):
        gm = gmaps[W.scene_of[b]]
        fe.set_map(b, gm["mp"], gm["desc"])
        fe.set_covis(b, gm["graph"])
        fe.set_rng(b, 1 + b)
    fe.set_source(frames, W.scene_of, W.phase)
    fe.bootstrap(T, V, 0.0)
    torch.cuda.synchronize()
    return W, gmaps, fe


def time_steps(fe, steps):
    fe.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fe.step()
    fe.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=[round(x, 4) for x in v])


def step_times(fe, steps, rounds):
    """(b): stage off / on (nobody creating: every mapper busy, SINCE reset), alternated."""
    off, on = [], []
    for _ in range(3):
        fe.step()  # sizes the scratch, settles the clocks
    for _ in range(rounds):
        fe.enable_keyframes(on=False)
        off.append(time_steps(fe, steps))
        fe.enable_keyframes()
        fe.set_keyframe_state(None, accept=0)
        on.append(time_steps(fe, steps))
        st = fe.keyframe_state()
        assert not st["pending"].any() and st["seq"].max() == 0, "a stream created a keyframe in the 'on' rounds"
    return dict(steps=steps, off_ms=spread(off), on_ms=spread(on),
                on_minus_off_ms=statistics.median(on) - statistics.median(off))


def kernel_and_take_times(fe):
    """(a) and the take_keyframes part of (c), on the front end's own outbox."""
    import torch

    import newkeyframe_scenes as S
    from gf_orb_slam_amd._lib import check, lib
    from gf_orb_slam_amd.pipeline import NewKfArgs

    B, cap = fe.B, fe.cap
    fe.enable_keyframes()
    d = fe.keyframes_dev()
    p = S.Problem(B, cap, 2, 512, seed=1)
    for b in range(B):
        p.set_row(b, 350, 9)      # a reference keyframe of 350 tracked points
        p.inliers[b] = 200
    p.nkp[:] = min(cap, 1000)
    names = ("nkp", "kps", "desc", "kp2mp", "Tcw", "t_cur", "track", "inliers", "working", "ref_kf", "kf_count",
             "kf_mp_off", "kf_mp")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(p, k))).cuda() for k in names}
    a = NewKfArgs(B, cap, *[t[k].data_ptr() for k in names], p.off_stride, p.kf_mp.shape[1], d["state"], d["hdr"],
                  d["kps"], d["desc"], d["slots"], 0, 12)
    torch.cuda.synchronize()

    def launch(ncreate):
        acc = np.zeros(B, np.int32)
        acc[:ncreate] = 1
        fe.set_keyframe_state(None, pending=0, accept=acc, since=0)  # the outbox slots are free again
        check(lib().gf_need_new_keyframe_dev(fe.ctx.handle, ctypes.byref(a), None))

    def prof(fn, kernels, rounds=5, launches=40):
        per = []
        fe.prof_enable(True)
        for _ in range(rounds):
            fe.prof_reset()
            for _ in range(launches):
                fn()
            torch.cuda.synchronize()
            fe.sync()
            rep = fe.prof_report()
            per.append(sum(rep[k][0] for k in kernels) / max(rep[kernels[0]][1], 1) * 1e3)
        fe.prof_enable(False)
        return spread(per)

    out = {"k_need_keyframe_us": {}, "k_keyframe_scan+pack_us": {}, "take_keyframes_host_ms": {}}
    for n in (0, 8, 256):
        out["k_need_keyframe_us"][str(n)] = prof(lambda n=n: launch(min(n, B)), ["k_need_keyframe"])
    for n in (8, 256):
        def take(n=n):
            launch(min(n, B))
            torch.cuda.synchronize()
            assert len(fe.take_keyframes()) == min(n, B)
        out["k_keyframe_scan+pack_us"][str(n)] = prof(take, ["k_keyframe_scan", "k_keyframe_pack"], launches=10)
    for n in (1, 8, 256):
        v = []
        for _ in range(5):
            launch(min(n, B))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fe.take_keyframes()
            v.append((time.perf_counter() - t0) * 1e3)
            assert len(got) == min(n, B)
        out["take_keyframes_host_ms"][str(n)] = spread(v)
    return out


def pump_and_mapper():
    """(c): one stream until its first keyframe, then pump() + run_mapper()."""
    from gf_orb_slam_amd import synth, tracking
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.localmapping import LocalMapper
    from gf_orb_slam_amd.matcher import FrameInfo

    W, gmaps, fe = build(1, 2600, 1)
    voc = ORBVocabulary(synth.synth_vocabulary_fast(11, k=10, L=5))
    info = FrameInfo.make(*synth.CAMERAS["euroc"])
    m = tracking.loopmap_from_global_map(info, gmaps[0], voc=voc)
    ins = tracking.KeyFrameInserter(fe, [LocalMapper(m, voc)])
    fe.enable_keyframes()
    steps = 0
    while not fe.keyframe_state()["pending"][0] and steps < 16:
        fe.step()
        steps += 1
    t0 = time.perf_counter()
    took = ins.pump()
    t1 = time.perf_counter()
    rep = ins.run_mapper(0) if took else None
    t2 = time.perf_counter()
    fe.close()
    return dict(steps_until_keyframe=steps, created=bool(took), pump_ms=(t1 - t0) * 1e3,
                run_mapper_ms=(t2 - t1) * 1e3,
                stages_ms={k: rep[k]["seconds"] * 1e3 for k in rep["order"]} if rep else None)


def off_only(args):
    """Child of the two-build comparison: the 'off' step time of the tree GF_BENCH_TREE names."""
    _, _, fe = build(args.batch, args.map, args.scenes)
    for _ in range(3):
        fe.step()
    v = [time_steps(fe, args.steps) for _ in range(args.rounds)]
    print("OFF_MS " + json.dumps(v), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--map", type=int, default=2000)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tree-a", default=None, help="a built checkout to compare 'off' against (e.g. the parent commit)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--off-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.off_only:
        return off_only(args)
    res = dict(shape=dict(batch=args.batch, nfeatures=1000, map=args.map, scenes=args.scenes))
    _, _, fe = build(args.batch, args.map, args.scenes)
    res["b_step_ms"] = step_times(fe, args.steps, args.rounds)
    res["a_kernels"] = kernel_and_take_times(fe)
    fe.close()
    res["c_pump_run_mapper"] = pump_and_mapper()
    if args.tree_a:
        got = {"a": [], "b": []}
        for which in ("a", "b", "a", "b"):  # a fresh process each: the package is chosen at import
            env = dict(os.environ)
            env.pop("GF_BENCH_TREE", None)
            if which == "a":
                env["GF_BENCH_TREE"] = os.path.abspath(args.tree_a)
            cmd = [sys.executable, os.path.abspath(__file__), "--off-only", "--batch", str(args.batch), "--map",
                   str(args.map), "--scenes", str(args.scenes), "--steps", str(args.steps), "--rounds", str(args.rounds)]
            o = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, check=True).stdout
            got[which] += json.loads([ln for ln in o.splitlines() if ln.startswith("OFF_MS ")][-1][7:])
        res["b_off_two_builds_ms"] = dict(tree_a=args.tree_a, a=spread(got["a"]), b_this_build=spread(got["b"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
