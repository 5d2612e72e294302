"""Timing of Optimizer::OptimizeEssentialGraph on the device (csrc/essgraph.hip)
over generated loops (tests/essgraph_scenes.py): N = 64, 256, 1024 each alone
and a batch of 64 maps of N = 128. Per problem one JSON line: the time of a
solve call after a warm-up (host clock around gf_essgraph_plan_solve: the call
reads three scalars back per Levenberg trial, so the host loop is part of it),
the trials, and the time per trial split by the library's kernel timing
(gf_prof_enable: linearise / assemble / factor / substitute / update, device
time from the kernels' own timestamps, taken in a run of its own).

  --device          the device timings above
  --envelope        N = 1024 once more with every lower tile visited
                    (GF_ESSGRAPH_FULL_ENVELOPE=1) against the envelope
  --host N [N ...]  the restatement (tests/helpers/essgraph_ref.cpp) on one
                    host core; its solve is dense, which at N = 1024 flatters
                    the device
DESIGN.md 'OptimizeEssentialGraph' quotes the output (profiles/essgraph/)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import essgraph_ref as R  # noqa: E402
import essgraph_scenes as S  # noqa: E402


def loop_scene(N, seed):
    # the drift per keyframe shrinks with N so that the loop error stays that of a real loop
    return S.make_scene(N, seed, past_loops=True, gaps=True, npts=2000, drift=min(1.0, 64.0 / N))


def prof_report(ctx):
    from gf_orb_slam_amd._lib import lib

    out, i, name = {}, 0, ctypes.create_string_buffer(64)
    while True:
        ms, cnt = ctypes.c_double(), ctypes.c_int()
        if lib().gf_prof_report(ctx.handle, i, name, 64, ctypes.byref(ms), ctypes.byref(cnt)) != 0:
            return out
        out[name.value.decode()] = (ms.value, cnt.value)
        i += 1


def time_device(label, scenes, reps=3):
    from gf_orb_slam_amd._lib import check, lib
    from gf_orb_slam_amd.optimizer import EssentialGraphPlan
    from gf_orb_slam_amd.orb import default_context

    ctx = default_context()
    t0 = time.perf_counter()
    plan = EssentialGraphPlan(scenes, ctx)
    create_ms = (time.perf_counter() - t0) * 1e3
    plan.solve()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        plan.solve()
        times.append((time.perf_counter() - t0) * 1e3)
    res = plan.results()
    trials = sum(r["trials"] for r in res)
    check(lib().gf_prof_enable(ctx.handle, 1))
    check(lib().gf_prof_reset(ctx.handle))
    plan.solve()
    prof = prof_report(ctx)
    check(lib().gf_prof_enable(ctx.handle, 0))
    check(lib().gf_prof_reset(ctx.handle))
    nedges = [len(plan.edges(p)) for p in range(len(scenes))]
    plan.close()
    call_ms = float(np.median(times))
    print(json.dumps({
        "problem": label, "maps": len(scenes), "edges": int(np.sum(nedges)), "create_ms": round(create_ms, 2),
        "solve_ms": [round(t, 2) for t in times], "solve_median_ms": round(call_ms, 2),
        "iterations": [r["iterations"] for r in res][:4], "trials": trials,
        "ms_per_trial": round(call_ms / trials, 3),
        "device_ms_per_trial": {k[3:]: round(v[0] / trials, 4) for k, v in prof.items() if k.startswith("eg_")},
        "chi2": [res[0]["chi2_initial"], res[0]["chi2_final"]]}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--envelope", action="store_true")
    ap.add_argument("--host", type=int, nargs="*", default=[])
    a = ap.parse_args()
    if a.device:
        for N in (64, 256, 1024):
            time_device(f"N={N}", [loop_scene(N, N)])
        time_device("64 x N=128", [loop_scene(128, 1000 + i) for i in range(64)])
    if a.envelope:
        sc = [loop_scene(1024, 1024)]
        os.environ.pop("GF_ESSGRAPH_FULL_ENVELOPE", None)
        time_device("N=1024 envelope", sc)
        os.environ["GF_ESSGRAPH_FULL_ENVELOPE"] = "1"
        time_device("N=1024 every lower tile", sc)
        os.environ.pop("GF_ESSGRAPH_FULL_ENVELOPE", None)
    for N in a.host:
        sc = loop_scene(N, N)
        t0 = time.perf_counter()
        r = R.solve(sc)
        ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"problem": f"N={N}", "restatement_one_core_ms": round(ms, 1), "dense_solve": True,
                          "iterations": r["iterations"], "trials": r["trials"],
                          "ms_per_trial": round(ms / r["trials"], 2),
                          "chi2": [r["chi2_initial"], r["chi2_final"]]}), flush=True)


if __name__ == "__main__":
    main()
