"""Timing of one CreateNewMapPoints call at the workload's shape (20
neighbours x 1000 keypoints, 2100 existing points) on one GPU: device time
from HIP events around the enqueue of gf_create_new_map_points_dev, the
kernels' own times from the library's profiler, and the CPU restatement
(tests/localmap_ref.py, with the CPU oracle's SearchForTriangulation) on one
core of the same host. Prints one JSON object."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import localmap_ref as R  # noqa: E402
import localmap_scenes as S  # noqa: E402
from gf_orb_slam_amd import localmapping as LM  # noqa: E402
from gf_orb_slam_amd._lib import check, lib, ptr  # noqa: E402
from gf_orb_slam_amd.orb import default_context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--neighbours", type=int, default=20)
ap.add_argument("--keypoints", type=int, default=1000)
args = ap.parse_args()

rng = np.random.default_rng(0)
poses = tuple(((float(rng.uniform(0.2, 0.6) * rng.choice([-1, 1])), float(rng.uniform(-0.15, 0.15)),
                float(rng.uniform(-0.1, 0.3))), tuple(float(x) for x in rng.normal(0, 0.02, 3)))
              for _ in range(args.neighbours))
n = args.keypoints
groups = (("existing", 3 * n // 10), ("good", n // 2), ("parallax", n // 25), ("behind", n // 50), ("behind2", n // 100),
          ("reproj1", n // 50), ("reproj2", n // 100), ("scale", n // 50), ("clutter", 10))
sc = S.scene(21, n, n, poses=poses, groups=groups, own=90, no_depth=None)
nn, cur = len(sc["neighbours"]), sc["cur"]

t0 = time.perf_counter()
ref = R.create_new_map_points(sc, chain=1)
cpu_ms = (time.perf_counter() - t0) * 1e3

dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
keep, start, tables = [], [], []


def kf(k):
    fv = sc["fv"][k]
    bufs = [t(fv.nodes), t(fv.start), t(fv.feats), t(sc["desc"][k]), t(sc["kps"][k].view(np.uint8)), t(sc["slots"][k])]
    keep.append(bufs)
    start.append(bufs[5].clone())
    tables.append(bufs[5])
    return LM.NewPointsKf.make(sc["Tcw"][k], bufs, len(fv.nodes), len(sc["desc"][k]))


c = kf(cur)
arr = (LM.NewPointsKf * nn)(*[kf(k) for k in sc["neighbours"]])
d_rep = torch.zeros(nn * LM.NEIGH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
d_pts = torch.zeros(n * LM.NEWPOINT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
d_ex = torch.zeros(nn * n, dtype=torch.int32, device=dev)
d_tot = torch.zeros(1, dtype=torch.int32, device=dev)
pos = t(sc["mps"]["pos"])
ctx = default_context()
s = torch.cuda.current_stream(dev)


def reset():
    for a, b in zip(tables, start):
        a.copy_(b)


def call():
    check(lib().gf_create_new_map_points_dev(ctx.handle, ctypes.byref(sc["info"]), ctypes.byref(c), nn, arr, ptr(pos),
                                             len(sc["mps"]), 0, n, ptr(d_rep), ptr(d_pts), ptr(d_ex), ptr(d_tot),
                                             s.cuda_stream))


ts = []
for rep in range(args.reps + 3):
    reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    call()
    e1.record(s)
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
ts = ts[3:]
total = int(d_tot.item())
pts = d_pts.cpu().numpy().view(LM.NEWPOINT_DTYPE)[:total]
assert pts.tobytes() == ref["points"].tobytes(), "device and restatement disagree"

# the kernels' own times (dispatch timestamps), to see what the chain leaves idle
check(lib().gf_prof_enable(ctx.handle, 1))
check(lib().gf_prof_reset(ctx.handle))
for _ in range(5):
    reset()
    call()
torch.cuda.synchronize()
kern, i = {}, 0
name, ms, cnt = ctypes.create_string_buffer(64), ctypes.c_double(), ctypes.c_int()
while lib().gf_prof_report(ctx.handle, i, name, 64, ctypes.byref(ms), ctypes.byref(cnt)) == 0:
    kern[name.value.decode()] = {"us_per_launch": round(1e3 * ms.value / max(cnt.value, 1), 2),
                                 "launches_per_call": cnt.value / 5}
    i += 1
check(lib().gf_prof_enable(ctx.handle, 0))
busy_us = sum(v["us_per_launch"] * v["launches_per_call"] for v in kern.values())
print(json.dumps({"neighbours": nn, "keypoints": n, "existing_points": len(sc["mps"]), "new_points": total,
                  "matches": int(ref["nmatches"].sum()), "status": ref["status"].tolist(),
                  "device_ms_median": round(float(np.median(ts)), 4), "device_ms_min": round(float(min(ts)), 4),
                  "device_ms_max": round(float(max(ts)), 4), "reps": len(ts), "kernels": kern,
                  "kernel_busy_us_per_call": round(busy_us, 1), "launches_per_call": 1 + 2 * nn,
                  "cpu_restatement_ms_1core": round(cpu_ms, 3)}))
