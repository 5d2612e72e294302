"""Timing of the SearchAndFuse searches (gf_fuse_sim3_dev) on a loop of 20
keyframes x 2000 loop points at n = 1000 keypoints:
  (i)   all 20 problems in one launch (device events, median of 20 after warm-up);
  (ii)  the same work as 20 single-keyframe launches;
  (iii) the restatement's searches (tests/helpers/loopfuse_ref.cpp) on one host core;
  (iv)  the whole search_and_fuse with its host part (host clock; it ends synchronised).
The candidates-per-workgroup chunk is read once per process (GF_FUSE_SIM3_CHUNK),
so `--chunks 128,256,512` runs one child process per value. Each run prints one
JSON line; --out appends them to a file. DESIGN.md quotes the figures."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", default="", help="comma-separated chunk sizes: one child process each")
ap.add_argument("--out", default="")
ap.add_argument("--nkf", type=int, default=20)
ap.add_argument("--npoints", type=int, default=2000)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

if args.chunks:
    for c in args.chunks.split(","):
        env = dict(os.environ, GF_FUSE_SIM3_CHUNK=c.strip())
        cmd = [sys.executable, os.path.abspath(__file__), "--nkf", str(args.nkf), "--npoints", str(args.npoints),
               "--reps", str(args.reps)] + (["--out", args.out] if args.out else [])
        rc = subprocess.run(cmd, env=env, timeout=280).returncode
        if rc:
            sys.exit(rc)
    sys.exit(0)

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import loopfuse_ref as R  # noqa: E402
import loopfuse_scenes as S  # noqa: E402
from gf_orb_slam_amd._lib import check, lib, ptr  # noqa: E402
from gf_orb_slam_amd.loopmap import LoopMap  # noqa: E402
from gf_orb_slam_amd.orb import default_context  # noqa: E402
from gf_orb_slam_amd.sim3 import FuseSim3Problem, search_and_fuse  # noqa: E402

sc = S.loop_scene(21, n_loop=args.npoints, n_cur=args.nkf, n_loopkf=2, kp_extra=300, plant=False,
                  cur_sizes=[1000] * args.nkf)
pts, kfs = sc["loop_points"], sc["cur"]
dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
d_mps, d_md, d_bad, d_pts = t(sc["mps"].view(np.uint8)), t(sc["mp_desc"]), t(sc["mp_bad"].astype(np.uint8)), t(pts)
keep, probs, outs = [], [], []
for k in kfs:
    bufs = [t(sc["kf_kps"][k].view(np.uint8)), t(sc["kf_desc"][k]), t(sc["kf_mp"][k]),
            torch.zeros(len(pts) * 2, dtype=torch.int32, device=dev)]
    keep += bufs
    outs.append(bufs[3])
    probs.append(FuseSim3Problem.make(sc["corrected"][k], bufs[0], bufs[1], len(sc["kf_kps"][k]), bufs[2], d_pts,
                                      len(pts), 4.0, bufs[3]))
arr = (FuseSim3Problem * len(probs))(*probs)
ctx = default_context()
s = torch.cuda.current_stream(dev)


def launch(first, count):
    a = (FuseSim3Problem * count).from_address(ctypes.addressof(arr) + first * ctypes.sizeof(FuseSim3Problem))
    check(lib().gf_fuse_sim3_dev(ctx.handle, ctypes.byref(sc["info"]), count, a, ptr(d_mps), ptr(d_md), ptr(d_bad),
                                 len(sc["mps"]), s.cuda_stream))


def timed(fn):
    ts = []
    for rep in range(args.reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts[3:]


one = timed(lambda: launch(0, len(kfs)))
batch = torch.stack(outs).cpu().numpy().copy()
many = timed(lambda: [launch(j, 1) for j in range(len(kfs))])
assert np.array_equal(batch, torch.stack(outs).cpu().numpy())
ref = R.RefMap(*S.map_args(sc))
t0 = time.perf_counter()
want = [ref.fuse(k, sc["corrected"][k], pts, 4.0) for k in kfs]
host_ms = (time.perf_counter() - t0) * 1e3
got = batch.reshape(len(kfs), len(pts), 2)
assert all(np.array_equal(got[j, :, 0], want[j]["kp"]) and np.array_equal(got[j, :, 1], want[j]["dist"])
           for j in range(len(kfs)))
whole = []
for rep in range(3):
    lm = LoopMap(*S.map_args(sc))
    t0 = time.perf_counter()
    rep_out = search_and_fuse(lm, sc["corrected"], pts, 4.0)
    whole.append((time.perf_counter() - t0) * 1e3)
line = json.dumps({"chunk": int(os.environ.get("GF_FUSE_SIM3_CHUNK", "256")), "nkf": len(kfs), "npoints": len(pts),
                   "n": [len(sc["kf_kps"][k]) for k in kfs][:3],
                   "one_launch_ms_median": float(np.median(one)), "one_launch_ms_min_max": [min(one), max(one)],
                   "single_launches_ms_median": float(np.median(many)),
                   "single_launches_ms_min_max": [min(many), max(many)],
                   "restatement_one_core_ms": host_ms, "fused_pairs": int((got[:, :, 0] >= 0).sum()),
                   "search_and_fuse_ms": whole, "nFused": int(sum(rep_out["nFused"].values()))})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
