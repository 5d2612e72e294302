"""Timing of the batched Optimizer::OptimizeSim3 (gf_optimize_sim3_dev): 256
problems x 100 pairs (20% permuted, 0.2 px noise), device events around the
launch (the first call, then five after it), and the restatement of
tests/helpers/sim3opt_ref.cpp on one host core for the same problems. Prints
one JSON line, with the worst deviation of the device from the restatement.
DESIGN.md §3 'OptimizeSim3' quotes it."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sim3opt_ref as O  # noqa: E402
from gf_orb_slam_amd.optimizer import Optimizer  # noqa: E402

P, N = 256, 100
dev = torch.device("cuda:0")
scenes = [O.opt_scene(N, 1000 + i, 0.2, noise=0.2) for i in range(P)]
t0 = time.perf_counter()
refs = [O.optimize(*O.args(sc)) for sc in scenes]
host_ms = (time.perf_counter() - t0) * 1e3
offs = (np.arange(P + 1) * N).astype(np.int32)
cat = lambda k: np.concatenate([sc[k].reshape(-1) for sc in scenes]).astype(np.float32)  # noqa: E731
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
bufs = [t(cat(k)) for k in ("X1", "X2", "z1", "z2", "w1", "w2")]
dK = t(np.stack([np.concatenate([sc["K1"], sc["K2"]]) for sc in scenes]).astype(np.float32))
dth = t(np.full(P, 10.0, np.float32))
dS0 = t(np.stack([sc["S0"] for sc in scenes]))
dS = dS0.clone()
dinl = torch.zeros(P * N, dtype=torch.uint8, device=dev)
dnin = torch.zeros(P, dtype=torch.int32, device=dev)
dst = torch.zeros(P * 4, dtype=torch.int32, device=dev)
doffs = t(offs)
s = torch.cuda.current_stream(dev)
times = []
for rep in range(6):
    dS.copy_(dS0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    Optimizer.optimize_sim3_batch_dev(*bufs, doffs, dK, dth, dS, dinl, dnin, dst, stream=s.cuda_stream)
    e1.record(s)
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1))
nin = dnin.cpu().numpy()
S = dS.cpu().numpy()
st = dst.cpu().numpy().reshape(P, 4)
same = sum(int(nin[p] == refs[p]["nin"]) for p in range(P))
dmax = max(float(np.abs(S[p] - refs[p]["S"]).max()) for p in range(P))
print(json.dumps({"first_ms": times[0], "warm_ms": times[1:], "warm_median_ms": float(np.median(times[1:])),
                  "host_one_core_ms": host_ms, "nin_equal": same, "max_abs_dS": dmax,
                  "mean_iterations": float(st[:, :2].sum(1).mean()), "mean_trials": float(st[:, 2:].sum(1).mean())}))
