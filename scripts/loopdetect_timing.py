"""Timing of one DetectLoopCandidates query (gf_detect_loop_candidates) at 2000
listed keyframes x ~1000 words with 30 keyframes connected to the query:
  - device time of each of the three passes and their sum, from the kernels'
    own HIP events (gf_prof_enable), median and min / max of 20 queries after 5
    warm-ups;
  - the whole call on the host clock (uploads of the connected list and the
    covisibility lists, the three kernels, the downloads; it ends synchronised);
  - the restatement (tests/helpers/loopdetect_ref.cpp) on one host core, median of 5 runs;
  - the floor of pass 1: the listed keyframes' words read once at the HBM peak;
  - the three passes when all 16,383 listed slots of a database are candidates
    (pass 3's ordering at its largest), median of 5 after 2 warm-ups.
Prints one JSON line; --out writes it to a file. DESIGN.md quotes the figures."""
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

import loopdetect_ref as R  # noqa: E402
import loopdetect_scenes as S  # noqa: E402
from gf_orb_slam_amd._lib import check, lib  # noqa: E402
from gf_orb_slam_amd.loopdetect import KeyFrameDatabase, covisibles_csr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nkf", type=int, default=2000)
ap.add_argument("--words", type=int, default=1000)
ap.add_argument("--connected", type=int, default=30)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s for the streaming floor")
ap.add_argument("--out", default="")
args = ap.parse_args()

rng = np.random.default_rng(1)
n = args.nkf + 1
nplaces = max(1, args.nkf // 25)
bases = [rng.choice(S.NWORDS, int(args.words * 1.2), replace=False) for _ in range(nplaces)]
place = np.arange(n) * nplaces // n
place[-1] = 0  # the query returns to the first place
vectors = [S.vec(rng, bases[place[i]], int(args.words * 0.8), int(args.words * 0.22)) for i in range(n)]
ordered = [[j for j in range(i - 6, i + 7) if 0 <= j < n - 1 and j != i] for i in range(n)]
q = n - 1
ordered[q] = list(range(q - args.connected, q))
connected = set(ordered[q])
off, cov = covisibles_csr(ordered)

db, ref = KeyFrameDatabase(), R.RefWorld()
for v in vectors:
    db.insert(*v)
    ref.insert(*v)
for k in range(n):
    ref.set_graph(k, ordered[k], connected if k == q else ordered[k])
for k in range(q):
    db.add(k)
    ref.add(k)
min_score = 0.02
ctx = db.ctx
KERNELS = ("k_ld_common", "k_ld_score", "k_ld_select")


def report():
    out, i, name = {}, 0, ctypes.create_string_buffer(64)
    ms, cnt = ctypes.c_double(), ctypes.c_int()
    while lib().gf_prof_report(ctx.handle, i, name, 64, ctypes.byref(ms), ctypes.byref(cnt)) == 0:
        out[name.value.decode()] = ms.value
        i += 1
    return out


check(lib().gf_prof_enable(ctx.handle, 1))
rows, host = [], []
for rep in range(args.warmup + args.reps):
    check(lib().gf_prof_reset(ctx.handle))
    t0 = time.perf_counter()
    g = db.detect_loop_candidates(q, connected, off, cov, min_score, full=True)
    host.append((time.perf_counter() - t0) * 1e3)
    r = report()
    rows.append([r[k] for k in KERNELS])
check(lib().gf_prof_enable(ctx.handle, 0))
rows, host = np.array(rows[args.warmup:]), np.array(host[args.warmup:])
total = rows.sum(1)

ref_ms = []
for rep in range(5):  # the wrapper's marshalling of the per-slot outputs is part of the figure
    t0 = time.perf_counter()
    want = ref.detect_candidates(q, min_score)
    ref_ms.append((time.perf_counter() - t0) * 1e3)
assert g["cands"].tolist() == want["cands"].tolist() and np.array_equal(g["words"], want["words"])

# pass 3 at its largest: 16,383 listed slots with the query's vector and no covisibles, so every one is a
# candidate of its own and the ordering runs over the whole database
big = KeyFrameDatabase()
bw, bv = np.array([3, 9, 11, 40], np.int32), np.full(4, 0.25)
for k in range(16384):
    big.insert(bw, bv)
for k in range(1, 16384):
    big.add(k)
big_off = np.zeros(16385, np.int32)
check(lib().gf_prof_enable(ctx.handle, 1))
big_rows = []
for rep in range(7):
    check(lib().gf_prof_reset(ctx.handle))
    bc = big.detect_loop_candidates(0, [], big_off, [], 0.5)
    r = report()
    big_rows.append([r[k] for k in KERNELS])
check(lib().gf_prof_enable(ctx.handle, 0))
assert len(bc) == 16383
big_rows = np.array(big_rows[2:])

listed_words = int(sum(len(vectors[k][0]) for k in range(q)))
line = json.dumps({
    "listed": q, "connected": len(connected), "words_per_keyframe_mean": listed_words / q,
    "listed_word_bytes": 4 * listed_words, "ncand": len(want["cands"]), "scored": want["trace"]["scored"],
    "device_ms_median": float(np.median(total)), "device_ms_min_max": [float(total.min()), float(total.max())],
    "pass_ms_median": {k: float(np.median(rows[:, i])) for i, k in enumerate(KERNELS)},
    "pass_ms_min_max": {k: [float(rows[:, i].min()), float(rows[:, i].max())] for i, k in enumerate(KERNELS)},
    "call_host_ms_median": float(np.median(host)), "call_host_ms_min_max": [float(host.min()), float(host.max())],
    "restatement_one_core_ms_median": float(np.median(ref_ms)),
    "restatement_one_core_ms_min_max": [min(ref_ms), max(ref_ms)],
    "pass1_stream_floor_ms": 4 * listed_words / (args.hbm_tbs * 1e12) * 1e3,
    "all_16383_candidates_pass_ms_median": {k: float(np.median(big_rows[:, i])) for i, k in enumerate(KERNELS)},
    "all_16383_candidates_pass3_ms_min_max": [float(big_rows[:, 2].min()), float(big_rows[:, 2].max())],
    "reps": args.reps, "warmup": args.warmup})
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
