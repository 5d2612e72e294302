"""Journals and tables for the resident map tables (tests/test_maptables_cpu.py,
tests/test_maptables_gpu.py).

:func:`planted` hand-places one journal on a table of 1100 keyframes with 8
keypoints each (a row holds at most one entry per keyframe, entry
``8 * kf + idx``); every case below is a row of it, named in ``rows``:

- Row lengths: ``len0`` .. ``len300`` hold 0, 1, 63, 64, 65 and 300 live
  entries.
- OBS_SET placement: ``len0`` gets an entry into the empty row; ``len1`` one in
  front of its entry and one behind it; ``len63`` one in the middle, which
  fills the row exactly to its capacity of 64; ``len64`` one onto a keyframe it
  holds (the value changes, the order stays).
- OBS_ERASE: ``len64`` of a keyframe it does not hold, ``len65`` of one it does.
- One row's journal: ``len65`` also erases a keyframe and then sets it again;
  ``len300`` sets, clears and sets (one entry is left); ``ops100`` takes 100
  random ops.
- Capacity: ``len63`` ends exactly at capacity; ``squeeze`` (4 of 4) takes two
  sets and then two erases, 6 entries on the way and 4 at the end; ``nofit``
  (2 of 2) takes one set too many: it keeps its bytes and ``status[0] == 1``.
- Out of range: a row id of -1 with two ops and one of nmp + 3 with one op, an
  op on keyframe -1, one on keyframe nkf, a set at idx 8 and one of an unknown
  kind on ``len1``, slot targets -1 and nkp, a bad flag for point nmp:
  ``status[1] == 10``.
- The rows in between are not touched.

:func:`slack_tables` turns tables of ``covis_scenes.thin_tables`` (1, 2, 65 and
1100 keyframes) into slack CSR, :func:`random_journal` draws a journal for a
chosen number of touched rows, :func:`move_case` plants the regrow's inputs
and :func:`random_walk` drives a LoopMap through its mutators.
"""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd.maptables import OBS_CLEAR, OBS_ERASE, OBS_SET
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

KP = 8  # keypoints per keyframe of the planted table
EMPTY = dict(slot_g=np.zeros(0, np.int32), slot_v=np.zeros(0, np.int32), bad_p=np.zeros(0, np.int32),
             row_ids=np.zeros(0, np.int32), row_op_off=np.zeros(1, np.int32), ops=np.zeros((0, 3), np.int32))


def _tables(nkf, rows, caps, kp=KP, seed=1):
    """Flat tables with ``rows[p]`` = the observing keyframes of point p
    (ascending) in a row of capacity ``caps[p]``; the entry of keyframe k in
    row p is ``kp * k + (k + p) % kp``."""
    rng = np.random.default_rng(seed)
    kf_off = (kp * np.arange(nkf + 1)).astype(np.int32)
    nmp = len(rows)
    obs_off = np.zeros(nmp + 1, np.int32)
    obs_off[1:] = np.cumsum(caps)
    obs_gkp = np.full(obs_off[-1], -1, np.int32)
    for p, r in enumerate(rows):
        assert len(r) <= caps[p] and list(r) == sorted(set(r))
        obs_gkp[obs_off[p]:obs_off[p] + len(r)] = [kp * k + (k + p) % kp for k in r]
    slots = rng.integers(-1, max(nmp, 1), kp * nkf).astype(np.int32)
    return dict(kf_off=kf_off, slots=slots, mp_bad=np.zeros(nmp, np.uint8), obs_off=obs_off, obs_gkp=obs_gkp)


def _journal(nmp, per_row, slot=(), bad=()):
    """Journal arrays from ``per_row`` = {row id: [(kind, kf, idx), ...]}."""
    ids = sorted(per_row)
    ops = [op for p in ids for op in per_row[p]]
    off = np.concatenate([[0], np.cumsum([len(per_row[p]) for p in ids])]).astype(np.int32)
    slot = np.asarray(list(slot), np.int32).reshape(-1, 2)
    return dict(slot_g=slot[:, 0].copy(), slot_v=slot[:, 1].copy(), bad_p=np.asarray(list(bad), np.int32),
                row_ids=np.asarray(ids, np.int32), row_op_off=off, ops=np.asarray(ops, np.int32).reshape(-1, 3))


def planted():
    """-> (tables, journal, rows: name -> row id, expect: name -> the keyframes
    the row must hold afterwards)."""
    nkf = 1100
    rng = np.random.default_rng(7)
    spread = lambda n: sorted(int(k) for k in rng.choice(np.arange(100, 1000), n, replace=False))  # noqa: E731
    rows, caps, names = [], [], {}

    def add(name, kfs, cap):
        names[name] = len(rows)
        rows.append(kfs)
        caps.append(cap)
        for _ in range(2):  # untouched neighbours, one full and one with slack
            rows.append(spread(5))
            caps.append(5 + len(rows) % 2 * 3)

    add("len0", [], 4)
    add("len1", [500], 3)
    add("len63", spread(63), 64)
    add("len64", spread(64), 70)
    add("len65", spread(65), 65)
    add("len300", spread(300), 300)
    add("ops100", spread(40), 160)
    add("squeeze", [200, 300, 400, 500], 4)
    add("nofit", [200, 300], 2)
    t = _tables(nkf, rows, caps)
    nmp, nkp = len(rows), KP * nkf
    r = {n: rows[i] for n, i in names.items()}
    mid = next(k for k in range(r["len63"][31] + 1, 1000) if k not in r["len63"])
    absent = next(k for k in range(100, 1000) if k not in r["len64"])
    per = {
        -1: [(OBS_SET, 3, 1), (OBS_CLEAR, 0, 0)],
        names["len0"]: [(OBS_SET, 700, 2)],
        names["len1"]: [(OBS_SET, 3, 7), (OBS_SET, -1, 0), (OBS_SET, 900, 0), (OBS_ERASE, nkf, 0), (OBS_SET, 600, KP),
                        (7, 600, 0)],
        names["len63"]: [(OBS_SET, mid, 5)],
        names["len64"]: [(OBS_SET, r["len64"][20], (r["len64"][20] + names["len64"] + 3) % KP), (OBS_ERASE, absent, 0)],
        names["len65"]: [(OBS_ERASE, r["len65"][0], 0), (OBS_ERASE, r["len65"][40], 0), (OBS_SET, r["len65"][40], 6)],
        names["len300"]: [(OBS_SET, 50, 1), (OBS_CLEAR, 0, 0), (OBS_SET, 1050, 4)],
        names["squeeze"]: [(OBS_SET, 250, 0), (OBS_SET, 1099, 7), (OBS_ERASE, 300, 0), (OBS_ERASE, 200, 0)],
        names["nofit"]: [(OBS_SET, 250, 3)],
        nmp + 3: [(OBS_ERASE, 5, 0)],
    }
    held = set(r["ops100"])
    ops = []
    for _ in range(100):
        k = int(rng.integers(0, nkf))
        if rng.random() < 0.35 and held:
            k = int(rng.choice(sorted(held)))
            held.discard(k)
            ops.append((OBS_ERASE, k, 0))
        else:
            held.add(k)
            ops.append((OBS_SET, k, int(rng.integers(0, KP))))
    per[names["ops100"]] = ops
    free = [g for g in range(0, nkp, 97)]
    j = _journal(nmp, per, slot=[(-1, 5)] + [(g, g % 11 - 1) for g in free] + [(nkp, 2)],
                 bad=[names["len300"], names["nofit"], nmp, 1])
    expect = dict(len0=[700], len1=[3, 500, 900], len63=sorted(r["len63"] + [mid]), len64=r["len64"],
                  len65=r["len65"][1:], len300=[1050], ops100=sorted(held), squeeze=[250, 400, 500, 1099],
                  nofit=r["nofit"])
    return t, j, names, expect


def slack_tables(thin, seed=3, extra=3):
    """The tables of ``covis_scenes.thin_tables`` as slack CSR: every row
    sorted, ``extra`` entries of -1 behind it."""
    kf_off, slots, mp_bad, obs_off, obs_gkp = (np.asarray(a) for a in thin[:5])
    live = np.diff(obs_off)
    off = np.zeros(len(live) + 1, np.int32)
    off[1:] = np.cumsum(live + extra)
    g = np.full(off[-1], -1, np.int32)
    for p in range(len(live)):
        g[off[p]:off[p] + live[p]] = np.sort(obs_gkp[obs_off[p]:obs_off[p + 1]])
    return dict(kf_off=kf_off.astype(np.int32), slots=slots.astype(np.int32).copy(), mp_bad=mp_bad.astype(np.uint8).copy(),
                obs_off=off, obs_gkp=g)


def wide_tables(nmp, nkf=65, seed=5):
    """``nmp`` rows of 0..12 random keyframes each with 3 entries of slack."""
    rng = np.random.default_rng(seed)
    rows = [sorted(int(k) for k in rng.choice(nkf, int(rng.integers(0, 13)), replace=False)) for _ in range(nmp)]
    return _tables(nkf, rows, [len(r) + 3 for r in rows], seed=seed)


def random_journal(t, nrows, seed=9, max_ops=3):
    """A journal touching ``nrows`` distinct random rows with 1..max_ops random
    ops each (sets of random keyframes, erases of held and absent ones, now and
    then a clear), some slot writes and bad flags."""
    rng = np.random.default_rng(seed)
    kf_off = t["kf_off"]
    nkf, nmp, nkp = len(kf_off) - 1, len(t["mp_bad"]), int(kf_off[-1])
    per = {}
    for p in rng.choice(nmp, min(nrows, nmp), replace=False):
        ops = []
        for _ in range(int(rng.integers(1, max_ops + 1))):
            k = int(rng.integers(0, nkf))
            n = int(kf_off[k + 1] - kf_off[k])
            u = rng.random()
            if u < 0.05:
                ops.append((OBS_CLEAR, 0, 0))
            elif u < 0.4 or not n:
                ops.append((OBS_ERASE, k, 0))
            else:
                ops.append((OBS_SET, k, int(rng.integers(0, n))))
        per[int(p)] = ops
    ng = min(nkp, 50)
    slot = [(int(g), int(rng.integers(-1, max(nmp, 1)))) for g in rng.choice(nkp, ng, replace=False)] if nkp else []
    return _journal(nmp, per, slot=slot, bad=rng.choice(nmp, min(nmp, 7), replace=False) if nrows else [])


def move_case():
    """-> (old_off, old_gkp, new_off, live per row, the row whose new capacity
    is below its live count). Old rows with -1 at the front, in the middle and
    at the end, everywhere and nowhere, of 0, 1, 7, 8, 9, 64, 65 and 300
    capacity; the new capacity equals the live count in every second row."""
    rng = np.random.default_rng(4)
    rows = []
    for cap in (0, 1, 7, 8, 9, 64, 65, 300, 5, 5, 5, 5, 5, 12):
        rows.append(np.sort(rng.choice(5000, cap, replace=False)).astype(np.int32))
    rows[8][:2] = -1      # front
    rows[9][2] = -1       # middle
    rows[10][3:] = -1     # end
    rows[11][:] = -1      # everywhere
    rows[5][::3] = -1
    rows[7][rng.random(300) < 0.5] = -1
    for _ in range(40):
        r = np.sort(rng.choice(5000, int(rng.integers(0, 20)), replace=False)).astype(np.int32)
        r[rng.random(len(r)) < 0.3] = -1
        rows.append(r)
    old_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    live = np.asarray([int((r >= 0).sum()) for r in rows])
    cap = live + np.where(np.arange(len(rows)) % 2, 0, 3)
    short = 13
    cap[short] = live[short] - 1
    new_off = np.concatenate([[0], np.cumsum(cap)]).astype(np.int32)
    return old_off, np.concatenate(rows).astype(np.int32), new_off, live, short


def thin_map(nkf=65, **kw):
    """A LoopMap of ``covis_scenes.thin_tables(nkf)``: its slot tables, and per
    point the observations its row lists."""
    import covis_scenes
    from gf_orb_slam_amd.loopmap import LoopMap
    from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE

    kf_off, slots, mp_bad, obs_off, obs_gkp = covis_scenes.thin_tables(nkf)[:5]
    rng = np.random.default_rng(nkf)
    n = np.diff(kf_off)
    kf = np.searchsorted(kf_off, obs_gkp, side="right") - 1
    obs = [{int(k): int(g - kf_off[k]) for k, g in zip(kf[obs_off[p]:obs_off[p + 1]], obs_gkp[obs_off[p]:obs_off[p + 1]])}
           for p in range(len(mp_bad))]
    kps = [np.zeros(c, KEYPOINT_DTYPE) for c in n]
    return LoopMap(None, kps, [rng.integers(0, 256, (c, 32), dtype=np.uint8) for c in n],
                   [slots[kf_off[k]:kf_off[k + 1]] for k in range(nkf)], np.zeros(len(mp_bad), MAP_POINT_DTYPE),
                   rng.integers(0, 256, (len(mp_bad), 32), dtype=np.uint8), mp_bad=mp_bad, observations=obs, **kw)


def keep_descriptors(desc, offsets, current):
    """A ``distinctive`` for the walks: the descriptors stay (the tables hold none)."""
    return None, current


def random_walk(m, steps, seed, flush=None, flush_p=0.06):
    """``steps`` random calls of the LoopMap mutators that write what the flat
    tables hold: add_observation, add_map_point, erase_map_point_match,
    erase_observation, set_bad_point, replace, set_bad_keyframe, new_map_point
    with its observations, and add_keyframe followed by its observations.
    ``flush()`` is called at random points and at the end. -> calls per kind."""
    rng = np.random.default_rng(seed)
    done = {}
    kinds = ("add_observation", "add_map_point", "erase_map_point_match", "erase_observation", "set_bad_point",
             "replace", "set_bad_keyframe", "new_map_point", "add_keyframe")
    weights = np.asarray([24, 10, 10, 16, 5, 10, 1, 14, 3], float)

    def some_kp():
        sized = [k for k in range(m.nkf) if len(m.kf_kps[k])]
        k = int(rng.choice(sized))
        return k, int(rng.integers(0, len(m.kf_kps[k])))

    for _ in range(steps):
        kind = str(rng.choice(kinds, p=weights / weights.sum()))
        done[kind] = done.get(kind, 0) + 1
        nmp = len(m.mps)
        p = int(rng.integers(0, nmp))
        if kind == "add_observation":
            m.add_observation(p, *some_kp())
        elif kind == "add_map_point":
            k, i = some_kp()
            m.add_map_point(k, p, i)
        elif kind == "erase_map_point_match":
            m.erase_map_point_match(*some_kp())
        elif kind == "erase_observation":
            held = sorted(m.obs[p])
            m.erase_observation(p, int(rng.choice(held)) if held and rng.random() < 0.8 else some_kp()[0])
        elif kind == "set_bad_point":
            m.set_bad_point(p)
        elif kind == "replace":
            m.replace(p, int(rng.integers(0, nmp)))
        elif kind == "set_bad_keyframe":
            m.set_bad_keyframe(int(rng.integers(0, m.nkf)))
        elif kind == "new_map_point":
            q = m.new_map_point(rng.normal(size=3), some_kp()[0])
            for _ in range(int(rng.integers(0, 4))):
                k, i = some_kp()
                m.add_observation(q, k, i)
                m.add_map_point(k, q, i)
        else:
            n = int(rng.integers(0, 40))
            slots = rng.integers(-1, nmp, n).astype(np.int32)
            kps = np.zeros(n, KEYPOINT_DTYPE)
            kps["octave"] = rng.integers(0, 8, n)
            kps["x"], kps["y"] = rng.random(n) * 600, rng.random(n) * 400
            k = m.add_keyframe(kps, rng.integers(0, 256, (n, 32), dtype=np.uint8), slots, np.eye(4, dtype=np.float32))
            for i in np.nonzero(slots >= 0)[0]:
                if rng.random() < 0.8:
                    m.add_observation(int(slots[i]), k, int(i))
        if flush is not None and rng.random() < flush_p:
            flush()
    if flush is not None:
        flush()
    return done


def assert_same_report(x, y, path=()):
    """Two stage reports equal field by field, arrays bit for bit; the host
    clock figures (``times``, ``seconds``) apart."""
    if isinstance(x, dict):
        assert set(x) == set(y), path
        for k in x:
            if k not in ("times", "seconds"):
                assert_same_report(x[k], y[k], path + (k,))
    elif isinstance(x, (list, tuple)) and len(x) and isinstance(x[0], (dict, list, tuple, np.ndarray)):
        assert len(x) == len(y), path
        for i, (u, v) in enumerate(zip(x, y)):
            assert_same_report(u, v, path + (i,))
    elif isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), path
    else:
        assert x == y, path
