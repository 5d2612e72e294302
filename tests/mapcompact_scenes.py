"""Maps, states and drop lists for the map-compaction tests
(tests/test_mapcompact_cpu.py, tests/test_mapcompact_gpu.py).

A map is ``dict(mp, desc, graph)`` as in mapupdate_scenes. :func:`restrict`
builds the map of the kept items from scratch with plain loops, independently
of the restatement and of the kernels; :func:`drops` names the drop patterns
the kernels can go wrong at; :func:`state_of_map` wraps a map and random
per-point state into a ``mapcompact_ref.State``."""
from __future__ import annotations

import numpy as np

import mapcompact_ref as R
import mapupdate_scenes as S

SENTINEL = S.SENTINEL


def restrict(m, keep_kf, keep_mp):
    """The map of the kept keyframes and points (boolean masks), renumbered in
    order, built item by item."""
    g = m["graph"]
    keep_kf, keep_mp = np.asarray(keep_kf, bool), np.asarray(keep_mp, bool)
    new_kf = np.full(len(keep_kf), -1, np.int64)
    new_kf[keep_kf] = np.arange(int(keep_kf.sum()))
    new_mp = np.full(len(keep_mp), -1, np.int64)
    new_mp[keep_mp] = np.arange(int(keep_mp.sum()))
    kf_rows, cov_rows, obs_rows = [], [], []
    slots, cov, obs = (S.rows_of(g["kf_mp_off"], g["kf_mp"]), S.rows_of(g["kf_cov_off"], g["kf_cov"]),
                       S.rows_of(g["mp_obs_off"], g["mp_obs"]))
    for k in range(len(keep_kf)):
        if keep_kf[k]:
            kf_rows.append([int(new_mp[v]) if v >= 0 else -1 for v in slots[k]])
            cov_rows.append([int(new_kf[c]) for c in cov[k] if keep_kf[c]])
    for p in range(len(keep_mp)):
        if keep_mp[p]:
            obs_rows.append([int(new_kf[k]) for k in obs[p] if keep_kf[k]])
    graph = S.graph_of(kf_rows, np.asarray(g["kf_bad"])[keep_kf], cov_rows, np.asarray(g["mp_bad"])[keep_mp], obs_rows)
    return dict(mp=m["mp"][keep_mp].copy(), desc=m["desc"][keep_mp].copy(), graph=graph), new_kf, new_mp


def drops(pattern, n, rng=None):
    """Indices of 0 .. n-1 to drop: "first", "last", "none", "alternate",
    "all", "random"."""
    if n == 0 or pattern == "none":
        return np.zeros(0, np.int32)
    pick = {"first": [0], "last": [n - 1], "alternate": np.arange(0, n, 2), "all": np.arange(n)}
    if pattern == "random":
        return np.nonzero(rng.random(n) < 0.4)[0].astype(np.int32)
    return np.asarray(pick[pattern], np.int32)


POINT_ROWS = (("map", None), ("map_desc", None), ("views", 20), ("mp_H", 112), ("mp_info", 392), ("mp_uv", 8),
              ("mp_upd", 4))


def state_of_map(seed, m, M, cap, holders=True, nkp=None):
    """A State over the map with random bytes in every per-point row (so that
    a row that moved wrongly shows), sentinels past the used rows, and frame
    state that holds random points (holders=False: nothing is pinned)."""
    rng = np.random.default_rng(seed)
    n = len(m["mp"])
    rows = {}
    for name, width in POINT_ROWS:
        if name == "map":
            a = np.zeros(M, m["mp"].dtype)
            a[:n] = m["mp"]
        elif name == "map_desc":
            a = np.zeros((M, 32), np.uint8)
            a[:n] = m["desc"]
        else:
            a = np.zeros((M, width), np.uint8)
            a[:n] = rng.integers(0, 256, (n, width), dtype=np.uint8)
        a[n:].view(np.uint8)[...] = SENTINEL
        rows[name] = a
    reloc = rng.integers(0, 256, (R.KC, 12), dtype=np.uint8)
    h = {}
    if holders and n:
        nk = int(rng.integers(cap // 2, cap + 1)) if nkp is None else nkp
        h = dict(kp2mp=np.where(rng.random(cap) < 0.3, rng.integers(0, n, cap), -1), nkp=nk,
                 last_kp2mp=np.where(rng.random(cap) < 0.3, rng.integers(0, n, cap), -1),
                 last_nkp=int(rng.integers(0, cap + 1)), left=rng.integers(0, n, M), nleft=int(rng.integers(0, n + 1)))
    return R.State(M, cap, m["graph"], point_rows=rows, kf_rows=dict(reloc=reloc), tail=SENTINEL, **h)


def map_of_state(st) -> dict:
    n = st.nmp
    return dict(mp=st.point_rows["map"][:n].copy(), desc=st.point_rows["map_desc"][:n].copy(), graph=st.graph())
