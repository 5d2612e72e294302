"""Maps and deltas for the map-feedback tests (tests/test_mapupdate_cpu.py,
tests/test_mapupdate_gpu.py).

A map here is ``dict(mp, desc, graph)``: MAP_POINT_DTYPE rows, [n, 32]
descriptors and the compact ``gf_covis_map`` arrays. :func:`random_map` draws
one, :func:`evolve` draws the map a mapper pass could leave behind it (points
and keyframes appended, points rewritten and turned bad, slots written,
observation rows replaced, covisibility lists reordered), and :func:`diff`
states the delta between two maps with plain loops, independently of
``tracking.MapFeedback``'s vectorised one."""
from __future__ import annotations

import numpy as np

from gf_orb_slam_amd.localmap import MapDelta
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE

SENTINEL = 0xA5


def csr(rows):
    off = np.zeros(len(rows) + 1, np.int32)
    if len(rows):
        off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, np.int32).reshape(-1) for r in rows]) if len(rows) else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)


def rows_of(off, flat):
    return [np.asarray(flat[off[i]:off[i + 1]], np.int32) for i in range(len(off) - 1)]


def points(rng, n):
    mp = np.zeros(n, MAP_POINT_DTYPE)
    mp["pos"] = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    mp["normal"] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    mp["min_dist"] = rng.uniform(0.5, 2, n).astype(np.float32)
    mp["max_dist"] = rng.uniform(5, 20, n).astype(np.float32)
    return mp, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def graph_of(kf_rows, kf_bad, cov_rows, mp_bad, obs_rows):
    kf_mp_off, kf_mp = csr(kf_rows)
    kf_cov_off, kf_cov = csr(cov_rows)
    mp_obs_off, mp_obs = csr(obs_rows)
    return dict(kf_bad=np.asarray(kf_bad, np.uint8), kf_mp_off=kf_mp_off, kf_mp=kf_mp, kf_cov_off=kf_cov_off,
                kf_cov=kf_cov, mp_bad=np.asarray(mp_bad, np.uint8), mp_obs_off=mp_obs_off, mp_obs=mp_obs)


def _obs_row(rng, nkf, most):
    return np.sort(rng.choice(nkf, int(rng.integers(0, min(most, nkf) + 1)), replace=False)).astype(np.int32)


def random_map(seed, nmp, nkf, slots=(0, 40), obs_most=4, odd_offsets=False):
    """``nmp`` points, ``nkf`` keyframes of slots[0] .. slots[1] slots each
    (odd_offsets: every row length odd, so that rows start at odd and even
    offsets), observation rows of up to obs_most random keyframes (rows and
    slots are separate state, as in the reference), random covisibility lists."""
    rng = np.random.default_rng(seed)
    mp, desc = points(rng, nmp)
    kf_rows = []
    for _ in range(nkf):
        n = int(rng.integers(slots[0], slots[1] + 1))
        if odd_offsets:
            n |= 1
        kf_rows.append(rng.integers(-1, max(nmp, 0), n).astype(np.int32) if nmp else np.full(n, -1, np.int32))
    cov = [rng.permutation(nkf)[:int(rng.integers(0, min(nkf, 12) + 1))].astype(np.int32) for _ in range(nkf)]
    obs = [_obs_row(rng, nkf, obs_most) if nkf else np.zeros(0, np.int32) for _ in range(nmp)]
    g = graph_of(kf_rows, rng.random(nkf) < 0.1, cov, rng.random(nmp) < 0.1, obs)
    return dict(mp=mp, desc=desc, graph=g)


def evolve(seed, m0, new_mp=0, new_kf=0, new_kf_slots=(0, 40), rewrite=0, bad_mp=0, bad_kf=0, slot_writes=0,
           obs="some", cov=True, obs_most=4):
    """The map after a mapper pass on ``m0``. obs: "none" (no old row changes;
    appended points get no row), "some" (a tenth of the rows), "all", "grow"
    (empty rows get entries), "shrink" (rows become empty), "ends" (the first
    and the last point's rows), or an int: exactly that many observations in
    total afterwards, made by refilling the first rows."""
    rng = np.random.default_rng(seed)
    g0 = m0["graph"]
    n0, k0 = len(m0["mp"]), len(g0["kf_bad"])
    n1, k1 = n0 + new_mp, k0 + new_kf
    mp, desc = m0["mp"].copy(), m0["desc"].copy()
    a, b = points(rng, new_mp)
    mp, desc = np.concatenate([mp, a]), np.concatenate([desc, b])
    for p in rng.choice(n0, min(rewrite, n0), replace=False) if n0 else []:
        mp["pos"][p] += rng.normal(0, 0.01, 3).astype(np.float32)
        mp["min_dist"][p] *= np.float32(1.01)
        desc[p] ^= rng.integers(0, 256, 32, dtype=np.uint8)
    mp_bad = np.concatenate([g0["mp_bad"].astype(bool), rng.random(new_mp) < 0.1])
    kf_bad = np.concatenate([g0["kf_bad"].astype(bool), rng.random(new_kf) < 0.1])
    if n1 and bad_mp:
        mp_bad[rng.choice(n1, min(bad_mp, n1), replace=False)] = True
    if k1 and bad_kf:
        kf_bad[rng.choice(k1, min(bad_kf, k1), replace=False)] = True
    kf_rows = [r.copy() for r in rows_of(g0["kf_mp_off"], g0["kf_mp"])]
    where = [(k, i) for k, r in enumerate(kf_rows) for i in range(len(r))]
    for j in rng.choice(len(where), min(slot_writes, len(where)), replace=False) if where else []:
        k, i = where[j]
        v = int(rng.integers(-1, n1)) if n1 else -1
        kf_rows[k][i] = v if v != kf_rows[k][i] else (-1 if v != -1 else (0 if n1 else -1))
    for _ in range(new_kf):
        n = int(rng.integers(new_kf_slots[0], new_kf_slots[1] + 1))
        kf_rows.append(rng.integers(-1, n1, n).astype(np.int32) if n1 else np.full(n, -1, np.int32))
    obs_rows = [r.copy() for r in rows_of(g0["mp_obs_off"], g0["mp_obs"])] + [np.zeros(0, np.int32)] * new_mp
    fresh = lambda: _obs_row(rng, k1, obs_most) if k1 else np.zeros(0, np.int32)  # noqa: E731
    if obs == "some":
        for p in rng.choice(n1, (n1 + 9) // 10, replace=False) if n1 else []:
            obs_rows[p] = fresh()
    elif obs == "all":
        obs_rows = [np.sort(rng.choice(k1, int(rng.integers(1, min(obs_most, k1) + 1)), replace=False)).astype(np.int32)
                    if k1 else np.zeros(0, np.int32) for _ in range(n1)]
        for p in range(min(n0, len(obs_rows))):  # every old row really differs
            if k1 and np.array_equal(obs_rows[p], rows_of(g0["mp_obs_off"], g0["mp_obs"])[p]):
                obs_rows[p] = np.asarray([(int(obs_rows[p][0]) + 1) % k1], np.int32)
    elif obs == "grow":
        for p in range(n1):
            if not len(obs_rows[p]) and k1:
                obs_rows[p] = np.sort(rng.choice(k1, min(2, k1), replace=False)).astype(np.int32)
    elif obs == "shrink":
        for p in range(0, n1, 2):
            obs_rows[p] = np.zeros(0, np.int32)
    elif obs == "ends":
        for p in {0, n1 - 1} if n1 else ():
            obs_rows[p] = np.asarray([k1 - 1], np.int32) if k1 and not np.array_equal(obs_rows[p], [k1 - 1]) \
                else np.zeros(0, np.int32)
    elif isinstance(obs, int):
        total, p = sum(len(r) for r in obs_rows), 0
        while total != obs:
            assert p < n1 and k1, "cannot reach the observation total"
            want = min(k1, max(0, len(obs_rows[p]) + obs - total))
            total += want - len(obs_rows[p])
            obs_rows[p] = np.arange(want, dtype=np.int32)
            p += 1
    cov_rows = rows_of(g0["kf_cov_off"], g0["kf_cov"]) + [np.zeros(0, np.int32)] * new_kf
    if cov:
        cov_rows = [rng.permutation(k1)[:int(rng.integers(0, min(k1, 12) + 1))].astype(np.int32) for _ in range(k1)]
    return dict(mp=mp, desc=desc, graph=graph_of(kf_rows, kf_bad, cov_rows, mp_bad, obs_rows))


def diff(stream, m0, m1) -> MapDelta:
    """The delta m0 -> m1, item by item."""
    g0, g1 = m0["graph"], m1["graph"]
    n0, n1, k0, k1 = len(m0["mp"]), len(m1["mp"]), len(g0["kf_bad"]), len(g1["kf_bad"])
    ch = [p for p in range(n0) if m0["mp"][p].tobytes() != m1["mp"][p].tobytes() or
          not np.array_equal(m0["desc"][p], m1["desc"][p])]
    bad_mp = [p for p in range(n0) if g1["mp_bad"][p] and not g0["mp_bad"][p]]
    bad_kf = [k for k in range(k0) if g1["kf_bad"][k] and not g0["kf_bad"][k]]
    r0, r1 = rows_of(g0["kf_mp_off"], g0["kf_mp"]), rows_of(g1["kf_mp_off"], g1["kf_mp"])
    sk, si, sv = [], [], []
    for k in range(k0):
        assert len(r0[k]) == len(r1[k])
        for i in np.nonzero(r0[k] != r1[k])[0]:
            sk.append(k), si.append(int(i)), sv.append(int(r1[k][i]))
    o0, o1 = rows_of(g0["mp_obs_off"], g0["mp_obs"]), rows_of(g1["mp_obs_off"], g1["mp_obs"])
    obs = {p: o1[p] for p in range(n1) if (p < n0 and not np.array_equal(o0[p], o1[p])) or (p >= n0 and len(o1[p]))}
    c0, c1 = rows_of(g0["kf_cov_off"], g0["kf_cov"]), rows_of(g1["kf_cov_off"], g1["kf_cov"])
    same = all(np.array_equal(a, b) for a, b in zip(c0, c1[:k0])) and not any(len(c) for c in c1[k0:])
    ch = np.asarray(ch, np.int64)
    return MapDelta(stream, new_mp=m1["mp"][n0:], new_mp_desc=m1["desc"][n0:], new_mp_bad=g1["mp_bad"][n0:],
                    set_mp_idx=ch, set_mp=m1["mp"][ch], set_mp_desc=m1["desc"][ch], bad_mp=bad_mp, new_kf=r1[k0:],
                    new_kf_bad=g1["kf_bad"][k0:], bad_kf=bad_kf, slot_kf=sk, slot_idx=si, slot_val=sv, obs_rows=obs,
                    kf_cov=None if same else c1)


def map_of_state(st) -> dict:
    """The compact map of a ``mapupdate_ref.State``."""
    n = st.nmp
    return dict(mp=st.map[:n].copy(), desc=st.desc[:n].copy(), graph=st.graph())


def same_map(a, b) -> list:
    """What differs between two compact maps (byte equality)."""
    import mapupdate_ref as R

    out = R.same_graph(a["graph"], b["graph"])
    if a["mp"].tobytes() != b["mp"].tobytes():
        out.append("mp")
    if not np.array_equal(a["desc"], b["desc"]):
        out.append("desc")
    return out
