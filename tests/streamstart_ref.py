"""Serial NumPy restatement of gf_frontend_start_streams: a start request and
what the stream held before -> every field the stream must hold afterwards.

``before`` / the result are dicts of one stream's arrays, named as
``pipeline.FIELDS`` names them (whole rows: [cap] or [M] first axis), plus
``graph`` (the dict ``FrontEnd.covis`` returns), ``kf`` ({word: int} of the
GF_KF_* words, or None without the keyframe stage) and ``nleft`` (GF_ST_NLEFT).
Rows past the new counts keep their bytes; fields the call does not touch
(mp_H, mp_info, mp_uv, velocity, rng, the current frame's keypoints) are not in
the result's ``written`` set."""
import numpy as np

from gf_orb_slam_amd.pipeline import TR

# fields of ``before`` the start rewrites (wholly or on [0, count))
MAP_ROWS = ("map", "map_desc", "views", "mp_upd")
LAST_ROWS = ("last_kps", "last_desc", "last_kp2mp", "last_outlier", "last_pos")
WRITTEN = MAP_ROWS + LAST_ROWS + ("nmp", "last_nkp", "Tcw_last", "t_prev", "t_cur", "kp2mp", "outlier", "track", "Xv",
                                  "Xv_next", "base", "reloc")
UNTOUCHED = ("mp_H", "mp_info", "mp_uv", "velocity", "rng", "kps", "desc", "nkp", "score", "Tcw", "left", "hist")


def graph_of_delta(d) -> dict:
    """The gf_covis_map arrays of a delta read against the empty map, item by item."""
    n, nkf = len(d.new_mp), len(d.new_kf_off) - 1
    kf_mp_off = np.zeros(nkf + 1, np.int32)
    kf_mp = []
    for k in range(nkf):
        row = d.new_kf_mp[d.new_kf_off[k]:d.new_kf_off[k + 1]]
        kf_mp.extend(int(v) for v in row)
        kf_mp_off[k + 1] = len(kf_mp)
    rows = {int(p): d.obs_kf[d.obs_off[r]:d.obs_off[r + 1]] for r, p in enumerate(d.obs_mp)}
    mp_obs_off = np.zeros(n + 1, np.int32)
    mp_obs = []
    for p in range(n):
        mp_obs.extend(int(v) for v in rows.get(p, ()))
        mp_obs_off[p + 1] = len(mp_obs)
    kf_cov_off = np.zeros(nkf + 1, np.int32)
    kf_cov = np.zeros(0, np.int32)
    if d.has_cov:
        kf_cov_off = np.asarray(d.kf_cov_off, np.int32).copy()
        kf_cov = np.asarray(d.kf_cov, np.int32).copy()
    return dict(kf_bad=np.asarray(d.new_kf_bad, np.uint8).copy(), kf_mp_off=kf_mp_off, kf_mp=np.asarray(kf_mp, np.int32),
                kf_cov_off=kf_cov_off, kf_cov=kf_cov, mp_bad=np.asarray(d.new_mp_bad, np.uint8).copy(),
                mp_obs_off=mp_obs_off, mp_obs=np.asarray(mp_obs, np.int32))


def start(before: dict, req) -> dict:
    """The stream after ``req`` (a localmap.StreamStart)."""
    d = req.map
    out = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    n, nl = len(d.new_mp), len(req.kps)
    # the map alone, with the per-point state of fresh points
    out["nmp"] = np.int32(n)
    for p in range(n):
        out["map"][p] = d.new_mp[p]
        out["map_desc"][p] = d.new_mp_desc[p]
        out["mp_upd"][p] = -1000
    out["views"][:n].view(np.uint8)[...] = 0
    out["graph"] = graph_of_delta(d)
    # the last frame
    out["last_nkp"] = np.int32(nl)
    for i in range(nl):
        out["last_kps"][i] = req.kps[i]
        out["last_desc"][i] = req.desc[i]
        mp = int(req.kp2mp[i])
        out["last_kp2mp"][i] = mp
        out["last_outlier"][i] = 0
        out["last_pos"][i] = d.new_mp["pos"][mp] if mp >= 0 else 0.0
    out["Tcw_last"] = np.asarray(req.Tcw, np.float32).reshape(16).copy()
    out["t_prev"] = np.float64(req.timestamp)
    out["t_cur"] = np.float64(req.timestamp)
    out["kp2mp"][:] = -1
    out["outlier"][:] = 0
    out["nleft"] = 0
    # the tracking words
    t = out["track"]
    t[TR["state"]], t[TR["vel"]], t[TR["since"]] = 0, 0, min(req.since_reloc, 1 << 30)
    t[TR["path"]], t[TR["query"]], t[TR["ok"]] = 2, req.frame_id, 1
    # the keyframe words
    if before.get("kf") is not None:
        out["kf"] = dict(before["kf"], since=0, pending=0, abort=0, decision=0, ref=req.ref_kf)
    # the observability state, the relocalisation query state
    for k in ("Xv", "Xv_next", "base"):
        out[k][:] = 0.0
    out["reloc"].view(np.uint8)[...] = 0
    return out


def database(req, transform_rows=None):
    """(kps, desc) lists of the keyframes the stream's database then holds: the request's rows, or nothing."""
    r = req.kf_rows
    if r is None:
        return [], []
    kps = [r.kps[r.kp_off[k]:r.kp_off[k + 1]] for k in range(r.nkf)]
    desc = [r.desc[r.kp_off[k]:r.kp_off[k + 1]] for k in range(r.nkf)]
    return kps, desc


def verdict(req, cap: int, M: int, named=(), nstreams=None, has_graph=True, db=None, slot_cap=None) -> int:
    """The error code gf_frontend_start_streams answers for one request (0,
    -1 GF_ERR_ARG, -3 GF_ERR_CAP, -4 GF_ERR_UNSUPPORTED), checks in the
    library's order. named: the streams the call's earlier requests name; db:
    None, "fixed", or (max_kf, max_rows) of a growable database."""
    d, b = req.map, req.stream
    slot_cap = 64 * cap if slot_cap is None else slot_cap
    if b < 0 or (nstreams is not None and b >= nstreams) or b in named:
        return -1
    if len(d.set_mp_idx) or len(d.bad_mp) or len(d.bad_kf) or len(d.slot_kf):
        return -1
    if len(req.kps) > cap:
        return -3
    n, nkf = len(d.new_mp), len(d.new_kf_off) - 1
    if np.any(req.kp2mp < -1) or np.any(req.kp2mp >= n):
        return -1
    if (nkf > 0 and not 0 <= req.ref_kf < nkf) or (nkf == 0 and req.ref_kf != -1):
        return -1
    if req.frame_id < 0 or req.since_reloc < 0:
        return -1
    if db == "fixed":
        return -4
    if not has_graph:
        return -1
    if n > M or nkf > 64:
        return -3
    koff = np.asarray(d.new_kf_off, np.int64)
    rows = req.kf_rows
    if rows is not None and (db is None or nkf == 0):
        return -1
    if nkf and db is not None and rows is None:
        return -4
    if rows is not None:
        if rows.nkf != nkf:
            return -1
        if rows.nkf > db[0] or len(rows.kps) > db[1]:
            return -3
    if nkf and (koff[0] != 0 or np.any(np.diff(koff) < 0)):
        return -1
    if rows is not None and np.any(np.diff(rows.kp_off) != np.diff(koff)):
        return -1
    nslots = int(koff[nkf]) if nkf else 0
    if nslots > slot_cap:
        return -3
    if np.any(d.new_kf_mp[:nslots] < -1) or np.any(d.new_kf_mp[:nslots] >= n):
        return -1
    seen, nobs = set(), 0
    for r, p in enumerate(d.obs_mp):
        row = d.obs_kf[d.obs_off[r]:d.obs_off[r + 1]]
        if not 0 <= p < n or int(p) in seen or d.obs_off[r] > d.obs_off[r + 1]:
            return -1
        if np.any(row < 0) or np.any(row >= nkf) or np.any(np.diff(row) <= 0):
            return -1
        seen.add(int(p))
        nobs += len(row)
    if nobs > slot_cap:
        return -3
    if d.has_cov:
        coff = np.asarray(d.kf_cov_off, np.int64)
        if coff[0] != 0 or np.any(np.diff(coff[:nkf + 1]) < 0):
            return -1
        if coff[nkf] > nkf * nkf:
            return -3
        if np.any(d.kf_cov[:coff[nkf]] < 0) or np.any(d.kf_cov[:coff[nkf]] >= nkf):
            return -1
    return 0
