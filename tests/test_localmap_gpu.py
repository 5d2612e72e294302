"""GPU parity of CreateNewMapPoints with its CPU restatement
(tests/helpers/localmap_ref.cpp): gf_create_new_map_points and its device
family bit for bit (per-neighbour report, every match's exit, every new
point, the final slot tables), the capacity and empty cases, the 4096-keypoint
size case, and localmapping.create_new_map_points on a LoopMap against the
restatement's world."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import localmap_ref as R
import localmap_scenes as S
from gf_orb_slam_amd import localmapping as LM
from gf_orb_slam_amd._lib import GFError, check, lib, ptr
from gf_orb_slam_amd.loopmap import LoopMap
from gf_orb_slam_amd.orb import default_context

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def world(check_ori=False):
    sc = S.scene(3)
    return sc, R.create_new_map_points(sc, chain=1, check_ori=check_ori)


@functools.lru_cache(maxsize=None)
def big_world():
    sc = S.big_scene()
    return sc, R.create_new_map_points(sc, chain=1)


def host_keyframes(sc, slots):
    kf = lambda k: (sc["Tcw"][k], sc["fv"][k], sc["desc"][k], sc["kps"][k], slots[k])  # noqa: E731
    return kf(sc["cur"]), [kf(k) for k in sc["neighbours"]]


def assert_same(sc, ref, rep, pts, exits, slots):
    assert np.array_equal(rep["status"], ref["status"])
    assert rep["F12"].reshape(-1, 3, 3).tobytes() == ref["F12"].tobytes()
    assert rep["median_depth"].tobytes() == ref["median"].tobytes()
    assert np.array_equal(rep["nmatches"], ref["nmatches"]) and np.array_equal(rep["naccepted"], ref["naccepted"])
    assert np.array_equal(exits, ref["exits"])
    assert pts.dtype == ref["points"].dtype and len(pts) == len(ref["points"])
    assert np.array_equal(pts[["neighbour", "idx1", "idx2"]], ref["points"][["neighbour", "idx1", "idx2"]])
    assert pts["pos"].tobytes() == ref["points"]["pos"].tobytes()
    assert pts.tobytes() == ref["points"].tobytes()
    for k in range(len(slots)):
        assert np.array_equal(slots[k], ref["slots"][k]), k


@pytest.mark.parametrize("check_ori", [False, True])
def test_host_entry_bit_exact(check_ori):
    """gf_create_new_map_points on the scene against the restatement."""
    sc, ref = world(check_ori)
    slots = [s.copy() for s in sc["slots"]]
    cur, neigh = host_keyframes(sc, slots)
    rep, pts, exits = LM.create_new_map_points_arrays(sc["info"], cur, neigh, sc["mps"]["pos"], check_ori)
    assert_same(sc, ref, rep, pts, exits, slots)


def device_call(sc, check_ori=False, cap=None, neighbours=None, pad=7):
    """gf_create_new_map_points_dev with sentinel-filled outputs, `pad`
    entries longer than needed -> (report, points, exits, total, slots) as
    host arrays, tails included."""
    import torch

    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    nb = sc["neighbours"] if neighbours is None else neighbours
    keep = []

    def kf(k):
        fv = sc["fv"][k]
        bufs = [t(fv.nodes), t(fv.start), t(fv.feats), t(sc["desc"][k]), t(sc["kps"][k].view(np.uint8)),
                t(sc["slots"][k])]
        keep.append(bufs)
        return LM.NewPointsKf.make(sc["Tcw"][k], bufs, len(fv.nodes), len(sc["desc"][k])), bufs[5]

    cur, cur_slots = kf(sc["cur"])
    arr = (LM.NewPointsKf * max(len(nb), 1))()
    nslots = []
    for i, k in enumerate(nb):
        arr[i], s = kf(k)
        nslots.append(s)
    n1 = cur.side.n
    cap = n1 if cap is None else cap
    sent = lambda nbytes: torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)  # noqa: E731
    d_rep = sent((len(nb) + pad) * LM.NEIGH_DTYPE.itemsize)
    d_pts = sent((cap + pad) * LM.NEWPOINT_DTYPE.itemsize)
    d_ex = sent((len(nb) + pad) * n1 * 4)
    d_tot = sent(4 * (1 + pad))
    pos = t(sc["mps"]["pos"])
    ctx = default_context()
    check(lib().gf_create_new_map_points_dev(ctx.handle, ctypes.byref(sc["info"]), ctypes.byref(cur), len(nb), arr,
                                             ptr(pos), len(sc["mps"]), int(check_ori), cap, ptr(d_rep), ptr(d_pts),
                                             ptr(d_ex), ptr(d_tot), ctx.stream))
    check(lib().gf_ctx_sync(ctx.handle))
    h = lambda x, dt: x.cpu().numpy().view(dt)  # noqa: E731
    slots = {sc["cur"]: cur_slots.cpu().numpy()}
    slots.update({k: s.cpu().numpy() for k, s in zip(nb, nslots)})
    return (h(d_rep, LM.NEIGH_DTYPE), h(d_pts, LM.NEWPOINT_DTYPE), h(d_ex, np.int32).reshape(-1, n1),
            h(d_tot, np.int32), slots)


SENT32 = np.int32(0x5A5A5A5A)


def test_dev_entry_same_bytes_and_tails_untouched():
    """The _dev entry gives the bytes of the host entry and leaves the
    sentinel-filled tails of its output buffers alone."""
    sc, ref = world()
    nn, n1 = len(sc["neighbours"]), len(sc["kps"][sc["cur"]])
    rep, pts, exits, tot, slots = device_call(sc)
    total = int(tot[0])
    assert total == len(ref["points"]) and np.all(tot[1:] == SENT32)
    assert_same(sc, ref, rep[:nn], pts[:total], exits[:nn], [slots[k] for k in range(len(sc["slots"]))])
    assert np.all(rep[nn:].view(np.int32) == SENT32)
    assert np.all(pts[total:].view(np.int32) == SENT32)
    assert np.all(exits[nn:] == SENT32)
    # and the host entry returns the same bytes
    hs = [s.copy() for s in sc["slots"]]
    cur, neigh = host_keyframes(sc, hs)
    hrep, hpts, hexits = LM.create_new_map_points_arrays(sc["info"], cur, neigh, sc["mps"]["pos"])
    assert hrep.tobytes() == rep[:nn].tobytes() and hpts.tobytes() == pts[:total].tobytes()
    assert hexits.tobytes() == exits[:nn].tobytes()
    # the host entry, too, writes its caller's record buffer only as far as the records go
    hs = [s.copy() for s in sc["slots"]]
    cur, neigh = host_keyframes(sc, hs)
    c, keep = LM.host_keyframe(*cur)
    arr = (LM.NewPointsKf * nn)()
    for i, k in enumerate(neigh):
        arr[i], kk = LM.host_keyframe(*k)
        keep.append(kk)
    pos = np.ascontiguousarray(sc["mps"]["pos"], np.float32)
    b_rep = np.full((nn + 3) * LM.NEIGH_DTYPE.itemsize // 4, SENT32, np.int32)
    b_pts = np.full((n1 + 3) * LM.NEWPOINT_DTYPE.itemsize // 4, SENT32, np.int32)
    b_ex = np.full((nn + 3) * n1, SENT32, np.int32)
    htot = ctypes.c_int()
    check(lib().gf_create_new_map_points(default_context().handle, ctypes.byref(sc["info"]), ctypes.byref(c), nn, arr,
                                         ptr(pos), len(pos), 0, n1, ptr(b_rep), ptr(b_pts), ptr(b_ex),
                                         ctypes.byref(htot)))
    assert htot.value == total
    assert b_pts.view(LM.NEWPOINT_DTYPE)[:total].tobytes() == pts[:total].tobytes()
    assert np.all(b_pts.view(LM.NEWPOINT_DTYPE)[total:].view(np.int32) == SENT32)
    assert np.all(b_rep.view(LM.NEIGH_DTYPE)[nn:].view(np.int32) == SENT32) and np.all(b_ex[nn * n1:] == SENT32)


def test_cap_one_below_total():
    """cap = total - 1: the host entry returns GF_ERR_CAP and leaves the
    caller's slot tables alone; the device entry drops the last record,
    reports the full total and writes nothing past cap."""
    sc, ref = world()
    total = len(ref["points"])
    slots = [s.copy() for s in sc["slots"]]
    cur, neigh = host_keyframes(sc, slots)
    with pytest.raises(GFError) as e:
        LM.create_new_map_points_arrays(sc["info"], cur, neigh, sc["mps"]["pos"], cap=total - 1)
    assert e.value.code == -3
    for a, b in zip(slots, sc["slots"]):
        assert np.array_equal(a, b)
    _, pts, _, tot, dslots = device_call(sc, cap=total - 1)
    assert int(tot[0]) == total
    assert pts[:total - 1].tobytes() == ref["points"][:total - 1].tobytes()
    assert np.all(pts[total - 1:].view(np.int32) == SENT32)
    assert np.array_equal(dslots[sc["cur"]], ref["slots"][sc["cur"]])  # the chain itself does not depend on cap


def test_no_neighbours():
    """nneigh = 0: zero points, nothing touched."""
    sc, _ = world()
    slots = [s.copy() for s in sc["slots"]]
    cur, _ = host_keyframes(sc, slots)
    rep, pts, exits = LM.create_new_map_points_arrays(sc["info"], cur, [], sc["mps"]["pos"])
    assert len(rep) == 0 and len(pts) == 0 and exits.shape[0] == 0
    assert np.array_equal(slots[sc["cur"]], sc["slots"][sc["cur"]])
    rep, pts, exits, tot, dslots = device_call(sc, neighbours=[])
    assert int(tot[0]) == 0 and np.all(tot[1:] == SENT32)
    assert np.all(rep.view(np.int32) == SENT32) and np.all(pts.view(np.int32) == SENT32) and np.all(exits == SENT32)
    assert np.array_equal(dslots[sc["cur"]], sc["slots"][sc["cur"]])


def test_size_case_4096_keypoints():
    """Both keyframes of every pair at the 4096-keypoint limit, two
    neighbours: the median select and the compaction scan at full width, more
    than one match per lane."""
    sc, ref = big_world()
    assert len(sc["kps"][sc["cur"]]) == 4096 and all(len(sc["kps"][k]) == 4096 for k in sc["neighbours"])
    assert ref["nmatches"].max() > 1024 and (sc["slots"][0] >= 0).sum() > 2048
    slots = [s.copy() for s in sc["slots"]]
    cur, neigh = host_keyframes(sc, slots)
    rep, pts, exits = LM.create_new_map_points_arrays(sc["info"], cur, neigh, sc["mps"]["pos"])
    assert_same(sc, ref, rep, pts, exits, slots)


def loop_map(sc):
    m = LoopMap(sc["info"], sc["kps"], sc["desc"], sc["slots"], sc["mps"], sc["mp_desc"], observations=sc["obs"],
                kf_Tcw=sc["Tcw"], ref_kf=sc["ref_kf"])
    m.ordered[sc["cur"]] = list(sc["neighbours"])
    return m


def test_loopmap_against_the_restatements_world():
    """localmapping.create_new_map_points on a LoopMap: slot tables,
    observation rows, descriptors, position / normal / distances of the new
    points and the recent list equal the restatement's; a second call creates
    nothing from an already triangulated keypoint."""
    sc, ref = world()
    want = R.bookkeeping(sc, ref)
    m = loop_map(sc)
    nmp = len(sc["mps"])
    ids, rep = LM.create_new_map_points(m, sc["cur"], sc["fv"])  # default neighbours, check_ori False
    assert ids == want["recent"] == list(range(nmp, nmp + len(ref["points"])))
    assert rep["neighbours"] == list(sc["neighbours"])
    assert_same(sc, ref, rep, rep["points"], rep["exits"], m.slots)
    assert np.array_equal(m.observation_rows(), want["obs_rows"])
    assert np.array_equal(m.mp_desc, want["mp_desc"])
    geo = np.concatenate([m.mps["pos"], m.mps["normal"], m.mps["min_dist"][:, None], m.mps["max_dist"][:, None]], 1)
    assert geo.astype(np.float32).tobytes() == want["geometry"].tobytes()
    assert np.all(m.ref_kf[ids] == sc["cur"]) and np.all(m.first_kf[ids] == m.kf_id[sc["cur"]])
    assert np.all(m.found[ids] == 1) and np.all(m.visible[ids] == 1) and not m.mp_bad[ids].any()
    assert np.all(m.mps["min_dist"][ids] > 0) and np.all(m.mps["max_dist"][ids] > m.mps["min_dist"][ids])
    # second call: the restatement on the map as it is now, and no keypoint used twice
    before = [s.copy() for s in m.slots]
    sc2 = dict(sc, slots=before, mps=m.mps.copy())
    ref2 = R.create_new_map_points(sc2, chain=1)
    ids2, rep2 = LM.create_new_map_points(m, sc["cur"], sc["fv"])
    assert_same(sc2, ref2, rep2, rep2["points"], rep2["exits"], m.slots)
    assert ids2 == list(range(nmp + len(ids), nmp + len(ids) + len(ref2["points"])))
    for r in rep2["points"]:
        assert before[sc["cur"]][r["idx1"]] == -1 and before[sc["neighbours"][r["neighbour"]]][r["idx2"]] == -1
    first = set(ref["points"]["idx1"].tolist())
    assert not first & set(rep2["points"]["idx1"].tolist())
