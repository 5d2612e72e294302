"""ORBmatcher::SearchForInitialization on the device (csrc/searchinit.hip)
against the CPU restatement (tests/helpers/searchinit_ref.cpp): matches12,
nmatches and the vbPrevMatched bytes are equal on every scene, through the
host entry and the batch entry, with the stored candidate lists and with
GF_SI_DIRECT. tests/test_searchinit_cpu.py checks that the scenes take the
branches these comparisons are about."""
import numpy as np
import pytest

import searchinit_ref as R
import searchinit_scenes as S
from gf_orb_slam_amd import tracking
from gf_orb_slam_amd.matcher import GF_SI_DIRECT, Frame, ORBmatcher
from gf_orb_slam_amd.orb import KEYPOINT_DTYPE

pytestmark = pytest.mark.gpu
SI_CAP = 64  # csrc/searchinit.hip: stored candidates per query
_cache = {}

SCENES = [("two_view", 1), ("two_view", 2), ("contended", 1), ("contended", 2), ("contended", 3), ("crowded", 1)] + \
         [("edge", e) for e in S.EDGES]


def scene(name):
    if name not in _cache:
        _cache[name] = getattr(S, name[0])(name[1])
    return _cache[name]


def ref(name, check_ori=True):
    """The restatement's result of a scene, computed once."""
    key = ("ref", name, check_ori)
    if key not in _cache:
        s = scene(name)
        _cache[key] = R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"], check_ori=check_ori)
    return _cache[key]


def host(s, flags=0, check_ori=True, prev=None):
    F1, F2 = Frame(s["kps1"], s["desc1"], S.INFO), Frame(s["kps2"], s["desc2"], S.INFO)
    p = np.ascontiguousarray(s["prev"] if prev is None else prev, np.float32).copy()
    nm, m12 = ORBmatcher(0.9, check_ori).SearchForInitialization(F1, F2, p, 100, flags=flags)
    return nm, m12, p


def batch(scs, flags=0, check_ori=True):
    """-> (nmatches [P], matches12 [P, cap1], prev [P, cap1, 2]) as host arrays."""
    import torch

    P = len(scs)
    c1 = max(1, max(len(s["kps1"]) for s in scs))
    c2 = max(1, max(len(s["kps2"]) for s in scs))
    k1, k2 = np.zeros((P, c1), KEYPOINT_DTYPE), np.zeros((P, c2), KEYPOINT_DTYPE)
    d1, d2 = np.zeros((P, c1, 32), np.uint8), np.zeros((P, c2, 32), np.uint8)
    n1, n2, prev = np.zeros(P, np.int32), np.zeros(P, np.int32), np.full((P, c1, 2), -7.0, np.float32)
    for p, s in enumerate(scs):
        a, b = len(s["kps1"]), len(s["kps2"])
        n1[p], n2[p] = a, b
        k1[p, :a], k2[p, :b], d1[p, :a], d2[p, :b], prev[p, :a] = s["kps1"], s["kps2"], s["desc1"], s["desc2"], s["prev"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    pv = dev(prev)
    m12, nm = tracking.search_for_initialization_device(
        S.INFO, dev(k1.view(np.uint8).reshape(P, c1, 28)), dev(d1), dev(n1), dev(k2.view(np.uint8).reshape(P, c2, 28)),
        dev(d2), dev(n2), pv, check_ori=check_ori, flags=flags)
    torch.cuda.synchronize()
    return nm.cpu().numpy(), m12.cpu().numpy(), pv.cpu().numpy()


def same(got, want, n1):
    nm, m12, prev = got
    assert int(nm) == want[0], (int(nm), want[0])
    assert np.array_equal(np.asarray(m12)[:n1], want[1])
    assert np.asarray(prev)[:n1].tobytes() == want[2].tobytes()


@pytest.mark.parametrize("flags", [0, GF_SI_DIRECT], ids=["lists", "direct"])
@pytest.mark.parametrize("name", SCENES, ids=lambda n: f"{n[0]}-{n[1]}")
def test_host_entry_equals_the_restatement(name, flags):
    s = scene(name)
    same(host(s, flags), ref(name), len(s["kps1"]))


@pytest.mark.parametrize("flags", [0, GF_SI_DIRECT], ids=["lists", "direct"])
@pytest.mark.parametrize("name", SCENES, ids=lambda n: f"{n[0]}-{n[1]}")
def test_batch_entry_equals_the_restatement(name, flags):
    s = scene(name)
    nm, m12, prev = batch([s], flags)
    n1 = len(s["kps1"])
    same((nm[0], m12[0], prev[0]), ref(name), n1)
    assert (m12[0, n1:] == -1).all()


@pytest.mark.parametrize("flags", [0, GF_SI_DIRECT], ids=["lists", "direct"])
def test_without_the_orientation_check(flags):
    for name in (("contended", 1), ("two_view", 2)):
        s = scene(name)
        want = ref(name, check_ori=False)
        assert want[0] > ref(name)[0]  # the histogram removed something on these scenes
        same(host(s, flags, check_ori=False), want, len(s["kps1"]))


def test_the_crowded_scene_overflows_the_lists():
    """SI_CAP entries a query; the crowd has at least 600 in one window, so
    the centre queries take the in-place walk in the default mode too."""
    assert 600 > SI_CAP
    s = scene(("crowded", 1))
    c = np.array([S.W / 2, S.H / 2])
    k2 = s["kps2"]
    for i in range(3):
        q = s["prev"][i]
        assert ((k2["octave"] == 0) & (np.abs(k2["x"] - q[0]) <= 100) & (np.abs(k2["y"] - q[1]) <= 100)).sum() >= 600
    assert np.abs(s["prev"][0] - c).max() <= 0.5


@pytest.mark.parametrize("flags", [0, GF_SI_DIRECT], ids=["lists", "direct"])
def test_batch_of_seven_equals_the_single_calls(flags):
    names = [("two_view", 1), ("edge", "n1=0"), ("crowded", 1), ("contended", 2), ("edge", "n2=0"), ("contended", 1),
             ("edge", "one query, one candidate")]
    scs = [scene(n) for n in names]
    nm, m12, prev = batch(scs, flags)
    for p, (n, s) in enumerate(zip(names, scs)):
        n1 = len(s["kps1"])
        same((nm[p], m12[p], prev[p]), ref(n), n1)
        assert (m12[p, n1:] == -1).all() and (prev[p, n1:] == -7.0).all()


def test_second_call_on_a_third_frame_carries_prev_matched():
    fr = S.sequence(2, [(4.0, 0.0), (6.0, 0.35)])
    (k1, d1), (k2, d2), (k3, d3) = fr
    p0 = S.prev_of(k1)
    a = R.search(S.INFO, k1, d1, k2, d2, p0)
    b = R.search(S.INFO, k1, d1, k3, d3, a[2])
    assert a[0] >= 100 and b[0] >= 100 and not np.array_equal(a[2], p0) and not np.array_equal(a[2], b[2])
    for flags in (0, GF_SI_DIRECT):
        g1 = host(dict(kps1=k1, desc1=d1, kps2=k2, desc2=d2, prev=p0), flags)
        same(g1, a, len(k1))
        g2 = host(dict(kps1=k1, desc1=d1, kps2=k3, desc2=d3, prev=g1[2]), flags)
        same(g2, b, len(k1))


def test_4096_keypoints_in_both_frames():
    s = S.big(1)
    assert len(s["kps1"]) == len(s["kps2"]) == 4096
    want = R.search(S.INFO, s["kps1"], s["desc1"], s["kps2"], s["desc2"], s["prev"])
    assert want[0] > 100
    same(host(s), want, 4096)
    nm, m12, prev = batch([s], GF_SI_DIRECT)
    same((nm[0], m12[0], prev[0]), want, 4096)
