"""Tracking::CreateInitialMap on the device (csrc/initmap.hip,
gf_orb_slam_amd/tracking.py) against the CPU restatement
(tests/helpers/initmap_ref.cpp) and the CPU oracle's BundleAdjustment.

Stage 1 (gf_initial_map_points_dev) is compared bit for bit. Stage 2
(gf_initial_map_finish_dev) is fed the oracle's BA output, so that only the
kernel is under test, and compared bit for bit. End to end the solver takes
part, so poses and positions agree within 1e-5 relative (the solver's parity
bound, tests/test_lba_gpu.py) and everything integral is equal."""
import numpy as np
import pytest

import initmap_ref as R
import initmap_scenes as S
from gf_orb_slam_amd import synth, tracking
from gf_orb_slam_amd.matcher import MAP_POINT_DTYPE

pytestmark = pytest.mark.gpu
RTOL = 1e-5
_cache = {}


def scene(name):
    if name not in _cache:
        kind, *a = name
        _cache[name] = S.two_view(*a[:1], **dict(a[1])) if kind == "tv" else S.hand_made(*a[:2], **dict(a[2]))
    return _cache[name]


def ref(name):
    """The restatement + oracle BA of a scene, computed once."""
    key = ("ref", name)
    if key not in _cache:
        _cache[key] = R.create(S.INFO, *S.args(scene(name)))
    return _cache[key]


def hm(seed, n1, **kw):
    return ("hm", seed, n1, tuple(sorted(kw.items())))


def tv(seed, **kw):
    return ("tv", seed, tuple(sorted(kw.items())))


SHAPES = [hm(10, 0), hm(11, 1), hm(73, 63), hm(74, 64), hm(75, 65), hm(140, 130), hm(5, 1000, nmatch=700),
          hm(6, 300, nmatch=200, tri_frac=0.0), hm(5, 1000, nmatch=700, dup=3), hm(8, 400, nmatch=300, tie_depths=True),
          hm(9, 300, nmatch=250, ok=0)]
B7 = dict(n_match=110, n_extra=30, outlier_frac=0.0)


batch = S.device_batch


def check_points(out, p, a, n1, n2):
    """Problem p of stage 1's device output against the restatement's dict."""
    h = {k: v[p].cpu().numpy() for k, v in out.items()}
    n = a["npts"]
    assert int(h["status"]) == a["status"] and int(h["npts"]) == n
    assert np.array_equal(h["pt_kp"][:n], a["pt_kp"])
    assert np.array_equal(h["slots1"][:n1], a["slots1"]) and np.array_equal(h["slots2"][:n2], a["slots2"])
    assert (h["slots1"][n1:] == -1).all() and (h["slots2"][n2:] == -1).all()
    assert np.array_equal(h["mp_desc"][:n], a["mp_desc"])
    assert h["mps"].reshape(-1).view(MAP_POINT_DTYPE)[:n].tobytes() == a["mps"].tobytes()
    ba = a["ba"]
    assert h["kf_Tcw"].tobytes() == ba["kf_Tcw"].tobytes() and h["kf_kind"].tolist() == ba["kf_kind"].tolist()
    assert h["kf_cam"].tobytes() == ba["kf_cam"].tobytes()
    assert h["pt_pos"][:n].tobytes() == ba["pt_pos"].tobytes()
    assert np.array_equal(h["edge_pt"][:2 * n], ba["edge_pt"]) and np.array_equal(h["edge_kf"][:2 * n], ba["edge_kf"])
    assert h["edge_z"][:2 * n].tobytes() == ba["edge_z"].tobytes()
    assert h["edge_inv_sigma2"][:2 * n].tobytes() == ba["edge_inv_sigma2"].tobytes()


def finish_with(scs, outs, thres=100):
    """Both stages on a batch with the given (kf_Tcw [2, 16], pt_pos, iterations)
    per problem standing in for the solver. -> (report rows, mps [P, cap1])."""
    import torch

    tens = batch(scs)
    arg, out = tracking.initial_map_points_device(S.INFO, *tens)
    keep, tabs = [], np.zeros((3, len(scs)), np.int64)
    for p, (T, X, it) in enumerate(outs):
        X = np.zeros((1, 3), np.float32) if X is None or not len(X) else X
        T = np.zeros((2, 16), np.float32) if T is None else T
        ts = [torch.from_numpy(np.ascontiguousarray(T, np.float32)).cuda(),
              torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda(),
              torch.tensor([it, -1], dtype=torch.int32, device="cuda")]
        keep.append(ts)
        tabs[:, p] = [t.data_ptr() for t in ts]
    d = torch.from_numpy(tabs).cuda()
    rep, mps = tracking.initial_map_finish_device(S.INFO, arg, out, d[0], d[1], d[2], thres)
    torch.cuda.synchronize()
    return (rep.cpu().numpy().view(tracking.REPORT_DTYPE).reshape(-1),
            mps.cpu().numpy().reshape(len(scs), -1).view(MAP_POINT_DTYPE), out)


def check_finish(r, mps, b):
    n = b["npts"]
    assert int(r["status"]) == b["status"] and int(r["npts"]) == n and int(r["tracked"]) == b["tracked"]
    assert r["median_depth"].tobytes() == np.float32(b["median"]).tobytes()
    assert r["Tcw"].tobytes() == np.asarray(b["Tcw"], np.float32).tobytes()
    assert mps[:n].tobytes() == b["mps"].tobytes()


@pytest.mark.parametrize("name", SHAPES, ids=lambda n: f"{n[2]}-" + "-".join(f"{k}{v}" for k, v in n[3]))
def test_stages_bit_for_bit(name):
    """Stage 1 against the restatement; stage 2 on the oracle's BA output
    against the restatement's finish. The shapes put the ordered compaction
    across wave (64) and workgroup-round (256) boundaries and cover empty, all
    untriangulated, a duplicated KFcur index, tied depths and a failed
    initialisation."""
    sc = scene(name)
    a, b = ref(name)
    rep, mps, out = finish_with([sc], [(b.get("ba_Tcw"), b.get("ba_pos"), b.get("ba_iterations", -1))])
    check_points(out, 0, a, len(sc["kps1"]), len(sc["kps2"]))
    check_finish(rep[0], mps[0], b)
    if b["status"] != R.NOT_INITIALIZED and a["npts"]:
        assert int(rep[0]["ba_iterations"]) == b["ba_iterations"]


def test_negative_median_resets():
    """A hand-made solver output behind KFini: median < 0 -> GF_IM_RESET_DEPTH,
    nothing scaled."""
    name = hm(3, 300, nmatch=250)
    sc = scene(name)
    a = R.points(S.INFO, *S.args(sc))
    T, X = a["ba"]["kf_Tcw"], -a["ba"]["pt_pos"]
    b = R.finish(S.INFO, a, T, X)
    assert b["status"] == R.RESET_DEPTH
    rep, mps, _ = finish_with([sc], [(T, X, 7)])
    check_finish(rep[0], mps[0], b)
    assert int(rep[0]["status"]) == tracking.GF_IM_RESET_DEPTH and int(rep[0]["ba_iterations"]) == 7


@pytest.mark.parametrize("kw,mask,npts,status", [(B7, 0, 103, R.OK), (B7, 3, 100, R.OK), (B7, 4, 99, R.RESET_FEW),
                                                (dict(B7, n_match=100), 0, 97, R.RESET_FEW)])
def test_boundary_of_100(kw, mask, npts, status):
    """THRES_INIT_MPT_NUM: 100 tracked points pass, 99 reset."""
    name = tv(7, mask=mask, **kw)
    sc = scene(name)
    a, b = ref(name)
    assert a["npts"] == npts and b["status"] == status
    rep, mps, out = finish_with([sc], [(b["ba_Tcw"], b["ba_pos"], b["ba_iterations"])])
    check_points(out, 0, a, len(sc["kps1"]), len(sc["kps2"]))
    check_finish(rep[0], mps[0], b)


def test_failed_initialisation():
    sc = scene(tv(4))
    assert int(sc["init"]["ok"][0]) == 0
    m, rep = tracking.create_initial_map(S.INFO, sc["K"], *S.args(sc))
    assert m is None and rep["status"] == tracking.GF_IM_NOT_INITIALIZED and rep["npts"] == 0


def test_batch_of_five_equals_the_single_calls():
    """A failing problem between good ones, different sizes in one batch."""
    import torch

    names = [tv(1), hm(75, 65), tv(4), tv(7, mask=4, **B7), tv(5)]
    scs = [scene(n) for n in names]
    res = tracking.create_initial_maps_device(S.INFO, *batch(scs))
    rep = res["report"].cpu().numpy().view(tracking.REPORT_DTYPE).reshape(-1)
    P = len(scs)
    mps = res["mps"].cpu().numpy().reshape(P, -1).view(MAP_POINT_DTYPE)
    for p, sc in enumerate(scs):
        one = tracking.create_initial_maps_device(S.INFO, *batch([sc]))
        r1 = one["report"].cpu().numpy().view(tracking.REPORT_DTYPE).reshape(-1)[0]
        n, n1, n2 = int(r1["npts"]), len(sc["kps1"]), len(sc["kps2"])
        for k in ("status", "npts", "tracked", "ba_iterations"):
            assert rep[p][k] == r1[k], (p, k)
        assert int(res["npts"][p]) == n
        # the solver's split of the Schur product depends on the batch size: its parity bound, not bits
        m1 = one["mps"].cpu().numpy().reshape(1, -1).view(MAP_POINT_DTYPE)[0, :n]
        assert _close(rep[p]["median_depth"], r1["median_depth"]) and _close(rep[p]["Tcw"], r1["Tcw"])
        for k in ("pos", "normal", "min_dist", "max_dist"):
            assert _close(mps[p, :n][k], m1[k]), (p, k)
        for k in ("pt_kp", "mp_desc"):
            assert torch.equal(res[k][p, :n], one[k][0, :n]), k
        assert torch.equal(res["slots1"][p, :n1], one["slots1"][0, :n1])
        assert torch.equal(res["slots2"][p, :n2], one["slots2"][0, :n2])
    assert [int(s) for s in rep["status"]] == [0, 3, 1, 3, 0]


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("seed", [1, 2, 3, 5])
def test_create_initial_map_end_to_end(seed):
    sc = scene(tv(seed))
    a, b = ref(tv(seed))
    m, rep = tracking.create_initial_map(S.INFO, sc["K"], *S.args(sc))
    assert m is not None and rep["status"] == b["status"] == R.OK
    n = a["npts"]
    assert rep["npts"] == n == len(m.mps) and rep["tracked"] == b["tracked"] and rep["ba_iterations"] == b["ba_iterations"]
    assert np.array_equal(m.slots[0], a["slots1"]) and np.array_equal(m.slots[1], a["slots2"])
    assert m.obs == [{0: int(i), 1: int(j)} for i, j in a["pt_kp"]]
    assert np.array_equal(m.mp_desc, a["mp_desc"])
    assert m.kf_id.tolist() == [0, 1] and (m.ref_kf == 1).all() and (m.first_kf == 1).all()
    # both keyframes list each other with weight = the point count (no duplicated slot here)
    assert b["tracked"] == n
    assert m.weights == [{1: n}, {0: n}] and m.ordered == [[1], [0]] and m.ordered_w == [[n], [n]]
    assert m.parent == [-1, 0]
    print("median", rep["median_depth"], b["median"], "max |dT|", np.abs(m.Tcw - b["Tcw"]).max(), "max |dX|",
          np.abs(m.mps["pos"] - b["mps"]["pos"]).max())
    assert _close(rep["median_depth"], b["median"])
    assert _close(m.Tcw, b["Tcw"]) and _close(m.mps["pos"], b["mps"]["pos"])
    for k in ("normal", "min_dist", "max_dist"):
        assert _close(m.mps[k], b["mps"][k]), k
    z = np.sort(np.asarray([m.Tcw[0][2, :3].astype(np.float64) @ x + m.Tcw[0][2, 3] for x in m.mps["pos"]]))
    assert abs(z[(n - 1) // 2] - 1.0) <= 1e-5


def test_global_bundle_adjustment_on_the_unscaled_twin():
    """GlobalBundleAdjustemnt on a LoopMap holding the map as stage 1 leaves it
    gives the poses and points of the batched path before its scaling."""
    from gf_orb_slam_amd.loopmap import LoopMap
    from gf_orb_slam_amd.optimizer import global_bundle_adjustment

    sc = scene(tv(2))
    a, b = ref(tv(2))
    m, rep = tracking.create_initial_map(S.INFO, sc["K"], *S.args(sc))
    twin = LoopMap(S.INFO, [sc["kps1"], sc["kps2"]], [sc["desc1"], sc["desc2"]], [a["slots1"], a["slots2"]], a["mps"],
                   a["mp_desc"], observations=[{0: int(i), 1: int(j)} for i, j in a["pt_kp"]],
                   kf_Tcw=a["ba"]["kf_Tcw"].reshape(2, 4, 4), ref_kf=np.ones(a["npts"], np.int32), kf_id=[0, 1])
    out = global_bundle_adjustment(twin, 20)
    assert out["iterations"] == rep["ba_iterations"] == b["ba_iterations"]
    inv = np.float32(1.0) / rep["median_depth"]
    assert _close(twin.Tcw[0], m.Tcw[0]) and _close(twin.Tcw[1][:3, :3], m.Tcw[1][:3, :3])
    assert _close(twin.Tcw[1][:3, 3] * inv, m.Tcw[1][:3, 3])
    assert _close(twin.mps["pos"] * inv, m.mps["pos"])
    for k in ("normal", "min_dist", "max_dist"):  # unscaled in both
        assert _close(twin.mps[k], m.mps[k]), k
    assert _close(twin.Tcw, b["ba_Tcw"]) and _close(twin.mps["pos"], b["ba_pos"])


def test_local_mapper_takes_the_map_over():
    from gf_orb_slam_amd.bow import ORBVocabulary
    from gf_orb_slam_amd.localmapping import LocalMapper

    voc = ORBVocabulary(synth.synth_vocabulary(7, k=10, L=3))
    sc = scene(tv(3))
    m, rep = tracking.create_initial_map(S.INFO, sc["K"], *S.args(sc), voc=voc, levelsup=2)
    assert m is not None and m.kf_bow[0] is not None and m.kf_fv[1] is not None
    lm = LocalMapper(m, voc, levelsup=2)
    for k in (0, 1):
        assert lm.step(k)["to_loop_closer"] == k
    assert not m.kf_bad.any()
    assert 1 in m.weights[0] and 0 in m.weights[1] and m.parent[1] == 0
