"""Named, seeded batches of small local-BA windows for the batched solver
(gf_ba_plan_*, csrc/ba.hip) on both sides of its switch between the two Schur
products: k_ba_spgemm (a host-built task list) for up to 8 windows, k_ba_gemm
(dense split-K through LDS) from 9 on.

Plain Python on synth.synth_lba_problem; nothing here touches the GPU.
``geometry`` restates the plan's layout rule (gf_ba_plan_create) so that
tests/test_ba_batch_cpu.py can assert that every named window reaches the code
it is named for. A window is a gf_ba_problem dict with a ``name`` key added
(the cache key of the oracle results); windows are built once and shared
between batches, and nobody modifies them."""
import numpy as np

from gf_orb_slam_amd.synth import synth_lba_problem

BA_GCH = 8          # k-steps per LDS chunk of k_ba_gemm
BA_MAXSPLIT = 64
SPARSE_MAX = 8      # gf_ba_plan_create: sparse = nprob <= 8
_EDGE_KEYS = ("edge_pt", "edge_kf", "edge_z", "edge_inv_sigma2")
_KF_KEYS = ("kf_Tcw", "kf_kind", "kf_cam")
_win = {}
_batch = {}


# ---------------------------------------------------------------- the plan's geometry
def nsplit_of(nprob):
    nprob = max(nprob, 1)
    return max(1, min(BA_MAXSPLIT, (256 + nprob - 1) // nprob))


def free_cols(p):
    """Free-pose column of every keyframe (-1: fixed), as gf_ba_plan_create numbers them."""
    col, n = [], 0
    for k in np.asarray(p["kf_kind"]):
        col.append(n if k == 0 else -1)
        n += int(k == 0)
    return np.asarray(col, np.int64), n


def geometry(p, nprob):
    """BADesc of window p inside a plan of nprob windows, and its kmask words."""
    col, nfree = free_cols(p)
    npts = len(p["pt_pos"])
    n = 6 * nfree
    npad = ((n + 1 + 15) // 16) * 16
    steps = max(1, (3 * npts + 3) // 4)
    nsplit = nsplit_of(nprob)
    sps = (steps + nsplit - 1) // nsplit
    nt = npad // 16
    mask = np.zeros(nsplit * sps, np.uint16)
    straddle = False
    for i, k in zip(np.asarray(p["edge_pt"]), np.asarray(p["edge_kf"])):
        c = int(col[k])
        if c < 0:
            continue
        lo, hi = (6 * c) >> 4, (6 * c + 5) >> 4
        straddle |= lo != hi
        for r in range(3 * int(i), 3 * int(i) + 3):
            mask[r // 4] |= (1 << lo) | (1 << hi)
    return dict(sparse=nprob <= SPARSE_MAX, nfree=nfree, n=n, npad=npad, steps=steps, nsplit=nsplit, sps=sps,
                K=nsplit * sps * 4, nt=nt, tdb=n >> 4, ntiles=nt * (nt + 1) // 2 + (n >> 4),
                lds=8 * 2 * BA_GCH * 4 * (npad + 2), mask=mask, straddle=straddle)


# ---------------------------------------------------------------- windows
def _named(name, make):
    if name not in _win:
        p = make()
        p["name"] = name
        _win[name] = p
    return _win[name]


def family(b):
    """The plain family: 2-5 free keyframes, 24-60 points, 0-2 fixed cameras.
    The point counts start at 38 so that window 0 has 29 k-steps (work in every
    one of the 29 splits of a batch of 9) and window 3 has 31 (work in the last
    of the 16 splits of a batch of 16, sps = 2)."""
    return _named(("fam", b), lambda: synth_lba_problem(100 + b, 3 + b % 4, 24 + (b + 14) % 37, nfixed=b % 3))


def window(seed, nfree, npts, nfixed=1, **kw):
    """nfree free keyframes (+ the fixed mnId == 0 one + nfixed fixed cameras), npts points."""
    key = ("win", seed, nfree, npts, nfixed, tuple(sorted(kw.items())))
    return _named(key, lambda: synth_lba_problem(seed, nfree + 1, npts, nfixed=nfixed, **kw))


def _edit(name, base, fn):
    def make():
        p = {k: np.array(v, copy=True) for k, v in base.items() if k != "name"}
        fn(p)
        return p
    return _named(name, make)


def with_idle_keyframe(base):
    """base + one free keyframe that no point observes (n grows by 6)."""
    def fn(p):
        for k in _KF_KEYS:
            p[k] = np.concatenate([p[k], p[k][1:2]])
        p["kf_kind"][-1] = 0
    return _edit(("idle_kf", base["name"]), base, fn)


def with_idle_point(base):
    """base + one map point without an observation, placed first (panel rows 0-2 stay zero)."""
    def fn(p):
        p["pt_pos"] = np.concatenate([p["pt_pos"][:1] + np.float32(0.5), p["pt_pos"]])
        p["edge_pt"] = p["edge_pt"] + 1
    return _edit(("idle_pt", base["name"]), base, fn)


def fixed_only_first(base):
    """base with its points reordered: those seen by fixed keyframes only come
    first, so whole k-steps (4 panel rows) have an all-zero mask."""
    def fn(p):
        col, _ = free_cols(p)
        npts = len(p["pt_pos"])
        seen_free = np.zeros(npts, bool)
        np.logical_or.at(seen_free, p["edge_pt"], col[p["edge_kf"]] >= 0)
        order = np.r_[np.nonzero(~seen_free)[0], np.nonzero(seen_free)[0]]
        new = np.empty(npts, np.int64)
        new[order] = np.arange(npts)
        e = np.argsort(new[p["edge_pt"]], kind="stable")  # a point's edges stay contiguous and in order
        for k in _EDGE_KEYS:
            p[k] = p[k][e]
        p["edge_pt"] = new[p["edge_pt"]].astype(np.int32)
        p["pt_pos"] = p["pt_pos"][order]
    return _edit(("fixed_first", base["name"]), base, fn)


def without_edges(base):
    def fn(p):
        for k in _EDGE_KEYS:
            p[k] = p[k][:0]
    return _edit(("no_edge", base["name"]), base, fn)


def nothing():
    """No keyframe, no point, no edge."""
    def fn(p):
        for k in _EDGE_KEYS + _KF_KEYS + ("pt_pos",):
            p[k] = p[k][:0]
    return _edit(("nothing",), family(0), fn)


# named windows: the smallest shapes that reach each piece of k_ba_gemm
def free_window(nfree):
    seed, npts, nfixed = {0: (501, 20, 2), 1: (502, 24, 1), 2: (503, 30, 1), 3: (504, 40, 1), 8: (505, 60, 0),
                          16: (506, 80, 2), 24: (507, 100, 1), 32: (508, 120, 0)}[nfree]
    return window(seed, nfree, npts, nfixed)


def one_point_fixed():
    return window(521, 0, 1, 3)


def one_point_free():
    """The smallest shape the dense product works on: one point under one free
    pose, one k-step (3 rows and a row of padding), one pose tile. All five
    keyframes observe the point (min_obs = 5): 10 residuals for 9 unknowns.
    With the default two observations it is an exact fit, 4 residuals for 9
    unknowns: chi2 falls to rounding noise and that noise decides the stop
    rules, so such a window cannot be held to equal iteration counts."""
    return window(521, 1, 1, 3, min_obs=5)


def three_points():
    """One free pose over three points: 3 k-steps, a pose tile, 29 splits."""
    return window(533, 1, 3, 3)


def five_points():
    return window(523, 1, 5, 2)


def big_window():
    """About 320 points: 240 k-steps, sps = 9 at 29 splits (chunks of 8 and 1)."""
    return window(524, 5, 320, 2)


def fifty_points(b):
    """38 k-steps: sps = 10 at the 4 splits of a batch of 64 (chunks of 8 and 2)."""
    return window(600 + b, 2 + b % 4, 50, b % 3)


def noisy(b):
    return window(700 + b, 3 + b % 3, 60 + 7 * b, 2, noise_px=0.5, outlier_frac=0.4)


def fixed_only_window():
    return fixed_only_first(window(525, 2, 40, 3))


# ---------------------------------------------------------------- batches
SIZES = (8, 9, 16, 64, 255, 256, 300)   # nsplit -, 29, 16, 4, 2, 1, 1
PLACED = family(3)                      # the window of the placement batches


def _build(name):
    fam = family
    if name[0] == "size":
        return [fam(b) for b in range(name[1])]
    if name == "free_small":     # n = 0, 6, 12, 18
        return [free_window(0), fam(0), free_window(1), free_window(2), fam(1), free_window(3), fam(2), fam(4), fam(5)]
    if name == "free_mult16":    # n = 48, 96, 144: db alone in the last tile column
        return [fam(37), free_window(8), fam(7), free_window(16), fam(8), free_window(24), fam(9), fam(10), fam(11)]
    if name == "free_limit":     # n = 192, 103 tiles, 107,520 bytes of LDS
        return [fam(74), fam(13), free_window(32), fam(14), fam(15), fam(16), fam(17), fam(18), fam(19)]
    if name == "pts_small":      # nsplit = 29: 1, 3, 5, 6 and 7 points
        return [one_point_fixed(), fam(111), three_points(), five_points(), window(526, 2, 6, 2), window(527, 2, 7, 2),
                one_point_free(), fam(22), fam(23)]
    if name == "pts_sps10":      # 64 windows of 50 points: nsplit = 4, sps = 10
        return [fifty_points(b) for b in range(64)]
    if name == "pts_big":        # nsplit = 29, sps = 9
        return [fam(148), fam(25), fam(26), fam(27), big_window(), fam(28), fam(29), fam(30), fam(31)]
    if name == "ragged":         # every window's npad against a max_npad of 208
        return [free_window(3), one_point_fixed(), free_window(32), five_points(), nothing(), free_window(0),
                big_window(), free_window(16), fam(32), without_edges(fam(33)), free_window(1), one_point_free()]
    if name == "graphs":
        return [fam(33), with_idle_keyframe(fam(35)), with_idle_point(fam(36)), fixed_only_window(), nothing(),
                without_edges(fam(37)), fam(38), with_idle_keyframe(free_window(2)), fam(39), fam(40)]
    if name == "noisy":
        return [noisy(b) for b in range(9)]
    if name == "placed_dense":   # PLACED at 0, 5 and 11
        return [PLACED, free_window(8), fam(41), five_points(), free_window(16), PLACED, fam(42), three_points(),
                fam(43), free_window(2), fam(28), PLACED]
    if name == "placed_sparse":  # PLACED at 0, 3 and 7
        return [PLACED, free_window(8), fam(41), PLACED, five_points(), free_window(16), fam(42), PLACED]
    raise KeyError(name)


GEOMETRY = ("free_small", "free_mult16", "free_limit", "pts_small", "pts_sps10", "pts_big", "ragged", "graphs", "noisy")
LOCAL = tuple(("size", n) for n in SIZES) + GEOMETRY
SHORT = GEOMETRY + (("size", 9), ("size", 64), ("size", 256))
PLACEMENT = (("placed_dense", (0, 5, 11)), ("placed_sparse", (0, 3, 7)))
ALL = LOCAL + tuple(n for n, _ in PLACEMENT)


# fillers fam(0), fam(37), ... have 38 points = 29 k-steps, fam(33) 26 and fam(28) 22: in every dense batch
# some window has work in the last split (tests/test_ba_batch_cpu.py asserts it)


def batch(name):
    if name not in _batch:
        _batch[name] = _build(name)
    return _batch[name]


def batch_id(name):
    return name if isinstance(name, str) else f"{name[0]}{name[1]}"
