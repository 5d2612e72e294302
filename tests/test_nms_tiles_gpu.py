"""k_nms_tiles + k_cell_lists (non-maximum suppression on whole levels, one
wave per cell for the listing) against the CPU oracle extractor, bit for bit,
on the smallest frames at which they can go wrong: one frame of at most
160x120 px per case. The extractor takes levels of at least 40 px, so these
frames run 8 levels at scale factor 1.1 (level 7 of 97x83 is 50x43).

Cell windows (ORBextractor.cc:540-618): the detectable area of a level is
[16, w - 16) x [16, h - 16), cut into levelCols x levelRows windows of
cellW x cellH px (the last column and row trimmed). A corner is suppressed
only by a stronger-or-equal neighbour in its own window."""
import math

import numpy as np
import pytest

import oracle_lib as O
from gf_orb_slam_amd import ORBextractor, synth

pytestmark = pytest.mark.gpu

SCALE, NLEVELS = 1.1, 8


def _diff(kg, ko):
    for i in range(min(len(kg), len(ko))):
        if kg[i].tobytes() != ko[i].tobytes():
            return f"first mismatch at {i}: gpu={kg[i]} oracle={ko[i]}"
    return f"len gpu={len(kg)} oracle={len(ko)}"


def _check(img, nf=1000, score_type=1, fast_th=20, oracle=None):
    """One frame through the GPU extractor, compared with the oracle's."""
    ko, do = oracle if oracle is not None else O.extract(img, nf, SCALE, NLEVELS, fast_th, score_type)
    ex = ORBextractor(nf, SCALE, NLEVELS, score_type, fast_th)
    kg, dg = ex(img)
    assert kg.tobytes() == ko.tobytes(), _diff(kg, ko)
    assert np.array_equal(dg, do)
    return ex, ko


def _windows(n, ncell):
    """[start, end) of the windows along one axis of a level of n px."""
    lo, hi = 16, n - 16
    size = math.ceil(float(np.float32(hi - lo) / np.float32(ncell)))
    out = []
    for k in range(ncell):
        s = lo + k * size
        e = s + size if k < ncell - 1 else hi
        if e > s:
            out.append((s, e))
    return out


def _grid(w0, h0, lw, lh, ndesired):
    """Window ranges in x and y of a level (lw x lh, ndesired features) of a w0 x h0 frame."""
    ratio = np.float32(w0) / np.float32(h0)
    cols = int(np.sqrt(np.float32(ndesired) / (np.float32(5) * ratio)))
    rows = int(ratio * np.float32(cols))
    return _windows(lw, cols), _windows(lh, rows)


def _oracle_grid(w, h, nf, lvl=0):
    lw, lh, fpl = O.plan(w, h, nf, SCALE, NLEVELS)[:3]
    return _grid(w, h, int(lw[lvl]), int(lh[lvl]), int(fpl[lvl]))


def _extractor_grid(ex, w, h, lvl=0):
    """The same from the bound extractor: its level size and its per-level quota."""
    lh, lw = ex.debug_level(lvl, 1).shape
    return _grid(w, h, lw, lh, ex.features_per_level()[lvl])


def _level0(k):
    k = k[k["octave"] == 0]
    return {(int(x), int(y)) for x, y in zip(k["x"], k["y"])}


def _dots(w, h, pts, bg=0):
    """Isolated corners: single pixels on a flat frame (FAST score value - bg - 1
    each; two adjacent ones do not lie on each other's radius-3 ring)."""
    img = np.full((h, w), bg, np.uint8)
    for x, y, v in pts:
        img[y, x] = v
    return img


# ------------------------------------------------------------------ level shapes
@pytest.mark.parametrize("nf", [200, 1000])
@pytest.mark.parametrize("w,h", [(97, 83), (130, 101), (160, 120)])
def test_small_levels(w, h, nf):
    """Level widths that are no multiple of 4, 64 or 256, one cell column on
    some levels and several on others."""
    img = synth.synth_frame(w, h, synth.frame_seed(3, w + nf), n_shapes=60)
    ko = O.extract(img, nf, SCALE, NLEVELS)
    assert len(ko[0]) >= 20 and len(set(ko[0]["octave"])) == NLEVELS, "the oracle must find corners on every level"
    _check(img, nf, oracle=ko)


def test_small_levels_cover_one_and_many_columns():
    """(CPU) the shapes above include levels with one cell column and with several."""
    seen = set()
    for w, h in [(97, 83), (130, 101), (160, 120)]:
        for nf in (200, 1000):
            seen |= {len(_oracle_grid(w, h, nf, l)[0]) for l in range(NLEVELS)}
    assert 1 in seen and max(seen) >= 3


# ------------------------------------------------------------------ window boundaries
W, H, NF = 160, 120, 1000


def _pair_frame(where):
    """Two corners of equal score on adjacent pixels: astride the boundary of
    the first two windows in x / in y (both survive), or inside the first
    window (neither does; a third corner there keeps the cell non-empty)."""
    xs, ys = _oracle_grid(W, H, NF)
    assert len(xs) >= 2 and len(ys) >= 2
    xb, yb = xs[1][0], ys[1][0]              # first column / row of the second window
    xc, yc = xs[0][0] + 5, ys[0][0] + 4      # inside the first window
    assert xc + 1 < xb - 1 and yc + 1 < yb - 1
    if where == "x":
        pts, gone = [(xb - 1, yc), (xb, yc)], []
    elif where == "y":
        pts, gone = [(xc, yb - 1), (xc, yb)], []
    else:
        far = (xs[0][1] - 3, ys[0][1] - 3)
        assert far[0] - xc >= 8 and far[1] - yc >= 5
        pts, gone = [far], [(xc, yc), (xc + 1, yc)]
    img = _dots(W, H, [(x, y, 255) for x, y in pts + gone])
    return img, pts, gone, (xs, ys)


@pytest.mark.parametrize("where", ["x", "y", "inside"])
def test_equal_neighbours_at_window_boundaries(where):
    img, kept, gone, grid = _pair_frame(where)
    ko = O.extract(img, NF, SCALE, NLEVELS)
    found = _level0(ko[0])
    assert all(p in found for p in kept), "the oracle must keep the corners under test"
    assert not any(p in found for p in gone)
    ex, _ = _check(img, NF, oracle=ko)
    assert _extractor_grid(ex, W, H) == grid, "the test's windows are the extractor's"


def test_first_and_last_detectable_columns_and_rows():
    """Corners on the first / last detectable column and row of level 0 are
    found, corners one pixel outside are not, and a stronger corner just
    outside does not suppress its neighbour inside."""
    inside = [(16, 30), (W - 17, 50), (60, 16), (90, H - 17), (16, 80)]
    outside = [(15, 45), (W - 16, 70), (40, 15), (110, H - 16), (15, 81)]
    xs, ys = _oracle_grid(W, H, NF)
    assert xs[0][0] == 16 and xs[-1][1] == W - 16 and ys[0][0] == 16 and ys[-1][1] == H - 16
    img = _dots(W, H, [(x, y, 200) for x, y in inside] + [(x, y, 255) for x, y in outside])
    ko = O.extract(img, NF, SCALE, NLEVELS)
    found = _level0(ko[0])
    assert all(p in found for p in inside) and not any(p in found for p in outside)
    _check(img, NF, oracle=ko)


# ------------------------------------------------------------------ threshold retry
def _mixed_texture_frame():
    rng = np.random.default_rng(4)
    img = np.full((H, W), 128, np.uint8)
    img += rng.integers(0, 12, img.shape, dtype=np.uint8)
    img[25:45, 50:80] = 40
    img[60:100, 90:150] = rng.integers(0, 256, (40, 60), dtype=np.uint8)
    return img


@pytest.mark.parametrize("score_type", [1, 0])
def test_low_texture_some_cells_retry(score_type):
    """Weak noise, one dark rectangle and one patch of strong texture: the
    cells of the patch keep their corners at fast_th, the others retry at the
    minimum threshold."""
    img = _mixed_texture_frame()
    kf = O.extract(img, NF, SCALE, NLEVELS)[0]  # FAST scores as responses
    k0 = kf[kf["octave"] == 0]
    # a corner of score < 20 can only come from a retry; four corners of score >= 20 in one
    # window survive NMS at fast_th too (fewer competitors), so that cell did not retry
    assert np.any(k0["response"] < 20), "some cell must retry"
    xs, ys = _oracle_grid(W, H, NF)
    strong = k0[k0["response"] >= 20]
    per_cell = max(np.sum((strong["x"] >= x0) & (strong["x"] < x1) & (strong["y"] >= y0) & (strong["y"] < y1))
                   for x0, x1 in xs for y0, y1 in ys)
    assert per_cell >= 4, "some cell must not retry"
    _check(img, NF, score_type)


# ------------------------------------------------------------------ thresholds, score types
@pytest.mark.parametrize("score_type", [1, 0])
@pytest.mark.parametrize("fast_th", [0, 7])
def test_fast_threshold_rule(fast_th, score_type):
    """fast_th 0 and 7: a map entry counts when it exceeds max(th, 1)."""
    img = synth.synth_frame(W, H, synth.frame_seed(3, 50 + fast_th), n_shapes=60)
    ko = O.extract(img, NF, SCALE, NLEVELS, fast_th, score_type)
    assert len(ko[0]) >= 50
    _check(img, NF, score_type, fast_th, oracle=ko)


# ------------------------------------------------------------------ batches
def test_batch_of_three_frames():
    """Three different frames through the batched device entry equal the three
    single-frame results (frame strides of the survivor plane)."""
    import torch
    frames = np.stack([synth.synth_frame(W, H, synth.frame_seed(3, 70 + s), n_shapes=60) for s in range(3)])
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    single = ORBextractor(NF, SCALE, NLEVELS, 1, 20)
    ex = ORBextractor(NF, SCALE, NLEVELS, 1, 20, width=W, height=H, max_batch=3)
    cap = ex.capacity
    kps = torch.zeros((3, cap, 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((3, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    imgs = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ex.extract_batch_dev(imgs, kps, desc, cnt)
    ex.ctx.sync()
    for f in range(3):
        ko, do = O.extract(frames[f], NF, SCALE, NLEVELS)
        assert len(ko) >= 50
        ks, ds = single(frames[f])
        n = int(cnt[f])
        kb, db = kps[f, :n].cpu().numpy().tobytes(), desc[f, :n].cpu().numpy()
        assert n == len(ks) == len(ko)
        assert kb == ks.tobytes() == ko.tobytes()
        assert np.array_equal(db, ds) and np.array_equal(db, do)
