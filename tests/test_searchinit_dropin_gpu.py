"""The C++ drop-in ORBmatcher::SearchForInitialization
(include/gfslam/orbslam.h, csrc/dropin.cpp) through tests/cpp/searchinit_driver:
a C++ program that only links libgfslam matches an initial frame against a
second and then a third frame, carrying vbPrevMatched, and equals the CPU
restatement on both calls."""
import os
import subprocess

import numpy as np
import pytest

import searchinit_ref as R
import searchinit_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SI_BIN = os.path.join(ROOT, "tests", "cpp", "searchinit_driver")


def test_searchinit_driver_built():
    assert os.path.exists(SI_BIN), "run make (or __graft_entry__.build())"


@pytest.mark.gpu
def test_cpp_search_for_initialization_equals_the_restatement(tmp_path):
    frames = S.sequence(3, [(4.0, 0.0), (6.0, 0.35)])
    k1, d1 = frames[0]
    np.array([len(k) for k, _ in frames] + [S.INFO.min_x, S.INFO.max_x, S.INFO.min_y, S.INFO.max_y],
             np.int32).tofile(tmp_path / "si_sizes.i32")
    for f, (k, d) in enumerate(frames, 1):
        np.ascontiguousarray(k).tofile(tmp_path / f"si_k{f}.bin")
        np.ascontiguousarray(d).tofile(tmp_path / f"si_d{f}.bin")
    r = subprocess.run([SI_BIN, str(tmp_path), "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    prev = S.prev_of(k1)
    for tag, (k, d) in zip("ab", frames[1:]):
        nm, m12, prev, _ = R.search(S.INFO, k1, d1, k, d, prev)
        assert nm >= 100
        assert int(np.fromfile(tmp_path / f"si_{tag}_nm.i32", np.int32)[0]) == nm
        assert np.array_equal(np.fromfile(tmp_path / f"si_{tag}_m12.i32", np.int32), m12)
        assert np.fromfile(tmp_path / f"si_{tag}_prev.f32", np.float32).tobytes() == prev.tobytes()
