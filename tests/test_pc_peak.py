"""The sub-cell pose rule (csrc/pc_peak_rule.h) on the host: the library's
rs_pc_peak_host against the NumPy restatement bit for bit, known answers of the pose, the
refusals, and tests/pc_peak_main.cpp -- the header alone, built with the host compiler and
-fsanitize=address,undefined -ffp-contract=off and run as a child process (the sanitizer is
linked into the program; nothing is preloaded).  CPU only: no device call."""
import ctypes
import math

import numpy as np
import pytest

import _host_program
from pyratslam_amd import _build, _lib, numpy_peak_sums, peak_tables, pose_from_sums
from pyratslam_amd import pc_peak

GRIDS = [(7, 7, 7), (9, 12, 8), (21, 21, 36), (50, 50, 10)]


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def cells(shape):
    return [(0, 0, 0), tuple(s - 1 for s in shape), tuple(s // 2 for s in shape)]


def volumes(shape, seed):
    rng = np.random.default_rng(seed)
    v64 = rng.random(shape)
    v32 = rng.random(shape).astype(np.float32).astype(np.float64)
    v32[rng.random(shape) < 0.2] = 0.0
    return [v64, v32]


@pytest.mark.parametrize('shape', GRIDS)
@pytest.mark.parametrize('r', [1, 2, 3])
def test_host_rule_equals_the_numpy_restatement_bit_for_bit(lib, shape, r):
    for seed, vol in enumerate(volumes(shape, 7)):
        for cell in cells(shape):
            want = numpy_peak_sums(vol, cell, r)
            got = pc_peak.host_peak_sums(vol, cell, r)
            assert got.tobytes() == want.tobytes(), (shape, r, cell, seed, got, want)


def circ(a, b, n):
    d = abs(a - b) % n
    return min(d, n - d)


def test_two_half_cells_across_the_wrap_give_the_midpoint():
    vol = np.zeros((9, 12, 8))
    vol[8, 11, 7] = 0.5
    vol[0, 11, 7] = 0.5
    for cell in ((8, 11, 7), (0, 11, 7)):
        pose = pose_from_sums(numpy_peak_sums(vol, cell, 3), cell, vol.shape)
        for got, want, n in zip(pose, (8.5, 11.0, 7.0), vol.shape):
            assert circ(got, want, n) < 1e-12, (cell, pose)


@pytest.mark.parametrize('shape', GRIDS)
def test_single_cell_gives_its_own_index(lib, shape):
    for cell in cells(shape):
        vol = np.zeros(shape)
        vol[cell] = 0.75
        for sums in (numpy_peak_sums(vol, cell, 3), pc_peak.host_peak_sums(vol, cell, 3)):
            pose = pose_from_sums(sums, cell, shape)
            for got, want, n in zip(pose, cell, shape):
                assert circ(got, float(want), n) < 1e-12, (shape, cell, pose)


def test_all_zero_volume_gives_the_cell_and_six_zero_sums(lib):
    vol = np.zeros((9, 12, 8))
    for sums in (numpy_peak_sums(vol, (8, 0, 3), 2), pc_peak.host_peak_sums(vol, (8, 0, 3), 2)):
        assert sums.tobytes() == np.zeros(6).tobytes()   # +0.0 each
        pose = pose_from_sums(sums, (8, 0, 3), vol.shape)
        assert pose == (8.0, 0.0, 3.0) and all(isinstance(p, float) for p in pose)


def test_nan_in_the_box_gives_a_nan_pose_and_no_exception(lib):
    vol = np.random.default_rng(3).random((9, 12, 8))
    vol[1, 2, 3] = np.nan
    for sums in (numpy_peak_sums(vol, (0, 1, 2), 2), pc_peak.host_peak_sums(vol, (0, 1, 2), 2)):
        assert all(math.isnan(p) for p in pose_from_sums(sums, (0, 1, 2), vol.shape))
    # outside the box the NaN is not seen
    pose = pose_from_sums(numpy_peak_sums(vol, (5, 8, 7), 1), (5, 8, 7), vol.shape)
    assert all(math.isfinite(p) for p in pose)
    # an infinite sum is not a pose either
    assert math.isnan(pose_from_sums([np.inf, 1.0, 0.0, 1.0, 0.0, 1.0], (0, 0, 0), (9, 12, 8))[0])


def test_peak_tables_are_numpys_sin_then_cos():
    for n, tab in zip((9, 12, 8), peak_tables((9, 12, 8))):
        a = 2 * np.pi * np.arange(n) / n
        assert tab.dtype == np.float64 and tab.shape == (2 * n,)
        assert tab[:n].tobytes() == np.sin(a).tobytes() and tab[n:].tobytes() == np.cos(a).tobytes()


def test_refusals(lib):
    vol = np.zeros((21, 21, 36))
    for r in (0, 4):
        with pytest.raises(ValueError):
            numpy_peak_sums(vol, (0, 0, 0), r)
        with pytest.raises(ValueError):
            pc_peak.host_peak_sums(vol, (0, 0, 0), r)
    small = np.zeros((5, 21, 36))
    with pytest.raises(ValueError):
        numpy_peak_sums(small, (0, 0, 0), 3)
    with pytest.raises(ValueError):
        pc_peak.host_peak_sums(small, (0, 0, 0), 3)
    assert pc_peak.host_peak_sums(small, (0, 0, 0), 2).tobytes() == np.zeros(6).tobytes()
    with pytest.raises(ValueError):   # a cell outside the grid
        pc_peak.host_peak_sums(vol, (21, 0, 0), 3)
    # null tables
    tabs = peak_tables(vol.shape)
    xyz = np.zeros(3, dtype=np.int32)
    sums = np.empty(6)
    f64 = ctypes.c_double
    for missing in range(3):
        args = [_lib.ptr(t, f64) if a != missing else None for a, t in enumerate(tabs)]
        st = lib.rs_pc_peak_host(21, 21, 36, 3, _lib.ptr(vol, f64), _lib.ptr(xyz, ctypes.c_int32), *args,
                                 _lib.ptr(sums, f64))
        assert st == _lib.RS_ERR_ARG


def test_rule_header_alone_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'pc_peak_main.cpp', flags=('-ffp-contract=off',), timeout=60)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
