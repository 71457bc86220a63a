"""The host rules of feedback inside an ensemble run (csrc/pce_plan.h, DESIGN section 36: what
rs_pce_run_inject refuses before any device work, the device form of a run's injections, the
pose stage's scratch), on the host: tests/pce_inj_main.cpp checks them against its own
restatement on exact-size heap arrays.  It is built with the host compiler and
-fsanitize=address,undefined and run as a child process; the sanitizer is linked into the
program, nothing is preloaded.  The second half goes through the library and the Python class
without a device: rs_pce_fit's byte counts are what they were, and the refusals that need no
device.  CPU only."""
import ctypes

import numpy as np
import pytest

import _host_program
from pyratslam_amd import _build, _lib


def test_injection_rules_and_pose_scratch_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'pce_inj_main.cpp', include=('include',), timeout=120)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


# rs_pce_fit's bytes before the pose and the injections existed (the pose adds no LDS region)
FIT_BYTES = {(21, 21, 36): 135648, (32, 32, 18): 132160, (8, 8, 8): 11488, (12, 9, 10): 16256,
             (50, 50, 10): 157584, (7, 7, 7): 9248, (64, 64, 36): 812800}


def plan_bytes(shape):
    x, y, th = shape
    al = lambda v: (v + 15) // 16 * 16   # noqa: E731
    total = 0
    for n in (256, 4 * x * y * (th | 1), 4 * 2 * y * th * 11, 4 * 16 * 49, 2 * al(32 + 5 * th)):
        total = al(total + n)
    return total


@pytest.mark.parametrize('shape', sorted(FIT_BYTES))
def test_fit_bytes_are_unchanged(lib, shape):
    n = ctypes.c_size_t(0)
    lib.rs_pce_fit(*shape, ctypes.byref(n))
    assert n.value == FIT_BYTES[shape] == plan_bytes(shape)


def test_null_handle_and_symbols(lib):
    for name in ('rs_pce_set_peak_tables', 'rs_pce_get_peak', 'rs_pce_run_inject'):
        assert name in _lib.SIGNATURES
    t = np.zeros(16)
    p = _lib.ptr(t, ctypes.c_double)
    assert lib.rs_pce_set_peak_tables(None, 3, p, p, p) == _lib.RS_ERR_STATE
    assert lib.rs_pce_get_peak(None, None, None) == _lib.RS_ERR_STATE
    assert lib.rs_pce_run_inject(None, 0, None, None, None, None, 0, None, None, None, None, None, None,
                                 None) == _lib.RS_ERR_STATE


def test_python_refusals_need_no_device():
    from pyratslam_amd import PoseCellEnsemble as E
    for r in (0, 4, 1.5):
        with pytest.raises(ValueError, match='cells_to_avg'):
            E(4, (21, 21, 36), cells_to_avg=r)
    with pytest.raises(ValueError):                    # (the plan's refusal still comes first)
        E(4, (64, 64, 36), cells_to_avg=3)


def arrays(injections, members=3, shape=(12, 9, 10), n=6):
    from pyratslam_amd import PoseCellEnsemble as E
    return E.injection_arrays(members, shape, n, injections)


def test_injection_arrays_expand_and_remap():
    from pyratslam_amd import PoseCellEnsemble as E
    member, step, energy, loc = arrays([(None, 0, 0.5, E.AT_PEAK), (1, 2, 0.25, (1, -1, 3)), (None, 2, -1.0, ('same', 0)),
                                        (1, 6, 2.0, ('same', 1))])
    assert member.tolist() == [0, 1, 2, 1, 0, 1, 2, 1]
    assert step.tolist() == [0, 0, 0, 2, 2, 2, 2, 6]
    assert energy.tolist() == [0.5, 0.5, 0.5, 0.25, -1.0, -1.0, -1.0, 2.0]
    assert loc[:3, 0].tolist() == [_lib.RS_PC_INJ_AT_PEAK] * 3
    assert loc[3].tolist() == [1, 8, 3]                      # inject()'s index rule
    assert loc[4:7, :2].tolist() == [[_lib.RS_PC_INJ_SAME_AS, k] for k in (0, 1, 2)]   # the same member's copy
    assert loc[7, :2].tolist() == [_lib.RS_PC_INJ_SAME_AS, 3]
    assert all(len(a) == 0 for a in arrays([]))


@pytest.mark.parametrize('bad,exc', [
    ([(3, 0, 1.0, (0, 0, 0))], IndexError),                       # a member outside the ensemble
    ([(-1, 0, 1.0, (0, 0, 0))], IndexError),
    ([(0, 7, 1.0, (0, 0, 0))], ValueError),                       # a step outside 0 .. n
    ([(0, -1, 1.0, (0, 0, 0))], ValueError),
    ([(0, 1.5, 1.0, (0, 0, 0))], ValueError),
    ([(0, 3, 1.0, (0, 0, 0)), (1, 1, 1.0, (0, 0, 0)), (0, 2, 1.0, (0, 0, 0))], ValueError),   # order within a member
    ([(1, 3, 1.0, (0, 0, 0)), (None, 2, 1.0, (0, 0, 0))], ValueError),
    ([(0, 0, 1.0, (12, 0, 0))], IndexError),                      # a cell outside the grid
    ([(0, 0, 1.0, (0, 0, -11))], IndexError),
    ([(0, 0, 1.0, [0, 0, 0])], TypeError),                        # inject()'s tuple rule
    ([(0, 0, 1.0, ('same', 0))], ValueError),                     # same-as no earlier one
    ([(0, 0, 1.0, (0, 0, 0)), (0, 0, 1.0, ('same', 1))], ValueError),
    ([(0, 0, 1.0, (0, 0, 0)), (1, 0, 1.0, ('same', 0))], ValueError),      # same-as of another member
    ([(0, 0, 1.0, (0, 0, 0)), (None, 0, 1.0, ('same', 0))], ValueError),
    ([(0, 0, float('nan'), (0, 0, 0))], ValueError),              # not a finite float32
    ([(0, 0, float('inf'), (0, 0, 0))], ValueError),
    ([(0, 0, 1e39, (0, 0, 0))], ValueError),
])
def test_injection_arrays_refuse(bad, exc):
    with pytest.raises(exc):
        arrays(bad)


def test_injection_arrays_accept_free_order_across_members():
    member, step, _, _ = arrays([(2, 5, 1.0, (0, 0, 0)), (0, 1, 1.0, (0, 0, 0)), (2, 5, 1.0, (0, 0, 0)), (1, 0, 1.0, (0, 0, 0))])
    assert member.tolist() == [2, 0, 2, 1] and step.tolist() == [5, 1, 5, 0]
