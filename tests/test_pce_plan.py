"""The pose-cell ensemble's host rules (csrc/pce_plan.h: the LDS plan pce_fit, the control
record, the split of a run into launches), on the host: tests/pce_plan_main.cpp checks them
against its own restatement.  It is built with the host compiler and
-fsanitize=address,undefined and run as a child process; the sanitizer is linked into the
program, nothing is preloaded.  The second half goes through the library's C ABI without a
device: rs_pce_fit against the plan, and rs_pce_create's refusals.  CPU only."""
import ctypes
import re

import pytest

import _host_program
from pyratslam_amd import _build, _lib
from pyratslam_amd import filters as F

LDS_BYTES = 160 * 1024


def test_plan_record_and_chunks_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'pce_plan_main.cpp', include=('include',), timeout=60)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def plan_bytes(shape):
    """pce_plan.h's sizes restated: red, state (odd theta pitch), temp + ring (11 plane
    pairs), 16 filters, two control records, each region 16-byte aligned."""
    x, y, th = shape
    al = lambda v: (v + 15) // 16 * 16   # noqa: E731
    total = 0
    for n in (256, 4 * x * y * (th | 1), 4 * 2 * y * th * 11, 4 * 16 * 49, 2 * al(32 + 5 * th)):
        total = al(total + n)
    return total


@pytest.mark.parametrize('shape,fits', [((21, 21, 36), True), ((32, 32, 18), True), ((8, 8, 8), True),
                                        ((12, 9, 10), True), ((50, 50, 10), True), ((7, 7, 7), True),
                                        ((64, 64, 36), False), ((6, 21, 36), False), ((21, 21, 6), False)])
def test_fit_through_the_abi_agrees_with_the_plan(lib, shape, fits):
    n = ctypes.c_size_t(0)
    st = lib.rs_pce_fit(*shape, ctypes.byref(n))
    assert (st == _lib.RS_OK) == fits
    assert n.value == plan_bytes(shape)
    if fits:
        assert n.value <= LDS_BYTES
    else:
        assert st == _lib.RS_ERR_ARG
        msg = lib.rs_last_error().decode()
        if min(shape) >= 7:   # the message carries the bytes needed
            assert str(n.value) in msg and n.value > LDS_BYTES


def _params(precision=_lib.RS_PREC_F32):
    table = F.FilterTable()
    filters = table.filters.astype('float64').copy()
    ge, gi, scale = F.separable_factors()
    p = _lib.PcParams()
    p.precision = precision
    p.global_inhibition = F.PC_GLOBAL_INHIB
    p.ge[:] = list(ge)
    p.gi[:] = list(gi)
    p.k_scale = scale
    p.nfilters = filters.shape[0]
    p.xy_filters = _lib.ptr(filters, ctypes.c_double)
    return p, filters


@pytest.mark.parametrize('members,shape,precision', [(0, (21, 21, 36), _lib.RS_PREC_F32),
                                                     (4, (21, 6, 36), _lib.RS_PREC_F32),
                                                     (4, (64, 64, 36), _lib.RS_PREC_F32),
                                                     (4, (21, 21, 36), _lib.RS_PREC_F64)])
def test_create_refuses_before_any_device_call(lib, members, shape, precision):
    p, keep = _params(precision)
    h = ctypes.c_void_p(0xdead)
    st = lib.rs_pce_create(members, *shape, ctypes.byref(p), None, 0, ctypes.byref(h))
    assert st == _lib.RS_ERR_ARG
    assert not h.value
    assert lib.rs_last_error()
    if shape == (64, 64, 36):
        assert re.search(r'\b%d\b' % plan_bytes(shape), lib.rs_last_error().decode())
    del keep


def test_python_refusals_need_no_device():
    from pyratslam_amd import PoseCellEnsemble
    assert PoseCellEnsemble.fits((21, 21, 36)) and PoseCellEnsemble.fits((50, 50, 10))
    assert not PoseCellEnsemble.fits((64, 64, 36)) and not PoseCellEnsemble.fits((21, 21, 6))
    with pytest.raises(ValueError, match=str(plan_bytes((64, 64, 36)))):
        PoseCellEnsemble(4, (64, 64, 36))
    with pytest.raises(ValueError):
        PoseCellEnsemble(4, (21, 21, 36), precision='float64')
    with pytest.raises(ValueError):
        PoseCellEnsemble(0, (21, 21, 36))
