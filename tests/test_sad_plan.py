"""The summation plan of the float view-template scan, evaluated on the host
(rs_sad_plan_sum: no device), equals numpy's np.sum bit for bit -- the plan is
numpy's pairwise summation lowered to leaves, 8 accumulator chains per leaf, the
fixed chain combine, the sequential tail and the postfix tree over the leaves, and
the scan kernel executes the same plan with one chain per lane."""
import ctypes

import numpy as np
import pytest

from pyratslam_amd import _build, _lib

DTYPES = [(np.float32, _lib.RS_DT_F32), (np.float64, _lib.RS_DT_F64)]
EXTRA_N = [3, 140, 160, 512, 792, 1536, 4096, 65537]


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def plan_sum(lib, x, code):
    x = np.ascontiguousarray(x)
    out = np.empty(1, dtype=x.dtype)
    _lib.check(lib.rs_sad_plan_sum(code, x.size, ctypes.c_void_p(x.ctypes.data),
                                   ctypes.c_void_p(out.ctypes.data)))
    return out[0]


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize('dt,code', DTYPES)
@pytest.mark.parametrize('scale', [255.0, 1.0])
def test_every_n_to_2200(lib, dt, code, scale):
    """Leaves shorter than 8, every len % 8 tail, one leaf, two, the uneven trees."""
    data = (np.random.default_rng(5).random(2200) * scale).astype(dt)
    bad = [n for n in range(1, 2201) if not same_bits(plan_sum(lib, data[:n], code), np.sum(data[:n]))]
    assert not bad, bad[:10]


@pytest.mark.parametrize('dt,code', DTYPES)
@pytest.mark.parametrize('n', EXTRA_N)
def test_named_sizes(lib, dt, code, n):
    rng = np.random.default_rng(n)
    for scale in (255.0, 1.0):
        x = (rng.random(n) * scale).astype(dt)
        got = plan_sum(lib, x, code)
        assert got.dtype == dt and same_bits(got, np.sum(x)), (n, scale, got, np.sum(x))


@pytest.mark.parametrize('dt,code', DTYPES)
@pytest.mark.parametrize('n', [3, 140, 792, 1536])
def test_one_inf_and_subnormals(lib, dt, code, n):
    rng = np.random.default_rng(100 + n)
    x = (rng.random(n) * 255).astype(dt)
    x[n // 2] = np.inf
    assert same_bits(plan_sum(lib, x, code), np.sum(x)) and np.isinf(np.sum(x))
    tiny = np.finfo(dt).smallest_subnormal
    sub = (rng.integers(1, 1000, n) * tiny).astype(dt)
    assert 0 < np.sum(sub) < np.finfo(dt).tiny          # the sum itself stays subnormal
    assert same_bits(plan_sum(lib, sub, code), np.sum(sub))


def test_argument_errors(lib):
    x = np.zeros(4)
    out = np.zeros(1)
    xp, op = ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    with pytest.raises(TypeError):
        _lib.check(lib.rs_sad_plan_sum(7, 4, xp, op))
    with pytest.raises(ValueError):
        _lib.check(lib.rs_sad_plan_sum(_lib.RS_DT_F64, 0, xp, op))
    with pytest.raises(ValueError):
        _lib.check(lib.rs_sad_plan_sum(_lib.RS_DT_F64, 4, None, op))
