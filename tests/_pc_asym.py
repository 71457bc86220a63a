"""Asymmetric pose-cell cases shared by test_pc_orientation.py and test_pc_orientation_gpu.py.

The product's own step parameters hide an orientation mistake: its two Gaussians are
centred (``g[t] == g[6 - t]``), the two path filters its control can select equal their
transposes, and the inhibition is one value everywhere.  The cases built here break each
of those symmetries, deterministically from a seed and with no fixture file:

* ``ge``, ``gi``, every row of an 8-row filter table and every ``zf`` carry a linear tilt;
* per step and per layer, shifts in [-10, 10] and ``fidx = (3k + s) % 8``;
* three injections of unequal energy, one next to a corner.

The reference step is the float64 oracle's 343-tap periodic correlation
(``oracle.posecell.conv3d_wrap``) with the kernel built from ``ge``, ``gi`` and ``k_scale``,
then the relu at the inhibition, the normalisation, ``conv_xy_shift`` with ``table[fidx]``,
``conv_z_wrap`` and the first argmax in C order: the definition, not the separable form the
HIP kernels evaluate.
"""
import ctypes
import functools

import numpy as np

from oracle import posecell as P
from pyratslam_amd import filters as F

F32_TOL = 1e-5
F64_TOL = 1e-12
STEPS = 6
INHIBITION = 0.004
# the most rows the cols, stream and halo forms stage: row 7 sits at their limit
ORIGINS = [(-1, 0), (0, -1), (1, 0), (0, 1), (1, -1), (-1, 1), (0, 0), (-1, -1)]
# |shift| > 3 lies beyond the 7-tap window.  No form narrows it: every path kernel reduces
# a shift modulo the grid extent before it forms a window (rs::wrapi in the rows and stream
# kernels, co_centre in the cols and halo kernels and in the host's union window), so the
# single-conditional wraps behind them see |shift| <= extent / 2 whatever the control holds
SHIFT_MAX = 10
# seeds at which every step's peak is unambiguous (test_pc_orientation.py checks it)
SEEDS = {(16, 40, 10): 0, (24, 40, 13): 3, (16, 16, 36): 2, (17, 30, 18): 3, (20, 24, 10): 2}

MISTAKES = ('reverse_ge', 'reverse_gi', 'transpose_filters', 'flip_filters_x', 'flip_filters_y',
            'reverse_zf', 'swap_ox_oy', 'negate_ox', 'shift_fidx', 'inhibition_0.2')


def _tilt(n=7):
    return np.arange(n) - n // 2


def gaussians():
    """(ge, gi, k_scale): the product's factors tilted, ``k_scale = 1 / |sum K|``."""
    ge0, gi0, _ = F.separable_factors()
    ge = ge0 * (1 + 0.10 * _tilt())
    gi = gi0 * (1 - 0.07 * _tilt())
    return ge, gi, 1.0 / abs(kernel_sum(ge, gi))


def kernel_sum(ge, gi):
    return (np.einsum('i,j,k->ijk', ge, ge, ge) - np.einsum('i,j,k->ijk', gi, gi, gi)).sum()


def kernel_3d(ge, gi, k_scale):
    """The 343-tap kernel K = (ge x ge x ge - gi x gi x gi) * k_scale of rs_pc_params."""
    return (np.einsum('i,j,k->ijk', ge, ge, ge) - np.einsum('i,j,k->ijk', gi, gi, gi)) * k_scale


def filter_table():
    """(8, 7, 7): row r = filter_2d(ORIGINS[r]) tilted along both filter axes, x the first."""
    t = _tilt()
    tilt = 1 + 0.06 * t[:, None] - 0.04 * t[None, :]
    return np.ascontiguousarray(np.stack([F.filter_2d(o) * tilt for o in ORIGINS]), dtype=np.float64)


def product_table():
    return np.ascontiguousarray(F.FilterTable().filters, dtype=np.float64)


def control(shape, seed, steps=STEPS, nrows=8, tilt_zf=True, shift_max=SHIFT_MAX):
    """Per-step control, step-major as the batched ABI takes it: ox, oy, fidx (steps, TH)
    int32 and zf (steps, 7) float64."""
    th = shape[2]
    rng = np.random.default_rng(seed)
    ox = rng.integers(-shift_max, shift_max + 1, (steps, th)).astype(np.int32)
    oy = rng.integers(-shift_max, shift_max + 1, (steps, th)).astype(np.int32)
    k = np.arange(th)
    fidx = np.stack([(3 * k + s) % nrows for s in range(steps)]).astype(np.int32)
    zo = rng.integers(-2, 3, steps)
    zf = np.stack([F.filter_1d(int(o)) * (1 + 0.05 * _tilt() if tilt_zf else 1.0) for o in zo])
    return dict(ox=np.ascontiguousarray(ox), oy=np.ascontiguousarray(oy), fidx=np.ascontiguousarray(fidx),
                zf=np.ascontiguousarray(zf, dtype=np.float64))


def injections(shape):
    """Three unequal energies at non-centred cells; the last one's packet wraps round the
    (0, 0, 0) corner."""
    X, Y, TH = shape
    return [(1.0, (X // 3, (2 * Y) // 3, TH // 4)), (0.6, ((3 * X) // 4, Y // 5, (2 * TH) // 3)),
            (0.35, (X - 1, 1, 0))]


class Case:
    """One shape's inputs: the parameters of rs_pc_create, the injections and the control."""

    def __init__(self, shape, seed, ge, gi, k_scale, inhibition, table, ctl):
        self.shape, self.seed = tuple(shape), seed
        self.ge, self.gi, self.k_scale, self.inhibition, self.table = ge, gi, k_scale, inhibition, table
        self.ctl = ctl
        self.steps = ctl['ox'].shape[0]
        self.inject = injections(shape)


@functools.lru_cache(maxsize=None)
def asym_case(shape):
    ge, gi, k_scale = gaussians()
    return Case(shape, SEEDS[shape], ge, gi, k_scale, INHIBITION, filter_table(), control(shape, SEEDS[shape]))


# The product's Gaussians, table and theta filters at another inhibition.  The control keeps
# the packets whole (one shift for all layers of a step, still beyond the window), because a
# network whose activity the per-layer shifts scatter dies at an inhibition of this size.
PRODUCT_INHIBITION = 0.05


@functools.lru_cache(maxsize=None)
def product_case(shape):
    ge, gi, scale = F.separable_factors()
    table = product_table()
    ctl = control(shape, 100 + SEEDS[shape], nrows=table.shape[0], tilt_zf=False)
    ctl['ox'][:] = ctl['ox'][:, :1]
    ctl['oy'][:] = ctl['oy'][:, :1]
    return Case(shape, 100 + SEEDS[shape], ge, gi, scale, PRODUCT_INHIBITION, table, ctl)


# ----------------------------------------------------------------------------
# The reference, float64
# ----------------------------------------------------------------------------
def ref_excite(p, k3, inhibition):
    """Excitation, global inhibition, normalisation: what rs_pc_excite computes.  Returns
    the new state and the total it was divided by."""
    p = P.conv3d_wrap(p, k3)
    p = np.where(p < inhibition, 0.0, p - inhibition)
    total = p.sum()
    if total != 0:
        p = p / total
    return p, total


def ref_path(p, table, ox, oy, fidx, zf):
    p = P.conv_xy_shift(p, ox, oy, np.moveaxis(table[fidx], 0, -1))
    p[p < 0] = 0
    p = P.conv_z_wrap(p, zf)
    p[p < 0] = 0
    return p


def first_argmax(p):
    return tuple(int(v) for v in np.unravel_index(np.argmax(p), p.shape))


def initial_state(case):
    p = np.zeros(case.shape)
    for energy, loc in case.inject:
        p[loc] += energy
    return p


def reference(case, mistake=None):
    """The rollout of ``case``: (states after every step, peaks, totals).  ``mistake`` names
    one orientation mistake an implementation could make; the rollout then makes it."""
    ge, gi, table, inhibition = case.ge, case.gi, case.table, case.inhibition
    ctl = {k: v.copy() for k, v in case.ctl.items()}
    if mistake == 'reverse_ge':
        ge = ge[::-1]
    elif mistake == 'reverse_gi':
        gi = gi[::-1]
    elif mistake == 'transpose_filters':
        table = table.transpose(0, 2, 1)
    elif mistake == 'flip_filters_x':
        table = table[:, ::-1, :]
    elif mistake == 'flip_filters_y':
        table = table[:, :, ::-1]
    elif mistake == 'reverse_zf':
        ctl['zf'] = ctl['zf'][:, ::-1]
    elif mistake == 'swap_ox_oy':
        ctl['ox'], ctl['oy'] = ctl['oy'], ctl['ox']
    elif mistake == 'negate_ox':
        ctl['ox'] = -ctl['ox']
    elif mistake == 'shift_fidx':
        ctl['fidx'] = (ctl['fidx'] + 1) % table.shape[0]
    elif mistake == 'inhibition_0.2':
        inhibition = 0.2
    elif mistake is not None:
        raise ValueError(mistake)
    k3 = kernel_3d(ge, gi, case.k_scale)
    p = initial_state(case)
    states, peaks, totals = [], [], []
    for s in range(case.steps):
        p, total = ref_excite(p, k3, inhibition)
        p = ref_path(p, table, ctl['ox'][s], ctl['oy'][s], ctl['fidx'][s], ctl['zf'][s])
        states.append(p)
        peaks.append(first_argmax(p))
        totals.append(total)
    return states, peaks, totals


@functools.lru_cache(maxsize=None)
def asym_reference(shape):
    """reference(asym_case(shape)), computed once; the arrays are read-only."""
    out = reference(asym_case(shape))
    for p in out[0]:
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def product_reference(shape):
    out = reference(product_case(shape))
    for p in out[0]:
        p.setflags(write=False)
    return out


# ----------------------------------------------------------------------------
# The ctypes driver
# ----------------------------------------------------------------------------
def create(lib, shape, precision, table, ge=None, gi=None, k_scale=None, inhibition=0.2):
    """rs_pc_create with an explicit path-filter table (and, where given, Gaussians, scale
    and inhibition; the product's otherwise); returns the handle."""
    from pyratslam_amd import _lib
    if ge is None:
        ge, gi, k_scale = F.separable_factors()
    params = _lib.PcParams()
    params.precision = _lib.RS_PREC_F32 if precision == 'float32' else _lib.RS_PREC_F64
    params.global_inhibition = inhibition
    params.ge[:] = list(ge)
    params.gi[:] = list(gi)
    params.k_scale = k_scale
    params.nfilters = table.shape[0]
    params.xy_filters = _lib.ptr(table, ctypes.c_double)
    h = ctypes.c_void_p()
    _lib.check(lib.rs_pc_create(*shape, ctypes.byref(params), 0, ctypes.byref(h)))
    return h


def create_case(lib, case, precision):
    return create(lib, case.shape, precision, case.table, case.ge, case.gi, case.k_scale, case.inhibition)


def read_state(lib, h, shape):
    from pyratslam_amd import _lib
    vol = np.empty(shape, dtype=np.float64)
    _lib.check(lib.rs_pc_read(h, _lib.ptr(vol, ctypes.c_double)))
    return vol


def drive(lib, case, precision, batched):
    """A fresh handle through the case: rs_pc_update per step, or one rs_pc_run.  Returns
    (step form, peaks, final state)."""
    from pyratslam_amd import _lib
    i32, f64 = ctypes.c_int32, ctypes.c_double
    c, n, th = case.ctl, case.steps, case.shape[2]
    h = create_case(lib, case, precision)
    try:
        form = lib.rs_pc_step_form(h).decode()
        for energy, loc in case.inject:
            _lib.check(lib.rs_pc_inject(h, energy, *loc))
        out = np.full((n, 3), -1, dtype=np.int32)
        if batched:
            _lib.check(lib.rs_pc_run(h, n, _lib.ptr(c['ox'], i32), _lib.ptr(c['oy'], i32), _lib.ptr(c['fidx'], i32),
                                     _lib.ptr(c['zf'], f64), _lib.ptr(out, i32)))
        else:
            for s in range(n):
                ox, oy, fi, zf, o = (np.ascontiguousarray(a[s]) for a in (c['ox'], c['oy'], c['fidx'], c['zf'], out))
                assert len(ox) == th
                _lib.check(lib.rs_pc_update(h, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(fi, i32),
                                            _lib.ptr(zf, f64), _lib.ptr(o, i32)))
                out[s] = o
        state = read_state(lib, h, case.shape)
    finally:
        _lib.check(lib.rs_pc_destroy(h))
    return form, [tuple(int(v) for v in r) for r in out], state
