"""Dense pose-cell cases shared by test_pc_dense.py and test_pc_dense_gpu.py.

Every other pose-cell test steps a localised packet and compares states with an absolute
bound: most of the volume is exactly 0, so a tile seam, a grid face, a ragged tile or a
block's share of the global total that the packet never touches cannot change a compared
number.  The cases here start from ``uniform(0.5, 1.5)`` divided by its sum (rounded to
float32 values, so both precisions start from the same numbers) with an inhibition of a
quarter of the mean cell, ``0.25 / (X * Y * TH)``: every cell stays strictly positive
step after step, and the comparison is per cell and relative,

    |got - want| <= B * want,    B32 = 32 * e32,    B64 = B32 * 2^-29,

where ``e32`` is the largest per-cell relative difference between the reference below run
with float32 arrays and the same reference in float64 (measured on the CPU, per parameter
set, and kept in ``E32``; test_pc_dense.py recomputes it).  The factor 32 covers the
kernels' other summation order (separable passes against 343 direct taps) and fused
multiply-adds; 2^-29 is the ratio of the two formats' epsilons.

Wide filters average a fault away, so three of the four parameter sets isolate one stage
with the others one-hot (a single 1 at an off-centre tap, so orientation still matters):

    E    wide K, one-hot table rows (the 1 at eight different taps), one-hot zf
    P    one-hot K (ge one-hot, gi = 0, k_scale = 1), wide tilted table, one-hot zf
    Z    one-hot K, one-hot table, wide tilted zf
    ALL  all three wide: the state tends to uniform, the near-tie case of the halo form

"Wide" is a strictly positive 7-tap Gaussian with a linear tilt, normalised; the wide K
is ``(ge x ge x ge - gi x gi x gi) * k_scale`` with ``gi`` a small fraction of another wide
filter, so all 343 taps are positive.

The reference step is the float64 oracle's definition as in _pc_asym (the 343-tap periodic
correlation, the relu at the inhibition, the normalisation, conv_xy_shift with
table[fidx], conv_z_wrap, the first argmax in C order), restated here so that it runs in
either precision, skips taps that are exactly 0 and can make one planted mistake;
test_pc_dense.py checks it byte for byte against ``_pc_asym.ref_excite`` / ``ref_path``.
"""
import ctypes
import functools

import numpy as np

import _pc_asym as A
from oracle import posecell as P

SETS = ('E', 'P', 'Z', 'ALL')
STEPS = {'E': 2, 'P': 2, 'Z': 2, 'ALL': 3}
FACTOR = 32
F64_RATIO = 2.0 ** -29
HALO_NEAR = 2.0 ** -20          # the halo form's near-tie margin (RES_AMBIG), relative

# e32 per set: the largest over SHAPES and steps, as measured on the CPU (float32 emulation
# of the reference against the float64 reference; test_pc_dense.py::test_e32_constants)
E32 = {'E': 1.62e-6, 'P': 5.27e-7, 'Z': 2.92e-7, 'ALL': 4.09e-7}

SHAPES = [(16, 16, 36), (17, 30, 18), (21, 21, 36), (50, 50, 10), (64, 64, 36),   # halo
          (16, 40, 10), (48, 40, 20),                                            # rows
          (24, 40, 13), (32, 32, 20)]                                            # cols, stream
HALO_SHAPES = SHAPES[:5]
# seeds, chosen on the CPU, at which the reference's top-two gap exceeds 100 * B32 (P, Z: at
# every step; E: at the first, see reference()), and, on the halo shapes, at which ALL's
# last state has a cell within 2^-22 of its peak (any other case: seed 0)
SEEDS = {('E', (16, 16, 36)): 12, ('E', (17, 30, 18)): 9, ('E', (21, 21, 36)): 32, ('E', (50, 50, 10)): 19,
         ('E', (64, 64, 36)): 10, ('E', (16, 40, 10)): 58, ('E', (48, 40, 20)): 34, ('E', (24, 40, 13)): 50,
         ('E', (32, 32, 20)): 23,
         ('P', (16, 16, 36)): 0, ('P', (17, 30, 18)): 0, ('P', (21, 21, 36)): 1, ('P', (50, 50, 10)): 0,
         ('P', (64, 64, 36)): 0, ('P', (16, 40, 10)): 4, ('P', (48, 40, 20)): 1, ('P', (24, 40, 13)): 4,
         ('P', (32, 32, 20)): 1,
         ('Z', (16, 16, 36)): 0, ('Z', (17, 30, 18)): 0, ('Z', (21, 21, 36)): 0, ('Z', (50, 50, 10)): 0,
         ('Z', (64, 64, 36)): 0, ('Z', (16, 40, 10)): 0, ('Z', (48, 40, 20)): 1, ('Z', (24, 40, 13)): 0,
         ('Z', (32, 32, 20)): 1,
         ('ALL', (16, 16, 36)): 27, ('ALL', (17, 30, 18)): 4, ('ALL', (21, 21, 36)): 21, ('ALL', (50, 50, 10)): 82,
         ('ALL', (64, 64, 36)): 26}

MISTAKES = ('tap_E', 'tap_P', 'tap_Z', 'edge_x', 'edge_y', 'edge_th', 'halo_zero', 'ox_off', 'norm_tile')
TILE = 16                       # the tile of the planted halo and normalisation mistakes

# the product-parameter test through the Python class
PRODUCT_SHAPES = [(21, 21, 36), (32, 32, 18), (50, 50, 10), (64, 64, 36)]
PRODUCT_SEEDS = tuple(range(10))
PRODUCT_V = (0.37, 0.11)
# the float32 emulation's largest error relative to the reference's maximum, per shape
E32_PRODUCT = {(21, 21, 36): 2.06e-6, (32, 32, 18): 1.78e-6, (50, 50, 10): 1.72e-6, (64, 64, 36): 1.66e-6}


def b32(name):
    return FACTOR * E32[name]


def bound(name, precision):
    return b32(name) * (1.0 if precision == 'float32' else F64_RATIO)


# ----------------------------------------------------------------------------
# Filters
# ----------------------------------------------------------------------------
def wide(sigma, tilt):
    t = A._tilt().astype(np.float64)
    g = np.exp(-t * t / (2.0 * sigma * sigma)) * (1 + tilt * t)
    return g / g.sum()


def one_hot(at, n=7):
    g = np.zeros(n)
    g[at] = 1.0
    return g


def wide_k():
    ge = wide(5.0, 0.03)
    gi = 0.3 * wide(3.5, -0.07)
    return ge, gi, 1.0 / abs(A.kernel_sum(ge, gi))


def one_hot_k():
    return one_hot(4), np.zeros(7), 1.0


TABLE_TILT_X = (0.09, 0.07, 0.05, 0.03, -0.03, -0.05, -0.07, -0.09)
TABLE_TILT_Y = (-0.05, 0.08, -0.03, 0.06, -0.08, 0.04, -0.06, 0.03)


def wide_table():
    rows = []
    for r in range(8):
        f = np.outer(wide(2.0 + 0.2 * r, TABLE_TILT_X[r]), wide(3.4 - 0.2 * r, TABLE_TILT_Y[r]))
        rows.append(f / f.sum())
    return np.ascontiguousarray(np.stack(rows))


ONE_HOT_TAPS = [(0, 2), (6, 5), (2, 6), (5, 0), (1, 4), (4, 6), (6, 2), (2, 1)]


def one_hot_table():
    table = np.zeros((8, 7, 7))
    for r, (x, y) in enumerate(ONE_HOT_TAPS):
        table[r, x, y] = 1.0
    return table


def wide_zf(steps):
    return np.stack([wide(2.2 + 0.4 * s, 0.05 if s % 2 else -0.05) for s in range(steps)])


def one_hot_zf(steps):
    return np.stack([one_hot((2, 5, 1)[s % 3]) for s in range(steps)])


# ----------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------
def start_state(shape, seed):
    p = np.random.default_rng(1000 + seed).uniform(0.5, 1.5, shape)
    return (p / p.sum()).astype(np.float32).astype(np.float64)


class Case:
    """One set on one shape: the parameters of rs_pc_create (the attribute names of
    _pc_asym.Case, so _pc_asym.create_case takes it), the start state and the control."""

    def __init__(self, name, shape, seed):
        self.name, self.shape, self.seed = name, tuple(shape), seed
        self.steps = STEPS[name]
        self.ge, self.gi, self.k_scale = wide_k() if name in ('E', 'ALL') else one_hot_k()
        self.table = wide_table() if name in ('P', 'ALL') else one_hot_table()
        self.inhibition = 0.25 / float(np.prod(shape))
        self.ctl = A.control(shape, seed, steps=self.steps)
        zf = wide_zf(self.steps) if name in ('Z', 'ALL') else one_hot_zf(self.steps)
        self.ctl['zf'] = np.ascontiguousarray(zf, dtype=np.float64)
        self.start = start_state(shape, seed)
        self.start.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name, shape, seed=None):
    return Case(name, shape, SEEDS.get((name, shape), 0) if seed is None else seed)


# ----------------------------------------------------------------------------
# The reference, in either precision, with one planted mistake
# ----------------------------------------------------------------------------
def corr_valid(pp, k3):
    """sum_t k3[t] * pp[i + t] over the window that fits, taps in the oracle's order (x
    outer, then y, then z); a tap that is exactly 0 adds nothing and is skipped."""
    n = k3.shape[0]
    X, Y, Z = (s - n + 1 for s in pp.shape)
    acc = np.zeros((X, Y, Z), dtype=pp.dtype)
    for x in range(n):
        for y in range(n):
            for z in range(n):
                if k3[x, y, z] != 0:
                    acc += pp[x:x + X, y:y + Y, z:z + Z] * k3[x, y, z]
    return acc


def smallest_tap(f):
    """Index of the smallest non-zero tap."""
    return np.unravel_index(np.argmin(np.where(f != 0, f, np.inf)), f.shape)


def mistake_cell(shape):
    return (shape[0] // 3, (2 * shape[1]) // 3, shape[2] // 2)


def step(p, k3, inhibition, filters, ox, oy, zf, mistake=None, cell=None):
    """One update in p's precision.  ``filters`` is (7, 7, TH), a filter per layer.  Returns
    the new state and the total the excited state was divided by.  ``cell``: where a
    mistake that has a place is planted (mistake_cell otherwise)."""
    dt = p.dtype.type
    shape = p.shape
    X, Y, TH = shape
    h = P.HALF
    k3, filters, zf = k3.astype(dt), filters.astype(dt), zf.astype(dt)
    c = mistake_cell(shape) if cell is None else tuple(cell)
    tx, ty = min(TILE, X), min(TILE, Y)
    # excitation
    pp = np.pad(p, h, mode='wrap')
    if mistake == 'edge_x':                 # the high face pads with its edge, not the wrap
        pp[-h:] = pp[-h - 1:-h]
    elif mistake == 'edge_y':
        pp[:, -h:] = pp[:, -h - 1:-h]
    elif mistake == 'edge_th':
        pp[:, :, -h:] = pp[:, :, -h - 1:-h]
    q = corr_valid(pp, k3)
    if mistake == 'tap_E':                  # one cell loses its smallest excitation tap
        t = smallest_tap(k3)
        q[c] -= k3[t] * pp[c[0] + t[0], c[1] + t[1], c[2] + t[2]]
    elif mistake == 'halo_zero':            # the tile at the origin reads zeros beyond its high-x side
        win = pp[np.arange(tx + 2 * h)[:, None], np.arange(ty + 2 * h)[None, :], :].copy()
        win[tx + h:] = 0
        q[:tx, :ty] = corr_valid(win, k3)
    inh = dt(inhibition)
    q = np.where(q < inh, dt(0), q - inh)
    total = q.sum()
    if mistake == 'norm_tile':              # the total omits one tile's cells
        total = total - q[:tx, :ty].sum()
    if total != 0:
        q = q / total
    # path integration
    ox = np.array(ox)
    if mistake == 'ox_off':                 # one layer's shift is off by one
        ox[c[2]] += 1
    r = P.conv_xy_shift(q, ox, oy, filters)
    if mistake == 'tap_P':
        i, j, k = c
        t = smallest_tap(filters[:, :, k])
        r[c] -= filters[t[0], t[1], k] * q[(i + t[0] - h + ox[k]) % X, (j + t[1] - h + oy[k]) % Y, k]
    r[r < 0] = 0
    out = P.conv_z_wrap(r, zf)
    if mistake == 'tap_Z':
        t = smallest_tap(zf)[0]
        out[c] -= zf[t] * r[c[0], c[1], (c[2] + t - h) % TH]
    out[out < 0] = 0
    assert out.dtype == p.dtype and total.dtype == p.dtype
    return out, total


def rollout(cs, dtype=np.float64, mistake=None):
    """(states after every step, peaks, totals) of ``cs`` in ``dtype``."""
    k3 = A.kernel_3d(cs.ge, cs.gi, cs.k_scale)
    p = cs.start.astype(dtype)
    states, peaks, totals = [], [], []
    for s in range(cs.steps):
        c = cs.ctl
        filters = np.moveaxis(cs.table[c['fidx'][s]], 0, -1)
        p, total = step(p, k3, cs.inhibition, filters, c['ox'][s], c['oy'][s], c['zf'][s], mistake)
        states.append(p)
        peaks.append(A.first_argmax(p))
        totals.append(float(total))
    return states, peaks, totals


def top_gap(p):
    """The gap between the largest and the second largest cell, relative to the largest."""
    top = np.partition(p.ravel(), p.size - 2)[-2:]
    return float((top[1] - top[0]) / top[1])


@functools.lru_cache(maxsize=None)
def reference(name, shape):
    """rollout(case(name, shape)) in float64, computed once and read-only, with the
    conditions the GPU test leans on: every cell strictly positive, and a top-two gap of
    more than 100 * B32 at every step of P and Z and at the first step of E.

    E's second step cannot have that gap: its state is the start smoothed twice by the wide
    K, with a relative spread of about 0.7 %, and E's e32 is the largest of the four (343
    float32 additions in a row, which no later stage averages), so 100 * B32 is about
    5e-3.  Over 4,000 seeds per shape the best second-step gap was 1.2e-3 to 1.7e-3; a K
    narrow enough to widen it has a smallest tap too light for test_pc_dense.py's factor of
    20.  The GPU test compares a step's peak with the reference's only where the gap
    allows it, and with the handle's own state always."""
    out = rollout(case(name, shape))
    for s, p in enumerate(out[0]):
        assert np.isfinite(p).all() and (p > 0).all(), (name, shape, s)
        if name in ('P', 'Z') or (name == 'E' and s == 0):
            assert top_gap(p) > 100 * b32(name), (name, shape, s, top_gap(p))
        p.setflags(write=False)
    return out


def rel_err(got, want):
    """The largest per-cell |got - want| / want; want > 0 everywhere."""
    return float((np.abs(got - want) / want).max())


@functools.lru_cache(maxsize=None)
def measured_e32(name, shape):
    """e32 of one case: the float32 rollout against the float64 one, the largest over steps."""
    want = reference(name, shape)[0]
    got = rollout(case(name, shape), np.float32)[0]
    return max(rel_err(g.astype(np.float64), w) for g, w in zip(got, want))


# ----------------------------------------------------------------------------
# The product's parameters: a dense state stepped once by the oracle
# ----------------------------------------------------------------------------
def product_start(shape, seed):
    return np.random.default_rng(2000 + seed).uniform(0.0, 0.4, shape)


def product_step(shape, seed, dtype=np.float64):
    """One update(PRODUCT_V) of the float64 oracle's definition from product_start, in
    ``dtype``: (state, peak)."""
    ctl = P.step_control(PRODUCT_V[0], PRODUCT_V[1], shape, P.lut_2d())
    p = product_start(shape, seed).astype(np.float32).astype(dtype)
    out, _ = step(p, P.dog_kernel_3d(), P.PC_GLOBAL_INHIB, ctl['filters'], ctl['ox'], ctl['oy'], ctl['zf'])
    return out, A.first_argmax(out)


@functools.lru_cache(maxsize=None)
def product_reference(shape):
    """[(state, peak)] over PRODUCT_SEEDS in float64, read-only, with the conditions the
    GPU test leans on: a top-two gap of at least 1e-3 of the peak, and cells that are
    non-zero in at least one output covering 90 % of the grid."""
    outs = [product_step(shape, seed) for seed in PRODUCT_SEEDS]
    covered = np.zeros(shape, dtype=bool)
    for state, _ in outs:
        assert np.isfinite(state).all() and (state >= 0).all()
        assert top_gap(state) >= 1e-3, (shape, top_gap(state))
        covered |= state > 0
        state.setflags(write=False)
    assert covered.mean() >= 0.9, (shape, covered.mean())
    return outs


@functools.lru_cache(maxsize=None)
def measured_e32_product(shape):
    err = 0.0
    for seed, (want, _) in zip(PRODUCT_SEEDS, product_reference(shape)):
        got = product_step(shape, seed, np.float32)[0].astype(np.float64)
        err = max(err, float(np.abs(got - want).max() / want.max()))
    return err


# ----------------------------------------------------------------------------
# The ctypes driver
# ----------------------------------------------------------------------------
def drive(lib, cs, precision, batched):
    """A fresh handle through the case: rs_pc_write of the start state, then rs_pc_update
    per step with the state read back after each, or one rs_pc_run and a read.  Returns
    (step form, peaks, states read, RS_PC_DBG_HALO_AMBIG's count or None)."""
    from pyratslam_amd import _lib
    i32, f64 = ctypes.c_int32, ctypes.c_double
    c, n = cs.ctl, cs.steps
    h = A.create_case(lib, cs, precision)
    try:
        form = lib.rs_pc_step_form(h).decode()
        _lib.check(lib.rs_pc_write(h, _lib.ptr(np.ascontiguousarray(cs.start), f64)))
        out = np.full((n, 3), -1, dtype=np.int32)
        states = []
        if batched:
            _lib.check(lib.rs_pc_run(h, n, _lib.ptr(c['ox'], i32), _lib.ptr(c['oy'], i32), _lib.ptr(c['fidx'], i32),
                                     _lib.ptr(c['zf'], f64), _lib.ptr(out, i32)))
            states.append(A.read_state(lib, h, cs.shape))
        else:
            for s in range(n):
                ox, oy, fi, zf, o = (np.ascontiguousarray(a[s]) for a in (c['ox'], c['oy'], c['fidx'], c['zf'], out))
                _lib.check(lib.rs_pc_update(h, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(fi, i32),
                                            _lib.ptr(zf, f64), _lib.ptr(o, i32)))
                out[s] = o
                states.append(A.read_state(lib, h, cs.shape))
        ambig = None
        if form == 'halo':
            v = ctypes.c_int64(-1)
            _lib.check(lib.rs_pc_debug_value(h, _lib.RS_PC_DBG_HALO_AMBIG, ctypes.byref(v)))
            ambig = v.value
    finally:
        _lib.check(lib.rs_pc_destroy(h))
    return form, [tuple(int(v) for v in r) for r in out], states, ambig
