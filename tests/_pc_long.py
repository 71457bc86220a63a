"""Long pose-cell trajectories shared by test_pc_long.py and test_pc_long_gpu.py: the fixtures
``tests/golden/pc_long_<name>.npz`` (made by the reference, ``gen_golden.py --only long``),
the emulations whose errors the bounds are built from, and the bounds.  Nothing here comes
from the kernels.

Every other comparison of the pose-cell kernels with the reference stops within 40 steps of
the injection.  These trajectories follow ``synthetic.odometry(steps, seed=0)``, the stream
bench.py times, for 1,000 to 2,000 steps with centre injection (``_turn``: 0.10 rad added to
every vrot, so the packet goes round the theta axis); a fixture holds the
reference's peak and top-two gap at every step and its state at every ``WINDOW`` = 10th step
(checkpoint c is the state after 10 c steps, checkpoint 0 the state after the injection).

The reference's dynamics amplify rounding: the reference's own definition evaluated on
float32 arrays and run freely is 0.14 away from the float64 reference within 2,000 steps at
32x32x18, and float64 with noise of an ulp's size 3.5e-10, while restarted from the
reference's state every ten steps it stays within 2e-7 (median) to 7e-6 (worst).  So
"within 1e-5, identical argmax" is a statement about short windows, and the tests come in
two kinds, each with a bound made of an emulation's error, never of a kernel's output:

* anchored windows: window w starts from the reference's state at checkpoint w and ends at
  checkpoint w + 1.  ``e32w[w]`` is the error there of the float32 emulation (``step`` of
  _pc_dense.py on float32 arrays, started from the state rounded to float32), and

      Bw[w] = 32 * max(e32w[w], median(e32w)),      float64: Bw[w] * 2^-29;

* the free run: ``e32f[c]`` is the error at checkpoint c of the float32 emulation stepping
  on from checkpoint 0, ``e64n[c]`` that of the float64 oracle with every cell multiplied by
  ``1 + 2^-50 * N(0, 1)`` after every step (seed ``NOISE_SEED``), and

      Bf32[c] = 32 * max(e32f[:c + 1]),   used while it stays at or below 1e-3: the first
                                          checkpoint above is the float32 parity horizon;
      Bf64[c] = max(1e-12, 32 * max(e64n[:c + 1])).

An error is the largest absolute difference over the cells.  The factor 32 and the ratio
2^-29 are those of _pc_dense.py; 2^-50 is about four times the float64 per-step deviation
measured on the device."""
import functools
import os

import numpy as np

import _pc_dense as D
from oracle import posecell as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

WINDOW = 10
STREAM_SEED = 0                               # synthetic.odometry(steps, seed=STREAM_SEED)
TURN = 0.10                                   # added to vrot in the _turn trajectory
# name -> (shape, steps).  synthetic.odometry draws all of vtrans first: a run of any length
# has the same vtrans column, and its vrot column depends on the length
TRAJECTORIES = {'32x32x18': ((32, 32, 18), 2000), '50x50x10': ((50, 50, 10), 2000),
                '64x64x36': ((64, 64, 36), 1000), '32x32x18_turn': ((32, 32, 18), 1000)}
NAMES = tuple(TRAJECTORIES)

FACTOR = D.FACTOR                             # 32
F64_RATIO = D.F64_RATIO                       # 2^-29
NOISE = 2.0 ** -50
NOISE_SEED = 64
F32_TOL, F64_TOL = 1e-5, 1e-12                # the north-star bounds
TIGHT_E32W = 1e-6                             # windows at or below it are also held to F32_TOL
GAP_MIN = 2e-5                                # peaks are compared where the top-two gap exceeds it
HORIZON_BOUND = 1e-3
MIN_XY_CROSSINGS, MIN_TH_CROSSINGS_TURN = 10, 5


def odometry(name):
    """The odometry of trajectory ``name`` (the fixture stores the same rows)."""
    from pyratslam_amd import synthetic
    od = synthetic.odometry(TRAJECTORIES[name][1], seed=STREAM_SEED)
    if name.endswith('_turn'):
        od[:, 1] += TURN
    return od


# ----------------------------------------------------------------------------
# Fixture access
# ----------------------------------------------------------------------------
class Long:
    """One fixture: ``odom`` (n, 2), ``max_pc`` (n, 3) and ``gap`` (n,) per step, ``state(c)``
    per checkpoint, ``e32w`` (n / 10,), ``e32f`` and ``e64n`` (n / 10 + 1,)."""

    def __init__(self, name):
        f = np.load(os.path.join(GOLDEN, 'pc_long_%s.npz' % name))
        self.name = name
        self.shape = tuple(int(v) for v in f['shape'])
        self.inject = tuple(int(v) for v in f['inject'])
        self.odom, self.max_pc, self.gap = f['odom'], f['max_pc'], f['gap']
        self.e32w, self.e32f, self.e64n = f['e32w'], f['e32f'], f['e64n']
        self.steps = len(self.odom)
        self.windows = self.steps // WINDOW
        self._nnz, self._idx, self._val = f['nnz'], f['coo_idx'], f['coo_val']
        self._off = np.concatenate([[0], np.cumsum(self._nnz)])
        assert len(self._nnz) == self.windows + 1 and self.steps % WINDOW == 0
        for a in (self.odom, self.max_pc, self.gap, self.e32w, self.e32f, self.e64n):
            a.setflags(write=False)

    def state(self, c):
        """The reference's state at checkpoint c (after 10 c steps), float64, read-only."""
        return _state(self, c)

    def peaks(self):
        """max_pc as a list of tuples."""
        return [tuple(int(v) for v in r) for r in self.max_pc]


@functools.lru_cache(maxsize=256)
def _state(tr, c):
    out = np.zeros(int(np.prod(tr.shape)))
    lo, hi = tr._off[c], tr._off[c + 1]
    out[tr._idx[lo:hi]] = tr._val[lo:hi]
    out = out.reshape(tr.shape)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def load(name):
    return Long(name)


def face_crossings(max_pc, shape):
    """How often the peak crosses the x, y and theta face: a move of more than half the
    extent between two steps."""
    d = np.abs(np.diff(np.asarray(max_pc, dtype=np.int64), axis=0))
    return tuple(int((d[:, a] > shape[a] // 2).sum()) for a in range(3))


def top_two_gap(p):
    """The difference between the largest and the second largest cell."""
    top = np.partition(p.ravel(), p.size - 2)[-2:]
    return float(top[1] - top[0])


# ----------------------------------------------------------------------------
# The emulations
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lut():
    return P.lut_2d()


@functools.lru_cache(maxsize=None)
def _k3():
    k = P.dog_kernel_3d()
    k.setflags(write=False)
    return k


def step(p, v, mistake=None, cell=None):
    """One update((vtrans, vrot)) of the oracle's definition in p's precision (_pc_dense.step:
    byte for byte the oracle's in float64, test_pc_dense.py), with one planted mistake."""
    ctl = P.step_control(float(v[0]), float(v[1]), p.shape, _lut())
    return D.step(p, _k3(), P.PC_GLOBAL_INHIB, ctl['filters'], ctl['ox'], ctl['oy'], ctl['zf'], mistake, cell)[0]


def err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max())


def window_e32(start, odom, want):
    """e32w of one window: the float32 emulation from float32(start) over ``odom``."""
    q = start.astype(np.float32)
    for v in odom:
        q = step(q, v)
    return err(q, want)


def free_errors(start, odom, states, kind, upto=None):
    """e32f (kind 'e32f') or e64n (kind 'e64n') at checkpoints 0 .. upto; ``states(c)`` is the
    reference's state at checkpoint c."""
    n = len(odom) // WINDOW if upto is None else upto
    if kind == 'e32f':
        q, rng = start.astype(np.float32), None
    else:
        q, rng = start.astype(np.float64), np.random.default_rng(NOISE_SEED)
    out = [err(q, states(0))]
    for s in range(n * WINDOW):
        q = step(q, odom[s])
        if rng is not None:
            q = q * (1.0 + NOISE * rng.standard_normal(q.shape))
        if (s + 1) % WINDOW == 0:
            out.append(err(q, states((s + 1) // WINDOW)))
    return np.array(out)


# ----------------------------------------------------------------------------
# The bounds
# ----------------------------------------------------------------------------
def bw(tr, precision='float32'):
    """Bw per window."""
    b = FACTOR * np.maximum(tr.e32w, np.median(tr.e32w))
    return b * (1.0 if precision == 'float32' else F64_RATIO)


def bf32(tr):
    """Bf32 per checkpoint, beyond the horizon too."""
    return FACTOR * np.maximum.accumulate(tr.e32f)


def horizon(tr):
    """The float32 parity horizon: the first checkpoint at which Bf32 exceeds 1e-3, or None."""
    above = np.flatnonzero(bf32(tr) > HORIZON_BOUND)
    return int(above[0]) if len(above) else None


def bf64(tr):
    """Bf64 per checkpoint."""
    return np.maximum(F64_TOL, FACTOR * np.maximum.accumulate(tr.e64n))


def checkpoint_of_step(s):
    """The first checkpoint at or behind 0-based step s (the state after it)."""
    return (s + WINDOW) // WINDOW
