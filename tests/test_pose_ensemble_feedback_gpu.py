"""Injections and the sub-cell pose inside a PoseCellEnsemble run (csrc/pose_ensemble.hip,
DESIGN section 36): ``run(od, injections=...)`` against a twin ensemble that makes the same
``inject`` and one-step ``run`` calls one by one, bit for bit (peaks, resolved cells, volumes),
whatever the launch chunking, the ensemble's size and the member's place; the float64 oracle
through the same at-peak feedback; each step's six sums against ``pc_peak.numpy_peak_sums`` of
the twin's volume, bit for bit; every refusal with the state untouched; agreement with the
single network's ``run(od, injections=...)``.

The inputs are test_pose_ensemble_gpu.py's recipe, restated: member ``seed`` injects 1 at
``tuple((s // 2 + seed) % s for s in shape)`` and takes the 30 steps ``odometry(30, seed)``.
For the oracle test the seeds are chosen so that the oracle's two largest cells differ by at
least 1e-4 after every step (the state an at-peak injection resolves on is the state after the
step before it, and the start, one cell of 1.0): the test checks that on the CPU before it
compares anything, and the smallest margin found is 1.1e-3 on 12x9x10 (seed 401) and 8.3e-4 on
8x8x8 (seed 402).  An error of 1e-5 cannot move such an argmax."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import posecell as P

pytestmark = pytest.mark.gpu

STEPS = 30
SHAPE = (12, 9, 10)
PEAK = 'peak'


def odometry(n, seed, vmax=0.6, rmax=0.15):
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(0, vmax, n), r.uniform(-rmax, rmax, n)], axis=1)


def inject_cell(shape, seed):
    return tuple((s // 2 + seed) % s for s in shape)


@pytest.fixture(scope='module')
def E():
    from pyratslam_amd import PoseCellEnsemble, _lib
    _lib.require_device()
    assert PoseCellEnsemble.AT_PEAK == PEAK
    return PoseCellEnsemble


def make(E, shape, seeds, **kw):
    ens = E(len(seeds), shape, **kw)
    for m, seed in enumerate(seeds):
        if seed is not None:          # (None: a member that stays all zero)
            ens.inject(1.0, inject_cell(shape, seed), members=[m])
    return ens


def twin_run(twin, od, injections, r=None):
    """The sequence rs_pce_run_inject is defined as, call by call on ``twin``: peaks (B, n, 3),
    the resolved cells in expanded order, and with ``r`` each step's numpy_peak_sums of the
    volume read back after the step (B, n, 6)."""
    from pyratslam_amd import pc_peak
    B, n = len(twin), od.shape[1]
    first = np.cumsum([0] + [B if e[0] is None else 1 for e in injections])
    cells = np.full((first[-1], 3), -1, dtype=np.int32)
    peaks = np.empty((B, n, 3), dtype=np.int32)
    sums = np.empty((B, n, 6))
    for s in range(n + 1):
        for j, (who, st, energy, where) in enumerate(injections):
            if st != s:
                continue
            for i, m in enumerate(range(B) if who is None else [who], start=first[j]):
                if where == PEAK:
                    cell = tuple(int(v) for v in twin.get_pc_max()[m])
                elif where[0] == 'same':
                    k = where[1]
                    cell = tuple(int(v) for v in cells[first[k] + (m if injections[k][0] is None else 0)])
                else:
                    cell = tuple(int(v) % d for v, d in zip(where, twin.shape))
                twin.inject(energy, cell, members=[m])
                cells[i] = cell
        if s < n:
            peaks[:, s] = twin.run(od[:, s:s + 1])[:, 0]
            if r is not None:
                vols = twin.posecells
                for m in range(B):
                    sums[m, s] = pc_peak.numpy_peak_sums(vols[m], peaks[m, s], r)
    return peaks, cells, sums


# member m of the workhorse: its seed and what its list is about
SEEDS = list(range(100, 108))
FAR = (SHAPE[0] - 1, SHAPE[1] - 1, SHAPE[2] - 1)


def workhorse_list():
    inj = []
    # member 0: none at all.  member 1: one explicit injection before every step
    inj += [(1, s, 0.05, (3, 4, 5)) for s in range(STEPS)]
    # member 2: at-peak before every step (the first step of every launch under RS_PCE_CHUNK=4)
    inj += [(2, s, 0.02, PEAK) for s in range(STEPS)]
    # member 3: two at-peak injections at one boundary, which is a launch cut under RS_PCE_CHUNK=4,
    # with an explicit one between them
    inj += [(3, 8, 0.04, PEAK), (3, 8, 0.5, (0, 0, 0)), (3, 8, 0.03, PEAK), (3, 16, 0.02, (-1, -1, -1))]
    # member 4: same-as chains, across launch cuts (3 -> 5 -> 9) and within a boundary
    k = len(inj)
    inj += [(4, 3, 0.03, PEAK), (4, 5, 0.02, ('same', k)), (4, 9, 0.01, ('same', k + 1)), (4, 9, 0.05, FAR),
            (4, 9, 0.02, ('same', k + 3)), (4, 21, 0.02, ('same', k + 2))]
    # member 5: a negative energy that leaves a negative cell, then at-peak at the same boundary
    # (at the head of the run, in the middle of a launch, on a launch cut); the negative cell is
    # put right again behind it, but for a remainder at step 6 that goes into the step
    for s, back in ((0, 2.0), (6, 1.9375), (12, 2.0)):
        k = len(inj)
        inj += [(5, s, -2.0, PEAK), (5, s, 0.05, PEAK), (5, s, back, ('same', k))]
    # member 6: step == n, behind the last step
    k = len(inj)
    inj += [(6, 11, 0.02, PEAK), (6, STEPS, 0.3, (1, 2, 3)), (6, STEPS, 0.1, PEAK), (6, STEPS, 0.2, ('same', k + 1))]
    # member 7: every member's entries (None) would touch member 0; its own mix instead, out of
    # step order against the other members
    inj += [(7, 29, -0.01, (2, 2, 2)), (7, 29, 0.02, PEAK)]
    return inj


@pytest.fixture(scope='module')
def workhorse(E):
    """The direct run and the twin's sequence on the workhorse list, once for the module."""
    od = np.stack([odometry(STEPS, s) for s in SEEDS])
    inj = workhorse_list()
    with make(E, SHAPE, SEEDS) as ens:
        peaks, cells = ens.run(od, injections=inj)
        vols = ens.posecells
        max_pc = ens.max_pc.copy()
    with make(E, SHAPE, SEEDS) as twin:
        t_peaks, t_cells, _ = twin_run(twin, od, inj)
        t_vols = twin.posecells
    for a in (peaks, cells, vols, t_peaks, t_cells, t_vols):
        a.setflags(write=False)
    return dict(od=od, inj=inj, peaks=peaks, cells=cells, vols=vols, max_pc=max_pc, t_peaks=t_peaks, t_cells=t_cells,
                t_vols=t_vols)


def member_list(inj, m):
    """Member m's entries of a list as a list for an ensemble where it is member `0`, with the
    same-as indices renumbered; and the places of those entries in ``inj``."""
    idx = [j for j, e in enumerate(inj) if e[0] == m]
    out = []
    for j in idx:
        who, st, e, where = inj[j]
        if isinstance(where, tuple) and where[0] == 'same':
            where = ('same', idx.index(where[1]))
        out.append((0, st, e, where))
    return out, idx


# 1 -------------------------------------------------------------------------------------
def test_twin_equality(workhorse):
    w = workhorse
    assert w['peaks'].shape == (8, STEPS, 3) and w['peaks'].dtype == np.int32
    assert w['cells'].shape == (len(w['inj']), 3) and w['cells'].dtype == np.int32
    assert np.array_equal(w['peaks'], w['t_peaks'])
    assert np.array_equal(w['cells'], w['t_cells'])
    assert np.array_equal(w['vols'], w['t_vols'])
    assert np.array_equal(w['max_pc'], w['peaks'][:, -1])
    # the cases are what they claim: the negative injections left a negative cell for the
    # at-peak that follows them, and the feedback moved the result
    k = next(j for j, e in enumerate(w['inj']) if e[0] == 5)
    assert not np.array_equal(w['cells'][k], w['cells'][k + 1])
    assert np.array_equal(w['cells'][k], w['cells'][k + 2])
    assert w['vols'][6][1, 2, 3] > 0.49                     # the injections behind the last step
    assert not [e for e in w['inj'] if e[0] == 0]


def test_a_member_without_injections_is_the_plain_run(E, workhorse):
    with make(E, SHAPE, SEEDS[:1]) as ens:
        p = ens.run(workhorse['od'][:1])
        assert np.array_equal(p[0], workhorse['peaks'][0])
        assert np.array_equal(ens.posecells[0], workhorse['vols'][0])


def test_none_is_every_member(E):
    seeds = SEEDS[:3]
    od = np.stack([odometry(8, s) for s in seeds])
    inj = [(None, 0, 0.02, PEAK), (1, 2, 0.1, (1, 1, 1)), (None, 4, 0.03, ('same', 0)), (None, 8, 0.01, PEAK)]
    with make(E, SHAPE, seeds) as ens, make(E, SHAPE, seeds) as twin:
        peaks, cells = ens.run(od, injections=inj)
        t_peaks, t_cells, _ = twin_run(twin, od, inj)
        assert cells.shape == (10, 3)
        assert np.array_equal(peaks, t_peaks) and np.array_equal(cells, t_cells)
        assert np.array_equal(ens.posecells, twin.posecells)
        assert np.array_equal(cells[4:7], cells[0:3])


# 2 -------------------------------------------------------------------------------------
def test_twin_equality_however_the_run_is_cut(E, workhorse, monkeypatch):
    w = workhorse
    monkeypatch.setenv('RS_PCE_CHUNK', '4')     # 30 steps: 7 launches of 4 and one of 2
    with make(E, SHAPE, SEEDS) as ens:
        peaks, cells = ens.run(w['od'], injections=w['inj'])
        assert np.array_equal(peaks, w['t_peaks'])
        assert np.array_equal(cells, w['t_cells'])
        assert np.array_equal(ens.posecells, w['t_vols'])
    monkeypatch.setenv('RS_PCE_CHUNK', '1')
    with make(E, SHAPE, SEEDS) as ens:
        peaks, cells = ens.run(w['od'], injections=w['inj'])
        assert np.array_equal(peaks, w['t_peaks']) and np.array_equal(cells, w['t_cells'])
        assert np.array_equal(ens.posecells, w['t_vols'])


# 3 -------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [3, 5])
def test_one_member_alone(E, workhorse, m):
    w = workhorse
    inj, idx = member_list(w['inj'], m)
    with make(E, SHAPE, [SEEDS[m]]) as one:
        peaks, cells = one.run(w['od'][m:m + 1], injections=inj)
        assert np.array_equal(peaks[0], w['peaks'][m])
        assert np.array_equal(cells, w['cells'][idx])
        assert np.array_equal(one.posecells[0], w['vols'][m])


def test_the_member_last_of_300(E, workhorse):
    w, m, big = workhorse, 4, 300     # more workgroups than compute units
    inj, idx = member_list(w['inj'], m)
    inj = [(big - 1,) + e[1:] for e in inj]
    with E(big, SHAPE) as ens:
        ens.inject(1.0, inject_cell(SHAPE, SEEDS[0]), members=range(big - 1))
        ens.inject(1.0, inject_cell(SHAPE, SEEDS[m]), members=[big - 1])
        odb = np.broadcast_to(w['od'][0], (big,) + w['od'][0].shape).copy()
        odb[-1] = w['od'][m]
        peaks, cells = ens.run(odb, injections=inj)
        vols = ens.posecells
    assert np.array_equal(peaks[-1], w['peaks'][m]) and np.array_equal(vols[-1], w['vols'][m])
    assert np.array_equal(cells, w['cells'][idx])
    assert np.array_equal(peaks[0], w['peaks'][0]) and np.array_equal(vols[big - 2], w['vols'][0])


def test_no_steps_with_injections(E, workhorse):
    w, m = workhorse, 6
    inj, idx = member_list(w['inj'], m)
    head, tail = [e for e in inj if e[1] < STEPS], [e for e in inj if e[1] == STEPS]
    assert len(head) == 1 and len(tail) == 3
    tail = [(0, 0, tail[0][2], tail[0][3]), (0, 0, tail[1][2], tail[1][3]), (0, 0, tail[2][2], ('same', 0))]
    with make(E, SHAPE, [SEEDS[m]]) as one:
        peaks, cells = one.run(w['od'][m:m + 1], injections=head)
        assert np.array_equal(peaks[0], w['peaks'][m]) and np.array_equal(cells, w['cells'][idx[:1]])
        max_before = one.max_pc.copy()
        none, cells = one.run(w['od'][m:m + 1, :0], injections=tail)
        assert none.shape == (1, 0, 3)
        assert np.array_equal(cells, w['cells'][idx[1:]])
        assert np.array_equal(one.posecells[0], w['vols'][m])
        assert np.array_equal(one.max_pc, max_before)


# 4 -------------------------------------------------------------------------------------
ORACLE_SEEDS = {(12, 9, 10): (400, 401, 402, 404), (8, 8, 8): (400, 401, 402, 403)}
MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def oracle_feedback(shape, seed):
    """The oracle through 0.02 at-peak before every step from a 1.0 start: peaks, the resolved
    cells, the final volume and the smallest gap between its two largest cells."""
    ref = P.PoseCellOracle(shape)
    ref.inject(1.0, inject_cell(shape, seed))
    peaks, cells, margin = [], [], np.inf
    for v in odometry(STEPS, seed):
        top = np.sort(ref.posecells.ravel())[-2:]
        margin = min(margin, float(top[1] - top[0]))
        cell = tuple(int(c) for c in np.unravel_index(np.argmax(ref.posecells), shape))
        ref.inject(0.02, cell)
        cells.append(cell)
        peaks.append(ref.update(v))
    top = np.sort(ref.posecells.ravel())[-2:]
    margin = min(margin, float(top[1] - top[0]))
    return np.array(peaks, dtype=np.int32), np.array(cells, dtype=np.int32), ref.posecells.copy(), margin


@pytest.mark.parametrize('shape', sorted(ORACLE_SEEDS))
def test_oracle_parity_with_at_peak_feedback(E, shape):
    seeds = list(ORACLE_SEEDS[shape])
    refs = [oracle_feedback(shape, s) for s in seeds]
    for seed, ref in zip(seeds, refs):
        print('shape %r seed %d: oracle margin %.3e' % (shape, seed, ref[3]))
        assert ref[3] >= MARGIN, (shape, seed, ref[3])      # a condition on the inputs
    od = np.stack([odometry(STEPS, s) for s in seeds])
    inj = [(m, s, 0.02, PEAK) for m in range(len(seeds)) for s in range(STEPS)]
    with make(E, shape, seeds) as ens:
        peaks, cells = ens.run(od, injections=inj)
        vols = ens.posecells
    for m, (seed, (ref_peaks, ref_cells, ref_vol, _)) in enumerate(zip(seeds, refs)):
        err = float(np.abs(vols[m] - ref_vol).max())
        print('shape %r seed %d: max|d| = %.3e' % (shape, seed, err))
        assert np.array_equal(peaks[m], ref_peaks), (shape, seed)
        assert np.array_equal(cells[m * STEPS:(m + 1) * STEPS], ref_cells), (shape, seed)
        assert err < 1e-5, (shape, seed, err)


# 5 -------------------------------------------------------------------------------------
def check_poses(E, shape, seeds, od, r, inj=None, starts=None):
    """run(poses=True) against numpy_peak_sums of the twin's volume after every step."""
    from pyratslam_amd import pc_peak

    def start(ens):
        for m, c in enumerate(starts or []):
            ens.inject(1.0, c, members=[m])

    with make(E, shape, seeds, cells_to_avg=r) as ens, make(E, shape, seeds) as twin:
        start(ens), start(twin)
        got = ens.run(od, poses=True, injections=inj)
        peaks, poses = got[0], got[1]
        t_peaks, t_cells, t_sums = twin_run(twin, od, inj or [], r)
        assert np.array_equal(peaks, t_peaks)
        if inj is not None:
            assert np.array_equal(got[2], t_cells)
        assert ens.last_sums.shape == t_sums.shape and ens.last_sums.dtype == np.float64
        assert np.array_equal(ens.last_sums, t_sums)
        assert np.array_equal(ens.posecells, twin.posecells)
        assert poses.shape == peaks.shape and poses.dtype == np.float64
        for m in range(len(seeds)):
            for s in range(od.shape[1]):
                assert tuple(poses[m, s]) == pc_peak.pose_from_sums(t_sums[m, s], peaks[m, s], shape)
        if inj is None:   # the stored state's pose: the last step's
            cell, sums = ens.get_pc_peak()
            assert np.array_equal(cell, peaks[:, -1]) and np.array_equal(sums, t_sums[:, -1])
            assert np.array_equal(ens.get_pc_pose(), poses[:, -1])
    return peaks, poses, t_sums


@pytest.mark.parametrize('r', [1, 2, 3])
def test_poses_bit_for_bit(E, r):
    seeds = SEEDS[:3] + [None]                            # the last member stays all zero
    od = np.stack([odometry(12, s) for s in SEEDS[:4]])
    peaks, poses, sums = check_poses(E, SHAPE, seeds, od, r)
    assert not peaks[3].any() and not sums[3].any()       # the dead member: peak (0, 0, 0), sums 0,
    assert not poses[3].any()                             # the pose is the cell
    assert sums[:3].any(axis=2).all()


@pytest.mark.parametrize('shape,r', [((12, 9, 10), 3), ((8, 8, 8), 2), ((7, 7, 7), 3)])
def test_poses_where_the_box_wraps(E, shape, r):
    far = tuple(s - 1 for s in shape)
    od = np.stack([odometry(6, 504)] * 2)
    peaks, _, _ = check_poses(E, shape, [None, None], od, r, starts=[(0, 0, 0), far])
    # the box wraps on all three axes (7 x 7 x 7 at r = 3: it is the whole grid)
    assert tuple(peaks[0, 0]) == (0, 0, 0) and tuple(peaks[1, 0]) == far


def test_poses_and_injections_in_one_call(E):
    seeds = SEEDS[:3]
    od = np.stack([odometry(10, s) for s in seeds])
    inj = [(m, s, 0.02, PEAK) for m in range(3) for s in range(11)] + [(1, 10, -2.0, PEAK)]
    # (the twin reads step s's volume before it makes the injections of step s + 1)
    check_poses(E, SHAPE, seeds, od, 3, inj=sorted(inj, key=lambda e: e[0]))


def test_get_pc_pose_centres_on_the_first_of_equal_maxima(E):
    from pyratslam_amd import pc_peak
    rng = np.random.default_rng(7)
    vols = rng.uniform(0.0, 0.5, (2,) + SHAPE)
    firsts = []
    for m in range(2):
        cells = sorted({tuple(int(rng.integers(0, s)) for s in SHAPE) for _ in range(4)})
        for c in cells:
            vols[m][c] = 0.75
        firsts.append(cells[0])
    with E(2, SHAPE, cells_to_avg=2) as ens:
        ens.write(vols)
        stored = ens.posecells
        cell, sums = ens.get_pc_peak()
        assert np.array_equal(cell, np.array(firsts, dtype=np.int32))
        for m in range(2):
            assert np.array_equal(sums[m], pc_peak.numpy_peak_sums(stored[m], firsts[m], 2))
            assert tuple(ens.get_pc_pose()[m]) == pc_peak.pose_from_sums(sums[m], firsts[m], SHAPE)


# 6 -------------------------------------------------------------------------------------
BAD_LISTS = [
    ([(3, 0, 1.0, (0, 0, 0))], IndexError),                       # a member outside [0, B)
    ([(0, 7, 1.0, (0, 0, 0))], ValueError),                       # a step outside [0, n]
    ([(0, 3, 1.0, PEAK), (1, 0, 1.0, PEAK), (0, 2, 1.0, PEAK)], ValueError),   # out of order within a member
    ([(0, 0, 1.0, (0, 9, 0))], IndexError),                       # a cell outside the grid
    ([(0, 0, 1.0, PEAK), (0, 0, 1.0, ('same', 1))], ValueError),  # same-as k >= i
    ([(0, 0, 1.0, PEAK), (1, 0, 1.0, ('same', 0))], ValueError),  # same-as of another member
    ([(0, 0, float('nan'), PEAK)], ValueError),                   # not a finite float32
    ([(0, 0, 1e39, PEAK)], ValueError),
]


def test_refusals_leave_the_state_untouched(E):
    from pyratslam_amd import _lib
    seeds = SEEDS[:3]
    od = np.stack([odometry(6, s) for s in seeds])
    with make(E, SHAPE, seeds) as ens:
        ens.run(od[:, :2])
        before, max_before = ens.posecells, ens.max_pc.copy()
        for bad, exc in BAD_LISTS:
            with pytest.raises(exc):
                ens.run(od, injections=bad)
        with pytest.raises(ValueError, match='cells_to_avg'):
            ens.run(od, poses=True)
        with pytest.raises(ValueError, match='cells_to_avg'):
            ens.get_pc_pose()
        miss = od.copy()
        miss[1, 4, 0] = 0.1                                       # a LUT miss: before anything runs
        with pytest.raises(KeyError, match=r'member 1, step 4'):
            ens.run(miss, injections=[(0, 0, 1.0, PEAK)])
        # the same refusals at the ABI: RS_ERR_ARG, and RS_ERR_STATE for sums before the tables
        lib, i32, f64 = ens._lib, ctypes.c_int32, ctypes.c_double
        ctl = ens._control(od, False)
        ox, oy, fidx, zf = ctl
        out, sums = np.empty((3, 6, 3), dtype=np.int32), np.empty((3, 6, 6))

        def call(member, step, energy, loc, want_sums=False):
            a = [np.array(member, dtype=np.int32), np.array(step, dtype=np.int32), np.array(energy, dtype=np.float64),
                 np.array(loc, dtype=np.int32).reshape(-1, 3)]
            cells = np.empty((len(member), 3), dtype=np.int32)
            return lib.rs_pce_run_inject(ens._h, 6, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(fidx, i32),
                                         _lib.ptr(zf, f64), len(member), _lib.ptr(a[0], i32), _lib.ptr(a[1], i32),
                                         _lib.ptr(a[2], f64), _lib.ptr(a[3], i32), _lib.ptr(out, i32),
                                         _lib.ptr(cells, i32), _lib.ptr(sums, f64) if want_sums else None)

        at, same = _lib.RS_PC_INJ_AT_PEAK, _lib.RS_PC_INJ_SAME_AS
        for args in [([3], [0], [1.0], [0, 0, 0]), ([-1], [0], [1.0], [0, 0, 0]),
                     ([0], [7], [1.0], [at, 0, 0]), ([0], [-1], [1.0], [at, 0, 0]),
                     ([0, 1, 0], [3, 0, 2], [1.0] * 3, [at, 0, 0] * 3),
                     ([0], [0], [1.0], [12, 0, 0]), ([0], [0], [1.0], [0, 0, 10]), ([0], [0], [1.0], [-3, 0, 0]),
                     ([0, 0], [0, 0], [1.0] * 2, [at, 0, 0, same, 1, 0]),
                     ([0, 1], [0, 0], [1.0] * 2, [at, 0, 0, same, 0, 0]),
                     ([0], [0], [np.nan], [at, 0, 0]), ([0], [0], [np.inf], [at, 0, 0]), ([0], [0], [-1e39], [at, 0, 0])]:
            assert call(*args) == _lib.RS_ERR_ARG, args
            assert lib.rs_last_error()
        assert call([0], [0], [1.0], [at, 0, 0], want_sums=True) == _lib.RS_ERR_STATE
        cell3, sums6 = np.empty((3, 3), dtype=np.int32), np.empty((3, 6))
        assert lib.rs_pce_get_peak(ens._h, _lib.ptr(cell3, i32), _lib.ptr(sums6, f64)) == _lib.RS_ERR_STATE
        t = np.zeros(2 * max(SHAPE))
        for r in (0, 4):
            assert lib.rs_pce_set_peak_tables(ens._h, r, _lib.ptr(t, f64), _lib.ptr(t, f64), _lib.ptr(t, f64)) == _lib.RS_ERR_ARG
        assert np.array_equal(ens.posecells, before) and np.array_equal(ens.max_pc, max_before)
        # rs_pce_run_inject with no injection and no sums is rs_pce_run
        assert call([], [], [], []) == _lib.RS_OK
        vols = ens.posecells
    with make(E, SHAPE, seeds) as ens:
        ens.run(od[:, :2])
        assert np.array_equal(ens.run(od), out)
        assert np.array_equal(ens.posecells, vols)


# 7 -------------------------------------------------------------------------------------
def test_against_the_single_network(E):
    from pyratslam_amd import PoseCellNetwork
    shape, seed = (21, 21, 36), 100
    od = odometry(STEPS, seed)
    with make(E, shape, [seed]) as ens:
        peaks, cells = ens.run(od[None], injections=[(0, s, 0.02, PEAK) for s in range(STEPS)])
        vol = ens.posecells[0]
    with PoseCellNetwork(shape) as net:
        net.inject(1, inject_cell(shape, seed))
        single, single_cells = net.run(od, injections=[(s, 0.02, PoseCellNetwork.AT_PEAK) for s in range(STEPS)])
        assert np.array_equal(peaks[0], single)
        assert np.array_equal(cells, single_cells)
        assert float(np.abs(vol - net.posecells).max()) < 2e-5
