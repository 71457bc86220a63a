"""The sub-cell pose on the GPU (pc_peak_kernel): the six sums bit for bit
where the stored state is what was written, the poses after steps against the NumPy
restatement of the volume read back and against the float64 oracle, the batch edges of the
halo form's one-launch-late key, and the replay's pc_pose.

The pose bound, per axis: N/(2 pi) * sqrt(2) * eps * M / R, M the box mass and R = hypot(S, C),
both from the restatement's sums of the volume read back (never from the code under test).
A cell perturbed relatively by eps moves S and C by at most eps * M each, the angle by at most
sqrt(2) * eps * M / R.  eps = 2^-23 for float32 (the halo form's sums are of the unnormalised
state, the volume read back is that state times 1/total rounded once: 2^-24, doubled);
eps = 2^-47 for float64 (64 float64 roundings per sum)."""
import math

import numpy as np
import pytest

from conftest import load_golden
from oracle import posecell as P

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5   # the project's float32 state bound (tests/test_posecell_gpu.py)
EPS = {'float32': 2.0 ** -23, 'float64': 2.0 ** -47}
GRIDS = [(7, 7, 7), (9, 12, 8), (21, 21, 36), (50, 50, 10)]
HALO_GRIDS = [(21, 21, 36), (32, 32, 18), (50, 50, 10)]


@pytest.fixture(scope='module')
def pcn():
    from pyratslam_amd import _build
    _build.build()
    from pyratslam_amd import PoseCellNetwork
    return PoseCellNetwork


def odometry(n, seed, vmax=0.6, rmax=0.15):
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(0, vmax, n), r.uniform(-rmax, rmax, n)], axis=1)


def circ(a, b, n):
    d = abs(a - b) % n
    return min(d, n - d)


def restated(vol, cell, r, eps):
    """(pose, per-axis bound) of the restatement on a volume read back."""
    from pyratslam_amd import numpy_peak_sums, pose_from_sums
    sums = numpy_peak_sums(vol, cell, r)
    ix = [(int(p) + np.arange(2 * r + 1) - r) % n for p, n in zip(cell, vol.shape)]
    mass = float(np.abs(vol[np.ix_(*ix)]).sum())
    bound = []
    for a, n in enumerate(vol.shape):
        rad = math.hypot(sums[2 * a], sums[2 * a + 1])
        bound.append(n / (2 * math.pi) * math.sqrt(2) * eps * mass / rad if rad > 0 else math.inf)
    return pose_from_sums(sums, cell, vol.shape), bound


def assert_close(got, want, bound, shape, what):
    for a, n in enumerate(shape):
        d = circ(got[a], want[a], n)
        assert d <= bound[a], (what, a, got, want, d, bound[a])


# -- exact: the stored state is what was written -------------------------------------
def corner_cells(shape):
    return [(0, 0, 0), tuple(s - 1 for s in shape), tuple(s // 2 for s in shape)]


def f32_volume(shape, seed):
    v = np.random.default_rng(seed).random(shape).astype(np.float32).astype(np.float64) * 0.5
    return v


EXACT = [('', GRIDS), ('rows', GRIDS), ('cols', [(24, 40, 13)]), ('stream:1,8,1,2', [(24, 40, 13), (21, 21, 36)])]


@pytest.mark.parametrize('precision', ['float32', 'float64'])
@pytest.mark.parametrize('form,grids', EXACT)
def test_written_state_gives_the_rules_sums_bit_for_bit(pcn, monkeypatch, form, grids, precision):
    from pyratslam_amd import numpy_peak_sums, pose_from_sums
    monkeypatch.setenv('RS_PC_FORM', form)
    for shape in grids:
        base = f32_volume(shape, 11)
        for r in (1, 2, 3):
            net = pcn(shape, precision=precision, cells_to_avg=r)
            assert not form or net.step_form() == form.split(':')[0]
            for cell in corner_cells(shape):
                v = base.copy()
                v[cell] = 1.0
                net.posecells = v
                got_cell, sums = net.get_pc_peak()
                assert got_cell == cell
                want = numpy_peak_sums(v, cell, r)
                assert sums.tobytes() == want.tobytes(), (shape, form, precision, r, cell, sums, want)
                assert net.get_pc_pose() == pose_from_sums(want, cell, shape)
            net.close()


@pytest.mark.parametrize('precision', ['float32', 'float64'])
def test_two_equal_maxima_centre_the_box_on_the_first(pcn, monkeypatch, precision):
    from pyratslam_amd import numpy_peak_sums
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    shape = (9, 12, 8)
    v = f32_volume(shape, 5)
    v[2, 11, 7] = v[7, 0, 1] = 1.0
    net = pcn(shape, precision=precision, cells_to_avg=2)
    net.posecells = v
    cell, sums = net.get_pc_peak()
    assert cell == (2, 11, 7) == net.get_pc_max()
    assert sums.tobytes() == numpy_peak_sums(v, cell, 2).tobytes()


def test_refusals_before_any_device_work(pcn, monkeypatch):
    from pyratslam_amd import _lib
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    for r in (0, 4, 1.5):
        with pytest.raises(ValueError):
            pcn((21, 21, 36), cells_to_avg=r)
    net = pcn((5, 21, 36))    # never asks for a pose: no error
    assert net.update((0.13, 0.02)) is not None
    with pytest.raises(ValueError):
        net.get_pc_pose()
    with pytest.raises(ValueError):
        net.run([[0.1, 0.0]], poses=True)
    ok = pcn((5, 21, 36), cells_to_avg=2)
    assert len(ok.get_pc_pose()) == 3
    # the C ABI: a peaks call before the tables, a bad radius, null tables
    raw = pcn((21, 21, 36))
    out, sums = np.zeros(3, dtype=np.int32), np.zeros(6)
    import ctypes
    o, s = _lib.ptr(out, ctypes.c_int32), _lib.ptr(sums, ctypes.c_double)
    assert raw._lib.rs_pc_get_peak(raw._h, o, s) == _lib.RS_ERR_STATE
    assert raw._lib.rs_pc_update_odom_peak(raw._h, 0.1, 0.0, o, s) == _lib.RS_ERR_STATE
    od = np.array([[0.1, 0.0]])
    assert raw._lib.rs_pc_run_odom_peaks(raw._h, 1, _lib.ptr(od, ctypes.c_double), o, s, None) == _lib.RS_ERR_STATE
    from pyratslam_amd import peak_tables
    tabs = [_lib.ptr(t, ctypes.c_double) for t in peak_tables((21, 21, 36))]
    assert raw._lib.rs_pc_set_peak_tables(raw._h, 0, *tabs) == _lib.RS_ERR_ARG
    assert raw._lib.rs_pc_set_peak_tables(raw._h, 4, *tabs) == _lib.RS_ERR_ARG
    assert raw._lib.rs_pc_set_peak_tables(raw._h, 3, tabs[0], None, tabs[2]) == _lib.RS_ERR_ARG
    assert raw._lib.rs_pc_get_peak(raw._h, o, s) == _lib.RS_ERR_STATE
    assert raw._lib.rs_pc_set_peak_tables(raw._h, 3, *tabs) == _lib.RS_OK
    assert raw._lib.rs_pc_get_peak(raw._h, o, s) == _lib.RS_OK


# -- after steps ------------------------------------------------------------------------
STEPS = 30
AFTER = [((21, 21, 36), 'float32', '', 'halo'), ((32, 32, 18), 'float32', '', 'halo'),
         ((50, 50, 10), 'float32', '', 'halo'), ((64, 64, 36), 'float64', '', 'rows'),
         ((24, 40, 13), 'float32', 'cols', 'cols'), ((24, 40, 13), 'float64', 'cols', 'cols'),
         ((24, 40, 13), 'float32', 'stream:1,8,1,2', 'stream'), ((7, 7, 7), 'float32', '', None)]
_ORACLE = {}


def oracle_run(shape):
    """The oracle's trajectory over the shared odometry, computed once per grid: the peak
    per step and, on the halo grids, the restatement's pose and sums of its float64 state."""
    if shape not in _ORACLE:
        from pyratslam_amd import numpy_peak_sums, pose_from_sums
        od = odometry(STEPS, 23)
        loc = tuple(s // 2 for s in shape)
        if shape == (64, 64, 36):   # the C restatement of the same oracle (seconds in NumPy)
            from oracle import c_oracle as C
            ref = C.PoseCellC(shape)
        else:
            ref = P.PoseCellOracle(shape)
        ref.inject(1, loc)
        maxes, poses, radii = [], [], []
        for v in od:
            m = tuple(int(x) for x in ref.update(v))
            maxes.append(m)
            if shape in HALO_GRIDS:
                sums = numpy_peak_sums(ref.posecells, m, 3)
                poses.append(pose_from_sums(sums, m, shape))
                radii.append([math.hypot(sums[2 * a], sums[2 * a + 1]) for a in range(3)])
        _ORACLE[shape] = (od, loc, maxes, poses, radii)
    return _ORACLE[shape]


@pytest.mark.parametrize('shape,precision,form,want_form', AFTER)
def test_poses_after_steps(pcn, monkeypatch, shape, precision, form, want_form):
    monkeypatch.setenv('RS_PC_FORM', form)
    od, loc, maxes, oposes, oradii = oracle_run(shape)
    eps = EPS[precision]
    nets = [pcn(shape, precision=precision) for _ in range(3)]
    for net in nets:
        assert want_form is None or net.step_form() == want_form
        net.inject(1, loc)
    batched, plain, single = nets
    bm, bp = batched.run(od, poses=True)
    assert bp.dtype == np.float64 and bp.shape == (STEPS, 3)
    assert np.array_equal(bm, plain.run(od))
    assert [tuple(int(x) for x in m) for m in bm] == maxes
    assert batched.max_pc == maxes[-1]
    worst = 0.0
    for s, v in enumerate(od):
        pose = single.update_pose(v)
        assert single.max_pc == maxes[s] == single.get_pc_max()
        want, bound = restated(single.posecells, maxes[s], 3, eps)
        print('step %d axis bounds %s |batched - restated| %s |per-call - restated| %s'
              % (s, bound, [circ(bp[s][a], want[a], shape[a]) for a in range(3)],
                 [circ(pose[a], want[a], shape[a]) for a in range(3)]))
        assert_close(pose, want, bound, shape, ('per-call', s))
        assert_close(bp[s], want, bound, shape, ('batched', s))
        assert_close(bp[s], pose, bound, shape, ('batched vs per-call', s))
        if oposes:   # the float64 oracle's state, within the project's 1e-5 state bound per cell
            ob = [n / (2 * math.pi) * math.sqrt(2) * 7 ** 3 * F32_TOL / oradii[s][a] for a, n in enumerate(shape)]
            assert_close(bp[s], oposes[s], ob, shape, ('oracle', s))
            worst = max(worst, max(circ(bp[s][a], oposes[s][a], shape[a]) for a in range(3)))
        assert all(circ(bp[s][a], maxes[s][a], shape[a]) <= 3 for a in range(3))
    print('%r %s: largest |pose - oracle pose| = %.3e cells' % (shape, precision, worst))
    assert np.array_equal(batched.posecells, plain.posecells)
    for net in nets:
        net.close()


# -- batch edges of the halo form -----------------------------------------------------------
def per_call(pcn, shape, loc, od, **kw):
    """A twin stepped one update_pose at a time: (maxes, poses, restated poses, bounds)."""
    net = pcn(shape, **kw)
    net.inject(1, loc)
    maxes, poses, want, bounds = [], [], [], []
    for v in od:
        poses.append(net.update_pose(v))
        maxes.append(net.max_pc)
        w, b = restated(net.posecells, net.max_pc, 3, EPS['float32'])
        want.append(w)
        bounds.append(b)
    return net, maxes, poses, want, bounds


@pytest.mark.parametrize('n', [1, 2, 17, 65])   # 17: the sums' buffer grows; 65: past the finishing pass's own export
def test_halo_batch_lengths(pcn, monkeypatch, n):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    shape, loc = (21, 21, 36), (10, 10, 18)
    od = odometry(n, 41)
    twin, maxes, poses, want, bounds = per_call(pcn, shape, loc, od)
    net = pcn(shape)
    assert net.step_form() == 'halo'
    net.inject(1, loc)
    m, p = net.run(od, poses=True)
    assert [tuple(int(x) for x in q) for q in m] == maxes
    for s in range(n):
        assert_close(p[s], want[s], bounds[s], shape, ('restated', n, s))
        assert_close(p[s], poses[s], bounds[s], shape, ('per-call', n, s))
    assert np.array_equal(net.posecells, twin.posecells)


def test_halo_peaks_calls_between_lazy_calls_and_injections(pcn, monkeypatch):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    shape, loc = (21, 21, 36), (10, 10, 18)
    od = odometry(16, 43)
    # the twin: one step at a time, the same injection at the same place in the sequence
    twin = pcn(shape)
    twin.inject(1, loc)
    want, bounds, maxes = [], [], []
    for s, v in enumerate(od):
        if s == 9:
            twin.inject(0.05, (3, 4, 5))
        twin.update(v)
        maxes.append(twin.max_pc)
        w, b = restated(twin.posecells, twin.max_pc, 3, EPS['float32'])
        want.append(w)
        bounds.append(b)
    net = pcn(shape)
    net.inject(1, loc)
    got = {}
    net.run(od[0:3])                                  # lazy: leaves the state unnormalised
    m, p = net.run(od[3:6], poses=True)               # ... a peaks call consumes it
    got.update({3 + i: (tuple(m[i]), p[i]) for i in range(3)})
    net.run(od[6:8])                                  # the reverse order
    pose = net.update_pose(od[8])
    got[8] = (net.max_pc, pose)
    net.inject(0.05, (3, 4, 5))
    m, p = net.run(od[9:12], poses=True)
    got.update({9 + i: (tuple(m[i]), p[i]) for i in range(3)})
    net.update(od[12])                                # a lazy one-step call, then the stored state's pose
    got[12] = (net.get_pc_max(), net.get_pc_pose())
    m, p = net.run(od[13:16], poses=True)
    got.update({13 + i: (tuple(m[i]), p[i]) for i in range(3)})
    for s, (mx, pose) in got.items():
        assert tuple(int(x) for x in mx) == maxes[s], s
        assert_close(pose, want[s], bounds[s], shape, s)
    assert np.array_equal(net.posecells, twin.posecells)


def test_eager_readback_with_poses(pcn, monkeypatch):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    shape, loc = (21, 21, 36), (10, 10, 18)
    od = odometry(6, 47)
    twin, maxes, poses, want, bounds = per_call(pcn, shape, loc, od)
    net = pcn(shape, readback='eager')
    net.inject(1, loc)
    m, p = net.run(od[:4], poses=True)
    assert [tuple(int(x) for x in q) for q in m] == maxes[:4]
    net.update(od[4])                                   # exports eagerly
    assert net.posecells is not None
    pose = net.update_pose(od[5])
    assert net.max_pc == maxes[5]
    for s in range(4):
        assert_close(p[s], want[s], bounds[s], shape, s)
    assert_close(pose, want[5], bounds[5], shape, 5)
    assert np.array_equal(net.posecells, twin.posecells)


def test_lut_keyerror_mid_batch_keeps_the_earlier_poses(pcn, monkeypatch):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    case = load_golden('pc_keyerror')
    shape, loc = tuple(int(s) for s in case['shape']), (16, 16, 9)
    od = odometry(6, 53)
    od[3] = case['odom'][0]
    twin, maxes, poses, want, bounds = per_call(pcn, shape, loc, od[:3])
    plain = pcn(shape)
    net = pcn(shape)
    assert net.step_form() == 'halo'
    for x in (plain, net):
        x.inject(1, loc)
    with pytest.raises(KeyError):
        plain.run(od)
    with pytest.raises(KeyError):
        net.run(od, poses=True)
    assert net.max_pc == maxes[2] and net.last_poses.shape == (3, 3)
    for s in range(3):
        assert_close(net.last_poses[s], want[s], bounds[s], shape, s)
    assert np.array_equal(net.posecells, plain.posecells)
    with pytest.raises(KeyError):                      # per call: the same KeyError, the same state
        twin.update_pose(od[3])
    assert np.array_equal(twin.posecells, plain.posecells)


@pytest.mark.parametrize('precision,form', [('float32', ''), ('float64', 'rows'), ('float32', 'cols')])
def test_host_control_fallback_and_one_step_run(pcn, monkeypatch, precision, form):
    """Odometry outside the library's control tables (RS_ERR_CTL_RANGE: a theta origin far
    out) goes through rs_pc_run_peaks; run() of one step returns one pose."""
    monkeypatch.setenv('RS_PC_FORM', form)
    shape, loc = (24, 40, 36), (12, 20, 18)
    od = odometry(4, 59)
    od[1] = (0.3, 6.0)    # a theta origin of 34 layers: outside the uploaded filters
    a, b = pcn(shape, precision=precision), pcn(shape, precision=precision)
    for x in (a, b):
        x.inject(1, loc)
    m, p = a.run(od, poses=True)
    assert np.array_equal(m, b.run(od))
    want, bound = restated(a.posecells, tuple(m[-1]), 3, EPS[precision])
    assert_close(p[-1], want, bound, shape, 'last')
    m1, p1 = a.run(od[:1], poses=True)
    assert m1.shape == (1, 3) and p1.shape == (1, 3)
    want, bound = restated(a.posecells, tuple(m1[0]), 3, EPS[precision])
    assert_close(p1[0], want, bound, shape, 'one step')
    pose = a.update_pose(od[1])                         # the per-call fallback
    want, bound = restated(a.posecells, a.max_pc, 3, EPS[precision])
    assert_close(pose, want, bound, shape, 'update_pose fallback')


# -- replay ---------------------------------------------------------------------------------
def test_replay_records_the_subcell_pose(pcn, monkeypatch):
    monkeypatch.delenv('RS_PC_FORM', raising=False)
    from pyratslam_amd import PoseCellNetwork, replay, synthetic
    frames = np.stack([ev[2] for ev in synthetic.ros_stream(100, seed=3) if ev[0] != 'odom'])

    class Recording(PoseCellNetwork):
        """update_pose that also restates the pose from the volume read back."""
        def update_pose(self, v):
            pose = super().update_pose(v)
            self.restated.append(restated(self.posecells, self.max_pc, 3, EPS['float32']))
            return pose

    rec = Recording(replay.POSE_SIZE)
    rec.restated = []
    kw = dict(use_visual_odometry=True)
    plain = replay.RatslamReplay(**kw).replay_frames(frames, batch=64).results()
    one = replay.RatslamReplay(subcell_peak=True, batch=False, pcn=rec, **kw).replay_frames(frames).results()
    assert 'pc_pose' not in plain
    assert one['pc_pose'].dtype == np.float64 and one['pc_pose'].shape == (len(frames), 3)
    for s, (want, bound) in enumerate(rec.restated):
        assert_close(one['pc_pose'][s], want, bound, replay.POSE_SIZE, ('per frame', s))
    for batch in (64, 7):
        res = replay.RatslamReplay(subcell_peak=True, **kw).replay_frames(frames, batch=batch).results()
        for key in ('pc_max', 'template_index', 'em_points'):
            assert np.array_equal(res[key], plain[key]), (batch, key)
            assert np.array_equal(one[key], plain[key]), key
        assert res['pc_pose'].shape == (len(frames), 3)
        for s, (want, bound) in enumerate(rec.restated):
            assert_close(res['pc_pose'][s], want, bound, replay.POSE_SIZE, (batch, s))
            assert all(circ(res['pc_pose'][s][a], res['pc_max'][s][a], replay.POSE_SIZE[a]) <= 3 for a in range(3))


def test_replay_cli_subcell_peak(pcn, capsys):
    import json
    from pyratslam_amd import replay
    assert replay.main(['--synthetic', '12', '--subcell-peak']) == 0
    out = json.loads(capsys.readouterr().out)
    assert len(out['pc_pose']) == out['updates'] and len(out['pc_pose'][0]) == 3
