"""The scanline visual odometer on the GPU against the NumPy restatement, bit for bit:
profiles and tables as integers, deltas as float64 bytes -- no tolerance anywhere.
Then RatslamReplay's camera-only mode, per frame and batched."""
import numpy as np
import pytest

from pyratslam_amd.visual_odometer import CHUNK_FRAMES, NumpyVisualOdometer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def built():
    from pyratslam_amd import _build
    _build.build()


def reference(frames, **kw):
    """(deltas, tables (n, 2, 2S-1), profiles (n, Wd_t + Wd_r)) of the NumPy odometer."""
    tabs, profs = [], []
    d = NumpyVisualOdometer(**kw).run(frames, tables=tabs, profiles=profs)
    return d, np.stack(tabs), np.stack(profs)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(frames, splits=None, **kw):
    """One odometer over ``frames`` (in calls of ``splits`` frames) equals the reference."""
    from pyratslam_amd import SimpleVisualOdometer
    want = reference(frames, **kw)
    vo = SimpleVisualOdometer(**kw)
    parts, i = [], 0
    for n in splits or [len(frames)]:
        parts.append(vo.run(frames[i:i + n], tables=True, profiles=True))
        i += n
    assert i == len(frames)
    got = [np.concatenate([p[k] for p in parts]) for k in range(3)]
    vo.close()
    assert np.array_equal(got[2], want[2]), 'profiles'
    assert np.array_equal(got[1], want[1]), 'tables'
    assert same_bits(got[0], want[0]), 'deltas'
    return got


@pytest.fixture(scope='module')
def ros33():
    from pyratslam_amd import synthetic
    return np.stack([e[2] for e in synthetic.ros_stream(33, seed=0) if e[0] == 'image'])


def test_ros_geometry_one_call_per_frame_and_split(ros33):
    from pyratslam_amd import SimpleVisualOdometer
    assert ros33.shape == (33, 256, 256)
    d, _, _ = check(ros33)
    assert np.abs(d[1:, 1]).max() > 0
    check(ros33, splits=[1, 17, 15])      # the carried profile crosses calls
    vo = SimpleVisualOdometer()
    per = np.array([vo.update(f) for f in ros33])
    assert all(isinstance(v, float) for v in vo.update(ros33[0]))
    vo.close()
    assert same_bits(per, d)


def test_unaligned_overlapping_regions():
    rng = np.random.default_rng(1)
    kw = dict(trans_rows=(1, 30), trans_cols=(3, 40), rot_rows=(12, 39), rot_cols=(9, 47), max_shift=8)
    check(rng.integers(0, 256, size=(6, 40, 52), dtype=np.uint8), **kw)          # pitch 52: byte path
    check(rng.integers(0, 256, size=(6, 40, 64), dtype=np.uint8), **kw)          # pitch 64: 16-byte loads
    both = dict(trans_rows=(1, 39), trans_cols=(3, 47), rot_rows=(1, 39), rot_cols=(3, 47), max_shift=8)
    check(rng.integers(0, 256, size=(6, 40, 52), dtype=np.uint8), **both)
    check(rng.integers(0, 256, size=(6, 40, 64), dtype=np.uint8), **both)


def test_byte_path_odd_width():
    rng = np.random.default_rng(2)
    check(rng.integers(0, 256, size=(5, 37, 29), dtype=np.uint8), max_shift=5)


def test_wide_frames_take_several_column_tiles():
    # 2,080 columns = 130 sixteen-byte groups: three 64-group tiles, the last one partial;
    # the regions start in different tiles
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, size=(3, 5, 2080), dtype=np.uint8)
    check(f, max_shift=3)
    check(f, trans_cols=(1030, 2077), rot_cols=(5, 1500), max_shift=6)


@pytest.mark.parametrize('rows', [257, 258, 300])
def test_sixteen_bit_partial_sums_at_their_overflow_edge(rows):
    full = np.full((2, rows, 32), 255, dtype=np.uint8)
    _, _, prof = check(full, max_shift=4)
    assert (prof == rows * 255).all()
    holed = full.copy()
    holed[1, :, 7] = 0
    _, tab, prof = check(holed, max_shift=4)
    assert prof[1, 7] == 0 and prof[1, 8] == rows * 255 and tab[1].max() > 0


def test_one_thread_sums_more_rows_than_a_partial_sum_holds():
    # 16 columns = one column group, so each thread takes every 256th row: 66,100 rows
    # are 258 or 259 per thread, past the 257 a 16-bit partial sum can hold
    rows = 66100
    f = np.full((2, rows, 16), 255, dtype=np.uint8)
    f[1, ::3, 5] = 0
    _, _, prof = check(f, max_shift=2)
    assert prof[0, 0] == rows * 255


def test_shift_limits():
    rng = np.random.default_rng(4)
    check(rng.integers(0, 256, size=(4, 8, 48), dtype=np.uint8), max_shift=1)
    check(rng.integers(0, 256, size=(4, 8, 64), dtype=np.uint8), max_shift=64)
    check(rng.integers(0, 256, size=(3, 2, 4112), dtype=np.uint8), max_shift=9)   # wider than the LDS form


def test_a_call_longer_than_one_staging_chunk():
    assert CHUNK_FRAMES == 256      # host frames staged per chunk by rs_vo_run
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, size=(2 * CHUNK_FRAMES + 37, 16, 24), dtype=np.uint8)
    check(f, max_shift=6)
    check(f, max_shift=6, splits=[CHUNK_FRAMES - 1, CHUNK_FRAMES + 2, 36])


def test_device_resident_frames(ros33):
    from pyratslam_amd import SimpleVisualOdometer, _lib
    want = reference(ros33)
    fb = ros33[0].size
    buf = _lib.DeviceBuffer(ros33.nbytes + 64).upload(ros33)
    shifted = _lib.DeviceBuffer(ros33.nbytes + 64)
    for off in (0, 48, 5):             # frame-aligned; 16-byte aligned only; unaligned (byte path)
        if off:
            _lib.check(shifted._lib.rs_dev_copy(shifted.offset(off).ptr, buf.ptr, ros33.nbytes))
        base = shifted if off else buf
        view = base.offset(off) if off else buf
        vo = SimpleVisualOdometer().setup(ros33.shape[1:])
        d, tab, prof = vo.run((33, view), tables=True, profiles=True)
        assert np.array_equal(prof, want[2]) and np.array_equal(tab, want[1]) and same_bits(d, want[0])
        # the carried profile joins device and host calls
        vo.reset()
        mixed = np.concatenate([vo.run((10, view)), vo.run(ros33[10:20]),
                                vo.run((13, base.offset(off + 20 * fb)))])
        assert same_bits(mixed, want[0])
        with pytest.raises(ValueError):
            vo.run((34, view))         # past the end of the buffer
        vo.close()
    buf.close()
    shifted.close()


def test_timing_is_off_by_default_and_per_call(ros33):
    from pyratslam_amd import SimpleVisualOdometer
    vo = SimpleVisualOdometer()
    vo.run(ros33[:4])
    assert vo.device_ms() == (-1.0, -1.0)
    vo.set_timing(True)
    vo.run(ros33[4:8])
    assert all(ms > 0 for ms in vo.device_ms())
    vo.close()


def test_exceptions(ros33):
    from pyratslam_amd import SimpleVisualOdometer
    vo = SimpleVisualOdometer()
    with pytest.raises(TypeError):
        vo.update(ros33[0].astype(np.float32))
    vo.update(ros33[0])
    with pytest.raises(TypeError):
        vo.run(ros33[:2].astype(np.float64))
    with pytest.raises(ValueError):
        vo.update(ros33[0][:128])
    with pytest.raises(ValueError):
        SimpleVisualOdometer(max_shift=40).update(np.zeros((8, 32), dtype=np.uint8))
    assert vo.update(ros33[1]) == tuple(NumpyVisualOdometer().run(ros33[:2])[1].tolist())
    vo.reset()
    assert vo.update(ros33[2]) == (0.0, 0.0)
    vo.close()


# -- replay ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def events():
    from pyratslam_amd import synthetic
    return synthetic.ros_stream(120, seed=0)


def outputs(r):
    res = r.results()
    return (np.array(r.deltas, dtype=np.float64).reshape(-1, 2), res['pc_max'], res['template_index'],
            res['em_points'])


def same_outputs(a, b):
    assert same_bits(a[0], b[0]), 'deltas'
    assert np.array_equal(a[1], b[1]), 'peaks'
    assert np.array_equal(a[2], b[2]), 'template indices'
    assert same_bits(a[3], b[3]), 'experience-map points'


@pytest.fixture(scope='module')
def per_frame(events):
    from pyratslam_amd import replay
    return outputs(replay.RatslamReplay(use_visual_odometry=True).replay_events(events))


def test_replay_per_frame_equals_the_numpy_odometer(events, per_frame):
    from pyratslam_amd import replay
    r = replay.RatslamReplay(use_visual_odometry=True, vo=NumpyVisualOdometer()).replay_events(events)
    ref = outputs(r)
    assert ref[0].shape == (120, 2) and len(ref[1]) == 120 and len(ref[2]) == 120
    assert ref[0][0].tolist() == [0.0, 0.0] and np.abs(ref[0][1:, 1]).max() > 0
    same_outputs(per_frame, ref)
    # odometry messages were ignored: the deltas are the odometer's alone
    frames = np.stack([e[2] for e in events if e[0] == 'image'])
    assert same_bits(ref[0], NumpyVisualOdometer().run(frames))


@pytest.mark.parametrize('batch', [64, 7])
def test_replay_frames_batched_equals_per_frame(events, per_frame, batch):
    from pyratslam_amd import replay
    frames = np.stack([e[2] for e in events if e[0] == 'image'])
    r = replay.RatslamReplay(use_visual_odometry=True).replay_frames(frames, batch=batch)
    same_outputs(outputs(r), per_frame)


def test_replay_frames_with_feedback_goes_frame_by_frame(events):
    from pyratslam_amd import replay
    frames = np.stack([e[2] for e in events if e[0] == 'image'])[:40]
    a = replay.RatslamReplay(use_visual_odometry=True, feedback_energy=0.02).replay_frames(frames)
    b = replay.RatslamReplay(use_visual_odometry=True, feedback_energy=0.02,
                             vo=NumpyVisualOdometer()).replay_events(
        [e for e in events if e[0] == 'image'][:40])
    same_outputs(outputs(a), outputs(b))


def test_replay_cli_visual_odometry(capsys):
    import json
    from pyratslam_amd import replay
    assert replay.main(['--synthetic', '24', '--visual-odometry']) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out['updates'] == 24 and out['frames'] == 24
