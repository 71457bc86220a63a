"""The scanline visual odometer without a GPU: the NumPy restatement
(pyratslam_amd/visual_odometer.py) on the synthetic ROS stream, the selection rule of
the library (rs_vo_select, host only) against it bit for bit, first-frame / reset /
clamp behaviour and the create-time refusals of rs_vo_create (checked before any
device call)."""
import ctypes
import math

import numpy as np
import pytest

from pyratslam_amd import _build, _lib, synthetic
from pyratslam_amd.visual_odometer import NumpyVisualOdometer, profile, select, shift_table

PANO_W = 1024   # synthetic.ros_stream: the panorama is 4 * im_w columns wide


@pytest.fixture(scope='module')
def lib():
    _build.build()
    return _lib.load()


def stream(n, seed):
    """Frames, per-frame panorama offsets and headings of synthetic.ros_stream."""
    events = synthetic.ros_stream(n, seed=seed)
    frames = np.stack([e[2] for e in events if e[0] == 'image'])
    heading, heads = 0.0, []
    for e in events:
        if e[0] == 'odom':
            heading += e[3][2] / 10.0
            heads.append(heading)
    heads = np.array(heads)
    offs = np.floor((heads / (2 * np.pi)) % 1.0 * PANO_W).astype(np.int64)
    return frames, offs, heads


STREAMS = {seed: stream(120, seed) for seed in (0, 3)}


@pytest.mark.parametrize('rows', [None, (75, 240)])
@pytest.mark.parametrize('seed', [0, 3])
def test_exact_shift_recovery_on_the_synthetic_stream(seed, rows):
    frames, offs, heads = STREAMS[seed]
    vo = NumpyVisualOdometer(trans_rows=rows, rot_rows=rows, max_shift=40)
    d = vo.run(frames)
    rad = math.radians(90.0) / 256
    assert rad == 2 * math.pi / PANO_W
    true = (np.diff(offs) + PANO_W // 2) % PANO_W - PANO_W // 2
    got = np.rint(d[1:, 1] / rad).astype(np.int64)
    assert np.array_equal(d[1:, 1], true.astype(np.float64) * rad)   # every frame, exactly
    assert np.array_equal(got, true)
    assert np.abs(true).max() <= 39
    assert d[0, 0] == 0.0 and d[0, 1] == 0.0
    # so the integrated vrot stays within one column of the stream's integrated heading
    err = np.cumsum(d[:, 1]) - (heads - heads[0])
    err = (err + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(err).max() < 2 * np.pi / PANO_W + 1e-9


def test_small_region_recovery():
    frames, offs, _ = stream(64, 1)
    d = NumpyVisualOdometer(trans_rows=(100, 104), rot_rows=(100, 104)).run(frames)
    true = (np.diff(offs) + PANO_W // 2) % PANO_W - PANO_W // 2
    assert np.array_equal(d[1:, 1], true.astype(np.float64) * (math.radians(90.0) / 256))


def test_profile_and_table_definitions():
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, size=(9, 14), dtype=np.uint8)
    p = profile(f, (2, 7), (3, 12))
    assert p.dtype == np.uint32 and p.tolist() == [int(f[2:7, 3 + c].sum()) for c in range(9)]
    g = rng.integers(0, 256, size=(9, 14), dtype=np.uint8)
    q = profile(g, (2, 7), (3, 12))
    tab = shift_table(p, q, 4)
    assert tab.dtype == np.uint32 and tab.size == 7
    for s in range(-3, 4):
        want = sum(abs(int(p[k]) - int(q[k + s])) for k in range(9) if 0 <= k + s < 9)
        assert tab[s + 3] == want
    # new[k] == old[k + s] is a positive shift
    old = rng.integers(0, 1000, size=32).astype(np.uint32)
    new = np.roll(old, -2)
    assert select(shift_table(new, old, 5), 32, 1)[0] == 2


def c_select(lib, table, width, rows):
    t = np.ascontiguousarray(table, dtype=np.uint32)
    S = (t.size + 1) // 2
    shift, best = ctypes.c_int(), ctypes.c_double()
    _lib.check(lib.rs_vo_select(S, width, rows, _lib.ptr(t, ctypes.c_uint32), ctypes.byref(shift),
                                ctypes.byref(best)))
    return shift.value, best.value


def test_selection_order_on_hand_made_tables(lib):
    S, wd, rows = 8, 64, 3

    def table(entries, fill=50000):
        t = np.full(2 * S - 1, fill, dtype=np.uint32)
        for s, v in entries.items():
            t[s + S - 1] = v
        return t

    # all equal raw sums: the denominators shrink with |s|, shift 0 has the smallest quotient
    # (and with S = 1 there is nothing else to choose)
    cases = [(np.full(2 * S - 1, 7, dtype=np.uint32), 0),
             (np.zeros(2 * S - 1, dtype=np.uint32), 0),
             (table({-3: 100, 3: 100}), -3),
             # equal quotients at +2 and -5: m * (wd - |s|) each; the smaller |s| stays
             (table({2: 10 * (wd - 2), -5: 10 * (wd - 5)}), 2)]
    for t, want in cases:
        assert select(t, wd, rows)[0] == want
        assert c_select(lib, t, wd, rows)[0] == want
    # equal quotients everywhere: shift 0
    t = np.array([5 * (wd - abs(s)) for s in range(-(S - 1), S)], dtype=np.uint32)
    assert select(t, wd, rows) == (0, 5 * wd / (wd * rows * 255))
    assert c_select(lib, t, wd, rows)[0] == 0


def test_rs_vo_select_equals_numpy_bit_for_bit(lib):
    rng = np.random.default_rng(11)
    ties = 0
    for i in range(2000):
        S = (1, 2, 40, 64)[i % 4]
        wd = int(rng.integers(S, 400))
        rows = int(rng.integers(1, 300))
        absS = np.abs(np.arange(-(S - 1), S))
        if i % 8 < 4:
            # exact ties after the division: the minimum quotient m / (rows * 255) at
            # several shifts (tab = m * (wd - |s|)), everything else strictly larger
            m = int(rng.integers(0, rows * 255 // 2 + 1))
            t = (m + 1 + rng.integers(0, rows * 255 - m, size=absS.size)) * (wd - absS)
            tie = rng.random(absS.size) < 0.3
            tie[rng.integers(0, absS.size)] = True
            t[tie] = m * (wd - absS[tie])
            ties += int(tie.sum() > 1)
        else:
            t = rng.integers(0, rows * 255 + 1, size=absS.size) * (wd - absS)
            t -= rng.integers(0, np.maximum(t, 1))
        assert t.min() >= 0 and t.max() <= rows * 255 * wd < 1 << 32
        t = t.astype(np.uint32)
        want = select(t, wd, rows, S)
        got = c_select(lib, t, wd, rows)
        assert got[0] == want[0]
        assert np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes()
    assert ties > 400


def test_first_frame_reset_zero_frames_and_clamp():
    rng = np.random.default_rng(2)
    f = rng.integers(0, 256, size=(4, 24, 48), dtype=np.uint8)
    vo = NumpyVisualOdometer(max_shift=8)
    assert vo.update(f[0]) == (0.0, 0.0)
    moved = vo.update(f[1])
    assert moved[0] > 0.0
    vo.reset()
    assert vo.update(f[2]) == (0.0, 0.0)
    # state carries across calls and across the frames of one call
    a = NumpyVisualOdometer(max_shift=8).run(f)
    b = NumpyVisualOdometer(max_shift=8)
    assert np.array_equal(a, np.concatenate([b.run(f[:1]), b.run(f[1:3]), b.run(f[3:])]))
    z = NumpyVisualOdometer(max_shift=8).run(np.zeros((3, 24, 48), dtype=np.uint8))
    assert np.array_equal(z, np.zeros((3, 2))) and not np.signbit(z).any()
    # random frames differ by ~85/255 per pixel average of column sums: far over the clamp
    lo = NumpyVisualOdometer(max_shift=8, vtrans_scale=100.0, vtrans_max=0.5).run(f)
    free = NumpyVisualOdometer(max_shift=8, vtrans_scale=100.0, vtrans_max=1e9).run(f)
    assert (free[1:, 0] > 0.5).all() and (lo[1:, 0] == 0.5).all() and lo[0, 0] == 0.0
    assert np.array_equal(lo[:, 1], free[:, 1])
    with pytest.raises(TypeError):
        NumpyVisualOdometer().update(np.zeros((8, 64), dtype=np.float32))
    with pytest.raises(ValueError):
        vo.update(f[0][:, :47])


REFUSALS = [
    # (im_h, im_w, kwargs): Wd < S; S = 0; S = 65; empty regions; 32-bit overflow
    (16, 24, dict(max_shift=25)),
    (16, 64, dict(max_shift=40, rot_cols=(10, 49))),
    (16, 128, dict(max_shift=0)),
    (16, 128, dict(max_shift=65)),
    (16, 128, dict(trans_rows=(5, 5))),
    (16, 128, dict(rot_cols=(90, 60))),
    (16, 128, dict(trans_rows=(0, 17))),
    (4200, 4096, dict()),             # 4200 * 255 * 4096 >= 2^32
]


@pytest.mark.parametrize('im_h,im_w,kw', REFUSALS)
def test_create_time_refusals(lib, im_h, im_w, kw):
    with pytest.raises(ValueError):
        NumpyVisualOdometer(**kw).run(np.zeros((1, im_h, im_w), dtype=np.uint8))
    p = _lib.VoParams()
    rows = [kw.get('trans_rows') or (0, im_h), kw.get('rot_rows') or (0, im_h)]
    cols = [kw.get('trans_cols') or (0, im_w), kw.get('rot_cols') or (0, im_w)]
    (p.trans_y0, p.trans_y1), (p.rot_y0, p.rot_y1) = rows
    (p.trans_x0, p.trans_x1), (p.rot_x0, p.rot_x1) = cols
    p.max_shift = kw.get('max_shift', 40)
    p.rad_per_column, p.vtrans_scale, p.vtrans_max = 0.01, 100.0, 20.0
    h = ctypes.c_void_p()
    st = lib.rs_vo_create(im_h, im_w, ctypes.byref(p), 0, ctypes.byref(h))
    assert st == _lib.RS_ERR_ARG and not h.value, (st, lib.rs_last_error())


def test_largest_accepted_region_is_not_refused():
    # 4112 * 255 * 4096 = 2^32 - 65,536 < 2^32 (4113 rows would be over)
    assert 4112 * 255 * 4096 < 1 << 32 <= 4113 * 255 * 4096
    from pyratslam_amd.visual_odometer import _Params
    _Params((4112, 4096), None, None, None, None, 40, 90.0, 100.0, 20.0)
    with pytest.raises(ValueError):
        _Params((4113, 4096), None, None, None, None, 40, 90.0, 100.0, 20.0)


def test_no_cpu_fallback_without_device(lib):
    from pyratslam_amd import SimpleVisualOdometer
    if lib.rs_device_count() > 0:
        SimpleVisualOdometer().close()   # constructs without a frame, as the node does
        return
    with pytest.raises(_lib.HipLibraryError):
        SimpleVisualOdometer()
