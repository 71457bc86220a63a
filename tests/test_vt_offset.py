"""The row offset of a view-template match, on the CPU: the host rule
(rs_vt_offset_profile_host, csrc/vt_offset_rule.h) against the explicit NumPy loop written
here, with no tolerance; the header alone under -fsanitize=address,undefined
(tests/vt_offset_main.cpp, run as a child process; the sanitizer is linked into the program,
nothing is preloaded); ``rel_rad`` in the linked map on NumpyLinkedExperienceMap; the host side
of ``shift_axis='cols'``; ``refine_offset``; and the replay's command line."""
import ctypes

import numpy as np
import pytest

import _em_graphs as G
import _host_program
from oracle import view_templates as V
from pyratslam_amd import _lib, replay, synthetic
from pyratslam_amd import linked_experience_map as M
from pyratslam_amd import view_templates as VT

METRICS = ('wrapped', 'sad')


def restate(t, q, m=8, metric='wrapped'):
    """Section 1 of the rule, literally: (offset, profile uint32[2m-1])."""
    t, q = np.asarray(t).astype(np.int64), np.asarray(q).astype(np.int64)
    h = t.shape[0]
    prof = np.zeros(2 * m - 1, dtype=np.uint32)
    for k in range(2 * m - 1):
        o = k - (m - 1)
        d = t[m + o:h - m + o] - q[m:h - m]
        prof[k] = int((np.abs(d) if metric == 'sad' else np.mod(d, 256)).sum())
    best = 0
    for k in range(1, 2 * m - 1):
        if prof[k] < prof[best]:      # strict: the first minimal entry stays
            best = k
    return best - (m - 1), prof


def host_rule(t, q, m=8, metric='wrapped'):
    lib = _lib.load()
    t, q = np.ascontiguousarray(t, dtype=np.uint8), np.ascontiguousarray(q, dtype=np.uint8)
    prof = np.full(2 * m - 1, 0xDEADBEEF, dtype=np.uint32)
    off = ctypes.c_int32(99)
    _lib.check(lib.rs_vt_offset_profile_host(VT.METRICS[metric], t.shape[0], t.shape[1], m,
                                             _lib.ptr(t, ctypes.c_uint8), _lib.ptr(q, ctypes.c_uint8),
                                             _lib.ptr(prof, ctypes.c_uint32), ctypes.byref(off)))
    return off.value, prof


def images(shape, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, shape, dtype=np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8),
            np.where(rng.random(shape) < 0.5, 0, 255).astype(np.uint8), np.full(shape, 77, np.uint8)]


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('shape,m', [((64, 32), 8), ((32, 32), 8), ((64, 48), 8), ((24, 10), 8), ((16, 5), 8),
                                      ((10, 7), 3)])
def test_host_rule_equals_the_numpy_loop(shape, m, metric):
    ims = images(shape, seed=shape[0] * 100 + shape[1])
    noisy = np.clip(np.roll(ims[0], 3, axis=0).astype(np.int64)
                    + np.random.default_rng(1).integers(-3, 4, shape), 0, 255).astype(np.uint8)
    for t in ims:
        for q in ims + [noisy]:
            want_o, want_p = restate(t, q, m, metric)
            got_o, got_p = host_rule(t, q, m, metric)
            assert got_o == want_o and np.array_equal(got_p, want_p)
            np_o, np_p = VT.numpy_offset_profile(t, q, m, metric)       # the package's restatement too
            assert np_o == want_o and np.array_equal(np_p, want_p) and np_p.dtype == np.uint32
            if shape[0] == 2 * m:          # an empty window: zeros, the first offset
                assert got_o == -(m - 1) and not got_p.any()
            if t.min() == t.max() and q.min() == q.max():   # constant images: every offset ties
                assert len(set(got_p.tolist())) == 1 and got_o == -(m - 1)
    # the template rolled by each of the offsets: Q[r] = T[r - k], an exact zero at offset -k
    t = ims[0]
    if shape[0] > 2 * m:
        for k in range(-(m - 1), m):
            o, p = host_rule(t, np.roll(t, k, axis=0), m, metric)
            want_o, want_p = restate(t, np.roll(t, k, axis=0), m, metric)
            assert (o, p.tolist()) == (want_o, want_p.tolist())
            assert o == -k and p[m - 1 - k] == 0 and (np.delete(p, m - 1 - k) > 0).all()


@pytest.mark.parametrize('shape', [(64, 32), (32, 32), (64, 48), (24, 10), (16, 5)])
def test_profile_minimum_is_the_score(shape):
    lib = V.synthetic_library(6, shape[0], shape[1], seed=shape[1])
    rng = np.random.default_rng(shape[0])
    qs = [np.clip(np.roll(lib[i % 6], int(rng.integers(-7, 8)), axis=0).astype(np.int64)
                  + rng.integers(-3, 4, shape), 0, 255).astype(np.uint8) for i in range(8)]
    for q in qs:
        sad = VT.numpy_sad_u8_scores(lib, q)
        for j, t in enumerate(lib):
            assert host_rule(t, q, 8, 'wrapped')[1].min() == V.vt_score(t, q)
            assert host_rule(t, q, 8, 'sad')[1].min() == sad[j]


def test_host_rule_refuses_bad_arguments():
    lib = _lib.load()
    t = np.zeros((16, 4), np.uint8)
    prof = np.zeros(15, np.uint32)
    off = ctypes.c_int32(0)
    args = (_lib.ptr(t, ctypes.c_uint8), _lib.ptr(t, ctypes.c_uint8), _lib.ptr(prof, ctypes.c_uint32),
            ctypes.byref(off))
    assert lib.rs_vt_offset_profile_host(2, 16, 4, 8, *args) == _lib.RS_ERR_ARG      # unknown metric
    assert lib.rs_vt_offset_profile_host(0, 15, 4, 8, *args) == _lib.RS_ERR_ARG      # H < 2M
    assert lib.rs_vt_offset_profile_host(0, 16, 4, 0, *args) == _lib.RS_ERR_ARG
    assert lib.rs_vt_offset_profile_host(0, 16, 4, 8, None, *args[1:]) == _lib.RS_ERR_ARG
    assert lib.rs_vt_offset_profile_host(0, 16, 4, 8, *args) == _lib.RS_OK
    assert lib.rs_version() == 100


def test_offset_rule_header_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'vt_offset_main.cpp', timeout=120)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout


# --- the linked map ------------------------------------------------------------------
DELTA = 0.1


def drive_square(rel_rad):
    """A unit square driven back to its first corner, arriving turned by DELTA; the last
    on_template closes the loop with ``rel_rad``.  Relaxation is left to the test."""
    em = M.NumpyLinkedExperienceMap(exp_loops=0)
    em.on_template(0)
    em.update(1, 0)
    em.on_template(1)
    em.update(1, np.pi / 2)
    em.on_template(2)
    em.update(1, np.pi / 2)
    em.on_template(3)
    em.update(1, np.pi / 2)
    em.update(0, np.pi / 2 + DELTA)
    if rel_rad is None:
        em.on_template(0)
    else:
        em.on_template(0, rel_rad=rel_rad)
    return em


def test_rel_rad_closes_the_square_exactly():
    em = drive_square(DELTA)
    links = em.links()
    assert (links['a'][-1], links['b'][-1]) == (3, 0) and len(links) == 4
    ex, ey, df = M.residuals(em.poses(), links)
    assert abs(ex[-1]) < 1e-12 and abs(ey[-1]) < 1e-12 and abs(df[-1]) < 1e-12
    before = em.poses()
    em.iterate(100)
    assert np.abs(em.poses() - before).max() < 1e-12
    em.update(1, 0)
    x, y = em.get_current_point()
    assert abs(x - np.cos(DELTA)) < 1e-12 and abs(y - np.sin(DELTA)) < 1e-12


@pytest.mark.parametrize('rel', [None, 0.0])
def test_without_rel_rad_the_link_keeps_the_heading_error(rel):
    em = drive_square(rel)
    ex, ey, df = M.residuals(em.poses(), em.links())
    assert abs(ex[-1]) < 1e-12 and abs(ey[-1]) < 1e-12
    assert abs(abs(df[-1]) - DELTA) < 1e-12
    em.update(1, 0)
    x, y = em.get_current_point()
    assert abs(x - 1.0) < 1e-12 and abs(y) < 1e-12


def test_rel_rad_is_ignored_by_an_unseen_template_and_checked():
    a, b = M.NumpyLinkedExperienceMap(exp_loops=3), M.NumpyLinkedExperienceMap(exp_loops=3)
    for k in range(5):
        a.on_template(k, rel_rad=0.3 * k - 0.5)
        b.on_template(k)
        for em in (a, b):
            em.update(0.5, 0.4)
    assert np.array_equal(a.poses(), b.poses()) and np.array_equal(a.links(), b.links())
    assert a.theta_current == b.theta_current
    with pytest.raises(ValueError):
        a.on_template(0, rel_rad=float('nan'))


def test_explicit_zero_rel_rad_is_bit_identical_on_the_ring():
    """The ring of tests/_em_graphs.py driven with drifting odometry, three laps (every place
    revisited twice: closure links, then none): rel_rad=0.0 on every call against no argument."""
    maps = []
    for explicit in (False, True):
        em = M.NumpyLinkedExperienceMap(exp_loops=5)
        turn = 2 * np.pi / 40
        for k in range(3 * 40):
            if explicit:
                em.on_template(k % 40, rel_rad=0.0)
            else:
                em.on_template(k % 40)
            em.update(0.1 * 1.002, turn * 1.01)
        maps.append(em)
    assert maps[0].poses().tobytes() == maps[1].poses().tobytes()
    assert maps[0].links().tobytes() == maps[1].links().tobytes()
    assert maps[0].get_current_point() == maps[1].get_current_point()
    # and on the stored ring graph: loading and relaxing it does not depend on the new argument
    poses, links = G.ring(60)
    a = M.NumpyLinkedExperienceMap(exp_loops=7).load(poses, links)
    a.iterate()
    assert a.poses().tobytes() == M.relax(poses, links, 7).tobytes()


# --- shift_axis='cols', host side ------------------------------------------------------
def host_only(shift_axis):
    vts = VT.ViewTemplates.__new__(VT.ViewTemplates)
    return vts._set_geometry(replay.X_RANGE, replay.Y_RANGE, replay.X_STEP, replay.Y_STEP, *replay.IM_SIZE,
                             shift_axis)


def test_cols_is_the_transposed_gather():
    rows, cols = host_only('rows'), host_only('cols')
    assert rows.shape == (32, 32) == cols.shape
    frame = np.random.default_rng(3).integers(0, 256, replay.IM_SIZE, dtype=np.uint8)
    want = frame[rows.mask].reshape(rows.shape)
    assert np.array_equal(rows.subsample(frame), want)
    got = cols.subsample(frame)
    assert np.array_equal(got, want.T) and got.flags['C_CONTIGUOUS']
    assert np.array_equal(frame.reshape(-1)[cols.gather_pixels()].reshape(cols.shape), want.T)
    assert np.array_equal(frame.reshape(-1)[rows.gather_pixels()].reshape(rows.shape), want)
    assert np.array_equal(rows.gather_pixels(), np.flatnonzero(rows.mask.ravel()))
    with pytest.raises(ValueError, match='shift_axis'):
        host_only('diagonal')
    # a window that is not square: the stored shape is the transposed one
    wide = VT.ViewTemplates.__new__(VT.ViewTemplates)._set_geometry((32, 96), (32, 80), 2, 2, 256, 256, 'cols')
    tall = VT.ViewTemplates.__new__(VT.ViewTemplates)._set_geometry((32, 96), (32, 80), 2, 2, 256, 256, 'rows')
    assert wide.shape == tall.shape[::-1] and tall.shape == (32, 24)
    assert np.array_equal(wide.subsample(frame), tall.subsample(frame).T)
    assert np.array_equal(frame.reshape(-1)[wide.gather_pixels()].reshape(wide.shape), tall.subsample(frame).T)


def pano_template(vts, pano, c0):
    return vts.subsample(pano[:, (c0 + np.arange(256)) % pano.shape[1]])


def test_column_shift_is_the_offset_and_refines_to_half_steps():
    """The ROS window on the synthetic panorama, templates stored column-major: a frame cut
    2k columns further has its unique minimum, 0, at offset k under both metrics; a frame cut
    2k + 1 columns further (half a template row) refines to k + 0.5 within 0.1 rows."""
    cols = host_only('cols')
    pano = synthetic.panorama(256, 1024, 0)
    worst = 0.0
    for c0 in (0, 100, 517, 1000):
        t = pano_template(cols, pano, c0)
        for k in range(-7, 8):
            q = pano_template(cols, pano, c0 + 2 * k)
            for metric in METRICS:
                o, p = host_rule(t, q, 8, metric)
                assert o == k and p[k + 7] == 0 and np.sort(p)[1] >= 1522
        # half-steps -5.5 .. 5.5: the minimum is entry k or k + 1, both with two neighbours (at
        # +-6.5 it may be the profile's end, where the integer offset is the documented answer)
        for k in range(-6, 6):
            q = pano_template(cols, pano, c0 + 2 * k + 1)
            o, p = host_rule(t, q, 8, 'sad')
            fine = VT.refine_offset(p)
            worst = max(worst, abs(fine - (k + 0.5)))
            assert abs(fine - (k + 0.5)) < 0.1
            assert VT.ViewTemplate.refine_offset(p) == fine
    print('refine_offset: largest half-step error %.3f rows' % worst)


def test_refine_offset_edges():
    left = np.array([1, 5, 9, 12, 14, 20, 30, 40, 50, 60, 70, 80, 90, 95, 99], np.uint32)
    assert VT.refine_offset(left) == -7.0 and VT.refine_offset(left[::-1]) == 7.0
    assert VT.refine_offset(np.full(15, 42, np.uint32)) == -7.0            # flat: the first entry
    plateau = np.array([9, 9, 3, 3, 3, 9, 9], np.uint32)                   # the first of three equal minima
    assert VT.refine_offset(plateau) == pytest.approx(-1 + 0.5 * (9 - 3) / (9 - 6 + 3))
    flat_mid = np.array([9, 3, 3, 3, 9], np.uint32)
    assert VT.refine_offset(flat_mid[1:4]) == -1.0                          # three equal entries
    sym = np.array([10, 4, 2, 4, 10], np.uint32)
    assert VT.refine_offset(sym) == 0.0
    assert VT.refine_offset(np.array([10, 4, 2, 6, 10], np.uint32)) == pytest.approx(0.5 * (4 - 6) / (4 - 4 + 6))
    both = VT.refine_offset(np.stack([sym, sym[::-1]]))
    assert both.shape == (2,) and both.tolist() == [0.0, 0.0]
    # uint32 entries near the top do not wrap in the differences
    big = np.array([0xFFFFFFFF, 0xFFFFFFF0, 0xFFFFFFFF], np.uint32)
    assert VT.refine_offset(big) == 0.0
    with pytest.raises(ValueError):
        VT.refine_offset(np.zeros(4, np.uint32))


def test_replay_cli_view_shift_flags():
    ap = replay.build_parser()
    args = ap.parse_args(['--synthetic', '5'])
    assert args.view_shift is False and args.view_fov is None
    args = ap.parse_args(['--synthetic', '5', '--view-shift', '--view-fov', '1.2', '--loop-closure'])
    assert args.view_shift and args.view_fov == 1.2
    assert '--view-shift' in ap.format_help() and '--view-fov' in ap.format_help()


class _NoNetwork:
    def inject(self, energy, cell):
        pass


class _PlainTemplates:
    metric = 'wrapped'
    templates = []


def test_replay_refuses_view_shift_without_offsets_before_any_device_work():
    with pytest.raises(ValueError, match='view_fov'):
        replay.RatslamReplay(pcn=_NoNetwork(), vts=_PlainTemplates(), view_shift=True)
    with pytest.raises(ValueError, match="shift_axis='cols', offsets=True"):
        replay.RatslamReplay(pcn=_NoNetwork(), vts=_PlainTemplates(), view_shift=True, view_fov=np.pi / 2)
    r = replay.RatslamReplay(pcn=_NoNetwork(), vts=_PlainTemplates())
    assert r.view_shift is False and 'view_offset' not in r.results()
