"""Patch normalisation of uint8 view templates, on the CPU: the host rule
(rs_vt_normalise_host, csrc/vt_norm_rule.h) against the NumPy restatement ``normalise_u8`` with
no tolerance; the restatement against an explicit per-pixel loop with math.isqrt; the header
alone under -fsanitize=address,undefined (tests/vt_norm_main.cpp, run as a child process; the
sanitizer is linked into the program, nothing is preloaded); the exposure case the feature is
for; and the arguments of the Python classes and of the replay's command line."""
import ctypes

import numpy as np
import pytest

import _host_program
import _vt_norm_cases as C
from pyratslam_amd import _lib, replay
from pyratslam_amd import view_templates as VT

SHAPES = [(64, 32), (32, 32), (64, 48), (24, 10), (16, 5), (10, 7), (70, 130)]
RADII = (1, 3, 7)
GAINS = (1, 32, 127)


def host_rule(image, radius, gain):
    lib = _lib.load()
    src = np.ascontiguousarray(image, dtype=np.uint8)
    dst = np.full(src.shape, 0x5A, dtype=np.uint8)
    _lib.check(lib.rs_vt_normalise_host(src.shape[0], src.shape[1], radius, gain, _lib.ptr(src, ctypes.c_uint8),
                                        _lib.ptr(dst, ctypes.c_uint8)))
    return dst


@pytest.mark.parametrize('shape', SHAPES)
def test_host_rule_equals_the_restatement(shape):
    ims = C.images(shape, seed=shape[0] * 1000 + shape[1])
    for radius in RADII:
        for gain in GAINS:
            want = VT.normalise_u8(np.stack(ims), radius, gain)       # (n, H, W) at once
            assert want.dtype == np.uint8 and want.shape == (len(ims),) + shape
            for im, w in zip(ims, want):
                assert np.array_equal(host_rule(im, radius, gain), w)
                assert np.array_equal(VT.normalise_u8(im, radius, gain), w)          # (H, W) alone
            assert (want[1] == 128).all()                             # a constant image
            if gain == 127:
                # both clamps are reached (a 0/255 pattern's pixels lie about one deviation out:
                # 128 +- 127, the upper clamp's edge; random bytes pass both)
                assert want.min() == 0 and want.max() == 255 and want[2].max() == 255 and want[2].min() <= 1
            assert np.array_equal(VT.normalise_host(np.stack(ims), radius, gain), want)


def test_image_smaller_than_the_window_uses_all_of_itself():
    im = C.images((10, 7), seed=5)[0]
    got = host_rule(im, 7, 32)
    # rows 2..7 see every row and every pixel every column: one n, one S, one S2 for all of them
    p = im.astype(np.int64)
    n, s1, s2 = p.size, int(p.sum()), int((p * p).sum())
    import math
    s = math.isqrt(n * s2 - s1 * s1)
    for r in range(3, 7):
        for c in range(7):
            num = n * int(p[r, c]) - s1
            q = (32 * abs(num) + s // 2) // s
            assert got[r, c] == min(255, max(0, 128 + q if num > 0 else 128 - q))
    assert np.array_equal(got, VT.normalise_u8(im, 7, 32))


@pytest.mark.parametrize('shape', [(12, 9), (17, 6)])
def test_restatement_equals_an_independent_loop(shape):
    for im in C.images(shape, seed=shape[1]):
        for radius, gain in ((1, 127), (3, 32), (7, 1), (7, 127)):
            assert np.array_equal(VT.normalise_u8(im, radius, gain), C.loop_rule(im, radius, gain))


def test_a_constant_added_changes_no_byte():
    """What the rule is for: b added to every pixel cancels in N and in D."""
    im = np.random.default_rng(3).integers(40, 160, (32, 32), dtype=np.uint8)
    base = VT.normalise_u8(im, 3, 32)
    for b in (1, 40, 95):
        assert np.array_equal(VT.normalise_u8(im + np.uint8(b), 3, 32), base)
        assert np.array_equal(host_rule(im + np.uint8(b), 3, 32), base)


def test_host_rule_refuses_bad_arguments():
    lib = _lib.load()
    a = np.zeros((8, 6), np.uint8)
    b = np.zeros((8, 6), np.uint8)
    pa, pb = _lib.ptr(a, ctypes.c_uint8), _lib.ptr(b, ctypes.c_uint8)
    assert lib.rs_vt_normalise_host(8, 6, 0, 32, pa, pb) == _lib.RS_ERR_ARG
    assert lib.rs_vt_normalise_host(8, 6, 8, 32, pa, pb) == _lib.RS_ERR_ARG
    assert lib.rs_vt_normalise_host(8, 6, 3, 0, pa, pb) == _lib.RS_ERR_ARG
    assert lib.rs_vt_normalise_host(8, 6, 3, 128, pa, pb) == _lib.RS_ERR_ARG
    assert lib.rs_vt_normalise_host(0, 6, 3, 32, pa, pb) == _lib.RS_ERR_ARG
    assert lib.rs_vt_normalise_host(8, 6, 3, 32, pa, pa) == _lib.RS_ERR_ARG      # never in place
    assert lib.rs_vt_normalise_host(8, 6, 3, 32, None, pb) == _lib.RS_ERR_ARG
    assert lib.rs_vt_normalise_host(8, 6, 3, 32, pa, pb) == _lib.RS_OK
    assert lib.rs_version() == 100


def test_norm_rule_header_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'vt_norm_main.cpp', timeout=120)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout


# --- the exposure case ------------------------------------------------------------------
@pytest.fixture(scope='module')
def places():
    frames = C.place_frames()
    return frames, C.ros_templates(frames)


@pytest.mark.parametrize('a,b', C.EXPOSURES)
def test_normalised_revisits_score_below_every_other_place(places, a, b):
    frames, tpl = places
    rev = C.ros_templates(C.revisit_frames(frames, a, b))
    scores = C.score_matrix(VT.normalise_u8(tpl, 3, 32), VT.normalise_u8(rev, 3, 32))
    own = np.diag(scores)
    foreign = scores[~np.eye(16, dtype=bool)]
    print('(a, b) = (%s, %s): own <= %d, foreign >= %d' % (a, b, own.max(), foreign.min()))
    assert own.max() < foreign.min()
    assert np.array_equal(scores.argmin(axis=1), np.arange(16))


def test_raw_revisits_under_an_exposure_offset_go_wrong(places):
    frames, tpl = places
    rev = C.ros_templates(C.revisit_frames(frames, 1.0, 40))
    raw = C.score_matrix(tpl, rev)
    right = int((raw.argmin(axis=1) == np.arange(16)).sum())
    print('raw SAD at (1.0, 40): own <= %d, first argmin right for %d of 16' % (np.diag(raw).max(), right))
    assert right < 16


# --- Python and the command line --------------------------------------------------------------
@pytest.mark.parametrize('bad', [(0, 32), (8, 32), (3, 0), (3, 128), (3,), (3, 32, 1), 3, 'ab', (1.5, 32)])
def test_bad_settings_are_value_errors_before_anything_is_created(bad):
    with pytest.raises(ValueError):
        VT.ViewTemplates._from_shape((32, 32), 100, normalise=bad)
    with pytest.raises(ValueError):
        VT.ViewTemplates(**C.ROS, match_threshold=100, normalise=bad)
    with pytest.raises(ValueError):
        VT.ShardedViewTemplates(**C.ROS, match_threshold=100, rank=0, nranks=2, reducer=lambda k: k, normalise=bad)
    with pytest.raises(ValueError):
        VT.ShardedViewTemplates.from_shape((32, 32), 100, 0, 2, reducer=lambda k: k, normalise=bad)
    with pytest.raises(ValueError):
        replay.RatslamReplay(pcn=object(), vt_normalise=bad)
    if not isinstance(bad, tuple) or len(bad) != 2:
        return
    with pytest.raises(ValueError):
        VT.normalise_u8(np.zeros((8, 8), np.uint8), *bad)


def test_restatement_refuses_other_arrays():
    with pytest.raises(TypeError):
        VT.normalise_u8(np.zeros((8, 8), np.float32), 3, 32)
    with pytest.raises(ValueError):
        VT.normalise_u8(np.zeros(8, np.uint8), 3, 32)
    with pytest.raises(ValueError):
        VT.normalise_u8(np.zeros((2, 2, 8, 8), np.uint8), 3, 32)


class _Normalising(VT.ViewTemplates):
    """A normalising library's host side, with no device: the dtype check comes before any
    device work."""

    def __init__(self, normalise):
        self.mask, self.shape = VT.py2_mask(**C.ROS)
        self.shift_axis = 'rows'
        self.offsets = False
        self.normalise = normalise
        self.templates = []
        self.device, self.rank, self.nranks = 0, 0, 1
        self._float = False
        self._vtf = None
        self._h = None


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_float_frames_at_a_normalising_library_are_type_errors(dtype):
    vts = _Normalising((3, 32))
    frame = np.zeros((256, 256), dtype=dtype)
    tpl = np.zeros((2, 32, 32), dtype=dtype)
    for call in (lambda: vts.match(frame, 0, 0, 0), lambda: vts.match_batch([frame], [(0, 0, 0)]),
                 lambda: vts.add(tpl), lambda: vts.scores(tpl), lambda: vts.match_templates(tpl)):
        with pytest.raises(TypeError, match='normalise'):
            call()
    assert not vts._float and vts._vtf is None and vts.templates == []      # the float paths were not entered
    t = VT.ViewTemplate(0, 0, 0, 0, np.zeros((32, 32), np.uint8), _owner=vts)
    with pytest.raises(TypeError, match='normalise'):
        t.match(np.zeros((32, 32), dtype=dtype))


def test_replay_cli_vt_normalise_flag():
    ap = replay.build_parser()
    assert ap.parse_args(['--synthetic', '5']).vt_normalise is None
    assert ap.parse_args(['--synthetic', '5', '--vt-normalise', '3']).vt_normalise == (3, 32)
    assert ap.parse_args(['--synthetic', '5', '--vt-normalise', '7,127']).vt_normalise == (7, 127)
    assert ap.parse_args(['--synthetic', '5', '--vt-normalise', '1,1', '--vt-metric', 'sad']).vt_normalise == (1, 1)
    for bad in ('0', '8', '3,0', '3,128', '3,32,1', 'x', '3,', ''):
        with pytest.raises(SystemExit):
            ap.parse_args(['--synthetic', '5', '--vt-normalise', bad])
    assert '--vt-normalise' in ap.format_help()


class _Templates:
    metric = 'wrapped'
    templates = []

    def __init__(self, normalise):
        self.normalise = normalise


def test_replay_refuses_a_library_with_another_setting():
    with pytest.raises(ValueError, match='vt_normalise'):
        replay.RatslamReplay(pcn=object(), vts=_Templates(None), vt_normalise=(3, 32))
    with pytest.raises(ValueError, match='vt_normalise'):
        replay.RatslamReplay(pcn=object(), vts=_Templates((3, 32)))
    with pytest.raises(ValueError, match='vt_normalise'):
        replay.RatslamReplay(pcn=object(), vts=_Templates((3, 16)), vt_normalise=(3, 32))
