"""The true-SAD metric of the uint8 view templates, on the CPU: the NumPy restatement
(numpy_sad_u8_scores) against the reference's formula on float casts, the contrast with the
wrapped metric that motivates it, the replay's command line, the refusal of an unknown metric
before any device work, and the new dispatch rules of csrc/vt_plan.h (tests/vt_sad_plan_main.cpp,
built with -fsanitize=address,undefined and run as a child process; the sanitizer is linked
into the program, nothing is preloaded)."""
import numpy as np
import pytest

import _host_program
from oracle import view_templates as V
from pyratslam_amd import replay, synthetic
from pyratslam_amd.view_templates import (METRICS, ShardedViewTemplates, ViewTemplates,
                                          numpy_sad_u8_scores)


def two_sided(library, q, seed, noise=3):
    """Queries off a library: a template rolled by -7..7 rows plus noise in -noise..noise
    (two-sided, clipped to a byte), one in five a fresh image."""
    rng = np.random.default_rng(seed)
    t, h, w = library.shape
    out = np.empty((q, h, w), np.uint8)
    for i in range(q):
        if rng.random() < 0.8:
            b = np.roll(library[int(rng.integers(0, t))], int(rng.integers(-7, 8)), axis=0)
            out[i] = np.clip(b.astype(np.int64) + rng.integers(-noise, noise + 1, (h, w)), 0, 255)
        else:
            out[i] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return out


@pytest.mark.parametrize('shape', [(64, 32), (32, 32), (32, 30), (18, 8), (16, 32)])
def test_restatement_is_the_reference_formula_on_float_casts(shape):
    """numpy_sad_u8_scores == ViewTemplate.match (oracle.vt_score) on the same arrays cast to
    float64 and to float32 (every score is below 2^24: exact in float32 too), with all-0
    against all-255 pairs at the maximum (H - 16) * W * 255."""
    h, w = shape
    lib = V.synthetic_library(12, h, w, seed=h * w)
    lib[3], lib[4] = 0, 255
    lib[5] = np.where(np.random.default_rng(5).random((h, w)) < 0.5, 0, 255)
    qs = two_sided(lib, 7, seed=h + w)
    qs[0], qs[1] = 255, 0
    top = (h - 2 * V.MAX_OFFSET) * w * 255
    assert top < 2 ** 24
    for q in qs:
        got = numpy_sad_u8_scores(lib, q)
        assert got.dtype == np.uint64 and got.shape == (12,)
        for dt in (np.float64, np.float32):
            want = [V.vt_score(t.astype(dt), q.astype(dt)) for t in lib]
            assert np.array_equal(got, np.array(want, dtype=np.float64).astype(np.uint64)), dt
    assert numpy_sad_u8_scores(lib, qs[0])[3] == top and numpy_sad_u8_scores(lib, qs[1])[4] == top
    assert numpy_sad_u8_scores(lib, qs[0])[4] == 0 and numpy_sad_u8_scores(lib, qs[1])[3] == 0
    if h == 2 * V.MAX_OFFSET:     # an empty window: every score 0, as the reference's empty slices give
        assert not np.stack([numpy_sad_u8_scores(lib, q) for q in qs]).any()
    assert numpy_sad_u8_scores(lib[:0], qs[0]).shape == (0,)
    with pytest.raises(TypeError):
        numpy_sad_u8_scores(lib.astype(np.float32), qs[0])


def test_two_sided_noise_wrapped_against_sad():
    """Frames 14 and 15 of the synthetic ROS stream show the same heading with noise U{0..2}:
    the wrapped score of the pair sits on the shipped threshold (within 10 % of 45000: every
    pixel where the query is above the template scores 255 - d), the true SAD far below it."""
    frames = [ev[2] for ev in synthetic.ros_stream(16) if ev[0] == 'image']
    mask, shape = V.py2_mask(replay.X_RANGE, replay.Y_RANGE, replay.X_STEP, replay.Y_STEP, *replay.IM_SIZE)
    assert shape == (32, 32)
    t, q = (f[mask].reshape(shape) for f in frames[14:16])
    wrapped = int(V.vt_scores_library(t[None], q)[0])
    sad = int(numpy_sad_u8_scores(t[None], q)[0])
    print('frames 14 / 15: wrapped %d, sad %d' % (wrapped, sad))
    assert abs(wrapped - replay.MATCH_THRESHOLD) <= replay.MATCH_THRESHOLD // 10
    assert sad < 1024


def test_replay_cli_flags():
    ap = replay.build_parser()
    args = ap.parse_args(['--synthetic', '5'])
    assert args.vt_metric == 'wrapped' and args.match_threshold == 45000 == replay.MATCH_THRESHOLD
    args = ap.parse_args(['--synthetic', '5', '--vt-metric', 'sad', '--match-threshold', '2048'])
    assert args.vt_metric == 'sad' and args.match_threshold == 2048
    with pytest.raises(SystemExit):
        ap.parse_args(['--synthetic', '5', '--vt-metric', 'l2'])
    text = ap.format_help()
    assert '--vt-metric' in text and '--match-threshold' in text and '2048' in text


def test_unknown_metric_is_a_value_error_before_any_device_work():
    assert sorted(METRICS) == ['sad', 'wrapped']
    with pytest.raises(ValueError, match='unknown metric'):
        ViewTemplates._from_shape((64, 32), 45000, metric='l2')
    with pytest.raises(ValueError, match='unknown metric'):
        ViewTemplates(replay.X_RANGE, replay.Y_RANGE, 2, 2, 256, 256, 45000, metric='SAD')
    with pytest.raises(ValueError, match='unknown metric'):
        ShardedViewTemplates.from_shape((64, 32), 45000, 0, 2, reducer=lambda k: k, metric=None)
    with pytest.raises(ValueError, match='unknown metric'):
        replay.RatslamReplay(pcn=_NoNetwork(), vt_metric='l2')


class _NoNetwork:
    def inject(self, energy, cell):
        pass


def test_sad_plan_rules_under_sanitizers(tmp_path):
    r = _host_program.run(tmp_path, 'vt_sad_plan_main.cpp', timeout=60)
    assert r.returncode == 0, r.stdout
    assert ' 0 failed' in r.stdout
