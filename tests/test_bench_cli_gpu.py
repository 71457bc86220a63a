"""bench.py's plain run: the headline leg alone, --steps timed steps, and
--dump-outputs writing what the last timed step returned."""
import json
import sys

import numpy as np
import pytest

import bench
from oracle import view_templates as V
from pyratslam_amd import synthetic

pytestmark = pytest.mark.gpu

T, Q, BPS, STEPS = 96, 48, 2, 3


def _run(monkeypatch, capsys, out_dir, *extra):
    monkeypatch.setattr(sys, 'argv', [
        'bench.py', '--gpus', '1', '--steps', str(STEPS), '--warmup', '1', '--clock-warmup-ms', '0',
        '--templates-per-gpu', str(T), '--queries', str(Q), '--batches-per-step', str(BPS),
        '--dump-outputs', str(out_dir), *extra])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_last_one(monkeypatch, capsys, tmp_path):
    res = _run(monkeypatch, capsys, tmp_path / 'a')
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in res, key
    # only the headline leg ran, over exactly --steps steps
    for key in ('library_sharded', 'pose_cell', 'pose_cell_stress', 'replay', 'cpu_baseline',
                'template_scan'):
        assert key not in res, key
    assert res['steps'] == STEPS and res['config']['timed_batches'] == STEPS * BPS
    assert res['ms_per_step'] > 0
    assert abs(res['ms_per_step'] * STEPS - 1e3 * res['config']['timed_region_s']) < 1e-6
    assert res['known_answer_hits_correct'] is True
    idx = np.load(tmp_path / 'a' / 'index.npy')
    score = np.load(tmp_path / 'a' / 'score.npy')
    assert idx.dtype == np.float64 and score.dtype == np.float64
    assert idx.shape == (BPS, Q) and score.shape == (BPS, Q)
    # the last step (i = STEPS - 1) matched resident batches (STEPS - 1) * BPS + b; batch
    # k > 0 is synthetic.queries_fast(seed 2 + 1000 k): exact against the oracle
    lib = synthetic.library(T, seed=1)
    for b in range(BPS):
        k = (STEPS - 1) * BPS + b
        qs, _ = synthetic.queries_fast(lib, Q, seed=2 + 1000 * k)
        for i in range(Q):
            s = V.vt_scores_library(lib, qs[i])
            assert idx[b, i] == int(np.argmin(s)) and score[b, i] == s.min(), (b, i)
    # the same arguments give the same inputs, hence the same outputs
    _run(monkeypatch, capsys, tmp_path / 'b')
    assert np.array_equal(idx, np.load(tmp_path / 'b' / 'index.npy'))
    assert np.array_equal(score, np.load(tmp_path / 'b' / 'score.npy'))
