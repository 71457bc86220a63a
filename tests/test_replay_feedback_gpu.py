"""The view-template feedback on the batched paths: camera-only
``replay_frames`` with ``feedback_energy`` in one ``pcn.run(deltas, injections=...)`` per
batch, and ``RatslamReplay(window=K)`` for ``replay_events`` / ``replay_bag`` -- each equal,
in every output and every template's location, to the per-frame loop."""
import math

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FEEDBACK = 0.02


@pytest.fixture(scope='module', autouse=True)
def built():
    from pyratslam_amd import _build
    _build.build()


@pytest.fixture(scope='module')
def golden():
    return load_golden('ros_replay')


@pytest.fixture(scope='module')
def events(golden):
    from pyratslam_amd import synthetic
    return synthetic.ros_stream(int(golden['n']), seed=int(golden['seed']))


def everything(r):
    res = r.results()
    out = {k: res[k] for k in ('pc_max', 'template_index', 'em_points')}
    out['deltas'] = np.array(r.deltas, dtype=np.float64).reshape(-1, 2)
    out['locations'] = np.array([tuple(int(v) for v in t.location()) for t in r.vts.templates]).reshape(-1, 3)
    if hasattr(r.em, 'links'):
        out['poses'], out['links'] = r.em.poses(), r.em.links()
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def counted(pcn, calls):
    """pcn with run() counted (the bound method keeps its signature for the replay's probe)."""
    inner = pcn.run

    def run(odometry, poses=False, injections=None):
        calls.append((len(odometry), None if injections is None else len(injections)))
        return inner(odometry, poses=poses, injections=injections)
    pcn.run = run
    return pcn


# -- replay_frames with feedback --------------------------------------------------------
@pytest.fixture(scope='module')
def frames_per_frame():
    from pyratslam_amd import replay, synthetic
    ev = [e for e in synthetic.ros_stream(120, seed=0) if e[0] == 'image'][:40]
    want = everything(replay.RatslamReplay(use_visual_odometry=True, feedback_energy=FEEDBACK).replay_events(ev))
    assert len(want['locations']) > 1 and len(want['locations']) < 40    # templates made and re-matched
    return np.stack([e[2] for e in ev]), want


@pytest.mark.parametrize('batch', [64, 7])
def test_replay_frames_with_feedback_runs_batched(frames_per_frame, batch):
    from pyratslam_amd import PoseCellNetwork, replay
    frames, want = frames_per_frame
    calls = []
    pcn = counted(PoseCellNetwork(replay.POSE_SIZE), calls)
    r = replay.RatslamReplay(use_visual_odometry=True, feedback_energy=FEEDBACK, pcn=pcn)
    same(everything(r.replay_frames(frames, batch=batch)), want)
    assert len(calls) == math.ceil(40 / batch), calls
    assert all(n == ni for n, ni in calls) and sum(n for n, _ in calls) == 40


def test_replay_frames_with_feedback_and_subcell_peak(frames_per_frame):
    from pyratslam_amd import replay
    frames, want = frames_per_frame
    kw = dict(use_visual_odometry=True, feedback_energy=FEEDBACK, subcell_peak=True)
    r = replay.RatslamReplay(**kw).replay_frames(frames, batch=16)
    same(everything(r), want)
    # (the poses' own bound: tests/test_pc_inject_run_gpu.py; here, that each step has one,
    # inside the box round its peak)
    res = r.results()
    assert res['pc_pose'].shape == (40, 3)
    for ax, n in enumerate(replay.POSE_SIZE):
        d = np.abs(res['pc_pose'][:, ax] - res['pc_max'][:, ax]) % n
        assert np.minimum(d, n - d).max() <= 3


# -- window --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def window_one(events):
    from pyratslam_amd import LinkedExperienceMap, replay
    out = {}
    for fb in (None, FEEDBACK):
        for linked in (False, True):
            em = LinkedExperienceMap() if linked else None
            out[fb, linked] = everything(replay.RatslamReplay(feedback_energy=fb, em=em).replay_events(events))
    return out


@pytest.mark.parametrize('linked', [False, True])
@pytest.mark.parametrize('feedback', [None, FEEDBACK])
@pytest.mark.parametrize('window', [5, 64])
def test_window_equals_the_per_frame_loop(events, window_one, golden, window, feedback, linked):
    from pyratslam_amd import LinkedExperienceMap, PoseCellNetwork, replay
    calls = []
    pcn = counted(PoseCellNetwork(replay.POSE_SIZE), calls)
    em = LinkedExperienceMap() if linked else None
    r = replay.RatslamReplay(feedback_energy=feedback, em=em, window=window, pcn=pcn).replay_events(events)
    got = everything(r)
    same(got, window_one[feedback, linked])
    nframes = sum(e[0] == 'image' for e in events)
    assert len(calls) <= math.ceil(nframes / window) + 1, calls
    if not feedback:
        assert np.array_equal(got['pc_max'], golden['pc_max'])
        assert np.array_equal(got['template_index'], golden['template_index'])
        if not linked:
            assert np.array_equal(got['em_points'], golden['em_points'])


def test_window_bag_replay_and_cli(tmp_path, events, window_one, capsys):
    import json
    from pyratslam_amd import replay, synthetic
    path = synthetic.write_ros_bag(str(tmp_path / 'ds.bag'), events)
    r = replay.RatslamReplay(feedback_energy=FEEDBACK, window=8).replay_bag(path)
    same(everything(r), window_one[FEEDBACK, False])
    assert replay.main(['--synthetic', '24', '--window', '8', '--feedback', '0.02']) == 0
    a = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert replay.main(['--synthetic', '24', '--feedback', '0.02']) == 0
    b = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for k in ('pc_max', 'template_index', 'em_points', 'templates'):
        assert a[k] == b[k], k


def test_window_falls_back_where_it_cannot_batch(events):
    from pyratslam_amd import replay
    ev = events[:60]
    want = everything(replay.RatslamReplay(publish=True).replay_events(ev))
    r = replay.RatslamReplay(publish=True, window=8)
    assert not r._windowed()
    same(everything(r.replay_events(ev)), want)
    assert r.published == want['pc_max'].shape[0] * int(np.prod(replay.POSE_SIZE))
    assert not replay.RatslamReplay(use_visual_odometry=True, window=8)._windowed()
    with pytest.raises(ValueError):
        replay.RatslamReplay(window=0)
