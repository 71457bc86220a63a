"""RatslamReplay(window=K) on the CPU: the window scheduler as pure functions on hand-made
message lists, and the silent fall-back to the per-frame loop with drop-in classes that have
no ``run(injections=)`` (the oracle), against the golden replay."""
import numpy as np
import pytest

from conftest import load_golden
from pyratslam_amd import replay, rosbag, synthetic
from test_replay import oracle_replay


def odom(vx, wz):
    return ('odom', rosbag.Twist((vx, 0.0, 0.0), (0.0, 0.0, wz)))


FRAME = ('image', None)


def test_a_frame_before_any_twist_has_boundary_zero():
    steps, bounds = replay.window_boundaries([FRAME, odom(1.0, 0.5), FRAME])
    assert steps == [(0.1, 0.05)] and bounds == [0, 1]


def test_two_frames_with_no_twist_between_them_share_a_boundary():
    msgs = [odom(1.0, 0.0), FRAME, FRAME, odom(2.0, -1.0), odom(0.5, 0.0), FRAME]
    steps, bounds = replay.window_boundaries(msgs)
    assert bounds == [1, 1, 3]
    assert steps == [(0.1, 0.0), (0.2, -0.1), (0.05, 0.0)]


def test_filtered_twists_are_no_steps_and_the_rate_divides():
    # the node queues a twist only above 0.001 in |linear.x| or |angular.z| (ros_simulate.py:128)
    msgs = [odom(0.0, 0.0005), FRAME, odom(0.001, -0.001), odom(0.0, -0.002), FRAME, odom(0.0011, 0.0)]
    steps, bounds = replay.window_boundaries(msgs, odom_freq=4)
    assert bounds == [0, 1]
    assert steps == [(0.0, -0.0005), (0.0011 / 4, 0.0)]
    assert replay.window_boundaries([]) == ([], [])
    assert replay.window_boundaries([odom(1.0, 0.0)]) == ([(0.1, 0.0)], [])


def test_a_template_created_and_rematched_inside_one_window():
    # 3 templates known; frames: stored 1, new 3, stored 0, again 3, new 4, again 3, again 4
    kinds = replay.injection_kinds([1, 3, 0, 3, 4, 3, 4], known=3)
    assert kinds == [('stored', 1), ('peak',), ('stored', 0), ('same', 1), ('peak',), ('same', 1), ('same', 4)]
    assert replay.injection_kinds([], known=0) == []
    assert replay.injection_kinds(np.array([0, 0, 1]), known=0) == [('peak',), ('same', 0), ('peak',)]


def test_window_with_the_oracle_falls_back_and_reproduces_the_golden_replay():
    golden = load_golden('ros_replay')
    events = synthetic.ros_stream(int(golden['n']), seed=int(golden['seed']))
    r = oracle_replay(window=5)
    assert not r._windowed()
    res = r.replay_events(events).results()
    assert np.array_equal(res['pc_max'], golden['pc_max'])
    assert np.array_equal(res['template_index'], golden['template_index'])
    assert np.array_equal(res['em_points'], golden['em_points'])
    assert res['templates'] == int(golden['templates'])


def test_window_must_be_a_positive_integer():
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            oracle_replay(window=bad)
