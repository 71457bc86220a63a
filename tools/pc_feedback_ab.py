#!/usr/bin/env python3
"""A/B timing of the view-template feedback on the batched paths (GPU box).

usage: python tools/pc_feedback_ab.py [--rounds 5] [--frames 2000] [--messages 2000] [--steps 1000]
                                      [--batches 10] [--out profiles/pc_feedback/pc_feedback_ab.json]
One process alternates its legs, round by round, after a warm-up of every leg (a whole
replay, or one run() of the timed length); every replay leg builds a fresh RatslamReplay,
outside the clock.
  (a) frames    camera-only replay_frames of --frames synthetic frames with
                feedback_energy=0.02: batch=64 (one run(deltas, injections=...) per batch)
                against batch=1 (the per-frame path, what the parent commit takes); frames/s.
  (b) events    replay_events of synthetic.ros_stream(--messages) (an odometry message and
                a frame each) at window 1, 8 and 64, with and without feedback; messages/s
                (odometry messages and frames both counted).
  (c) run       device microseconds per step (HIP events round the call) of run(od) of
                --steps steps at 21x21x36 and 64x64x36: no injection, against an explicit
                injection in front of every step -- the finishing pass per injection that
                injecting on load inside the step kernel would save.
A host clock round whole replays, which end with their results on the host; device events
for (c).  Per leg: the median over the rounds and the spread (max - min over the median).
The legs of one comparison must have computed the same thing: the tool asserts it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEEDBACK = 0.02


def summary(values):
    import numpy as np
    med = float(np.median(values))
    return {'median': med, 'spread': (max(values) - min(values)) / med, 'rounds': [float(v) for v in values]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--messages', type=int, default=2000, help='odometry+frame pairs of the synthetic stream')
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--batches', type=int, default=10, help='(c): run() calls per round')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    from pyratslam_amd import PoseCellNetwork, replay, synthetic

    out = {'rounds': a.rounds, 'frames': a.frames, 'messages': a.messages, 'steps': a.steps, 'batches': a.batches}

    def outputs(r):
        res = r.results()
        return [res['pc_max'], res['template_index'], res['em_points'],
                np.array([t.location() for t in r.vts.templates], dtype=np.int64)]

    def replayed(make, go):
        """A fresh RatslamReplay (outside the clock) through its replay: (seconds, outputs)."""
        r = make()
        t0 = time.perf_counter()
        go(r)
        dt = time.perf_counter() - t0
        res = outputs(r)
        r.pcn.close()
        r.vts.close()
        if hasattr(r.vo, 'close'):
            r.vo.close()
        return dt, res

    def timed(legs, count):
        """legs: name -> (make, go).  The legs' outputs and their rates, count / seconds."""
        ref = {k: replayed(*leg)[1] for k, leg in legs.items()}       # warm-up of every leg
        rate = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, leg in legs.items():
                dt, res = replayed(*leg)
                rate[k].append(count / dt)
                assert all(np.array_equal(x, y) for x, y in zip(res, ref[k])), k
        return ref, {k: summary(v) for k, v in rate.items()}

    # (a) camera-only frames with feedback
    frames = np.stack([e[2] for e in synthetic.ros_stream(a.frames, seed=0) if e[0] == 'image'])
    legs = {'batch%d' % b: (lambda: replay.RatslamReplay(use_visual_odometry=True, feedback_energy=FEEDBACK),
                            lambda r, b=b: r.replay_frames(frames, batch=b)) for b in (1, 64)}
    ref, out['frames_per_s'] = timed(legs, len(frames))
    assert all(np.array_equal(x, y) for x, y in zip(ref['batch1'], ref['batch64']))
    print('(a) frames/s', {k: '%.0f (%.1f%%)' % (v['median'], 100 * v['spread'])
                           for k, v in out['frames_per_s'].items()}, flush=True)

    # (b) odometry-mode events by window
    events = synthetic.ros_stream(a.messages, seed=0)
    out['messages_per_s'] = {}
    for fb in (None, FEEDBACK):
        legs = {'window%d' % w: (lambda w=w: replay.RatslamReplay(feedback_energy=fb, window=w),
                                 lambda r: r.replay_events(events)) for w in (1, 8, 64)}
        ref, rates = timed(legs, len(events))
        for k in ('window8', 'window64'):
            assert all(np.array_equal(x, y) for x, y in zip(ref['window1'], ref[k])), (fb, k)
        out['messages_per_s']['feedback' if fb else 'plain'] = rates
        print('(b) messages/s', 'feedback' if fb else 'plain',
              {k: '%.0f (%.1f%%)' % (v['median'], 100 * v['spread']) for k, v in rates.items()}, flush=True)

    # (c) device time per step with an explicit injection in front of every step
    out['device_us_per_step'] = {}
    od = synthetic.odometry(a.steps, seed=7, vtrans_max=0.3, vrot_max=0.12)
    for shape in ((21, 21, 36), (64, 64, 36)):
        loc = tuple(s // 2 for s in shape)
        inj = [(s, FEEDBACK, loc) for s in range(a.steps)]
        nets = {'plain': PoseCellNetwork(shape), 'inject': PoseCellNetwork(shape)}
        legs = {'plain': lambda: nets['plain'].run(od), 'inject': lambda: nets['inject'].run(od, injections=inj)}
        for k, net in nets.items():
            net.inject(1, loc)
            net.set_profiling(True, per_kernel=False)
            legs[k]()
        us = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():
                ts = []
                for _ in range(a.batches):
                    f()
                    ts.append(nets[k].device_ms() * 1e3 / a.steps)
                us[k].append(float(np.median(ts)))
        rec = {'form': nets['plain'].step_form(), **{k: summary(v) for k, v in us.items()}}
        out['device_us_per_step']['x'.join(map(str, shape))] = rec
        print('(c)', shape, rec['form'], {k: '%.2f us (%.1f%%)' % (rec[k]['median'], 100 * rec[k]['spread'])
                                          for k in legs}, flush=True)
        for net in nets.values():
            net.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
