#!/usr/bin/env python3
"""A/B timing of the pose cells' sub-cell pose (GPU box).

usage: python tools/pc_peak_ab.py [--rounds 5] [--calls 2000] [--steps 1000] [--batches 20]
                                  [--shapes 64x64x36,21x21x36] [--out profiles/pc_peak/pc_peak_ab.json]
One process alternates its legs, round by round, after a warm-up of every leg; every leg
has a network of its own, all started from the same injection and fed the same odometry.
Per grid:
  update         update(v): the integer peak cell alone (what the parent commit offers);
  update_pose    update_pose(v): the step and the centroid queued behind it, one round trip;
  eager_numpy    the only way to the pose without the kernel: a readback='eager' network's
                 update(v), the volume it exported, and numpy_peak_sums on the host;
  run            run(od) of --steps steps, per step;
  run_poses      run(od, poses=True) of the same steps, per step.
A host clock around calls that end in the library's own wait (every call returns with its
results on the host).  Per leg: the median over all calls of all rounds, in microseconds, and
the spread (max - min of the per-round medians over the median).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=2000, help='per-call legs: calls per round')
    ap.add_argument('--steps', type=int, default=1000, help='batched legs: steps per run()')
    ap.add_argument('--batches', type=int, default=20, help='batched legs: run() calls per round')
    ap.add_argument('--shapes', default='64x64x36,21x21x36')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    from pyratslam_amd import PoseCellNetwork, numpy_peak_sums, pose_from_sums, synthetic

    out = {'rounds': a.rounds, 'calls': a.calls, 'steps': a.steps, 'batches': a.batches, 'unit': 'us', 'shapes': {}}
    for name in a.shapes.split(','):
        shape = tuple(int(s) for s in name.split('x'))
        loc = tuple(s // 2 for s in shape)
        od = synthetic.odometry(max(a.calls, a.steps), seed=7, vtrans_max=0.3, vrot_max=0.12)
        nets = {k: PoseCellNetwork(shape, readback='eager' if k == 'eager_numpy' else 'lazy')
                for k in ('update', 'update_pose', 'eager_numpy', 'run', 'run_poses')}
        for net in nets.values():
            net.inject(1, loc)

        def eager_numpy(v, net=nets['eager_numpy']):
            cell = net.update(v)
            return pose_from_sums(numpy_peak_sums(net.posecells, cell, net.cells_to_avg), cell, shape)

        per_call = {'update': nets['update'].update, 'update_pose': nets['update_pose'].update_pose,
                    'eager_numpy': eager_numpy}
        batched = {'run': lambda: nets['run'].run(od[:a.steps]),
                   'run_poses': lambda: nets['run_poses'].run(od[:a.steps], poses=True)}
        for f in per_call.values():     # warm-up of every leg
            for v in od[:50]:
                f(v)
        for f in batched.values():
            f()
        t = {k: [] for k in list(per_call) + list(batched)}
        for _ in range(a.rounds):
            for k, f in per_call.items():
                ts = np.empty(a.calls)
                for i in range(a.calls):
                    t0 = time.perf_counter()
                    f(od[i])
                    ts[i] = time.perf_counter() - t0
                t[k].append(ts * 1e6)
            for k, f in batched.items():
                ts = np.empty(a.batches)
                for i in range(a.batches):
                    t0 = time.perf_counter()
                    f()
                    ts[i] = time.perf_counter() - t0
                t[k].append(ts * 1e6 / a.steps)
        rec = {'form': nets['update'].step_form()}
        for k, rounds in t.items():
            med = float(np.median(np.concatenate(rounds)))
            per_round = [float(np.median(r)) for r in rounds]
            rec[k] = {'median_us': med, 'spread': (max(per_round) - min(per_round)) / med, 'round_medians_us': per_round}
        # the legs must have computed the same thing
        assert nets['update'].max_pc == nets['update_pose'].max_pc == nets['eager_numpy'].max_pc
        assert np.array_equal(nets['run'].posecells, nets['run_poses'].posecells)
        out['shapes'][name] = rec
        print(name, rec['form'], {k: '%.2f us (%.1f%%)' % (v['median_us'], 100 * v['spread'])
                                  for k, v in rec.items() if k != 'form'}, flush=True)
        for net in nets.values():
            net.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
