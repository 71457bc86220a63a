#!/usr/bin/env python3
"""A/B timing of the pose-cell ensemble against one PoseCellNetwork handle per member (GPU box).

usage: python tools/pc_ensemble_ab.py [--shapes 21x21x36,32x32x18] [--members 1,32,256,1024]
                                      [--steps 1000] [--repeats 3] [--out profiles/pc_ensemble/ab.jsonl]
Per shape and ensemble size B, member m injects 1 at the grid's centre and takes the steps
odometry(steps, seed m) (vtrans ~ U(0, 0.6), vrot ~ U(-0.15, 0.15)):
  ensemble  PoseCellEnsemble(B, shape).run(od): host clock round the call (control on the
            host, records, launches, one synchronisation) and rs_pce_last_ms, the device time
            of the launches alone;
  baseline  B PoseCellNetwork handles in this process, each run(od[m]) in turn (one host
            round trip per handle): the way to step B networks without the ensemble.
First the two are checked against each other from the same fresh states over the first 30
steps, the span over which each is within 1e-5 of the float64 oracle: peaks equal at every
step of every member, states within 2e-5 of each other.  The rest of the run is the warm-up;
how far the two float32 forms have drifted apart after all 1,000 steps is recorded
(long_run_*), not required: measured against the oracle, either form is 1e-3 off after some
hundred steps, and which of the two is closer varies by member.  Then `repeats` timed runs of
each, alternating; every run goes on from the state the one before left.
One JSON line per (shape, B); 'spread' is (max - min) /
median of the repeats' aggregate steps per second.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHECK_STEPS = 30


def odometry(n, seed, vmax=0.6, rmax=0.15):
    import numpy as np
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(0, vmax, n), r.uniform(-rmax, rmax, n)], axis=1)


def stats(rates):
    import numpy as np
    med = float(np.median(rates))
    return {'steps_per_s': med, 'spread': float((max(rates) - min(rates)) / med),
            'min_steps_per_s': float(min(rates)), 'max_steps_per_s': float(max(rates))}


def one_case(shape, members, steps, repeats):
    import numpy as np
    from pyratslam_amd import PoseCellEnsemble, PoseCellNetwork
    centre = tuple(s // 2 for s in shape)
    od = np.stack([odometry(steps, m) for m in range(members)])
    total = members * steps
    ens = PoseCellEnsemble(members, shape)
    ens.set_timing(True)
    ens.inject(1.0, centre)
    nets = [PoseCellNetwork(shape) for _ in range(members)]
    for net in nets:
        net.inject(1, centre)
    try:
        # agreement, from the same fresh states, over the first CHECK_STEPS steps: the span over
        # which either side is within 1e-5 of the float64 oracle (the tests' criterion)
        k = min(CHECK_STEPS, steps)
        pe = ens.run(od[:, :k])
        pb = np.stack([net.run(od[m, :k]) for m, net in enumerate(nets)])
        ve = ens.posecells
        diff = max(float(np.abs(ve[m] - net.posecells).max()) for m, net in enumerate(nets))
        mismatched = int((pe != pb).any(axis=2).sum())
        rec = {'shape': list(shape), 'members': members, 'steps': steps, 'repeats': repeats,
               'check_steps': k, 'peak_mismatches': mismatched, 'max_state_diff': diff,
               'agree': bool(mismatched == 0 and diff < 2e-5)}
        # warm-up over the whole run; how far two float32 forms of the same dynamics have
        # drifted apart by then is recorded, not required
        pe = ens.run(od[:, k:])
        pb = np.stack([net.run(od[m, k:]) for m, net in enumerate(nets)])
        ve = ens.posecells
        rec['long_run_peak_mismatches'] = int((pe != pb).any(axis=2).sum())
        rec['long_run_max_state_diff'] = max(float(np.abs(ve[m] - net.posecells).max())
                                             for m, net in enumerate(nets))
        wall_e, dev_e, wall_b = [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            ens.run(od)
            wall_e.append(time.perf_counter() - t0)
            dev_e.append(ens.device_ms() * 1e-3)
            t0 = time.perf_counter()
            for m, net in enumerate(nets):
                net.run(od[m])
            wall_b.append(time.perf_counter() - t0)
        rec['ensemble_wall'] = dict(stats([total / t for t in wall_e]), seconds=[round(t, 6) for t in wall_e])
        rec['ensemble_device'] = dict(stats([total / t for t in dev_e]), seconds=[round(t, 6) for t in dev_e])
        rec['baseline_wall'] = dict(stats([total / t for t in wall_b]), seconds=[round(t, 6) for t in wall_b])
        rec['ensemble_device_us_per_member_step'] = float(np.median(dev_e)) * 1e6 / total
        rec['ensemble_device_us_per_ensemble_step'] = float(np.median(dev_e)) * 1e6 / steps
        rec['baseline_us_per_member_step'] = float(np.median(wall_b)) * 1e6 / total
        rec['speedup_wall'] = rec['ensemble_wall']['steps_per_s'] / rec['baseline_wall']['steps_per_s']
        rec['speedup_device'] = rec['ensemble_device']['steps_per_s'] / rec['baseline_wall']['steps_per_s']
        # the requirement: the slowest ensemble repeat still beats the fastest baseline repeat
        rec['ensemble_beats_baseline_beyond_spread'] = bool(
            rec['ensemble_wall']['min_steps_per_s'] > rec['baseline_wall']['max_steps_per_s'])
        return rec
    finally:
        ens.close()
        for net in nets:
            net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='21x21x36,32x32x18')
    ap.add_argument('--members', default='1,32,256,1024')
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pc_ensemble', 'ab.jsonl'))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    sizes = [int(v) for v in args.members.split(',')]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ok = True
    with open(args.out, 'w') as f:
        for shape in shapes:
            for members in sizes:
                rec = one_case(shape, members, args.steps, args.repeats)
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + '\n')
                f.flush()
                ok = ok and rec['agree']
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
