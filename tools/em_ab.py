#!/usr/bin/env python3
"""A/B timing of the linked experience map's relaxation (GPU box).

usage: python tools/em_ab.py [--rounds 5] [--sizes 64,256,768,1000,3072,10000,100000] [--replay 300]
                             [--out profiles/linked_em/em_ab.json]
One process alternates its legs, round by round, after a warm-up of every leg.  Per size
(experiences; a dead-reckoned chain plus one closure link per ten experiences), per call of
iterate(100):
  numpy   NumpyLinkedExperienceMap -- the baseline: what a user would write without this map;
  lds     LinkedExperienceMap under RS_EM_FORM=lds (sizes up to its cap of 3,072);
  sweep   LinkedExperienceMap under RS_EM_FORM=sweep.
Every GPU call ends with a read of one pose, so a host clock around it is what a caller who
looks at the map pays; the poses are written back before each call, so every call relaxes
the same map.  Per leg: the median over all calls and the spread (max - min of the
per-round medians over the median).  A last pass, with rs_em_set_timing on, records the
device time of the launches alone.  --replay N: messages per second of the synthetic ROS
stream (2N messages) with the dead-reckoned ExperienceMap against LinkedExperienceMap
(on_template + iterate(100) per frame, one 24-byte read per step in get_current_point).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOOPS = 100


def graph(n, seed=0):
    """(poses (n, 3), links): a random walk dead-reckoned with drift, chain links i -> i+1
    as measured, n // 10 closure links between random pairs with their true measurement."""
    import numpy as np
    from pyratslam_amd import linked_experience_map as M
    rng = np.random.default_rng(seed)

    def walk(step, turn):
        th = M.wrap(np.cumsum(turn))
        return np.stack([np.cumsum(step * np.cos(th)), np.cumsum(step * np.sin(th)), th], axis=1)

    def measure(p, a, b):
        dx, dy = p[b, 0] - p[a, 0], p[b, 1] - p[a, 1]
        return np.hypot(dx, dy), M.wrap(np.arctan2(dy, dx) - p[a, 2]), M.wrap(p[b, 2] - p[a, 2])

    step, turn = rng.uniform(0.05, 0.3, n), rng.uniform(-0.2, 0.2, n)
    truth, poses = walk(step, turn), walk(step * 1.002, turn * 1.01)
    a = np.arange(n - 1)
    ca = rng.integers(0, n, n // 10)
    cb = (ca + rng.integers(1, n, n // 10)) % n if n > 1 else ca
    links = np.zeros(n - 1 + len(ca), dtype=M.LINK_DTYPE)
    links['a'], links['b'] = np.concatenate([a, ca]), np.concatenate([a + 1, cb])
    for k, v in zip('dhf', measure(poses, a, a + 1)):
        links[k][:n - 1] = v
    for k, v in zip('dhf', measure(truth, ca, cb)):
        links[k][n - 1:] = v
    _, first = np.unique(np.stack([links['a'], links['b']]), axis=1, return_index=True)
    return poses, links[np.sort(first)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', default='64,256,768,1000,3072,10000,100000')
    ap.add_argument('--replay', type=int, default=300, help='odometry+frame pairs of the replay legs (0: none)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    from pyratslam_amd import linked_experience_map as M

    def gpu(form, **kw):
        os.environ['RS_EM_FORM'] = form        # read at create
        try:
            return M.LinkedExperienceMap(**kw)
        finally:
            del os.environ['RS_EM_FORM']

    out = {'loops': LOOPS, 'rounds': a.rounds, 'sizes': {}}
    for n in (int(s) for s in a.sizes.split(',')):
        poses, links = graph(n)
        maps = {'numpy': M.NumpyLinkedExperienceMap()}
        if n <= 3072:
            maps['lds'] = gpu('lds', capacity=n)
        maps['sweep'] = gpu('sweep', capacity=n)
        for m in maps.values():
            m.load(poses, links)
        result = {}

        def leg(key):
            m = maps[key]
            m.set_poses(poses)
            t0 = time.perf_counter()
            m.iterate(LOOPS)
            m._pose(0)                         # (waits for the sweeps)
            dt = time.perf_counter() - t0
            result[key] = m.poses()
            return dt

        for k in maps:                          # warm-up, and the legs agree
            leg(k)
            leg(k)
        if 'lds' in maps:
            assert result['lds'].tobytes() == result['sweep'].tobytes()
        err = float(np.abs(result['sweep'] - result['numpy']).max())
        assert err <= 1e-9, err                # (recorded; the tests hold 1e-12 on their maps)
        reps = {'numpy': 1 if n > 20000 else 3, 'lds': 10, 'sweep': 10}
        times = {k: [] for k in maps}
        for _ in range(a.rounds):
            for k in maps:
                times[k].append([leg(k) for _ in range(reps[k])])
        row = {'links': int(len(links)), 'max_abs_diff_vs_numpy': err}
        for k, rows in times.items():
            arr = np.array(rows) * 1e3
            med, rm = float(np.median(arr)), np.median(arr, axis=1)
            row[k] = {'ms_per_call': med, 'spread_pct': float((rm.max() - rm.min()) / med * 100)}
        for k in maps:                          # device time of the launches, a pass of its own
            if k == 'numpy':
                continue
            maps[k].set_timing(True)
            ms = []
            for _ in range(15):
                leg(k)
                ms.append(maps[k].device_ms())
            maps[k].set_timing(False)
            row[k].update({'device_ms': float(np.median(ms)),
                           'device_ms_spread_pct': float((max(ms) - min(ms)) / np.median(ms) * 100)})
            maps[k].close()
        out['sizes'][str(n)] = row
        print(json.dumps({n: row}), flush=True)

    if a.replay:
        from pyratslam_amd import synthetic
        from pyratslam_amd.experience_map import ExperienceMap
        from pyratslam_amd.replay import RatslamReplay
        events = synthetic.ros_stream(a.replay, seed=4)
        made = {'ExperienceMap': ExperienceMap, 'LinkedExperienceMap': M.LinkedExperienceMap}
        info = {}

        def replay_leg(key):
            r = RatslamReplay(em=made[key]())
            t0 = time.perf_counter()
            r.replay_events(events)
            if key != 'ExperienceMap':
                r.em.poses()                   # (the queued sweeps are part of the run)
                info.update(experiences=r.em.count, links=int(len(r.em.links())), form=r.em.form())
            dt = time.perf_counter() - t0
            r.em.close() if hasattr(r.em, 'close') else None
            return len(events) / dt
        for k in made:
            replay_leg(k)
        rates = {k: [] for k in made}
        for _ in range(a.rounds):
            for k in made:
                rates[k].append(replay_leg(k))
        out['replay'] = {'messages': len(events), **info}
        for k, v in rates.items():
            med = float(np.median(v))
            out['replay'][k] = {'messages_per_s': med, 'spread_pct': float((max(v) - min(v)) / med * 100)}
        print(json.dumps({'replay': out['replay']}), flush=True)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')
    print('| experiences | links | numpy ms (spread) | lds ms (spread) | sweep ms (spread) | lds device ms | sweep device ms |')
    print('|---|---|---|---|---|---|---|')
    for n, row in out['sizes'].items():
        cell = lambda k: '%.3f (%.1f%%)' % (row[k]['ms_per_call'], row[k]['spread_pct']) if k in row else '-'
        dev = lambda k: '%.3f' % row[k]['device_ms'] if k in row else '-'
        print('| %s | %d | %s | %s | %s | %s | %s |' % (n, row['links'], cell('numpy'), cell('lds'), cell('sweep'),
                                                      dev('lds'), dev('sweep')))


if __name__ == '__main__':
    main()
