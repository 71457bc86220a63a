#!/usr/bin/env python3
"""Timing of the pose-cell ensemble's feedback inside a run, one process,
alternating legs (GPU box).

usage: python tools/pc_ensemble_feedback_ab.py [--parent PARENT.so] [--shapes 21x21x36,32x32x18] [--members 256]
                                               [--steps 1000] [--repeats 9] [--route-steps 20]
                                               [--out profiles/pc_ensemble_feedback/ab.json]
Member m injects 1 at the grid's centre and takes odometry(steps, seed m), tools/pc_ensemble_ab.py's
inputs.  Per shape:
  (a) plain   rs_pce_run over the whole run through this commit's library and through PARENT.so
              (a build of the parent commit, loaded beside it), on one ensemble each, alternating,
              `repeats` times: device time per ensemble step (rs_pce_last_ms) and the call's wall
              time.  'within_parent_spread': this commit's median lies within the parent's own
              (max - min) of the parent's median.  Without --parent the leg is not measured.
  (b) feature one at-peak injection of 0.02 before every step and poses=True, through
              PoseCellEnsemble.run; the same with the injections alone and the poses alone; and
              the plain run again, all alternating, `repeats` times: device time per step, the
              added device time of each over the plain run, member steps per second by the wall
              clock.  Against it the only route without the feature, over `route-steps` steps:
              per step one inject per member at the peak the step before returned, run(one
              step), posecells and pc_peak.numpy_peak_sums per member; and the same without the
              pose.  First the two are checked against each other over those steps: equal peaks,
              resolved cells, sums and volumes.
One JSON document; exit status 1 when a check fails or leg (a) misses its condition.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def odometry(n, seed, vmax=0.6, rmax=0.15):
    import numpy as np
    r = np.random.default_rng(seed)
    return np.stack([r.uniform(0, vmax, n), r.uniform(-rmax, rmax, n)], axis=1)


def med(v):
    import numpy as np
    return float(np.median(v))


def load_other(path):
    """Another build of the library beside the product's: its own handle, the signatures of the
    symbols it has."""
    from pyratslam_amd import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


class RawEnsemble:
    """An ensemble handle of library `lib` driven through the C ABI: rs_pce_run with control
    arrays computed once by the caller."""

    def __init__(self, lib, members, shape, centre):
        import numpy as np
        from pyratslam_amd import _lib, filters as F
        from pyratslam_amd.posecell_network import pc_params
        self.lib, self.b = lib, members
        table = np.ascontiguousarray(F.FilterTable().filters, dtype=np.float64)
        params = pc_params(_lib.RS_PREC_F32, F.PC_GLOBAL_INHIB, table)
        self.h = ctypes.c_void_p()
        self.ok(lib.rs_pce_create(members, *shape, ctypes.byref(params), None, 0, ctypes.byref(self.h)))
        self.ok(lib.rs_pce_set_timing(self.h, 1))
        self.ok(lib.rs_pce_inject(self.h, -1, 1.0, *centre))

    def ok(self, st):
        if st != 0:
            raise RuntimeError('rs status %d: %s' % (st, self.lib.rs_last_error().decode()))

    def run(self, n, ctl, out):
        """(wall seconds, device seconds) of one rs_pce_run."""
        from pyratslam_amd import _lib
        ox, oy, fidx, zf = ctl
        i32 = ctypes.c_int32
        t0 = time.perf_counter()
        self.ok(self.lib.rs_pce_run(self.h, n, _lib.ptr(ox, i32), _lib.ptr(oy, i32), _lib.ptr(fidx, i32),
                                    _lib.ptr(zf, ctypes.c_double), _lib.ptr(out, i32)))
        wall = time.perf_counter() - t0
        ms = ctypes.c_double()
        self.ok(self.lib.rs_pce_last_ms(self.h, ctypes.byref(ms)))
        return wall, ms.value * 1e-3

    def read(self):
        import numpy as np
        from pyratslam_amd import _lib
        shape = [ctypes.c_int() for _ in range(4)]
        self.ok(self.lib.rs_pce_shape(self.h, *(ctypes.byref(s) for s in shape)))
        out = np.empty([s.value for s in shape])
        self.ok(self.lib.rs_pce_read(self.h, 0, self.b, _lib.ptr(out, ctypes.c_double)))
        return out

    def close(self):
        self.ok(self.lib.rs_pce_destroy(self.h))


def leg_plain(shape, members, steps, repeats, parent_path, od, ctl):
    """Leg (a): this commit's rs_pce_run against the parent build's, alternating."""
    import numpy as np
    from pyratslam_amd import _lib
    if not parent_path:
        return {'measured': False, 'why': 'no --parent build given'}
    centre = tuple(s // 2 for s in shape)
    sides = {'parent': RawEnsemble(load_other(parent_path), members, shape, centre),
             'this': RawEnsemble(_lib.load(), members, shape, centre)}
    out = {k: np.empty((members, steps, 3), dtype=np.int32) for k in sides}
    try:
        for k, e in sides.items():                      # warm-up, and the same results from both
            e.run(steps, ctl, out[k])
        same = bool(np.array_equal(out['parent'], out['this'])
                    and np.array_equal(sides['parent'].read(), sides['this'].read()))
        wall = {k: [] for k in sides}
        dev = {k: [] for k in sides}
        for _ in range(repeats):
            for k, e in sides.items():
                w, d = e.run(steps, ctl, out[k])
                wall[k].append(w)
                dev[k].append(d)
        rec = {'measured': True, 'same_results': same, 'repeats': repeats}
        for k in sides:
            us = [1e6 * d / steps for d in dev[k]]
            rec[k] = {'device_us_per_step': med(us), 'device_us_per_step_all': [round(u, 3) for u in us],
                      'device_us_spread': max(us) - min(us),
                      'wall_member_steps_per_s': members * steps / med(wall[k]),
                      'wall_seconds': [round(w, 5) for w in wall[k]]}
        rec['median_difference_us'] = rec['this']['device_us_per_step'] - rec['parent']['device_us_per_step']
        rec['within_parent_spread'] = bool(abs(rec['median_difference_us']) <= rec['parent']['device_us_spread'])
        return rec
    finally:
        for e in sides.values():
            e.close()


def route(ens, od, k, first_peaks, pose_r):
    """The route without the feature, k steps: per step an inject per member at its peak, a
    one-step run, and with pose_r the volumes read back and numpy_peak_sums per member.
    Returns (peaks, cells, sums, seconds by part)."""
    import numpy as np
    from pyratslam_amd import pc_peak
    members = len(ens)
    peaks = np.empty((members, k, 3), dtype=np.int32)
    cells = np.empty((members, k, 3), dtype=np.int32)
    sums = np.zeros((members, k, 6))
    parts = {'inject_and_run': 0.0, 'posecells': 0.0, 'numpy_peak_sums': 0.0}
    at = first_peaks
    for s in range(k):
        t0 = time.perf_counter()
        for m in range(members):
            ens.inject(0.02, tuple(int(v) for v in at[m]), members=[m])
        cells[:, s] = at
        at = peaks[:, s] = ens.run(od[:, s:s + 1])[:, 0]
        t1 = time.perf_counter()
        parts['inject_and_run'] += t1 - t0
        if pose_r:
            vols = ens.posecells
            t2 = time.perf_counter()
            for m in range(members):
                sums[m, s] = pc_peak.numpy_peak_sums(vols[m], at[m], pose_r)
            parts['posecells'] += t2 - t1
            parts['numpy_peak_sums'] += time.perf_counter() - t2
    return peaks, cells, sums, parts


def leg_feature(shape, members, steps, repeats, route_steps, od):
    """Leg (b): the feature's four forms alternating, and the route without it."""
    import numpy as np
    from pyratslam_amd import PoseCellEnsemble
    centre = tuple(s // 2 for s in shape)
    r = 3
    inj = [(None, s, 0.02, PoseCellEnsemble.AT_PEAK) for s in range(steps)]
    k = min(route_steps, steps)
    rec = {'cells_to_avg': r, 'route_steps': k, 'repeats': repeats}
    ens = PoseCellEnsemble(members, shape, cells_to_avg=r)
    twin = PoseCellEnsemble(members, shape)
    ens.set_timing(True)
    try:
        for e in (ens, twin):
            e.inject(1.0, centre)
        # the check, and the route's time, over the first k steps from the same fresh states
        peaks, poses, cells = ens.run(od[:, :k], poses=True, injections=inj[:k])
        t0 = time.perf_counter()
        r_peaks, r_cells, r_sums, parts = route(twin, od, k, twin.get_pc_max(), r)
        t_route = time.perf_counter() - t0
        rec['agree'] = bool(np.array_equal(peaks, r_peaks) and np.array_equal(cells.reshape(k, members, 3).transpose(1, 0, 2), r_cells)
                            and np.array_equal(ens.last_sums, r_sums) and np.array_equal(ens.posecells, twin.posecells))
        t0 = time.perf_counter()
        route(twin, od[:, k:], min(k, steps - k), twin.max_pc, 0)
        t_route_nopose = time.perf_counter() - t0
        rec['route'] = {'member_steps_per_s': members * k / t_route, 'seconds_per_step': t_route / k,
                        'seconds_per_step_by_part': {p: v / k for p, v in parts.items()}}
        if steps - k > 0:
            kk = min(k, steps - k)
            rec['route_without_pose'] = {'member_steps_per_s': members * kk / t_route_nopose,
                                         'seconds_per_step': t_route_nopose / kk}
        forms = {'plain': {}, 'injections': {'injections': inj}, 'poses': {'poses': True},
                 'both': {'poses': True, 'injections': inj}}
        for kw in forms.values():                       # warm-up of every instantiation
            ens.run(od, **kw)
        wall = {f: [] for f in forms}
        dev = {f: [] for f in forms}
        for _ in range(repeats):
            for f, kw in forms.items():
                t0 = time.perf_counter()
                ens.run(od, **kw)
                wall[f].append(time.perf_counter() - t0)
                dev[f].append(ens.device_ms() * 1e-3)
        for f in forms:
            us = [1e6 * d / steps for d in dev[f]]
            rec[f] = {'device_us_per_step': med(us), 'device_us_per_step_all': [round(u, 3) for u in us],
                      'device_member_steps_per_s': members * steps / med(dev[f]),
                      'wall_member_steps_per_s': members * steps / med(wall[f]),
                      'wall_seconds': [round(w, 5) for w in wall[f]]}
        for f in ('injections', 'poses', 'both'):
            rec[f]['added_device_us_per_step'] = rec[f]['device_us_per_step'] - rec['plain']['device_us_per_step']
            rec[f]['added_share_of_plain_step'] = rec[f]['added_device_us_per_step'] / rec['plain']['device_us_per_step']
        rec['speedup_wall_over_route'] = rec['both']['wall_member_steps_per_s'] / rec['route']['member_steps_per_s']
        return rec
    finally:
        ens.close()
        twin.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='')
    ap.add_argument('--shapes', default='21x21x36,32x32x18')
    ap.add_argument('--members', type=int, default=256)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--route-steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pc_ensemble_feedback', 'ab.json'))
    args = ap.parse_args()
    import numpy as np
    from pyratslam_amd import PoseCellEnsemble, _lib
    _lib.require_device()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    doc = {'members': args.members, 'steps': args.steps, 'parent': os.path.basename(args.parent) if args.parent else None,
           'cases': []}
    ok = True
    for s in args.shapes.split(','):
        shape = tuple(int(v) for v in s.split('x'))
        od = np.stack([odometry(args.steps, m) for m in range(args.members)])
        with PoseCellEnsemble(args.members, shape) as ens:
            ctl = ens._control(od, False)               # the control arrays, once for every plain run
        case = {'shape': list(shape)}
        case['plain'] = leg_plain(shape, args.members, args.steps, args.repeats, args.parent, od, ctl)
        case['feature'] = leg_feature(shape, args.members, args.steps, max(3, args.repeats // 3), args.route_steps, od)
        print(json.dumps(case), flush=True)
        doc['cases'].append(case)
        with open(args.out, 'w') as f:                  # (after every case: a later failure keeps the earlier ones)
            json.dump(doc, f, indent=1)
            f.write('\n')
        ok = ok and case['feature']['agree']
        if case['plain']['measured']:
            ok = ok and case['plain']['same_results'] and case['plain']['within_parent_spread']
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
